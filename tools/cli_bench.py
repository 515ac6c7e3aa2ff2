#!/usr/bin/env python3
"""tools/cli_bench.py — end-to-end rate of the gnumap driver binary (FASTQ file -> SAM + .sgr files) on a synthetic
reference; the numbers quoted in DESIGN.md for SURVEY §8 row (f2).  Usage:
    python tools/cli_bench.py [--mbp 100] [--reads 2000000] [--args "-a 0.9"] [--dir /tmp/gm_cli]
Writes the FASTA / FASTQ with numpy (substitution-only reads, 50 % reverse strand), builds the index through the binary on
its first run, then times a second run (index already on disk)."""
import argparse, glob, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=6)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--args", default="-a 0.9")
    ap.add_argument("--dir", default="/tmp/gm_cli")
    ap.add_argument("--sweep", default="", help="further argument sets for the timed run, separated by ';' (each one more run on the same files)")
    ap.add_argument("--bam_index", action="store_true", help="two more timed runs: --sam_format=bam --sam_sort=coordinate, then the same with --bam_index (<out>.bam.bai)")
    ap.add_argument("--bam_lz77", action="store_true", help="three more timed runs: --sam_format=bam, the same with --bam_lz77, and --sam_format=bam --sam_sort=coordinate --bam_lz77 --bam_index")
    ap.add_argument("--sam_md", action="store_true", help="four more timed runs: --sam_text=device and --sam_format=bam, each without and with --sam_md --sam_cigar=forward")
    ap.add_argument("--mates", action="store_true", help="paired reads (inserts around 300 bases) in two files, and four more timed runs: the two files concatenated and mapped "
                                                         "unpaired, and --mates=, each as --sam_text=device and as --sam_format=bam --sam_sort=coordinate")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    fa = os.path.join(a.dir, "g%g.fa" % a.mbp); fq = os.path.join(a.dir, "r%d.fq" % a.reads)
    bench.make_genome(fa, a.mbp, 42, a.contigs)
    raw = np.fromfile(fa, np.uint8)                                # FASTA text -> 2-bit codes: drop the header lines and the newlines
    keep = np.ones(len(raw), bool)
    for h in np.flatnonzero(raw == ord(">")):
        e = h + int(np.argmax(raw[h:h + 4096] == 10))
        keep[h:e + 1] = False
    keep &= raw != 10
    codes = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), raw[keep]).astype(np.uint8)
    del raw, keep
    rng = np.random.default_rng(7)
    L, n = a.len, a.reads
    acgt = np.frombuffer(b"ACGT", np.uint8)
    with open(fq, "wb") as f:
        for s in range(0, n, 250_000):
            m = min(250_000, n - s)
            pos = rng.integers(0, len(codes) - L - 1, m)
            c = codes[pos[:, None] + np.arange(L)[None, :]].astype(np.int64)
            sub = rng.random((m, L)) < 0.01
            c = np.where(sub, (c + rng.integers(1, 4, (m, L))) % 4, c)
            rev = rng.random(m) < 0.5
            c = np.where(rev[:, None], 3 - c[:, ::-1], c)
            q = (rng.integers(20, 41, (m, L)) + 33).astype(np.uint8)
            rec = np.empty((m, 2 * L + 16), np.uint8)
            names = np.char.zfill((np.arange(s, s + m)).astype(str), 9).astype("S9")
            rec[:, 0] = ord("@"); rec[:, 1] = ord("r"); rec[:, 2:11] = np.frombuffer(names.tobytes(), np.uint8).reshape(m, 9)
            rec[:, 11] = 10; rec[:, 12:12 + L] = acgt[c]; rec[:, 12 + L] = 10; rec[:, 13 + L] = ord("+"); rec[:, 14 + L] = 10
            rec[:, 15 + L:15 + 2 * L] = q; rec[:, 15 + 2 * L] = 10
            f.write(rec.tobytes())
    def write_records(f, first, c, q):                           # m records "@r<9 digits>\n<bases>\n+\n<qualities>\n"
        m = len(c)
        rec = np.empty((m, 2 * L + 16), np.uint8)
        names = np.char.zfill((np.arange(first, first + m)).astype(str), 9).astype("S9")
        rec[:, 0] = ord("@"); rec[:, 1] = ord("r"); rec[:, 2:11] = np.frombuffer(names.tobytes(), np.uint8).reshape(m, 9)
        rec[:, 11] = 10; rec[:, 12:12 + L] = acgt[c]; rec[:, 12 + L] = 10; rec[:, 13 + L] = ord("+"); rec[:, 14 + L] = 10
        rec[:, 15 + L:15 + 2 * L] = q; rec[:, 15 + 2 * L] = 10
        f.write(rec.tobytes())

    fq1, fq2, fq12 = (os.path.join(a.dir, "p%d_%s.fq" % (n, k)) for k in ("1", "2", "12"))
    if a.mates:
        # n / 2 pairs: the plus-strand mate at a random place, the minus-strand mate ending `insert` bases on (normal around 300, sd 30,
        # at least L); the first mate is the minus one in half of the pairs; 1 % substitutions.  fq12 = fq1 followed by fq2: the same
        # reads for an unpaired run
        with open(fq1, "wb") as f1, open(fq2, "wb") as f2:
            for s in range(0, n // 2, 250_000):
                m = min(250_000, n // 2 - s)
                ins = np.clip(np.rint(rng.normal(300, 30, m)).astype(np.int64), L, 600)
                pos = rng.integers(0, len(codes) - 700, m)
                cf = codes[pos[:, None] + np.arange(L)[None, :]].astype(np.int64)
                cr = 3 - codes[(pos + ins - L)[:, None] + np.arange(L)[None, :]].astype(np.int64)[:, ::-1]
                cf = np.where(rng.random((m, L)) < 0.01, (cf + rng.integers(1, 4, (m, L))) % 4, cf)
                cr = np.where(rng.random((m, L)) < 0.01, (cr + rng.integers(1, 4, (m, L))) % 4, cr)
                swap = (rng.random(m) < 0.5)[:, None]
                write_records(f1, s, np.where(swap, cr, cf), (rng.integers(20, 41, (m, L)) + 33).astype(np.uint8))
                write_records(f2, s, np.where(swap, cf, cr), (rng.integers(20, 41, (m, L)) + 33).astype(np.uint8))
        with open(fq12, "wb") as f:
            for src in (fq1, fq2):
                with open(src, "rb") as g:
                    while True:
                        buf = g.read(1 << 26)
                        if not buf:
                            break
                        f.write(buf)
    exe = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
    out = os.path.join(a.dir, "out")
    env = dict(os.environ)
    runs = [("index+map", a.args), ("map", a.args)] + [("map " + x.strip(), a.args + " " + x.strip()) for x in a.sweep.split(";") if x.strip()]
    if a.bam_index:
        sorted_bam = "--sam_format=bam --sam_sort=coordinate"
        runs += [("map " + x, a.args + " " + x) for x in (sorted_bam, sorted_bam + " --bam_index")]
    if a.bam_lz77:
        runs += [("map " + x, a.args + " " + x) for x in ("--sam_format=bam", "--sam_format=bam --bam_lz77", "--sam_format=bam --sam_sort=coordinate --bam_lz77 --bam_index")]
    if a.sam_md:
        tags = " --sam_md --sam_cigar=forward"
        runs += [("map " + x, a.args + " " + x) for x in ("--sam_text=device", "--sam_text=device" + tags, "--sam_format=bam", "--sam_format=bam" + tags)]
    reads_of = {}                                                # run -> its read file, where that is not fq
    if a.mates:
        for form in ("--sam_text=device", "--sam_format=bam --sam_sort=coordinate"):
            runs.append(("map unpaired, both files " + form, a.args + " " + form)); reads_of[runs[-1][0]] = fq12
            runs.append(("map --mates= " + form, a.args + " " + form + " --mates=" + fq2)); reads_of[runs[-1][0]] = fq1
    def shard_files():                                           # <out>.<k>.sam of a --sam_shards=K run
        return [f for f in glob.glob(glob.escape(out) + ".*.sam") if f[len(out) + 1:-4].isdigit()]

    sam_bytes = 0
    for run, args in runs:
        for f in [out + ext for ext in (".sam", ".bam", ".bam.bai", ".sgr", ".gmp")] + shard_files():     # fresh output files each time (overwriting 8 GB of page cache is a different test)
            if os.path.exists(f):
                os.remove(f)
        t0 = time.time()
        with open(out + ".stderr", "w+") as log:                  # os.wait4: this child's own peak resident set
            child = subprocess.Popen([exe, "-g", fa, "-o", out, "-v", "1"] + args.split() + [reads_of.get(run, fq)], stdout=subprocess.DEVNULL, stderr=log, env=env)
            _, status, usage = os.wait4(child.pid, 0)
            child.returncode = os.waitstatus_to_exitcode(status)
            dt = time.time() - t0
            log.seek(0); err = log.read()
        print(f"--- {run}: {dt:.2f} s wall, {n / dt / 1e6:.3f} M reads/s end to end (rc {child.returncode}), peak resident host memory {usage.ru_maxrss / 1048576:.2f} GB")
        print("\n".join(l for l in err[-3000:].splitlines() if not l.startswith("[gm_")))
        print("track files:", ", ".join(f"{ext} {os.path.getsize(out + ext)} bytes" for ext in (".sgr", ".gmp") if os.path.exists(out + ext)))
        sam_bytes = sum(os.path.getsize(f) for f in ([out + ".sam"] if os.path.exists(out + ".sam") else []) + shard_files())
        if os.path.exists(out + ".bam"):                          # --sam_format=bam
            print("BAM bytes", os.path.getsize(out + ".bam"))
        if os.path.exists(out + ".bam.bai"):                      # --bam_index
            print("BAI bytes", os.path.getsize(out + ".bam.bai"))
    print("SAM bytes", sam_bytes, "FASTQ bytes", os.path.getsize(fq))


if __name__ == "__main__":
    main()
