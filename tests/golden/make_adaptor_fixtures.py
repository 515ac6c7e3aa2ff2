#!/usr/bin/env python3
"""-A / --adaptor fixtures, produced by the UNMODIFIED reference program.

Run in the build container only (needs the reference sources):
    make -C oracle refbin && python tests/golden/make_adaptor_fixtures.py

Inputs written (deterministic, derived from the committed syn.fq; our own generator):

    syn_adapt.fq       the reads of syn.fq (8 .. 150 bp) with their tails overwritten by a prefix of a 60-character adaptor (whose
                       first 34 characters are the adaptor most modes trim) followed by random bases: tails of 0, 3, 5, 8, 12, 20, 34, 45
                       and 60 bases, clean or with 1 or 3 mismatches; tails that sit exactly on the 0.85 boundary (17/20, 34/40, 51/60)
                       and one mismatch below it (16/20); a few reads in lower case (the compare is case-sensitive: nothing matches);
                       36- and 50-bp reads whose kept length falls below -m; an adaptor occurrence in mid-read
    syn_adapt_ill.fq   90 of those reads re-encoded Phred+64.  Read 60 keeps one Phred+33 character among its last four bases, which the
                       trim always drops: it must NOT trigger the --illumina fallback.  Read 75 has one at position 5: that one does.
    syn_adapt_u100.fq  200 of the 100-bp reads of syn.fq untouched, none of which resembles the adaptor at any offset (not even in the
                       5 .. 7 characters compared near its end): every read keeps 96 bases, a block of ONE length

Outputs committed, one set per entry of MODES (reference run with -c 1):

    tests/golden/ref_runs_adaptor/<mode>.sam.gz           the SAM file, @PG line dropped
    tests/golden/ref_runs_adaptor/<mode>.sgr.gz|.gmp.gz   the coverage / per-nucleotide track text
    tests/golden/ref_runs_adaptor/manifest.json           argv, adaptor and FASTQ per mode

Everything committed is DATA (our inputs, the reference's outputs on them); no reference source text.
"""
import gzip, json, os, shutil, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from adaptor_model import kept_length        # tests/adaptor_model.py: only to pick the reads of syn_adapt_u100.fq
REFBIN = os.path.join(ROOT, "oracle", "_ref", "gnumap_ref")
OUT = os.path.join(HERE, "ref_runs_adaptor")

AD60 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCTCGTATGCCGTCTTCTGCTTGAA"
AD34 = AD60[:34]
AD6 = AD60[:6]
TAILS = [0, 3, 5, 8, 12, 20, 34, 45, 60]

# name -> (adaptor, reference argv between "-a 0.9 -A <adaptor>" and the FASTQ, fastq)
MODES = {
    "default":   (AD34, [], "syn_adapt.fq"),
    "all":       (AD34, ["--print_all_sam"], "syn_adapt.fq"),
    "no_nw":     (AD34, ["--no_nw"], "syn_adapt.fq"),
    "bs":        (AD34, ["-b"], "syn_adapt.fq"),
    "illumina":  (AD34, ["--illumina"], "syn_adapt_ill.fq"),
    "m14_j7":    (AD34, ["-m", "14", "-j", "7"], "syn_adapt.fq"),
    "down":      (AD34, ["--down_strand"], "syn_adapt.fq"),
    "M5_a80":    (AD34, ["-M", "5", "-a", "0.8"], "syn_adapt.fq"),
    "a6":        (AD6, [], "syn_adapt.fq"),
    "a60":       (AD60, [], "syn_adapt.fq"),
    "u100":      (AD34, [], "syn_adapt_u100.fq"),
}


def read_fastq(path):
    recs = []
    with open(path, "rb") as f:
        while True:
            name = f.readline()
            if not name:
                break
            seq = f.readline().rstrip(b"\n"); f.readline(); qual = f.readline().rstrip(b"\n")
            recs.append((name.rstrip(b"\n"), seq, qual))
    return recs


def write_fastq(path, recs):
    with open(path, "wb") as f:
        for name, seq, qual in recs:
            f.write(name + b"\n" + seq + b"\n+\n" + qual + b"\n")


def with_tail(seq, tail, mism, rng):
    """the last `tail` bases of seq replaced by (AD60 + random bases)[:tail], `mism` of the adaptor's characters changed"""
    if tail == 0:
        return seq
    t = bytearray((AD60 + "".join("ACGT"[k] for k in rng.integers(0, 4, 64)))[:tail].encode())
    span = min(tail, len(AD60))
    for k in sorted(rng.choice(span, min(mism, span), replace=False)):
        t[k] = ord("ACGT"[("ACGT".index(chr(t[k])) + 1 + int(rng.integers(0, 3))) % 4])
    return seq[:len(seq) - tail] + bytes(t)


def make_adaptor_fastq(src):
    rng = np.random.default_rng(20240611)
    out = []
    for i, (name, seq, qual) in enumerate(read_fastq(src)):
        L = len(seq)
        tail = TAILS[i % len(TAILS)]
        while tail >= L:                                    # a read keeps at least one base of its own
            tail = max(t for t in TAILS if t < tail)
        mism = (0, 1, 0, 3, 0)[i % 5] if tail >= 8 else 0
        if L >= 100 and i % 23 == 7: tail, mism = 20, 3      # 17/20 = 0.85 exactly: qualifies
        if L >= 100 and i % 23 == 8: tail, mism = 20, 4      # 16/20: does not qualify at that offset
        if L >= 100 and i % 23 == 9: tail, mism = 40, 6      # 34/40 with the 60-character adaptor
        if L >= 100 and i % 23 == 10: tail, mism = 60, 9     # 51/60 with the 60-character adaptor
        s = with_tail(seq, tail, mism, rng)
        if L >= 100 and i % 37 == 11:                        # an adaptor occurrence in mid-read, nothing at the end
            s = seq[:30] + AD34.encode() + seq[64:]
        if i % 41 == 5:                                      # lower case: the upper-case adaptor matches nowhere
            s = s.lower()
        assert len(s) == L
        out.append((name, s, qual))
    return out


def make_illumina(recs):
    rng = np.random.default_rng(7)
    idx = sorted(rng.choice([i for i, r in enumerate(recs) if len(r[1]) >= 36], 90, replace=False))
    out = []
    for k, i in enumerate(idx):
        name, seq, qual = recs[i]
        q = bytearray(min(126, c + 31) for c in qual)
        if k == 60: q[len(seq) - 2] = ord("5")               # inside the four bases every read loses: never looked at
        if k == 75: q[5] = ord("5")                          # inside the kept part: the fallback happens here
        out.append((name, seq, bytes(q)))
    return out


def main():
    assert os.path.exists(REFBIN), "make -C oracle refbin first"
    os.makedirs(OUT, exist_ok=True)
    base = read_fastq(os.path.join(HERE, "syn.fq"))
    recs = make_adaptor_fastq(os.path.join(HERE, "syn.fq"))
    write_fastq(os.path.join(HERE, "syn_adapt.fq"), recs)
    write_fastq(os.path.join(HERE, "syn_adapt_ill.fq"), make_illumina(recs))
    write_fastq(os.path.join(HERE, "syn_adapt_u100.fq"), [r for r in base if len(r[1]) == 100 and kept_length(r[1], AD34.encode()) == 96][:200])
    work = tempfile.mkdtemp()
    for f in os.listdir(HERE):
        if f.startswith("syn.") or f.startswith("syn_adapt"):
            shutil.copy(os.path.join(HERE, f), work)
    only = set(sys.argv[1:])
    manifest = json.load(open(os.path.join(OUT, "manifest.json"))) if only else {}
    for name, (adaptor, args, fq) in MODES.items():
        if only and name not in only:
            continue
        r = subprocess.run([REFBIN, "-g", "syn.fa", "-o", name, "-a", "0.9", "-c", "1", "-A", adaptor] + args + [fq], cwd=work, capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        sam = [l for l in open(os.path.join(work, name + ".sam"), "rb") if not l.startswith(b"@PG")]
        with gzip.GzipFile(os.path.join(OUT, name + ".sam.gz"), "wb", mtime=0) as g:
            g.write(b"".join(sam))
        tracks = []
        for ext in ("sgr", "gmp"):
            p = os.path.join(work, name + "." + ext)
            if os.path.exists(p):
                with gzip.GzipFile(os.path.join(OUT, name + "." + ext + ".gz"), "wb", mtime=0) as g:
                    g.write(open(p, "rb").read())
                tracks.append(ext)
        manifest[name] = dict(adaptor=adaptor, argv=args, fastq=fq, sam_lines=len(sam), tracks=tracks)
        print(f"{name:12s} {len(sam):5d} SAM lines  {tracks}")
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
