#!/usr/bin/env python3
"""Edge fixtures: a small genome whose contigs begin and end in mid-word, reads at every begin and end of it, and what the
UNMODIFIED reference program writes for them.

Run in the build container only (needs the reference sources):
    make -C oracle refbin && python tests/golden/make_edge_fixtures.py

Inputs written (deterministic; our own generator, fixed seed):

    edge.fa        three contigs of 5003, 3001 and 2003 bp: inner offsets 5003 (= 11 mod 16, 3 mod 4) and 8004 (= 4 mod 16),
                   l_pac = 10007 (= 7 mod 16, 3 mod 4): a contig starts inside a 16-base word and inside a pac byte, the last word and
                   the last pac byte are partial.  One 14-mer X stands at [3, 17) and [20, 34) of the first contig AND of the second:
                   a seed of a read that holds X at offset i >= 20 votes for max(0, c - i) = 0 with BOTH copies at the start of the
                   reference (the only way one seed reaches -k 2 alone), while at the start of the second contig c - i lies in the
                   first contig and the contig test has to reject the window.
    edge.fq        100-bp reads, qualities 'I', forward and reverse-complemented:
                     s<c>_<k>     exact read at start(c) + k, k = 0 .. 19
                     hs<c>_<d>    d random bases + the first 100 - d bases of contig c, d = 1 .. 6
                     e<c>_<k>     exact read ending at end(c) - k, k = 0 .. 19
                     he<c>_<d>    the last 100 - d bases of contig c + d random bases, d = 1 .. 6
                     dv<o>        random bases with X at offset o = 17, 20, 23, 40, 60, 85, 86
                     sh<d>        d random bases + the first 100 - d bases of the reference, d = 20, 30
    edge_mixed.fq  the same recipe at the lengths 16, 19, 24, 36, 50 and 150, one length after the other read by read (a block of mixed
                   lengths), with k = 0, 1, 3, 15, 16, 19 and d = 1, 4, 6

Outputs committed, one set per entry of MODES (reference run with -c 1; the reference builds its own index of edge.fa):

    tests/golden/ref_runs_edge/<mode>.sam.gz           the SAM file, @PG line dropped
    tests/golden/ref_runs_edge/<mode>.sgr.gz|.gmp.gz   the coverage / per-nucleotide track text
    tests/golden/ref_runs_edge/manifest.json           argv, oracle / product parameters, FASTQ, tracks, SAM lines per mode

Everything committed is DATA (our inputs, the reference's outputs on them); no reference source text.
"""
import gzip, json, os, shutil, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFBIN = os.path.join(ROOT, "oracle", "_ref", "gnumap_ref")
OUT = os.path.join(HERE, "ref_runs_edge")

CONTIGS = [("edgeA", 5003), ("edgeB", 3001), ("edgeC", 2003)]
X = b"GATTACAGCCTAGT"                      # the planted 14-mer
X_AT = (3, 20)                             # ... at these offsets of the first and of the second contig
LENS_MIXED = (16, 19, 24, 36, 50, 150)
DV_OFFSETS = (17, 20, 23, 40, 60, 85, 86)

# name -> (reference argv between "-a 0.9 -c 1" and the FASTQ, oracle / product parameter overrides, fastq)
MODES = {
    "default":       ([], {}, "edge.fq"),
    "no_nw":         (["--no_nw"], dict(nw=0), "edge.fq"),
    "m14_j7":        (["-m", "14", "-j", "7"], dict(mer=14, jump=7), "edge.fq"),
    "m14_j7_no_nw":  (["-m", "14", "-j", "7", "--no_nw"], dict(mer=14, jump=7, nw=0), "edge.fq"),
    "k1_m14":        (["-k", "1", "-m", "14"], dict(min_seed_hits=1, mer=14), "edge.fq"),
    # everything that is scored is accepted: the score of a clamped window is SAM text
    "raw_all":       (["-r", "-a", "-1000000"], dict(align_is_fraction=0, align_score=-1000000.0), "edge.fq"),
    "up":            (["--up_strand"], dict(neg_strand=0), "edge.fq"),
    "down":          (["--down_strand"], dict(pos_strand=0), "edge.fq"),
    "M5":            (["-M", "5"], dict(max_gap=5), "edge.fq"),
    "bs":            (["-b"], dict(mode=1), "edge.fq"),
    "bin1":          (["--bin_size=1"], dict(bin_size=1), "edge.fq"),       # the first and the last base of every contig are rows
    "mixed":         ([], {}, "edge_mixed.fq"),
    "mixed_m14_no_nw": (["-m", "14", "-j", "7", "--no_nw"], dict(mer=14, jump=7, nw=0), "edge_mixed.fq"),
}

sys.path.insert(0, os.path.dirname(HERE))
from edge_ref_env import REF_MALLOC_ENV       # tests/edge_ref_env.py: why the reference runs with a malloc setting
REF_ENV = dict(os.environ, **REF_MALLOC_ENV)

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rand_bases(rng, n):
    return bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))


def make_genome():
    rng = np.random.default_rng(20240917)
    seqs = []
    for ci, (name, n) in enumerate(CONTIGS):
        s = bytearray(rand_bases(rng, n))
        if ci < 2:
            for o in X_AT:
                s[o:o + len(X)] = X
                s[o - 1] = s[o + len(X)] = ord("A")           # the dv reads carry C there: no 14-mer of theirs but X itself occurs
        seqs.append(bytes(s))
    return seqs


def geometry():
    """[(start, end)] of every contig in reference coordinates, and l_pac"""
    out, o = [], 0
    for _, n in CONTIGS:
        out.append((o, o + n)); o += n
    return out, o


def write_fasta(path, seqs):
    with open(path, "wb") as f:
        for (name, _), s in zip(CONTIGS, seqs):
            f.write(b">" + name.encode() + b"\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + b"\n")


def make_reads(seqs, L, ks, ds, rng):
    """[(name, sequence)] of the recipe at length L, forward reads only (the caller adds the reverse complements)"""
    out = []
    for ci, s in enumerate(seqs):
        n = len(s)
        for k in ks:
            out.append((f"s{ci}_{k}", s[k:k + L]))
        for d in ds:
            out.append((f"hs{ci}_{d}", rand_bases(rng, d) + s[:L - d]))
        for k in ks:
            out.append((f"e{ci}_{k}", s[n - k - L:n - k]))
        for d in ds:
            out.append((f"he{ci}_{d}", s[n - (L - d):] + rand_bases(rng, d)))
    for o in DV_OFFSETS:
        if o + len(X) <= L:
            r = bytearray(rand_bases(rng, L)); r[o:o + len(X)] = X
            r[o - 1] = ord("C")
            if o + len(X) < L:
                r[o + len(X)] = ord("C")
            out.append((f"dv{o}", bytes(r)))
    for d in (20, 30):
        if d < L - 10:
            out.append((f"sh{d}", rand_bases(rng, d) + seqs[0][:L - d]))
    for name, s in out:
        assert len(s) == L, (name, len(s), L)
    return out


def both_strands(reads, L):
    out = []
    for name, s in reads:
        out.append((f"{name}_L{L}_f", s)); out.append((f"{name}_L{L}_r", revcomp(s)))
    return out


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for name, s in reads:
            f.write(b"@" + name.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")


def main():
    assert os.path.exists(REFBIN), "make -C oracle refbin first"
    os.makedirs(OUT, exist_ok=True)
    seqs = make_genome()
    (_, l_pac) = geometry()
    assert l_pac % 16 and l_pac % 4 and all(b % 16 for b, _ in geometry()[0][1:]) and any(b % 4 for b, _ in geometry()[0][1:])
    write_fasta(os.path.join(HERE, "edge.fa"), seqs)
    rng = np.random.default_rng(20240918)
    write_fastq(os.path.join(HERE, "edge.fq"), both_strands(make_reads(seqs, 100, range(20), range(1, 7), rng), 100))
    per_len = [both_strands(make_reads(seqs, L, (0, 1, 3, 15, 16, 19), (1, 4, 6), rng), L) for L in LENS_MIXED]
    mixed = []
    for j in range(max(len(p) for p in per_len)):                 # one length after the other, read by read
        mixed += [p[j] for p in per_len if j < len(p)]
    write_fastq(os.path.join(HERE, "edge_mixed.fq"), mixed)

    work = tempfile.mkdtemp()
    for f in ("edge.fa", "edge.fq", "edge_mixed.fq"):
        shutil.copy(os.path.join(HERE, f), work)
    only = set(sys.argv[1:])
    manifest = json.load(open(os.path.join(OUT, "manifest.json"))) if only else {}
    for name, (args, kw, fq) in MODES.items():
        if only and name not in only:
            continue
        r = subprocess.run([REFBIN, "-g", "edge.fa", "-o", name, "-a", "0.9", "-c", "1"] + args + [fq], cwd=work, capture_output=True, text=True,
                           env=REF_ENV)
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
        manifest[name] = dict(argv=args, params=kw, fastq=fq, sam_lines=len(sam), tracks=tracks)
        print(f"{name:16s} {len(sam):5d} SAM lines  {tracks}")
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
