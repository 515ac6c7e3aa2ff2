#!/usr/bin/env python3
"""BUILD CONTAINER ONLY (needs the reference tree).  --snp at the edges: a genome that holds one segment on BOTH strands, reads cut from it,
and what the UNMODIFIED reference program (built with its own vendored GSL by make_snp_call_fixtures.build, outside the repository)
writes with --snp for them and for the edge reads of make_edge_fixtures.py.

    python tests/golden/make_snp_edge_fixtures.py        (GSL_PREFIX=<dir> reuses a built GSL, GNUMAP_REF_GSL_BIN=<program> a built program)

Inputs written (our own generator, seed 5):

    both.fa   three contigs of 1500, 1203 and 1101 bp (no multiple of 16; inner starts 1500 and 2703, l_pac = 3804).  A 150-base segment S
              stands at [300, 450) of the first contig, its reverse complement at [500, 650) of the second, S at the very start of the
              third and its reverse complement at the very end of the third, where it ends at l_pac.  Every read cut from S therefore has
              four places, two of them on the other strand than the kept sequence's first strand: the `same == false` branch of
              k_snp_deposit, the mirrored row with a/t and c/g swapped (reverse_comp_cpy_phmm, inc/SequenceOperations.h:164-181).
    both.fq   reads cut from S: lengths 150, 100, 50, 36, 24 x offsets 0, 7, 150 - L x {as cut, an N in the middle, one substitution}
              x {as cut, reverse-complemented}, qualities Phred 5 .. 40 at random: 90 reads.

Before anything is written the oracle has to find what the fixture is for (counts asserted below).

Outputs committed, the reference program's `-a 0.9 -c 1 --snp` runs with the malloc setting of tests/edge_ref_env.py:

    ref_runs_snp_edge/both|edge|mixed.gmp.gz, .sam.gz    the nine-column .gmp and the SAM file (@PG dropped)
    ref_runs_snp_edge/manifest.json                      argv, genome, fastq, rows per run

Everything committed is DATA (our inputs, the reference's outputs on them)."""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_snp_call_fixtures import build          # noqa: E402
from edge_ref_env import REF_MALLOC_ENV           # noqa: E402

OUT = os.path.join(HERE, "ref_runs_snp_edge")
SEED = 5
CONTIGS = [("bothA", 1500), ("bothB", 1203), ("bothC", 1101)]
S_AT = (300, 500)                                 # S in the first contig, its reverse complement in the second
LENS = (150, 100, 50, 36, 24)
RUNS = {"both": ("both.fa", "both.fq"), "edge": ("edge.fa", "edge.fq"), "mixed": ("edge.fa", "edge_mixed.fq")}
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def make():
    """(contig sequences, reads [(name, sequence, qualities)])"""
    rng = np.random.default_rng(SEED)
    rb = lambda n: bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))
    S = rb(150); R = revcomp(S)
    A = bytearray(rb(CONTIGS[0][1])); A[S_AT[0]:S_AT[0] + 150] = S
    B = bytearray(rb(CONTIGS[1][1])); B[S_AT[1]:S_AT[1] + 150] = R
    Cc = bytearray(rb(CONTIGS[2][1])); Cc[0:150] = S; Cc[CONTIGS[2][1] - 150:] = R
    reads = []
    for L in LENS:
        for off in (0, 7, 150 - L):
            s = S[off:off + L]
            for var, tag in enumerate(("cut", "n", "sub")):
                t = bytearray(s)
                if var == 1:
                    t[L // 2] = ord("N")
                if var == 2:
                    t[L // 3] = b"ACGT"[(b"ACGT".index(t[L // 3]) + 1) % 4]
                q = bytes((33 + rng.integers(5, 41, L)).astype(np.uint8))
                reads.append((f"b{off}_{tag}_L{L}_f", bytes(t), q))
                reads.append((f"b{off}_{tag}_L{L}_r", revcomp(t), q[::-1]))
    return [bytes(A), bytes(B), bytes(Cc)], reads


def check_with_oracle(work):
    """the counts the fixture is for, from the oracle alone"""
    import edge_fixture as ef
    import gnumap_amd as g
    from conftest import read_fastq
    from reflib import OracleLib
    fa = os.path.join(work, "both.fa")
    g.index_build(fa, g.GM_BUILD_HOST)
    o = OracleLib(); oix = o.index_load(fa)
    rd = read_fastq(os.path.join(work, "both.fq"))
    info = ef.snp_info(o, oix, rd)
    mapped = len({k[0] for k in info["kept"]})
    other = ef.guard_snp_other_strand(info); n_seq = ef.guard_snp_n_sequences(info)
    print(f"both.fq: {len(rd)} reads, {mapped} mapped, {len(info['kept'])} kept sequences, {len(info['places'])} places, {other} on the other strand, "
          f"{n_seq} kept sequences with an N")
    assert len(rd) == 90 and mapped == 90 and len(info["places"]) == 348 and other == 168 and n_seq == 30
    ctg, l_pac = ef.geometry(oix)
    assert l_pac == 3804 and all(b % 16 for b, _ in ctg[1:]) and l_pac % 16
    ef.guard_snp_deposits_touch(info, ef.snp_edge_positions(oix, "both"))


def gz_write(path, data):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)


def main():
    work = tempfile.mkdtemp()
    seqs, reads = make()
    with open(os.path.join(work, "both.fa"), "wb") as f:
        for (name, n), s in zip(CONTIGS, seqs):
            assert len(s) == n and n % 16
            f.write(b">" + name.encode() + b"\n")
            for i in range(0, n, 70):
                f.write(s[i:i + 70] + b"\n")
    with open(os.path.join(work, "both.fq"), "wb") as f:
        for name, s, q in reads:
            f.write(b"@" + name.encode() + b"\n" + s + b"\n+\n" + q + b"\n")
    check_with_oracle(work)
    exe = os.environ.get("GNUMAP_REF_GSL_BIN") or build(work)[0]
    for f in ("both.fa", "both.fq"):
        shutil.copy(os.path.join(work, f), HERE)
    os.makedirs(OUT, exist_ok=True)
    manifest = {}
    for name, (fa, fq) in RUNS.items():
        d = tempfile.mkdtemp(dir=work)                              # the reference builds its own index of the genome
        for f in (fa, fq):
            shutil.copy(os.path.join(HERE, f), d)
        argv = ["--snp"]
        r = subprocess.run([exe, "-g", fa, "-o", name, "-a", "0.9", "-c", "1"] + argv + [fq], cwd=d, capture_output=True, text=True,
                           env=dict(os.environ, **REF_MALLOC_ENV))
        assert r.returncode == 0, (name, r.stderr[-2000:])
        sam = b"".join(l for l in open(os.path.join(d, name + ".sam"), "rb") if not l.startswith(b"@PG"))
        gmp = open(os.path.join(d, name + ".gmp"), "rb").read()
        assert not os.path.exists(os.path.join(d, name + ".sgr"))
        rows = gmp.splitlines()
        assert rows and all(len(l.split(b"\t")) == 9 for l in rows)
        gz_write(os.path.join(OUT, name + ".sam.gz"), sam); gz_write(os.path.join(OUT, name + ".gmp.gz"), gmp)
        manifest[name] = dict(argv=argv, genome=fa, fastq=fq, sam_lines=sam.count(b"\n"), gmp_rows=len(rows))
        print(f"{name:6s} {manifest[name]['sam_lines']:5d} SAM lines, {len(rows):6d} .gmp rows")
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
