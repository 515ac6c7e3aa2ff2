"""Shared by the edge tests (tests/test_edge_cpu.py, tests/test_gpu_edge_*.py, the edge cases of tests/test_gpu_driver_golden.py): the edge
genome of tests/golden/make_edge_fixtures.py indexed in a temporary directory, its geometry, its reads by name, and the GUARDS - the facts
about the oracle's answers that keep a comparison of the device with the oracle from going vacuous (a fixture that no longer reaches the
clamped window start would still compare equal).  Every guard is computed from the oracle alone."""
import json
import os
import re
import shutil

import numpy as np

from conftest import GOLDEN, read_fastq
from edge_ref_env import REF_MALLOC_ENV          # noqa: F401  (why the reference runs with a malloc setting)
from reflib import revcomp_str

RUNS = os.path.join(GOLDEN, "ref_runs_edge")
MANIFEST = json.load(open(os.path.join(RUNS, "manifest.json")))
MER = 14
_NAME = re.compile(r"^(s|hs|e|he|dv|sh)(\d+)(?:_(\d+))?_L(\d+)_([fr])$")


def build_index(tmp_path_factory):
    """edge.fa copied into a session directory and indexed there with the library's host builder (byte-compatible with bwa_index,
    tests/test_index_build.py): returns the FASTA path"""
    import gnumap_amd as g
    d = tmp_path_factory.mktemp("edge")
    fa = str(d / "edge.fa")
    shutil.copy(os.path.join(GOLDEN, "edge.fa"), fa)
    g.index_build(fa, g.GM_BUILD_HOST)
    return fa


def reads(which="edge.fq"):
    return read_fastq(os.path.join(GOLDEN, which))


def parse(name):
    """(kind, contig or offset, k or d or None, length, strand letter) of a read name of make_edge_fixtures.py"""
    m = _NAME.match(name)
    assert m, name
    return m.group(1), int(m.group(2)), None if m.group(3) is None else int(m.group(3)), int(m.group(4)), m.group(5)


def geometry(oix):
    """([(start, end)] of every contig, l_pac) from the oracle's index"""
    ix = oix.contents
    return [(int(ix.contigs[i].offset), int(ix.contigs[i].offset) + int(ix.contigs[i].len)) for i in range(ix.n_seqs)], int(ix.l_pac)


def check_geometry(oix):
    """what the fixture is for: no inner contig offset on a 16-base word, one not on a pac byte, a partial last word and last byte"""
    ctg, l_pac = geometry(oix)
    assert len(ctg) == 3 and 9000 < l_pac < 11000
    assert all(b % 16 for b, _ in ctg[1:]) and any(b % 4 for b, _ in ctg[1:])
    assert l_pac % 16 and l_pac % 4
    return ctg, l_pac


def oracle_results(oracle, oix, op, rd):
    return [oracle.map_read(oix, op, oracle.pwm(s, q), s) for _, s, q in rd]


def kmer_occurrences(oracle, oix, seq):
    """[(strand, offset, [reference coordinates])] of every MER-mer of the read, in either orientation, that occurs in the reference"""
    out = []
    for st, t in ((0, seq), (1, revcomp_str(seq).upper())):
        for i in range(len(t) - MER + 1):
            s, e = oracle.sa_interval(oix, t[i:i + MER])
            if s or e:
                out.append((st, i, sorted(int(oracle.lib.gmo_locate(oix, k, None)) for k in range(s, e + 1))))
    return out


def guard_double_vote(oracle, oix, rd, ores):
    """(a): indices of the reads that reach -k 2 with ONE seed.  ores: the oracle's results at mer=14, jump=7, nw=0.  Exactly one 14-mer of
    such a read occurs in the reference; two of its occurrences lie nearer to the start of the reference than the 14-mer lies to the
    start of the read, so that both vote for the clamped window start 0 (its other occurrences, at the start of the second contig, vote
    for windows that begin in the first contig and fail the contig test); the result is one hit at 0 with score 2."""
    found = []
    for i, (name, s, q) in enumerate(rd):
        occ = kmer_occurrences(oracle, oix, s)
        if len(occ) != 1:
            continue
        st, off, coords = occ[0]
        if sum(c <= off for c in coords) != 2:
            continue
        o = ores[i]
        if o["status"] == 0 and len(o["hits"]) == 1 and o["hits"][0]["score"] == 2.0 and o["hits"][0]["pos"] == [(0, st)]:
            found.append(i)
    assert len(found) >= 8, [rd[i][0] for i in found]
    return found


def guard_position_zero(rd, ores):
    """(b): at default parameters at least 6 reads have an accepted hit at position 0"""
    found = [i for i, o in enumerate(ores) if o["status"] == 0 and any(p == 0 for h in o["hits"] for p, _ in h["pos"])]
    assert len(found) >= 6, [rd[i][0] for i in found]
    return found


def guard_contig_ends(oix, rd, ores):
    """(c): for every contig end (l_pac included) a read is accepted with its window ending exactly there"""
    ctg, l_pac = geometry(oix)
    for _, e in ctg:
        assert any(o["status"] == 0 and any(p + len(rd[i][1]) == e for h in o["hits"] for p, _ in h["pos"]) for i, o in enumerate(ores)), e
    assert ctg[-1][1] == l_pac


def guard_no_hit_across_a_start(oix, rd, ores):
    """(d): a read that hangs off an inner contig start by d >= 1 bases has no hit that begins in the previous contig"""
    ctg, _ = geometry(oix)
    n = 0
    for i, (name, s, q) in enumerate(rd):
        kind, c, d, L, _ = parse(name)
        if kind == "hs" and c >= 1:
            n += 1
            assert not any(ctg[c - 1][0] <= p < ctg[c][0] for h in ores[i]["hits"] for p, _ in h["pos"]), name
    assert n >= 24


def guard_windows_inside_one_contig(oix, rd, ores):
    """no hit's window lies across a contig boundary or the end of the reference, and the reads that hang off a contig are among those asked"""
    ctg, l_pac = geometry(oix)
    n = 0
    for i, (name, s, q) in enumerate(rd):
        for h in ores[i]["hits"]:
            for p, _ in h["pos"]:
                assert any(b <= p and p + len(s) <= e for b, e in ctg), (name, p)
                n += 1
    assert n > 100 and sum(parse(r[0])[0] in ("hs", "he") for r in rd) >= 72


def guard_single_votes(oracle, oix, op, rd):
    """(e): the read with the planted 14-mer at offset 17 votes once for window start 0 and once for 3 (and once for a window in the
    second contig): no position reaches -k 2, the read is unmapped at -m 14 --no_nw.  With the 14-mer at L - mer (offset 86), which the
    seed walk never reaches, nothing is looked up and the read is unmapped."""
    n = 0
    for i, (name, s, q) in enumerate(rd):
        kind, off, _, L, _ = parse(name)
        if kind != "dv" or L != 100 or off not in (17, 86):
            continue
        occ = kmer_occurrences(oracle, oix, s)
        assert len(occ) == 1 and occ[0][1] == off, name
        o = oracle.map_read(oix, op, oracle.pwm(s, q), s)
        assert o["status"] == 2 and not o["hits"], name
        if off == 17:
            begins = [max(0, c - off) for c in occ[0][2]]
            assert sorted(begins)[:2] == [0, 3] and len(set(begins)) == len(begins), (name, begins)
            assert o["ctr"]["locates"] == len(begins)
        else:
            assert o["ctr"]["locates"] == 0, name
        n += 1
    assert n == 4


def ref_text(mode, ext):
    import gzip
    return gzip.open(os.path.join(RUNS, f"{mode}.{ext}.gz"), "rb").read()
