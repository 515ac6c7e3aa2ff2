"""The mates rule without a GPU: tests/mates_model.py on hand-written records, the fixture's guards from the oracle's records, the
binding, and the driver's refusals that come before a device is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
import mates_fixture as mx
import mates_model as mm
from conftest import GOLDEN, ROOT
from gnumap_amd import api

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")


def rec(read, contig, pos, strand, post=1.0):
    return dict(read=read, contig=contig, chr_pos=pos, strand=strand, post_prob=np.float32(post))


def fields(recs, cigars=None, n=2, lo=0, hi=500, rows=None):
    return mm.row_fields(recs, cigars or [b"100M"] * len(recs), n, lo, hi, rows)


# ---- the span parser and the QNAME rule ------------------------------------------------------------------------------------------
def test_span():
    assert mm.span(b"*") == 1 and mm.span(b"100M") == 100
    assert mm.span(b"52M2D46M2I") == 100 and mm.span(b"51M2I46M2D1M") == 100 and mm.span(b"50M2I48M") == 98
    assert mm.span(b"5I") == 1                                    # nothing of the reference: the .bai's rule


def test_qname_rule():
    assert mm.qnames(b"x/1", b"x/2") == (b"x", b"x")
    assert mm.qnames(b"x 1:N:0", b"x 2:N:0") == (b"x", b"x")
    assert mm.qnames(b"x\t1", b"x") == (b"x", b"x")
    assert mm.qnames(b"x", b"x") == (b"x", b"x")
    assert mm.qnames(b"x/1 1:N", b"x/2 2:N") == (b"x", b"x")      # the cut at the blank comes first
    assert mm.qnames(b"x/1", b"x/1") == (b"x/1", b"x/1")          # only /1 with /2
    assert mm.qnames(b"x/2", b"x/1") == (b"x/2", b"x/1")
    assert mm.qnames(b"x/1", b"y") == (b"x/1", b"y")
    assert mm.first_mismatch([b"a/1", b"a/2", b"b", b"c", b"d", b"e"]) == 1
    assert mm.first_mismatch([b"a/1", b"a/2", b"b x", b"b y"]) is None
    long = b"n" * 1023
    assert mm.first_mismatch([long + b"A", long + b"B"]) is None and mm.first_mismatch([long + b"A", long + b"B"], cut=2000) == 0


# ---- one record list per flag situation ------------------------------------------------------------------------------------------
CASES = {
    # name: (recs, cigars, kwargs, wanted fields in record order)
    "proper_fr": ([rec(0, 0, 101, 0), rec(1, 0, 301, 1)], None, {}, [(0x1 | 0x40 | 0x20 | 0x2, 0, 301, 300), (0x1 | 0x80 | 0x10 | 0x2, 0, 101, -300)]),
    "proper_rf_order": ([rec(0, 0, 301, 1), rec(1, 0, 101, 0)], None, {}, [(0x1 | 0x40 | 0x10 | 0x2, 0, 101, -300), (0x1 | 0x80 | 0x20 | 0x2, 0, 301, 300)]),
    "insert_at_max": ([rec(0, 0, 1, 0), rec(1, 0, 401, 1)], None, {}, [(99, 0, 401, 500), (147, 0, 1, -500)]),
    "insert_over_max": ([rec(0, 0, 1, 0), rec(1, 0, 402, 1)], None, {}, [(97, 0, 402, 501), (145, 0, 1, -501)]),
    "insert_at_min": ([rec(0, 0, 1, 0), rec(1, 0, 21, 1)], None, dict(lo=120), [(99, 0, 21, 120), (147, 0, 1, -120)]),
    "insert_under_min": ([rec(0, 0, 1, 0), rec(1, 0, 20, 1)], None, dict(lo=120), [(97, 0, 20, 119), (145, 0, 1, -119)]),
    "both_plus": ([rec(0, 0, 1, 0), rec(1, 0, 201, 0)], None, {}, [(0x1 | 0x40, 0, 201, 300), (0x1 | 0x80, 0, 1, -300)]),
    "outward": ([rec(0, 0, 201, 0), rec(1, 0, 1, 1)], None, {}, [(97, 0, 1, -300), (145, 0, 201, 300)]),
    "two_contigs": ([rec(0, 0, 1, 0), rec(1, 1, 201, 1)], None, {}, [(97, 1, 201, 0), (145, 0, 1, 0)]),
    "first_unmapped": ([rec(1, 0, 201, 1)], None, {}, [(0x1 | 0x80 | 0x10 | 0x8, -1, 0, 0)]),
    "second_unmapped": ([rec(0, 0, 201, 0)], None, {}, [(0x1 | 0x40 | 0x8, -1, 0, 0)]),
    "same_pos": ([rec(0, 0, 50, 1), rec(1, 0, 50, 0)], [b"100M", b"125M"], {}, [(0x1 | 0x40 | 0x10 | 0x2, 0, 50, 125), (0x1 | 0x80 | 0x20 | 0x2, 0, 50, -125)]),
    "span_from_cigar": ([rec(0, 0, 1, 0), rec(1, 0, 201, 1)], [b"50M2I48M", b"53M2D44M2I1M"], {}, [(99, 0, 201, 300), (147, 0, 1, -300)]),
    "star_spans_one": ([rec(0, 0, 1, 0), rec(1, 0, 201, 1)], [b"*", b"*"], {}, [(99, 0, 201, 201), (147, 0, 1, -201)]),
    # three places of the first mate with one posterior: the concordant one is the third, and only it is primary
    "mate_decides": ([rec(0, 0, 1001, 0, .3), rec(0, 0, 5001, 0, .3), rec(0, 0, 9001, 0, .3), rec(1, 0, 9201, 1)], None, {},
                     [(0x1 | 0x40 | 0x20 | 0x100, 0, 9201, 0), (0x1 | 0x40 | 0x20 | 0x100, 0, 9201, 0), (99, 0, 9201, 300), (147, 0, 9001, -300)]),
    # no concordant place: the largest posterior, the first on ties
    "best_single": ([rec(0, 0, 1001, 0, .2), rec(0, 0, 5001, 0, .4), rec(0, 0, 9001, 0, .4), rec(1, 1, 1, 1)], None, {},
                    [(0x1 | 0x40 | 0x20 | 0x100, 1, 1, 0), (0x1 | 0x40 | 0x20, 1, 1, 0), (0x1 | 0x40 | 0x20 | 0x100, 1, 1, 0), (0x1 | 0x80 | 0x10, 0, 5001, 0)]),
    # two concordant combinations: the larger product wins; on equal products the smaller first index, then the smaller second
    "largest_product": ([rec(0, 0, 1001, 0, .5), rec(0, 0, 5001, 0, .5), rec(1, 0, 1201, 1, .2), rec(1, 0, 5201, 1, .6)], None, {},
                        [(0x1 | 0x40 | 0x20 | 0x100, 0, 5201, 0), (99, 0, 5201, 300), (0x1 | 0x80 | 0x10 | 0x100, 0, 5001, 0), (147, 0, 5001, -300)]),
    "tie_takes_the_first": ([rec(0, 0, 1001, 0, .5), rec(0, 0, 5001, 0, .5), rec(1, 0, 1201, 1, .5), rec(1, 0, 5201, 1, .5)], None, {},
                            [(99, 0, 1201, 300), (0x1 | 0x40 | 0x20 | 0x100, 0, 1201, 0), (147, 0, 1001, -300), (0x1 | 0x80 | 0x10 | 0x100, 0, 1001, 0)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_on_hand_written_records(name):
    recs, cigars, kw, want = CASES[name]
    got = fields(recs, cigars, **kw)
    assert got == want
    # symmetry: A's PNEXT is B's POS, opposite TLENs, 0x20 of A is 0x10 of B's primary, 0x2 on both primaries or on neither
    prim, proper = mm.resolve(recs, cigars or [b"100M"] * len(recs), 2, kw.get("lo", 0), kw.get("hi", 500))
    a, b = prim
    if a is not None and b is not None:
        fa, fb = got[a], got[b]
        assert fa[2] == recs[b]["chr_pos"] and fb[2] == recs[a]["chr_pos"] and fa[3] == -fb[3]
        assert bool(fa[0] & 0x20) == bool(fb[0] & 0x10) and bool(fb[0] & 0x20) == bool(fa[0] & 0x10)
        assert bool(fa[0] & 0x2) == bool(fb[0] & 0x2) == proper[0]
    assert sum(bool(f[0] & 0x2) for f in got) in (0, 2)
    for rd in (0, 1):
        mine = [f for f, r in zip(got, recs) if r["read"] == rd]
        assert sum(not f[0] & 0x100 for f in mine) == (1 if mine else 0)


def test_rows_of_reads_without_a_record():
    recs = [rec(1, 1, 201, 1)]
    rows = [("u", 0), ("r", 0), ("u", 2), ("u", 3)]
    got = fields(recs, n=4, rows=rows)
    assert got == [(0x4 | 0x1 | 0x40 | 0x20, 1, 201, 0), (0x1 | 0x80 | 0x10 | 0x8, -1, 0, 0), (0x4 | 0x1 | 0x40 | 0x8, -1, 0, 0), (0x4 | 0x1 | 0x80 | 0x8, -1, 0, 0)]
    assert mm.stats(recs, [b"100M"], 4, 0, 500) == dict(pairs=2, both_mapped=0, proper=0, one_mapped=1, none_mapped=1)
    row = b"r0 extra\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\tYU:i:2\n"
    assert mm.text_row(row, got[0], b"r0", ["mA", "mB"]) == b"r0\t101\t*\t0\t0\t*\tmB\t201\t0\tACGT\tIIII\tYU:i:2\n"
    assert mm.text_row(row, got[2], b"r0", ["mA", "mB"]) == b"r0\t77\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\tYU:i:2\n"


def test_tlen_beyond_int32_is_zero():
    recs = [rec(0, 0, 1, 0), rec(1, 0, 2 ** 31, 1)]
    got = fields(recs, hi=2 ** 32 - 1)
    assert got[0][3] == 0 and got[1][3] == 0 and got[0][0] & 0x2
    recs = [rec(0, 0, 1, 0), rec(1, 0, 2 ** 31 - 100, 1)]
    assert fields(recs, hi=2 ** 32 - 1)[0][3] == 2 ** 31 - 1


def test_text_row_and_bam_record():
    row = b"q/1\t16\tmB\t301\t30\t100M\t*\t0\t0\tACGT\tIIII\tXA:f:1\tXP:f:1\tX0:i:1\n"
    assert mm.text_row(row, (147, 1, 101, -300), b"q", ["mA", "mB"]) == b"q\t147\tmB\t301\t30\t100M\t=\t101\t-300\tACGT\tIIII\tXA:f:1\tXP:f:1\tX0:i:1\n"
    assert mm.text_row(row, (145, 0, 7, 0), b"q", ["mA", "mB"]).split(b"\t")[6:9] == [b"mA", b"7", b"0"]
    import bam_model as bm
    r = bytes(bm.sam_row_to_record(row, [("mA", 0), ("mB", 40000)]))
    out = mm.bam_record(r, (147, 1, 101, -300), b"q")
    assert mm.bam_fields(out) == (147, 1, 100, -300, b"q") and len(out) == len(r) - 2
    assert out[36 + 2:] == r[36 + 4:] and out[4:12] == r[4:12]
    assert mm.bam_fields(mm.bam_record(r, (73, -1, 0, 0), b"q"))[1:3] == (-1, -1)


# ---- the fixture's guards, from the oracle's records -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    w = mx.World(tmp_path_factory.mktemp("mates_cpu"), g.index_build)
    recs, cigars = mx.oracle_records(w, oracle)
    return w, recs, cigars


def test_fixture_realises_every_situation(world):
    w, recs, cigars = world
    seen = mx.self_check(w, recs, cigars)                         # asserts the table, the repeat pair's index >= 64 and != the mate-less choice
    assert len(w.pairs) == 110 and len(recs) > 256                # the row kernels get more than one workgroup
    st = mm.stats(recs, cigars, len(w.reads), mx.MIN_INSERT, mx.MAX_INSERT)
    assert st == dict(pairs=110, both_mapped=105, proper=99, one_mapped=4, none_mapped=1)
    assert mm.first_mismatch([r[0] for r in w.reads]) is None
    styles = set((p.name1.endswith(b"/1"), b" " in p.name1) for p in w.pairs)
    assert styles == {(True, False), (False, True), (False, False)}
    inserts = sorted(f[0][3] for f in seen["ordinary"] if f[0] and f[0][3] > 0) + sorted(f[1][3] for f in seen["ordinary"] if f[1] and f[1][3] > 0)
    assert min(inserts) == 150 and max(inserts) == 450 and len(inserts) == mx.N_ORDINARY
    # every case: symmetry of the model's fields on the fixture
    f = mm.row_fields(recs, cigars, len(w.reads), mx.MIN_INSERT, mx.MAX_INSERT)
    prim, proper = mm.resolve(recs, cigars, len(w.reads), mx.MIN_INSERT, mx.MAX_INSERT)
    for i in range(len(w.pairs)):
        a, b = prim[2 * i], prim[2 * i + 1]
        if a is None or b is None:
            continue
        assert f[a][2] == recs[b]["chr_pos"] and f[b][2] == recs[a]["chr_pos"] and f[a][3] == -f[b][3]
        assert bool(f[a][0] & 0x20) == bool(f[b][0] & 0x10) and bool(f[a][0] & 0x2) == bool(f[b][0] & 0x2) == proper[i]


# ---- the binding -----------------------------------------------------------------------------------------------------------------
def test_binding_and_header():
    L = g.load_library()
    header = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    for name in ("gm_batch_set_mates", "gm_batch_mate_rows", "gm_batch_mate_stats"):
        assert hasattr(L, name) and name in api.EXPORTS and f"int {name}(" in header, name
    assert api.MATE_ROW_DTYPE.itemsize == 16 and api.MATE_ROW_DTYPE.names == ("flag", "rnext", "pnext", "tlen")
    assert "GM_K_MATES, GM_K_COUNT" in header and api.GM_K_COUNT == 9
    assert L.gm_kernel_name(api.GM_K_COUNT - 1).decode() == "k_mate_*"
    assert L.gm_batch_set_mates(None, 1, 0, 500) == -1 and L.gm_batch_mate_stats(None, None) == -1
    n = api.u64()
    assert L.gm_batch_mate_rows(None, None, 0, C.byref(n)) == -1
    for m in ("set_mates", "mate_rows", "mate_stats"):
        assert callable(getattr(api.Batch, m))


# ---- the driver's refusals before a device is opened -------------------------------------------------------------------------------
def refuse(args, tmp_path):
    fa, fq = os.path.join(GOLDEN, "syn.fa"), os.path.join(GOLDEN, "syn.fq")
    r = subprocess.run([EXE, "-g", fa, "-o", str(tmp_path / "o")] + args + [fq], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr[-500:])
    assert not os.path.exists(str(tmp_path / "o.sam")) and "no usable HIP device" not in r.stderr
    return r.stderr


def test_driver_refusals(tmp_path):
    fq = os.path.join(GOLDEN, "syn.fq")
    other = tmp_path / "reads.fa"
    other.write_bytes(b">r\nACGTACGTAC\n")
    assert "--mates" in refuse([f"--mates={fq}", "--interleaved"], tmp_path) and "--interleaved" in refuse([f"--mates={fq}", "--interleaved"], tmp_path)
    assert "--min_insert" in refuse(["--min_insert=10"], tmp_path)
    assert "--max_insert" in refuse(["--max_insert=10"], tmp_path)
    err = refuse([f"--mates={fq}", "--min_insert=9", "--max_insert=3"], tmp_path)
    assert "--min_insert=9" in err and "--max_insert=3" in err
    assert "--sam_text=host" in refuse([f"--mates={fq}", "--sam_text=host"], tmp_path)
    assert "--read_text=device" in refuse(["--interleaved", "--read_text=device"], tmp_path)
    assert "--batch=7" in refuse(["--interleaved", "--batch=7"], tmp_path)
    missing = str(tmp_path / "nope.fq")
    err = refuse([f"--mates={missing}"], tmp_path)
    assert "--mates" in err and missing in err
    err = refuse([f"--mates={other}"], tmp_path)
    assert "--mates" in err and str(other) in err and "FASTQ" in err
