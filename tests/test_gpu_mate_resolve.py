"""The mate kernels alone (k_mate_spans, k_mate_resolve, k_mate_fields through gm_dev_mate_resolve) on the cases of tests/mates_cases.py:
what no mapped block gives them - several trips of 64 first-mate records against several LDS chunks of 256 second-mate records, the
winner at every edge of both, every tie-break, fp32 products that tie, NaN and zero posteriors, the limits' edges, the record seam of
k_mate_spans, TLEN at 2^31.  Every comparison is with tests/mates_model.py, for equality: the span of every record, the primary of every
read, every pair's proper bit, the five counters and all four fields of every row.  Then the case's `planted` answer is checked on the
device's own result.  The model's answers are computed once per process (mates_cases.model) and shared with
tests/test_mate_cases_cpu.py, which checks the cases themselves without a GPU."""
import numpy as np
import pytest

import gnumap_amd as g
import mates_cases as mc
from gnumap_amd import api

pytestmark = pytest.mark.gpu
CASES = mc.cases()
NONE = 0xFFFFFFFFFFFFFFFF
GM_E_ARG = -1


@pytest.fixture(scope="module")
def ix(syn_fa):
    ix = g.Index(syn_fa, device=0)
    yield ix
    ix.close()


def run(ix, case):
    """the device's answer in the model's shapes: dict(span, prim, proper, fields, stats)"""
    recs, pool, src = mc.pack(case)
    out = ix.dev_mate_resolve(recs, pool, case.n_reads, case.lo, case.hi, src)
    assert len(out["span"]) == len(case.recs) and len(out["prim"]) == case.n_reads and len(out["proper"]) == case.n_reads // 2
    assert len(out["rows"]) == (len(case.recs) if case.rows is None else len(case.rows))
    assert set(int(v) for v in out["proper"]) <= {0, 1}
    return dict(span=[int(v) for v in out["span"]], prim=[None if int(v) == NONE else int(v) for v in out["prim"]], proper=[bool(v) for v in out["proper"]],
                fields=[tuple(int(v) for v in x) for x in out["rows"]], stats=out["stats"])


def compare(case, got):
    want = mc.model(case)
    assert got["span"] == want["span"]
    assert got["prim"] == want["prim"]
    assert got["proper"] == [bool(v) for v in want["proper"]]
    assert got["stats"] == want["stats"]
    assert got["fields"] == want["fields"]
    mc.check_planted(case, got["prim"], got["proper"], got["span"], got["fields"], got["stats"])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_equals_the_model(ix, case):
    mc.self_check(case)                                 # from the model alone, before the device's answer is looked at
    compare(case, run(ix, case))


def test_one_workgroup_gives_what_the_whole_grid_gives(ix):
    case = next(c for c in CASES if c.name == "G_3000_pairs")
    whole = run(ix, case)
    g.set_option("GM_TEST_GRID_CAP", 1)
    try:
        capped = run(ix, case)                          # k_mate_resolve: one wavefront walks all 3000 pairs
    finally:
        g.set_option("GM_TEST_GRID_CAP", None)
    assert capped == whole
    compare(case, capped)


def test_refusals_launch_nothing(ix):
    case = next(c for c in CASES if c.name == "H_row_source_and_secondary_rows")
    recs, pool, src = mc.pack(case)
    with pytest.raises(g.GnumapError, match="odd number of reads") as e:
        ix.dev_mate_resolve(recs, pool, 7, 100, 500, src)
    assert e.value.code == GM_E_ARG
    with pytest.raises(g.GnumapError, match="min_insert 501 is above max_insert 500") as e:
        ix.dev_mate_resolve(recs, pool, 6, 501, 500, src)
    assert e.value.code == GM_E_ARG
    bad = recs.copy()
    bad["cigar_off"][3] = len(pool)                     # one past the pool's last byte
    with pytest.raises(g.GnumapError, match="cigar_off of record 3 lies outside the pool") as e:
        ix.dev_mate_resolve(bad, pool, 6, 100, 500, src)
    assert e.value.code == GM_E_ARG
    with pytest.raises(g.GnumapError, match="does not end in a NUL"):
        ix.dev_mate_resolve(recs, pool[:-1] + b"M", 6, 100, 500, src)
    bad = recs.copy()
    bad["read"][2] = 4                                  # behind it comes read 1 again
    with pytest.raises(g.GnumapError, match="record 3 is not in read order"):
        ix.dev_mate_resolve(bad, pool, 6, 100, 500, src)
    bad = recs.copy()
    bad["read"][5] = 6
    with pytest.raises(g.GnumapError, match="names no read of the block"):
        ix.dev_mate_resolve(bad, pool, 6, 100, 500, src)
    compare(case, run(ix, case))                        # and the entry is still good


def test_rows_that_name_nothing_come_back_empty(ix):
    case = next(c for c in CASES if c.name == "H_row_source_and_secondary_rows")
    recs, pool, _ = mc.pack(case)
    src = np.array([1, len(recs), api.ROW_UNMAPPED | 6, api.ROW_UNMAPPED | 2], np.uint64)      # a record, no record, no read, a read
    out = ix.dev_mate_resolve(recs, pool, 6, 100, 500, src)
    rows = [tuple(int(v) for v in x) for x in out["rows"]]
    assert rows == [(0x63, 0, 1200, 300), (0, -1, 0, 0), (0, -1, 0, 0), (0x65, 2, 777, 0)]
