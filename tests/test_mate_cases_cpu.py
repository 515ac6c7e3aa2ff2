"""The cases of tests/mates_cases.py and the model they are judged by, without a GPU: every case holds what it was planted for
(self_check), the NaN cases follow the rule include/gnumap_hip.h settles, and the model agrees with a second formulation of the rule
that shares no code with it: all concordant combinations of a pair sorted by (-product, a, b), the first one taken.

The cases and the model's answers are built once per process (mates_cases.cases / mates_cases.model)."""
import os
import re

import numpy as np
import pytest

import mates_cases as mc
import mates_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_holds_what_it_was_planted_for(case):
    mc.self_check(case)
    assert any(k in case.planted for k in ("pick", "single", "proper", "span", "field", "stats", "many"))


def test_the_groups_of_the_issue_are_all_there():
    names = [c.name for c in CASES]
    for ca, cb in mc.SIZES_A:
        mine = [n for n in names if n.startswith("A_%dx%d_at_" % (ca, cb))]
        at = {tuple(int(v) for v in n.split("_at_")[1].split("_")) for n in mine}
        assert {(0, 0), (ca - 1, cb - 1), (0, cb - 1), (ca - 1, 0)} <= at
        assert {a for a, _ in at} == {a for a in (0, 63, 64, 127, 128, ca - 1) if a < ca} and {b for _, b in at} == {b for b in (0, 255, 256, 511, 512, cb - 1) if b < cb}
    for letter in "BCDEFGH":
        assert any(n.startswith(letter + "_") for n in names)
    biggest = max(len(c.recs) for c in CASES if not c.planted.get("many"))
    assert biggest <= 1200                              # no pair beyond 600 x 600


def sorted_pick(case, pair):
    """the second formulation: (a, b) within the two mates' records, or None"""
    a = [r for r in case.recs if r["read"] == 2 * pair]; b = [r for r in case.recs if r["read"] == 2 * pair + 1]
    first_a = next(k for k, r in enumerate(case.recs) if r["read"] == 2 * pair); first_b = first_a + len(a)
    col = lambda rs, f, t: np.array([r[f] for r in rs], t)
    sa = np.array([mm.span(c) for c in case.cigars[first_a:first_a + len(a)]], np.int64); sb = np.array([mm.span(c) for c in case.cigars[first_b:first_b + len(b)]], np.int64)
    ca, cb, pa, pb = col(a, "contig", np.int64)[:, None], col(b, "contig", np.int64)[None, :], col(a, "chr_pos", np.int64)[:, None], col(b, "chr_pos", np.int64)[None, :]
    ta, tb = col(a, "strand", np.int64)[:, None], col(b, "strand", np.int64)[None, :]
    a_fwd = ta == 0
    pf, pr, er = np.where(a_fwd, pa, pb), np.where(a_fwd, pb, pa), np.where(a_fwd, pb + sb[None, :] - 1, pa + sa[:, None] - 1)
    ins = er - pf + 1
    ok = (ca == cb) & (ta != tb) & (pf <= pr) & (ins >= case.lo) & (ins <= case.hi)
    prod = np.multiply.outer(col(a, "post_prob", np.float32), col(b, "post_prob", np.float32))
    assert prod.dtype == np.float32
    ia, ib = np.nonzero(ok)
    if len(ia) == 0:
        return None
    order = np.lexsort((ib, ia, -prod[ia, ib].astype(np.float64)))
    return int(ia[order[0]]), int(ib[order[0]])


@pytest.mark.parametrize("case", [c for c in CASES if c.name[0] in "AB"], ids=[c.name for c in CASES if c.name[0] in "AB"])
def test_model_equals_the_sorted_formulation(case):
    m = mc.model(case)
    for pair in range(case.n_reads // 2):
        want = sorted_pick(case, pair)
        assert bool(m["proper"][pair]) == (want is not None)
        if want is not None:
            got = (m["prim"][2 * pair] - m["ranges"][2 * pair][0], m["prim"][2 * pair + 1] - m["ranges"][2 * pair + 1][0])
            assert got == want, (case.name, pair)
            assert case.planted["pick"][pair] == want


def test_the_sorted_formulation_on_the_3000_pairs():
    case = next(c for c in CASES if c.name == "G_3000_pairs")
    m = mc.model(case)
    for pair in range(0, 3000, 7):
        want = sorted_pick(case, pair)
        assert bool(m["proper"][pair]) == (want is not None)
        if want is not None:
            assert (m["prim"][2 * pair] - m["ranges"][2 * pair][0], m["prim"][2 * pair + 1] - m["ranges"][2 * pair + 1][0]) == want


# ---- the NaN rule ------------------------------------------------------------------------------------------------------------------
def test_above_is_the_headers_order():
    nan, f = np.float32("nan"), np.float32
    assert mm.above(f(0.0), nan) and mm.above(f(-1.0), nan) and mm.above(f("-inf"), nan)       # below every number
    assert not mm.above(nan, f(0.0)) and not mm.above(nan, nan)                                 # two NaNs rank alike
    assert mm.above(f(0.5), f(0.25)) and not mm.above(f(0.25), f(0.25)) and not mm.above(f(0.0), f(-0.0)) and not mm.above(f(-0.0), f(0.0))


def test_nan_cases_follow_the_rule():
    by = {c.name: c for c in CASES}
    # the divergence the issue reports: [0.1, NaN, 0.1 x 63, 0.9 at 65] is 65 by the sequential rule
    c = by["D_nan_singles"]
    m = mc.model(c)
    posts = [float(r["post_prob"]) for r in c.recs if r["read"] == 0]
    assert len(posts) == 66 and posts[0] == np.float32(0.1) and posts[1] != posts[1] and posts[65] == np.float32(0.9) and m["prim"][0] == 65
    assert not any(m["proper"])
    # stated again without the model: the primary is the first record that no other record ranks above
    for rd in range(c.n_reads):
        ps = [np.float32(r["post_prob"]) for r in c.recs if r["read"] == rd]
        nums = [p for p in ps if p == p]
        want = ps.index(max(nums)) if nums else 0
        assert m["prim"][rd] - m["ranges"][rd][0] == want == c.planted["single"][rd]
    c = by["D_all_nan_products_are_proper"]
    assert all(mc.model(c)["proper"]) and mc.model(c)["stats"]["proper"] == 4
    c = by["D_nan_product_against_a_number"]
    assert all(mc.model(c)["proper"])
    for name in ("D_nan_product_against_a_number", "D_all_nan_products_are_proper", "D_nan_singles"):
        assert any(r["post_prob"] != r["post_prob"] for r in by[name].recs)


def test_the_header_states_the_nan_rule_and_the_kernel_says_the_same():
    head = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    rule = head[head.index("paired-end reads: mate choice"):head.index("} gm_mate_row;")]
    rule = re.sub(r"\s*\n \*\s*", " ", rule)
    assert "a NaN post_prob, and a NaN product, ranks below every number" in rule
    assert "among records that are all NaN the first one is the primary" in rule
    assert "all have NaN products is still PROPER" in rule
    src = open(os.path.join(ROOT, "gnumap_amd", "csrc", "gm_mates.hip")).read()
    assert "mt_above" in src and "a NaN posterior or product ranks below every number" in re.sub(r"\s*\n//\s*", " ", src)


# ---- one fp32 multiply -------------------------------------------------------------------------------------------------------------
def test_the_fp32_search_finds_ties_and_no_reversal():
    ties = mc.fp32_ties()
    assert len(ties) >= 4
    for x1, y1, x2, y2 in ties:
        assert x1.dtype == np.float32 and x1 * y1 == x2 * y2 and float(x1) * float(y1) < float(x2) * float(y2)
        assert np.float32(float(x1) * float(y1)) == x1 * y1        # the exact product rounded once IS the fp32 product ...
    one = mc.fp32_ties_one_factor()
    assert len(one) >= 4 and all(x * y1 == x * y2 and float(x) * float(y1) < float(x) * float(y2) for x, y1, y2 in one)
    assert mc.fp32_reversals() == []                            # ... so no order can be reversed by it: the search comes back empty


def test_the_entry_refuses_on_the_host_before_it_asks_for_a_device(syn_fa):
    """gm_dev_mate_resolve checks every index a kernel would use before it uploads or launches: on a host-only index the refusals come
    back as GM_E_ARG, and only a call that passes them is told that there is no device"""
    import gnumap_amd as g
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    case = next(c for c in CASES if c.name == "H_row_source_and_secondary_rows")
    recs, pool, src = mc.pack(case)
    try:
        for kw, text in ((dict(n_reads=7), "odd number of reads"), (dict(lo=501), "min_insert 501 is above max_insert 500"),
                         (dict(off=len(pool)), "cigar_off of record 3 lies outside the pool"), (dict(off=0xFFFFFFFF), "cigar_off of record 3 lies outside the pool"),
                         (dict(pool=pool[:-1] + b"M"), "does not end in a NUL"), (dict(read=(2, 4)), "record 3 is not in read order"),
                         (dict(read=(5, 6)), "names no read of the block")):
            bad = recs.copy()
            if "off" in kw:
                bad["cigar_off"][3] = kw["off"]
            if "read" in kw:
                bad["read"][kw["read"][0]] = kw["read"][1]
            with pytest.raises(g.GnumapError, match=text) as e:
                ix.dev_mate_resolve(bad, kw.get("pool", pool), kw.get("n_reads", 6), kw.get("lo", 100), 500, src)
            assert e.value.code == -1
        with pytest.raises(g.GnumapError, match="no usable HIP device"):
            ix.dev_mate_resolve(recs, pool, 6, 100, 500, src)
    finally:
        ix.close()


def test_the_two_sided_repeat_world_is_70_x_70_of_one_product(tmp_path, oracle):
    """tests/mates_repeat2_fixture.py on the oracle's records: what tests/test_gpu_mates.py asserts again from the device's"""
    import gnumap_amd as g
    import mates_fixture as mx
    import mates_repeat2_fixture as r2
    w = r2.World(tmp_path, g.index_build)
    recs, cigars = mx.oracle_records(w, oracle)
    assert r2.self_check(w, recs, cigars) == 422
    f = mm.row_fields(recs, cigars, len(w.reads), r2.MIN_INSERT, r2.MAX_INSERT)
    assert [sum(not x[0] & 0x100 for x in f[k:k + 140]) for k in (0, 140, 280)] == [2, 2, 2]


def test_pack_keeps_every_cigar_inside_the_pool():
    for case in CASES:
        if not case.recs:
            continue
        recs, pool, src = mc.pack(case)
        assert pool.endswith(b"\0") and int(recs["cigar_off"].max()) < len(pool)
        for k in (0, len(recs) // 2, len(recs) - 1):
            off = int(recs["cigar_off"][k])
            assert pool[off:pool.index(b"\0", off)] == case.cigars[k]
        assert list(recs["read"]) == sorted(recs["read"]) and int(recs["read"].max()) < case.n_reads
        if src is not None:
            assert len(src) == len(case.rows)
