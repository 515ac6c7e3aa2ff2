"""The unique map of gm_output.hip (k_group_multi / k_group_write_multi, and the path for more than GM_GROUP_BIG hits, k_group_big /
k_group_write_big, with its three hand-backs) on repeat-rich reads (tests/golden/make_repeat_fixtures.py), against the ORACLE read by
read: status, self / top score bits, denominator, matches in key order, score bits, first strand, the exact ordered position list
(_compare of test_gpu_parity.py), and first_pos equal to the oracle's first hit.

What these reads ask that syn.fq and edge.fq do not: 2, 63, 64, 65, 66, 129, 180, 300 and 3001 accepted hits per read - every lane
stride of the all-pairs kernel, both sides of the `k > big_min` switch, sorts of more than one 64-element pass, the set's limit of 3000
keys and -T met exactly; keys that tie on their first word and differ in word 1, 2, 3, in the partial last word or in word 19 of 20;
keys shared between a plus-strand hit and a minus-strand hit at a lower position; a window that is its own reverse complement; copies
that reach -k votes at a later seed step than their neighbours.  The host sums exp(score) in processing order in fp64, so `denominator
==` is a test of that order (guard_order_sensitive of tests/repeat_fixture.py: another order gives other bits on more than 100 reads).

One process: the switches go through gm_set_option (read on every call) and are cleared in `finally`.  The guards are asserted on the
oracle's side before the first comparison that relies on them."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import gnumap_amd as g
import repeat_fixture as rf
from conftest import ROOT
from test_gpu_driver_golden import compare_tracks
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")

CONFIGS = {
    "default": {},
    "no_nw": dict(nw=0),
    "u": dict(unique_only=1),
    "u_no_nw": dict(unique_only=1, nw=0),
    "up": dict(neg_strand=0),
    "down": dict(pos_strand=0),
    "T_keys": dict(max_matches=rf.T_KEYS),                  # -T met exactly by the 180 keys of t_L150_f / _r ...
    "T_keys_less1": dict(max_matches=rf.T_KEYS - 1),        # ... and missed by one
    "T3000": dict(max_matches=3000),                        # the set-limit reads: 3001 keys
    "T3001": dict(max_matches=3001),
    "T100000": dict(max_matches=100000),
    "up_T3000": dict(neg_strand=0, max_matches=3000),       # 3000 keys: -T and the set's limit met exactly
}
FORMS = {
    "default": {},                                          # GM_GROUP_BIG = 64: 65 hits and more take the big path
    "big": dict(GM_GROUP_BIG_MIN="1"),                      # everything with 2 or more hits through the big path
    "all_pairs": dict(GM_GROUP_BIG_MIN="1000000"),          # everything through the all-pairs kernels, the 3001-key reads included
}
TRACE = re.compile(r"grouping done: (\d+) accepted hits -> (\d+) matches; reads: (\d+) all-pairs list \(incl\. handed back\), (\d+) big path; "
                   r"handed back: (\d+) \(-u --no_nw\), (\d+) \(> set limit\), (\d+) \(hash collision\)")


@pytest.fixture(scope="module")
def rep_fa(tmp_path_factory):
    return rf.build_index(tmp_path_factory)


@pytest.fixture(scope="module")
def ix(rep_fa):
    i = g.Index(rep_fa, flags=g.GM_INDEX_FULL_SA)
    yield i
    i.close()


@pytest.fixture(scope="module")
def oix(oracle, rep_fa):
    o = oracle.index_load(rep_fa)
    rf.check_geometry(o)
    return o


_BLOCKS, _ORACLE = {}, {}


def block_reads(name):
    if name not in _BLOCKS:
        rd = rf.all_reads()
        if name == "reversed_odd":                          # the same reads the other way round, without the first: an odd count
            rd = rd[:0:-1]
            assert len(rd) % 2 == 1
        _BLOCKS[name] = rd
    return _BLOCKS[name]


def oracle_for(oracle, oix, cfg):
    """{read name: the oracle's result} in a configuration, computed once and never changed; the guards are asserted with the first"""
    if not _ORACLE:
        rd = rf.reads()
        print("guards:", rf.guards(oracle, oix, rd, rf.oracle_results(oracle, oix, oracle.params(), rd)))
        assert rf.guard_set_limit(oracle, oix) == (3000, 3001)
        rf.guard_T_pair(oracle, oix, rd)
    if cfg not in _ORACLE:
        rd = block_reads("all")
        _ORACLE[cfg] = dict(zip((r[0] for r in rd), rf.oracle_results(oracle, oix, oracle.params(**CONFIGS[cfg]), rd)))
    return _ORACLE[cfg]


def run(ix, rd, kw, switches):
    p = g.Params(**kw)
    B, Q, Ln = g.pack_reads([r[1] for r in rd], [r[2] for r in rd])
    for k, v in switches.items():
        g.set_option(k, v)
    try:
        batch = g.Batch(ix, len(Ln), B.shape[1])
        t0 = time.perf_counter()
        res = batch.map(p, B, Q, Ln)
        dt = time.perf_counter() - t0
    finally:
        for k in switches:
            g.set_option(k, None)
    return dict(res=res, batch=batch, p=p, seconds=dt)


def compare(res, ores, rd):
    _compare(res, ores, rd)
    mb = res["match_begin"]
    n = 0
    for i, o in enumerate(ores):
        for m, h in zip(res["matches"][int(mb[i]):int(mb[i + 1])], o["hits"]):
            assert (int(m["first_pos"]), int(m["first_strand"])) == (h["first_pos"], h["first_strand"]), rd[i][0]      # the leader: the first hit in processing order
            n += 1
    return n


def trace_counts(err):
    """(accepted hits, matches, reads on the all-pairs list, reads on the big path, handed back: -u --no_nw, > set limit, hash collision)
    of ONE grouping: Batch.map repeats gm_map_batch with larger buffers after GM_E_CAPACITY, the repeated call only copies and traces the
    same counts again"""
    m = TRACE.findall(err)
    assert m and len(set(m)) == 1, err[-1500:]
    return tuple(int(x) for x in m[0])


@pytest.mark.parametrize("block", ["all", "reversed_odd"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_repeat_reads_match_oracle(cfg, form, block, ix, oracle, oix, capfd):
    """every read of rep.fq and rep_limit.fq in one block, then in reversed order in a block with an odd count: the order in which
    atomicAdd lists the reads for the two kernels must not matter"""
    by_name = oracle_for(oracle, oix, cfg)
    rd = block_reads(block)
    ores = [by_name[r[0]] for r in rd]
    o = run(ix, rd, CONFIGS[cfg], dict(FORMS[form], GM_TRACE="1"))
    try:
        hits, matches, n_multi, n_big, back_u, back_limit, back_hash = trace_counts(capfd.readouterr().err)
        print(f"{cfg}/{form}/{block}: gm_map_batch {o['seconds'] * 1e3:.0f} ms; {hits} hits -> {matches} matches; lists: {n_multi} all-pairs, {n_big} big; "
              f"handed back: {back_u} (-u --no_nw), {back_limit} (> set limit), {back_hash} (hash collision)")
        n = compare(o["res"], ores, rd)
        assert n == matches == sum(len(x["hits"]) for x in ores)
        many = sum(x["status"] == 1 for x in ores)
        assert n > 500 or CONFIGS[cfg].get("unique_only") and many > 150           # (-u: a second place of a key ends the read)
        # (a read is listed by its accepted hits before grouping: at least the places it ends with, unknown where -T or -u ended it)
        ok2 = [rf.n_places(x) for x in ores if x["status"] == 0 and rf.n_places(x) >= 2]
        if form == "big":
            assert n_big >= len(ok2) > 15 and n_multi == back_u + back_limit + back_hash
        if form == "all_pairs":
            assert n_big == 0 and n_multi >= len(ok2)
        if form == "default":
            assert n_big >= sum(k > 64 for k in ok2) and n_big + n_multi - (back_u + back_limit + back_hash) >= len(ok2)
        kw = CONFIGS[cfg]
        if kw.get("unique_only") and not kw.get("nw", 1):
            assert back_u == n_big and (form != "big" or back_u >= len(ok2))             # the per-strand drop rule is the all-pairs kernel's
        else:
            assert back_u == 0
        # the two 3001-key reads pass the set's limit where neither -T nor -u stops them first, and nowhere else
        over = form != "all_pairs" and (cfg in ("T3001", "T100000", "no_nw"))
        assert back_limit == (2 if over else 0), (cfg, form, back_limit)
    finally:
        o["batch"].destroy()


def _pair(prefix):
    by = {r[0]: r for r in rf.all_reads()}
    return [by[prefix + "_f"], by[prefix + "_r"]]


def test_the_switch_to_the_big_path_lies_between_64_and_65_hits(ix, oracle, oix, capfd):
    """GM_GROUP_BIG = 64: a read with exactly 64 accepted hits is on the all-pairs list, one with 65 on the big path (two reads a batch)"""
    by_name = oracle_for(oracle, oix, "default")
    for prefix, want in (("s64_L150", (2, 0)), ("s65_L150", (0, 2)), ("s64_L31", (2, 0)), ("s65_L31", (0, 2))):
        rd = _pair(prefix)
        ores = [by_name[r[0]] for r in rd]
        assert [rf.n_places(x) for x in ores] == [int(prefix[1:3])] * 2
        o = run(ix, rd, {}, dict(GM_TRACE="1"))
        try:
            t = trace_counts(capfd.readouterr().err)
            assert t[2:4] == want and t[4:] == (0, 0, 0), (prefix, t)
            compare(o["res"], ores, rd)
        finally:
            o["batch"].destroy()


@pytest.mark.parametrize("cfg,form,limit,u", [("no_nw", "default", 2, 0), ("T100000", "default", 2, 0), ("T3001", "big", 2, 0), ("up_T3000", "default", 0, 0),
                                              ("up_T3000", "big", 0, 0), ("T3000", "default", 0, 0), ("u_no_nw", "big", 0, 2)])
def test_hand_backs_of_the_set_limit_reads(cfg, form, limit, u, ix, oracle, oix, capfd):
    """the two reads of rep_limit.fq alone: 3001 keys pass the set's limit of 3000 and go back to the all-pairs kernel unless -T stops
    the read first; the 3000 keys of the forward strand stay on the big path; -u --no_nw is the all-pairs kernel's"""
    by_name = oracle_for(oracle, oix, cfg)
    rd = _pair("x_L100")
    ores = [by_name[r[0]] for r in rd]
    o = run(ix, rd, CONFIGS[cfg], dict(FORMS[form], GM_TRACE="1"))
    try:
        t = trace_counts(capfd.readouterr().err)
        print(f"{cfg}/{form}: gm_map_batch {o['seconds'] * 1e3:.0f} ms, trace {t}")
        assert t[5] == limit and t[4] == u, t
        if cfg == "up_T3000":
            assert [len(x["hits"]) for x in ores] == [3000, 1] and t[3] == 1          # one read on the big path, finished there
        compare(o["res"], ores, rd)
    finally:
        o["batch"].destroy()


# ------------------------------------------------------------------ the output half: SAM records and the coverage deposit
def _track_close(got, want):
    """the tolerance of compare_tracks (tests/test_gpu_driver_golden.py) on whole arrays: fp32 atomic adds in another order"""
    tol = 1e-4 * np.maximum(1.0, np.abs(want)) + 2e-5
    bad = np.flatnonzero(np.abs(got - want) > tol)
    assert len(bad) == 0, [(int(k), float(got[k]), float(want[k])) for k in bad[:8]]


@pytest.mark.parametrize("bin_size", [1, 8])
@pytest.mark.parametrize("cfg", ["default", "T3001"])
def test_output_records_and_coverage_of_repeat_reads(cfg, bin_size, ix, oracle, oix):
    """batch.output against gmo_read_output: one record per place of the printed sequence, sim_matches, CIGAR, MAPQ, posterior bits; the
    coverage deposit of every place of every key within the tolerance of compare_tracks"""
    kw = dict(CONFIGS[cfg], bin_size=bin_size)
    rd = block_reads("all")
    p = g.Params(**kw); op = oracle.params(**kw)
    B, Q, Ln = g.pack_reads([r[1] for r in rd], [r[2] for r in rd])
    ix.coverage_reset(bin_size)
    batch = g.Batch(ix, len(rd), B.shape[1])
    try:
        res = batch.map(p, B, Q, Ln)
        recs, cigars = batch.output(p, res)
        cov = ix.coverage_download()
    finally:
        ix.coverage_reset(8)
        batch.destroy()
    want_cov = np.zeros(len(cov), np.float64)
    want_recs = []
    for i, (name, seq, qual) in enumerate(rd):
        st, orecs, deps = oracle.read_output(oix, op, oracle.pwm(seq, qual), seq)
        want_recs += [(i, r["contig"], r["chr_pos"], r["strand"], r["mapq"], r["cigar"], r["sim_matches"], np.float32(r["post_prob"]).view(np.uint32))
                      for r in orecs]
        for pos, span, w, codes in deps:
            np.add.at(want_cov, (pos + np.arange(span)) // bin_size, float(np.float32(w)))
    got_recs = [(int(r["read"]), int(r["contig"]), int(r["chr_pos"]), int(r["strand"]), int(r["mapq"]), c, int(r["sim_matches"]),
                 np.float32(r["post_prob"]).view(np.uint32)) for r, c in zip(recs, cigars)]
    assert got_recs == want_recs
    assert len(want_recs) > 14000 and max(r[6] for r in want_recs) == 300
    _track_close(cov.astype(np.float64), want_cov)
    assert want_cov.sum() > 10000 and (want_cov > 0).sum() > 100000 // bin_size          # (the reads' bases; the copies of the families read here)


# ------------------------------------------------------------------ the driver against the reference program
VARIANTS = {"full_sa": [], "sampled_sa": ["--locate=sampled"], "batch64": ["--batch=64"], "sam_text_device": ["--sam_text=device"]}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mode", sorted(rf.MANIFEST))
def test_cli_on_the_repeat_genome_equals_reference_program(mode, variant, rep_fa, tmp_path):
    """the reference's argv on rep.fa / rep.fq / rep_limit.fq: SAM byte-identical including record order, tracks up to the order of the
    fp32 atomic adds"""
    m = rf.MANIFEST[mode]
    out = str(tmp_path / "mine")
    r = subprocess.run([EXE, "-g", rep_fa, "-o", out, "-a", "0.9"] + m["argv"] + VARIANTS[variant] + [rf.fastq_path(rep_fa, m["fastq"])],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sam = "".join(l for l in open(out + ".sam") if not l.startswith("@PG"))
    ref = rf.ref_text(mode, "sam").decode()
    if sam != ref:
        a, b = sam.splitlines(), ref.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{mode}: {len(a)} vs {len(b)} lines, first difference at line {first}:\n  mine {a[first] if first < len(a) else None}\n  ref  {b[first] if first < len(b) else None}")
    assert m["tracks"] == ["sgr"] and not os.path.exists(out + ".gmp")
    compare_tracks(open(out + ".sgr").read(), rf.ref_text(mode, "sgr").decode(), 3)
