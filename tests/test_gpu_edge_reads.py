"""The whole map path on the edge reads (tests/golden/make_edge_fixtures.py), every vote form, against the ORACLE read by read: status,
self / top score bits, denominator, matches in key order, position sets (_compare of test_gpu_parity.py).

What these reads ask that syn.fq does not: the clamped window start b = max(0, c - i) (inc/align_seq2_raw.cpp:267) - the only position
ONE seed can vote for twice (guard (a) of tests/edge_fixture.py: reads that reach -k 2 with a single 14-mer) and that every vote kernel
treats as a case of its own (k_vote_fast: per-step counters; the sorted-key path: duplicate keys; k_vote_bucket / k_vote_pair: reads with
an early position go to the list kernel / are flagged; the others: their own copy of the clamp); the same 14-mer pair at the start of
the second contig, where c - i lies in the first contig and the contig test has to reject the window; reads at and across every contig
start and end, on a reference whose contigs begin and end inside a 16-base word.

One process: the switches go through gm_set_option (read on every call) and are cleared in `finally`.  The guards are asserted again here
on the oracle's side of every comparison that relies on them."""
import re

import numpy as np
import pytest

import edge_fixture as ef
import gnumap_amd as g
from reflib import revcomp_str
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

CONFIGS = {
    "default": {},
    "no_nw": dict(nw=0),
    "m14_j7": dict(mer=14, jump=7),
    "m14_j7_no_nw": dict(mer=14, jump=7, nw=0),
    "k1_m14": dict(min_seed_hits=1, mer=14),
    "raw_all": dict(align_score=-1e6, align_is_fraction=0),
    "up": dict(neg_strand=0),
    "down": dict(pos_strand=0),
    "M5": dict(max_gap=5),
}
# further configurations for k_vote_pair (at most 16 seeds per strand): one strand off, 8 seeds per strand (its <4> form), the band kernels
PAIR_CONFIGS = {
    "m14_j7": CONFIGS["m14_j7"], "m14_j7_no_nw": CONFIGS["m14_j7_no_nw"],
    "m14_j7_up": dict(mer=14, jump=7, neg_strand=0), "m14_j7_down_no_nw": dict(mer=14, jump=7, pos_strand=0, nw=0),
    "m10_j12": dict(mer=10, jump=12), "m12_j6_M5": dict(mer=12, jump=6, max_gap=5),
}
ALL_CONFIGS = dict(CONFIGS, **PAIR_CONFIGS)

BUCKET = dict(GM_SEED_BUCKET="1", GM_KMER_TABLE="mer")            # "mer": replaced by the configuration's -m
# name -> (switches, what batch.path() has to show, index flags).  None: the exact string expected_path() works out from the dispatch rules
# (seed lookup, vote kernel, locate, where the candidates go); the bucket forms: a pattern (the instantiation depends on the seeds per strand)
FORMS = {
    "default": ({}, None, "full"),
    "wave": (dict(GM_VOTE="wave"), None, "full"),                                                              # k_vote_sparse (+ list kernel)
    "wave_fast": (dict(GM_VOTE="wave", GM_VOTE_SPARSE="0"), None, "full"),                                     # k_vote_fast for every read x strand
    "block": (dict(GM_VOTE="block"), None, "full"),
    "big": (dict(GM_VOTE="big"), None, "full"),
    "big_nopipe": (dict(GM_VOTE="big", GM_SLOTS_PIPE="0"), None, "full"),
    "block_kernel": (dict(GM_VOTE="block", GM_VOTE_KERNEL="block"), None, "full"),                             # k_vote_block in one round
    "rounds": (dict(GM_VOTE="rounds"), None, "full"),
    "heavy": (dict(GM_HEAVY_MIN="8"), None, "full"),                                                           # sorted-key path (proved by the trace)
    "fixed0": (dict(GM_VOTE="block", GM_VOTE_FIXED="0"), None, "full"),
    "fixed0_default": (dict(GM_VOTE_FIXED="0"), None, "full"),
    "pair": (dict(BUCKET), r"seeds=bucket-table \(in the vote kernel\) vote=k_vote_pair<\d> \+ k_vote_bucket<\d> locate=full-SA cands=shards ", "full"),
    "bucket": (dict(BUCKET, GM_VOTE_PAIR="0"), r"seeds=bucket-table \(in the vote kernel\) vote=k_vote_bucket<\d> locate=full-SA cands=own-slots ", "full"),
    "pair_gather": (dict(BUCKET, GM_PAIR_HANDOFF="gather"),
                    r"seeds=bucket-table \(in the vote kernel\) vote=k_vote_pair<\d> \+ k_vote_bucket<\d> locate=full-SA cands=own-slots ", "full"),
    "sampled": ({}, None, "sampled"),
    "sampled_block": (dict(GM_VOTE="block"), None, "sampled"),
}
for _s in (0, -1, 10, 20, 40):
    FORMS[f"slots{_s}_seed"] = (dict(GM_VOTE="block", GM_VOTE_SLOTS=str(_s), GM_SEED_FUSED="0"), None, "full")
    FORMS[f"slots{_s}_fused"] = (dict(GM_VOTE="block", GM_VOTE_SLOTS=str(_s), GM_SEED_FUSED="1", GM_KMER_TABLE="mer"), None, "full")

L_PAC = 10007                                                       # edge.fa (checked against the index by check_geometry's caller below)


def expected_path(kw, stride, sw, full):
    """what gm_batch_path() has to say for a block of this row stride - the dispatch rules of gm_map_batch_device restated: expected SA hits
    per seed = reference length / 4^mer, expected seeds per strand from the stride; more than 14 expected hits per read x strand -> one
    workgroup (or wave) per read x strand: k_vote_tiny / k_vote_tiny2 while the hits fit 28 / 56 sixteen-rank groups and -k >= 2, else
    k_vote_slots; GM_VOTE forces the class, GM_VOTE_SLOTS the slot form, GM_VOTE_KERNEL=block k_vote_block; fewer expected hits:
    k_vote_sparse ("sparse"), GM_VOTE_SPARSE=0 k_vote_fast; more than 64 seeds per strand: the ordered k_vote whatever else is set"""
    import math
    mer = kw.get("mer", 10); jump = kw.get("jump", mer // 2); k = kw.get("min_seed_hits", 2)
    per_seed = L_PAC / 4.0 ** mer
    max_seeds = (stride - mer) // jump + 2
    ns = min(math.floor((stride - mer - 1) / jump) + 1, max_seeds)
    e_exp = ns * (1.0 + per_seed)
    spread = per_seed + 3.0 * math.sqrt(per_seed) + 1.0
    slots_exp = ns * math.ceil(spread / 64.0); groups_exp = ns * math.ceil(spread / 16.0)
    dense = (1 if slots_exp <= 38 else 2 if slots_exp <= 60 else 3) if e_exp > 14.0 else 0
    slots_hint = int(min(1000.0, slots_exp))
    if dense == 1 and k >= 2 and e_exp + 4.0 * math.sqrt(e_exp) <= 230.0 and groups_exp <= 28.0:
        slots_hint = 0
    elif dense == 1 and k >= 2 and e_exp + 4.0 * math.sqrt(e_exp) <= 350.0 and groups_exp <= 56.0:
        slots_hint = -1
    if "GM_VOTE_SLOTS" in sw:
        slots_hint = int(sw["GM_VOTE_SLOTS"])
    dense = dict(block=1, big=2, rounds=3, wave=0).get(sw.get("GM_VOTE"), dense)
    kenv = sw.get("GM_VOTE_KERNEL")
    wg = dense != 0 and max_seeds <= 64
    slots_form = wg and (kenv == "slots" if kenv else dense <= 2)
    pp_env = int(sw.get("GM_SLOTS_PIPE", -1))
    slots_pp = full and not kenv and (dense == 2 if pp_env < 0 else pp_env != 0)
    if not wg:
        vote = "k_vote" if max_seeds > 64 else "k_vote_fast" if sw.get("GM_VOTE_SPARSE") == "0" else "sparse"
    elif not slots_form:
        vote = "k_vote_block"
    elif dense == 2:
        vote = "k_vote_slots_pp<64>" if slots_pp else "k_vote_slots<64>"
    else:
        vote = "k_vote_tiny" if slots_hint == 0 else "k_vote_tiny2" if slots_hint < 0 else "k_vote_slots_pp" if slots_pp else "k_vote_slots"
    fused = sw.get("GM_SEED_FUSED") == "1" and full and dense in (1, 2) and not kenv and max_seeds <= 64 and mer <= 16       # (by default only where a k-mer occurs >= 4 times)
    own = sw.get("GM_VOTE_FIXED") != "0" and dense in (1, 2) and not kenv
    return (f"seeds={'k-mer table (in the vote kernel)' if fused else 'k_seed'} vote={vote} locate={'full-SA' if full else 'sampled-SA'} "
            f"cands={'own-slots' if own else 'shards'} ")


def assert_path(o, form, kw, stride):
    sw, shows, which = FORMS[form]
    if shows is None:
        want = expected_path(kw, stride, sw, which == "full")
        assert want in o["path"], (want, o["path"])
    else:
        assert re.search(shows, o["path"]), o["path"]


def precondition(form, kw, longest):
    """None, or the documented precondition of the form that this configuration does not meet (gm_api.cpp, gm_map_batch_device)"""
    mer = kw.get("mer", 10); jump = kw.get("jump", mer // 2)
    max_reg = (max(longest - mer, 0) + jump - 1) // jump
    if form in ("pair", "bucket", "pair_gather"):
        if kw.get("min_seed_hits", 2) < 2:
            return "k_vote_bucket needs -k >= 2 (with -k 1 every hit is a candidate: nothing to filter)"
        if max_reg > 32:
            return "k_vote_bucket takes at most 32 seeds per strand"
    if form in ("pair", "pair_gather") and max_reg > 16:
        return f"k_vote_pair takes at most 16 seeds per strand ({max_reg} here: k_vote_bucket alone, the `bucket` form)"
    return None


@pytest.fixture(scope="module")
def edge_fa(tmp_path_factory):
    return ef.build_index(tmp_path_factory)


@pytest.fixture(scope="module")
def indexes(edge_fa):
    """ONE full-SA index for every form (the k-mer and bucket tables of a seed length are built once and kept), one without the full SA"""
    d = dict(full=g.Index(edge_fa, flags=g.GM_INDEX_FULL_SA), sampled=g.Index(edge_fa, flags=0))
    yield d
    for i in d.values():
        i.close()


@pytest.fixture(scope="module")
def oix(oracle, edge_fa):
    o = oracle.index_load(edge_fa)
    assert ef.check_geometry(o)[1] == L_PAC
    return o


_ORACLE = {}


def oracle_for(oracle, oix, block, rd, cfg):
    """the oracle's results of a block of reads in a configuration, computed once and never changed; the guards that belong to the
    configuration are asserted when it is first asked for"""
    key = (block, cfg)
    if key not in _ORACLE:
        ores = ef.oracle_results(oracle, oix, oracle.params(**ALL_CONFIGS[cfg]), rd)
        if block in ("edge", "clamped_last"):
            ef.guard_windows_inside_one_contig(oix, rd, ores)
            if cfg == "m14_j7_no_nw":
                ef.guard_double_vote(oracle, oix, rd, ores)
                ef.guard_single_votes(oracle, oix, oracle.params(mer=14, nw=0), rd)
            if cfg == "default":
                ef.guard_position_zero(rd, ores)
                ef.guard_contig_ends(oix, rd, ores)
                ef.guard_no_hit_across_a_start(oix, rd, ores)
        _ORACLE[key] = ores
    return _ORACLE[key]


_BLOCKS = {}


def block_reads(name, oracle=None, oix=None):
    if name in _BLOCKS:
        return _BLOCKS[name]
    if name == "edge":
        rd = ef.reads("edge.fq")
    elif name == "mixed":
        rd = ef.reads("edge_mixed.fq")
    elif name == "clamped_last":
        # an ODD number of reads with the ones whose seeds clamp to window start 0 at the end: the last of them is k_vote_pair's tail pair
        rd = ef.reads("edge.fq")
        clamp = [r for r in rd if ef.parse(r[0])[0] in ("dv", "sh") or (ef.parse(r[0])[0] in ("s", "hs") and ef.parse(r[0])[1] == 0)]
        rest = [r for r in rd if r not in clamp]
        rd = rest + clamp
        if len(rd) % 2 == 0:
            rd = rd[1:]
        assert len(rd) % 2 == 1 and ef.parse(rd[-1][0])[0] in ("dv", "sh") and len(clamp) > 60
    else:
        raise KeyError(name)
    _BLOCKS[name] = rd
    return rd


def run(ix, rd, kw, switches, tile=1):
    p = g.Params(**kw)
    sw = {k: (str(p.mer) if v == "mer" else v) for k, v in switches.items()}
    B, Q, Ln = g.pack_reads([r[1] for r in rd], [r[2] for r in rd])
    if tile > 1:
        B = np.tile(B, (tile, 1)); Q = np.tile(Q, (tile, 1)); Ln = np.tile(Ln, tile)
    for k, v in sw.items():
        g.set_option(k, v)
    try:
        batch = g.Batch(ix, len(Ln), B.shape[1])
        res = batch.map(p, B, Q, Ln)
        out = dict(res=res, raw=batch.raw_hits(), ctr=batch.counters(), path=batch.path(), batch=batch, p=p)
    finally:
        for k in sw:
            g.set_option(k, None)
    return out


_DOUBLE = {}


def assert_double_votes_present(oracle, oix, rd, ores, res):
    """every read of guard (a) is in the results with its one hit at 0, score 2: a missed flag or clamp loses or miscounts it"""
    mb = res["match_begin"]
    if id(rd) not in _DOUBLE:
        _DOUBLE[id(rd)] = ef.guard_double_vote(oracle, oix, rd, ores)
    for i in _DOUBLE[id(rd)]:
        ms = res["matches"][int(mb[i]):int(mb[i + 1])]
        assert res["status"][i] == 0 and len(ms) == 1 and float(ms[0]["score"]) == 2.0 and int(ms[0]["first_pos"]) == 0, rd[i][0]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_edge_reads_every_vote_form_matches_oracle(cfg, form, indexes, oracle, oix, capfd):
    rd = block_reads("edge")
    sw, shows, which = FORMS[form]
    why = precondition(form, CONFIGS[cfg], 100)
    if why:
        pytest.skip(why)
    ores = oracle_for(oracle, oix, "edge", rd, cfg)
    if form == "heavy":
        sw = dict(sw, GM_TRACE="1")
    o = run(indexes[which], rd, CONFIGS[cfg], sw)
    assert_path(o, form, CONFIGS[cfg], 104)
    nw_form = "k_nw_band" if cfg == "M5" else "k_nw_rows/" if CONFIGS[cfg].get("nw", 1) else "k_nw_lane"      # (--no_nw: no DP rows to order)
    assert f"nw={nw_form}" in o["path"], o["path"]                       # one length: the rows-in-DP-order kernel (or the band kernel)
    _compare(o["res"], ores, rd)
    if cfg == "m14_j7_no_nw":
        assert_double_votes_present(oracle, oix, rd, ores, o["res"])
    if form == "heavy":
        n_heavy = [int(x) for x in re.findall(r"(\d+) read x strands on the heavy path", capfd.readouterr().err)]
        assert n_heavy and max(n_heavy) > 100, n_heavy
    if form in ("pair", "bucket", "pair_gather") and cfg in ("default", "m14_j7"):
        assert o["ctr"]["sa_hits"] == sum(x["ctr"]["locates"] for x in ores)
    o["batch"].destroy()


@pytest.mark.parametrize("cfg", list(PAIR_CONFIGS))
@pytest.mark.parametrize("block", ["edge", "clamped_last"])
def test_pair_kernel_on_and_off_give_the_same_raw_hits(block, cfg, indexes, oracle, oix):
    """the A/B of k_vote_pair: raw hits, statuses, self and top scores with GM_VOTE_PAIR on and off are equal field for field, also with
    an odd number of reads whose last ones all vote for the clamped window start"""
    rd = block_reads(block)
    assert precondition("pair", PAIR_CONFIGS[cfg], 100) is None
    ores = oracle_for(oracle, oix, block, rd, cfg)
    on = run(indexes["full"], rd, PAIR_CONFIGS[cfg], BUCKET)
    off = run(indexes["full"], rd, PAIR_CONFIGS[cfg], dict(BUCKET, GM_VOTE_PAIR="0"))
    gather = run(indexes["full"], rd, PAIR_CONFIGS[cfg], dict(BUCKET, GM_PAIR_HANDOFF="gather"))
    assert "k_vote_pair<" in on["path"] and "k_vote_pair<" in gather["path"] and "k_vote_pair" not in off["path"] and "k_vote_bucket<" in off["path"]
    for other in (off, gather):
        for a, b in zip(on["raw"], other["raw"]):
            np.testing.assert_array_equal(a, b)
    assert len(on["raw"][0]) > 100
    for o in (on, off, gather):
        _compare(o["res"], ores, rd)
        if cfg == "m14_j7_no_nw":
            assert_double_votes_present(oracle, oix, rd, ores, o["res"])
        o["batch"].destroy()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_mixed_lengths_match_oracle(cfg, form, indexes, oracle, oix, capfd):
    """16 .. 150 bases in one block: k_nw_lane; lengths below k_nw_rows' floor; 16 bases at -m 14 leave two seed positions"""
    rd = block_reads("mixed")
    sw, shows, which = FORMS[form]
    why = precondition(form, CONFIGS[cfg], 150)
    if why:
        pytest.skip(why)
    ores = oracle_for(oracle, oix, "mixed", rd, cfg)
    if form == "heavy":
        sw = dict(sw, GM_TRACE="1")
    o = run(indexes[which], rd, CONFIGS[cfg], sw)
    assert_path(o, form, CONFIGS[cfg], 152)
    if form == "heavy":
        n_heavy = [int(x) for x in re.findall(r"(\d+) read x strands on the heavy path", capfd.readouterr().err)]
        assert n_heavy and max(n_heavy) > 100, n_heavy
    assert ("nw=k_nw_band" if cfg == "M5" else "nw=k_nw_lane") in o["path"], o["path"]
    _compare(o["res"], ores, rd)
    assert sum(x["status"] == 0 for x in ores) > 100
    if "mer" not in CONFIGS[cfg]:
        assert any(x["status"] == 0 and len(rd[i][1]) == 16 for i, x in enumerate(ores))
    o["batch"].destroy()


@pytest.mark.parametrize("nw", ["lane", "wave", "cells_b32"])
@pytest.mark.parametrize("cfg", [c for c in CONFIGS if CONFIGS[c].get("nw", 1) and "max_gap" not in CONFIGS[c]])
def test_edge_reads_every_dp_form_matches_oracle(cfg, nw, indexes, oracle, oix):
    rd = block_reads("edge")
    sw, shows = dict(lane=(dict(GM_NW="lane"), r" nw=k_nw_lane<(13|0)>$"), wave=(dict(GM_NW="wave"), r" nw=k_nw$"),     # (<13>: rows of up to 104 bytes
                     cells_b32=(dict(GM_NW_CELLS="b32"), r" nw=k_nw_rows/cells$"))[nw]                                   #  in registers, <0>: streamed)
    o = run(indexes["full"], rd, CONFIGS[cfg], sw)
    assert re.search(shows, o["path"]), o["path"]
    _compare(o["res"], oracle_for(oracle, oix, "edge", rd, cfg), rd)
    o["batch"].destroy()


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_pipelined_sub_batches_on_the_edge_reads(cfg, indexes, oracle, oix):
    """GM_PIPELINE=4096 on the reads tiled to more than 3 x 4096: every copy of a read gets the oracle's answer (sub-batch boundaries
    fall between any two reads of the set)"""
    rd = block_reads("edge")
    ores = oracle_for(oracle, oix, "edge", rd, cfg)
    tile = (3 * 4096) // len(rd) + 2
    o = run(indexes["full"], rd, CONFIGS[cfg], dict(GM_PIPELINE="4096"), tile=tile)
    assert len(o["res"]["status"]) >= 3 * 4096 + len(rd)
    assert o["path"] == "", o["path"]              # the single-pass dispatch (which records its choice) never ran on this fresh batch
    _compare(o["res"], ores * tile, rd * tile)
    o["batch"].destroy()


def _long_edge_reads(genome, l_pac):
    """700-bp reads that hang off position 0 and end at (or hang off) l_pac: at -j 5 more than 64 seeds per strand -> the ordered k_vote"""
    rng = np.random.default_rng(700)
    rb = lambda n: bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))
    out = []
    for d in (0, 1, 3, 5):
        out.append((f"l0_{d}", rb(d) + genome[:700 - d]))
        out.append((f"lend_{d}", genome[l_pac - 700 + d:l_pac] + rb(d)))
    for d in (20, 40):
        out.append((f"lsh_{d}", rb(d) + genome[:700 - d]))
    rd = []
    for name, s in out:
        assert len(s) == 700
        rd.append((name + "_f", s, b"I" * 700)); rd.append((name + "_r", revcomp_str(s).upper(), b"I" * 700))
    return rd


@pytest.mark.parametrize("cfg", ["default", "no_nw", "M5", "raw_all"])
def test_long_reads_off_both_ends_of_the_reference(cfg, indexes, oracle, oix, edge_fa):
    genome = b"".join(l.strip() for l in open(edge_fa, "rb") if not l.startswith(b">")).upper()
    _, l_pac = ef.geometry(oix)
    rd = _long_edge_reads(genome, l_pac)
    kw = CONFIGS[cfg]
    assert (700 - 10) // 5 > 64                                            # more seeds than a 64-bit step mask holds
    ores = ef.oracle_results(oracle, oix, oracle.params(**kw), rd)
    assert sum(x["status"] == 0 and any(p == 0 for h in x["hits"] for p, _ in h["pos"]) for x in ores) >= 4
    assert sum(x["status"] == 0 and any(p + 700 == l_pac for h in x["hits"] for p, _ in h["pos"]) for x in ores) >= 2
    for which in ("full", "sampled"):
        o = run(indexes[which], rd, kw, {})
        assert " vote=k_vote " in o["path"], o["path"]                  # the ordered kernel, not one of the step-mask forms
        _compare(o["res"], ores, rd)
        o["batch"].destroy()


# ------------------------------------------------------------------ the output half: SAM records and the coverage deposit
def _track_close(got, want):
    """the tolerance of compare_tracks (tests/test_gpu_driver_golden.py) on whole arrays: fp32 atomic adds in another order"""
    tol = 1e-4 * np.maximum(1.0, np.abs(want)) + 2e-5
    bad = np.flatnonzero(np.abs(got - want) > tol)
    assert len(bad) == 0, [(int(k), float(got[k]), float(want[k])) for k in bad[:8]]


@pytest.mark.parametrize("bin_size", [1, 8])
@pytest.mark.parametrize("cfg", ["default", "bs", "M5"])
def test_output_records_and_coverage_at_the_edges(cfg, bin_size, indexes, oracle, oix):
    kw = dict(dict(default={}, bs=dict(mode=1), M5=dict(max_gap=5))[cfg], bin_size=bin_size)
    rd = block_reads("edge")
    ix = indexes["full"]
    p = g.Params(**kw); op = oracle.params(**kw)
    B, Q, Ln = g.pack_reads([r[1] for r in rd], [r[2] for r in rd])
    ix.coverage_reset(bin_size)
    if cfg == "bs":
        ix.coverage_enable_nuc()
    batch = g.Batch(ix, len(rd), B.shape[1])
    try:
        res = batch.map(p, B, Q, Ln)
        recs, cigars = batch.output(p, res)
        cov = ix.coverage_download()
        nuc = ix.coverage_download_nuc().reshape(5, -1) if cfg == "bs" else None
    finally:
        ix.coverage_reset(8)
        batch.destroy()
    want_cov = np.zeros(len(cov), np.float64); want_nuc = np.zeros((5, len(cov)), np.float64)
    want_recs = []
    for i, (name, seq, qual) in enumerate(rd):
        st, orecs, deps = oracle.read_output(oix, op, oracle.pwm(seq, qual), seq)
        want_recs += [(i, r["contig"], r["chr_pos"], r["strand"], r["mapq"], r["cigar"]) for r in orecs]
        for pos, span, w, codes in deps:
            w = float(np.float32(w))
            for t in range(span):
                want_cov[(pos + t) // bin_size] += w
                if codes is not None and codes[t] < 5:
                    want_nuc[codes[t], (pos + t) // bin_size] += w
    got_recs = [(int(r["read"]), int(r["contig"]), int(r["chr_pos"]), int(r["strand"]), int(r["mapq"]), c) for r, c in zip(recs, cigars)]
    assert got_recs == want_recs
    assert len(want_recs) > 200
    _track_close(cov.astype(np.float64), want_cov)
    if nuc is not None:
        _track_close(nuc.astype(np.float64).ravel(), want_nuc.ravel())
        assert want_nuc.sum() > 0.9 * want_cov.sum()
    # the bins this is about are covered: bin 0, the last (partial) bin, and the bins either side of each inner boundary
    ctg, l_pac = ef.geometry(oix)
    for pos in [0, l_pac - 1] + [x for b, _ in ctg[1:] for x in (b - 1, b)]:
        assert want_cov[pos // bin_size] > 0.5, pos
