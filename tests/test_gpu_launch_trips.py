"""Every looping kernel of the map and output paths with SEVERAL trips per wave or workgroup, on the fixtures the suite already has.

The launchers size their grids for blocks of 10 M reads; with the 64 .. 1 000 reads of the other GPU tests every wave runs its loop body
once, and whatever exists only because there is a next trip (state re-zeroed between two items, counters summed over trips, a prefetch of
the next item, a `continue` followed by live work, a partial last trip) runs in the benchmark alone.  Here the geometry is forced down to
test sizes, every result is compared for EXACT equality - with the oracle read by read, and with the same form at default geometry byte
for byte (raw hits, statuses, self and top scores, counters()) - and every case asserts from the run's own numbers that the later trip
happened.

kernel                     launcher's cap                        second trip at default geometry        forced here by
-------------------------  ------------------------------------  -------------------------------------  ----------------------------------------
k_vote_pair                >= 4096 workgroups or 16-pair chunks   131 041 pairs (two groups/workgroup)   GM_TEST_PAIR_MIN_GRID=1 GM_PAIR_CHUNK=32/48/176
k_vote_bucket              CUs x 4 x waves/SIMD x 4 waves         16 385 .. 32 769 reads                 GM_BUCKET_GRID=1/2/3/7/n-1
k_seed                     3072 workgroups x 128 reads            393 217 reads                          GM_SEED_GRID=1/2
k_locate_flat              2048 workgroups x 256 lanes            524 289 SA hits                        GM_LOCATE_GRID=1/2
k_vote_fast_list           5120 workgroups x 4 read x strands     20 481 listed read x strands           GM_TEST_GRID_CAP=1/2 (form `wave` at -m 10, see below)
k_heavy_collect            1024 (list form 256) x 256 lanes       524 289 reads                          GM_TEST_GRID_CAP=1/2
k_prep_rows                5120 workgroups x 256 reads            1 310 721 reads                        GM_TEST_GRID_CAP=1/2
k_prep                     resident round x 64 .. 256 reads       ~50 000 .. 200 000 reads               GM_TEST_GRID_CAP=1/2 (reads of 300 and 600 bases)
k_scatter_hits             2048 workgroups x 256 lanes            524 289 candidates                     GM_TEST_GRID_CAP=1/2
k_nw_rows                  one resident round x 256 lanes         ~262 145 candidates                    GM_NW_GRID=1/2
k_nw_lane (4 forms)        max(2048, candidates / 1024) x 256     524 289 candidates                     GM_NW_GRID=1/2 (<13>, <19>, <0>, <13 / 19,lds>)
k_nw                       2048 x 32 (8192 x 8) candidates        65 537 candidates                      GM_TEST_GRID_CAP=1/2
k_nw_band                  max(256, candidates / 512) x 128       32 769 candidates                      GM_TEST_GRID_CAP=1/2
k_group_multi / _write_    16 384 workgroups, one read each       16 385 multi-hit reads                 GM_TEST_GRID_CAP=1/2
k_group_big / _write_      4096 workgroups, one read each         4097 reads on the big path             GM_TEST_GRID_CAP=1/2
k_out_text_rows            resident round x 4 records             4 097 .. 8 193 records (4 .. 8 per CU) GM_TEST_GRID_CAP=1/2
k_bam_rows                 4096 workgroups x 4 records            16 385 records                         GM_TEST_GRID_CAP=1/2
k_traceback_lane<128>      16 384 workgroups x 128 items          2 097 153 items                        GM_TEST_GRID_CAP=1/2
k_traceback_lane<64>       16 384 workgroups x 64 items           1 048 577 items                        GM_TEST_GRID_CAP=1/2
k_traceback                8192 workgroups x 32 (8) items         262 145 (65 537) items                 GM_TEST_GRID_CAP=1/2
k_traceback_band           items per launch: 512 MB of moves      ~640 000 items at L = 100 (i0 > 0)     GM_TEST_GRID_CAP=1/2 (N x 128 items per launch)
k_adaptor_trim             8192 workgroups x 4 reads              32 769 reads                           GM_TEST_GRID_CAP=1/2
k_scan_sums                one workgroup, ceil(tiles / 1024) each 1 048 577 scanned values               gm_dev_scan_u32 at those sizes
k_rt_scan / k_rt_phase_scan the same                              4 MiB of text / 262 145 lines          texts of those sizes

k_vote_fast_list's later trips are asserted where the size of its list follows from the run's numbers: form `wave` at -m 10 -j 5, where
every 100-base strand has 18 seeds and k_vote_sparse lists all of them.  In the forms `default`, `heavy` and `fixed0` it runs under the
cap too, on a list whose length no counter shows; those cases assert the trips of k_prep_rows, k_heavy_collect and k_scatter_hits.

Left out, with the reason:
  k_track_scan                 tests/test_gpu_track_text.py::test_sgr_equals_the_host_writer[1] and ::test_gmp_equals_the_host_writer[*-1]
                               run syn.fa (280 000 positions) at bin size 1 with GM_TRACK_SLICE unset: 1094 tiles, per = 2; so does
                               tests/test_gpu_snp_text.py::test_device_writer_equals_the_host_writer for the nine-column text
  k_snp_scan                   tests/test_gpu_snp_text.py::test_vcf and tests/test_gpu_snp_call.py call gm_snp_calls on the same 280 000
                               positions with GM_TRACK_SLICE unset: 1094 workgroup counts, per = 2
  k_traceback_band's kernel    takes one item per lane (no loop); what the cap bounds is the items of one launch
  k_vote_slots_pp              GM_SLOTS_CHUNK in tests/test_gpu_parity.py
  k_bgzf_deflate_lz            test_many_payloads_through_a_grid_smaller_than_their_number in tests/test_gpu_bgzf_lz77.py

A capped run is slower than the default one by design; nothing here is a timing."""
import re

import numpy as np
import pytest

import bam_model as bm
import edge_fixture as ef
import fastq_text_model as FM
import gnumap_amd as g
import repeat_fixture as rf
import test_gpu_edge_reads as er
import test_gpu_edge_windows as ew
import test_gpu_pair_filter as pf
from adaptor_model import kept_lengths
from conftest import GOLDEN, read_fastq
from test_gpu_adaptor import AD34
from test_gpu_bam import check_records
from test_gpu_pair_handoff import CONFIGS as PLANTED_CONFIGS, planted  # noqa: F401  (the planted-repeat fixture)
from test_gpu_parity import _compare, _oracle_results
from test_gpu_read_text import check_probe
from test_gpu_repeat_groups import TRACE as GROUP_TRACE, compare as repeat_compare
from test_gpu_sam_text import check_text

pytestmark = pytest.mark.gpu

PAIR_GEO = [dict(GM_TEST_PAIR_MIN_GRID="1", GM_PAIR_CHUNK=c) for c in ("32", "48", "176")]


# ------------------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def edge_fa(tmp_path_factory):
    return ef.build_index(tmp_path_factory)


@pytest.fixture(scope="module")
def indexes(edge_fa):
    d = dict(full=g.Index(edge_fa, flags=g.GM_INDEX_FULL_SA), sampled=g.Index(edge_fa, flags=0))
    yield d
    for i in d.values():
        i.close()


@pytest.fixture(scope="module")
def oix(oracle, edge_fa):
    o = oracle.index_load(edge_fa)
    assert ef.check_geometry(o)[1] == er.L_PAC
    return o


@pytest.fixture(scope="module")
def genome(edge_fa):
    return b"".join(l.strip() for l in open(edge_fa, "rb") if not l.startswith(b">")).upper()


@pytest.fixture(scope="module")
def syn_ix(syn_fa):
    i = g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)
    yield i
    i.close()


@pytest.fixture(scope="module")
def syn_oix(oracle, syn_fa):
    return oracle.index_load(syn_fa)


@pytest.fixture(scope="module")
def pf_world():
    return pf.World()


@pytest.fixture(scope="module")
def pf_index(pf_world, tmp_path_factory, oracle):
    fa = str(tmp_path_factory.mktemp("trips_pf") / "pf.fa")
    with open(fa, "wb") as f:
        f.write(b">pf\n")
        s = pf_world.G.tobytes()
        for k in range(0, len(s), 100):
            f.write(s[k:k + 100] + b"\n")
    g.index_build(fa, g.GM_BUILD_HOST)
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA)
    yield ix, oracle.index_load(fa)
    ix.close()


@pytest.fixture(scope="module")
def rep(tmp_path_factory, oracle):
    fa = rf.build_index(tmp_path_factory)
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA)
    yield ix, oracle.index_load(fa)
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------ helpers
def go(ix, rd, kw, sw, tile=1):
    """one mapping (run of test_gpu_edge_reads.py) with its batch given back: results, raw hits, counters, path, flagged reads"""
    o = er.run(ix, rd, kw, sw, tile)
    try:
        o["flagged"] = o["batch"].pair_flagged()
    finally:
        o.pop("batch").destroy()
    return o


_BASE = {}


def base_run(key, make):
    """the run at default geometry of a (fixture, configuration, form): made once, never changed"""
    if key not in _BASE:
        _BASE[key] = make()
    return _BASE[key]


def same_bytes(a, b):
    """equal dtype, shape and bytes; a record array field by field (the padding between its fields is nobody's)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names)
    return a.tobytes() == b.tobytes()


def assert_same_run(o, base, what):
    """raw hits, statuses, self and top scores byte for byte; the work counters and the flagged reads equal"""
    for k, (a, b) in enumerate(zip(o["raw"], base["raw"])):
        assert same_bytes(a, b), (what, k, a.shape, b.shape)
    assert o["ctr"] == base["ctr"], (what, o["ctr"], base["ctr"])
    assert o["flagged"] == base["flagged"], (what, o["flagged"], base["flagged"])
    for k in ("status", "self_score", "top_score", "denominator", "match_begin", "matches"):
        assert same_bytes(o["res"][k], base["res"][k]), (what, k)


def cdiv(a, b):
    return (a + b - 1) // b


def assert_pair_groups(n_reads, chunk):
    """a workgroup of `chunk` pairs holds at least two 16-pair groups of this block, and the block's last group is a partial one"""
    npairs = (n_reads + 1) // 2
    assert cdiv(min(chunk, npairs), 16) >= 2 and npairs % 16 != 0, (n_reads, chunk)
    return cdiv(min(chunk, npairs), 16)


class switches:
    def __init__(self, **sw):
        self.sw = sw

    def __enter__(self):
        for k, v in self.sw.items():
            g.set_option(k, v)

    def __exit__(self, *a):
        for k in self.sw:
            g.set_option(k, None)


# ------------------------------------------------------------------------------------------------------------------------ a. vote kernels
def _pair_cfgs(block):
    longest = 150 if block == "mixed" else 100
    return [c for c in ("m14_j7", "m10_j12", "m14_j7_no_nw", "m14_j7_up") if er.precondition("pair", er.PAIR_CONFIGS[c], longest) is None]


@pytest.mark.parametrize("form", ["pair", "pair_gather"])
@pytest.mark.parametrize("block,cfg", [(b, c) for b in ("edge", "clamped_last", "mixed") for c in _pair_cfgs(b)])
def test_vote_pair_with_several_groups_per_workgroup(block, cfg, form, indexes, oracle, oix):
    """k_vote_pair: GM_PAIR_CHUNK pairs per workgroup (32 and 48: two and three groups; 176: ONE workgroup for the block, eleven groups,
    the last one partial - on clamped_last ended by the half-empty tail pair).  What crosses a group boundary: the LDS results zeroed at
    (pair & 15) == 0, the flagged-read mask and the further-candidate count cleared after a flush, the work counters summed over groups
    (counters() equal), the software pipeline running on across a flush.  With GM_BUCKET_GRID 1 and 3 on top the list kernel takes
    several flagged reads per wave"""
    rd = er.block_reads(block)
    kw = er.PAIR_CONFIGS[cfg]
    sw, shows, which = er.FORMS[form]
    ix = indexes[which]
    ores = er.oracle_for(oracle, oix, block, rd, cfg)
    base = base_run((block, cfg, form), lambda: go(ix, rd, kw, sw))
    assert re.search(shows, base["path"]), base["path"]
    _compare(base["res"], ores, rd)
    assert base["flagged"] > 6                                      # (the list kernel has more reads than the largest grid below twice over)
    for geo in PAIR_GEO:
        n_groups = assert_pair_groups(len(rd), int(geo["GM_PAIR_CHUNK"]))
        if geo["GM_PAIR_CHUNK"] == "176":
            assert n_groups == 11                                   # (edge, clamped_last: 165 pairs, ONE workgroup holds every group of the block)
        for bgrid in (None, "1", "3"):
            more = dict(geo, GM_BUCKET_GRID=bgrid) if bgrid else geo
            o = go(ix, rd, kw, dict(sw, **more))
            assert re.search(shows, o["path"]), o["path"]
            if bgrid:
                assert o["flagged"] > 2 * int(bgrid)                # every wave of the list kernel takes a third read
            _compare(o["res"], ores, rd)
            assert_same_run(o, base, (block, cfg, form, more))
            if cfg == "m14_j7" and block != "mixed":
                assert o["ctr"]["sa_hits"] == sum(x["ctr"]["locates"] for x in ores)
            if cfg == "m14_j7_no_nw" and block != "mixed":
                er.assert_double_votes_present(oracle, oix, rd, ores, o["res"])


@pytest.mark.parametrize("block,cfg", [("edge", c) for c in er.CONFIGS if er.precondition("bucket", er.CONFIGS[c], 100) is None] +
                         [("clamped_last", "m14_j7"), ("clamped_last", "default"), ("mixed", "m14_j7"), ("mixed", "default")])
def test_vote_bucket_waves_take_several_reads(block, cfg, indexes, oracle, oix):
    """k_vote_bucket's persistent waves: one wave for the whole block, two, seven, and n - 1 (exactly one wave takes a second read).  The
    next read's words are requested while a read is voted on; a dead read's `continue` and a non-ACGT read are followed by ordinary reads"""
    rd = er.block_reads(block)
    kw = er.ALL_CONFIGS[cfg]
    assert er.precondition("bucket", kw, 150 if block == "mixed" else 100) is None
    sw, shows, which = er.FORMS["bucket"]
    ix = indexes[which]
    ores = er.oracle_for(oracle, oix, block, rd, cfg)
    base = base_run((block, cfg, "bucket"), lambda: go(ix, rd, kw, sw))
    assert re.search(shows, base["path"]), base["path"]
    _compare(base["res"], ores, rd)
    for grid in (1, 2, 7, len(rd) - 1):
        assert len(rd) > grid                                       # a wave takes a second read
        o = go(ix, rd, kw, dict(sw, GM_BUCKET_GRID=str(grid)))
        assert re.search(shows, o["path"]), o["path"]
        _compare(o["res"], ores, rd)
        assert_same_run(o, base, (block, cfg, grid))
        if cfg in ("default", "m14_j7") and block != "mixed":
            assert o["ctr"]["sa_hits"] == sum(x["ctr"]["locates"] for x in ores)


@pytest.mark.parametrize("form", ["default", "wave", "block", "slots10_seed", "sampled"])
@pytest.mark.parametrize("cfg", ["default", "m14_j7", "k1_m14"])
def test_seed_kernel_with_several_tiles_per_workgroup(cfg, form, indexes, oracle, oix):
    """k_seed (GM_SEED_FUSED=0): tiles of 128 reads, one and two workgroups for the three tiles of the block"""
    rd = er.block_reads("edge")
    kw = er.CONFIGS[cfg]
    sw, _, which = er.FORMS[form]
    sw = dict(sw, GM_SEED_FUSED="0")
    ores = er.oracle_for(oracle, oix, "edge", rd, cfg)
    base = base_run(("edge", cfg, form, "seed"), lambda: go(indexes[which], rd, kw, sw))
    assert "seeds=k_seed " in base["path"], base["path"]
    _compare(base["res"], ores, rd)
    for grid in (1, 2):
        assert cdiv(len(rd), 128) > grid and len(rd) % 128 != 0     # a second tile for a workgroup, the last tile partial
        o = go(indexes[which], rd, kw, dict(sw, GM_SEED_GRID=str(grid)))
        assert o["path"] == base["path"]
        _compare(o["res"], ores, rd)
        assert_same_run(o, base, (cfg, form, grid))


@pytest.mark.parametrize("form", ["sampled", "sampled_block"])
@pytest.mark.parametrize("cfg", ["default", "m14_j7", "raw_all"])
def test_locate_lanes_walk_several_hits(cfg, form, indexes, oracle, oix):
    """k_locate_flat: every lane takes each (grid x 256)-th SA hit of the block's list"""
    rd = er.block_reads("edge")
    kw = er.CONFIGS[cfg]
    sw, _, which = er.FORMS[form]
    ores = er.oracle_for(oracle, oix, "edge", rd, cfg)
    base = base_run(("edge", cfg, form, "locate"), lambda: go(indexes[which], rd, kw, sw))
    assert "locate=sampled-SA" in base["path"], base["path"]
    _compare(base["res"], ores, rd)
    for grid in (1, 2):
        o = go(indexes[which], rd, kw, dict(sw, GM_LOCATE_GRID=str(grid)))
        assert o["ctr"]["sa_hits"] > 2 * 256 * grid and o["ctr"]["sa_hits"] % (256 * grid) != 0
        assert o["path"] == base["path"]
        _compare(o["res"], ores, rd)
        assert_same_run(o, base, (cfg, form, grid))


@pytest.mark.parametrize("cfg,form", [(c, f) for f in ("wave", "heavy", "default", "fixed0") for c in ("default", "m14_j7", "no_nw")
                                      if not (f == "wave" and c == "m14_j7")])      # (-m 14 -j 7: 13 seeds a strand, the list's length is not known)
def test_capped_grids_of_the_map_step(cfg, form, indexes, oracle, oix, capfd):
    """GM_TEST_GRID_CAP 1 and 2 on four copies of the edge reads (1320 reads): k_prep_rows (256 reads a trip), k_heavy_collect (256 lanes of
    four read x strands) and k_scatter_hits (256 candidates a trip) loop in every case; k_vote_fast_list (four listed read x strands a
    trip) provably in form `wave`, whose two configurations have 18 seeds on every strand"""
    rd = er.block_reads("edge")
    tile = 4
    kw = er.CONFIGS[cfg]
    sw, _, which = er.FORMS[form]
    sw = dict(sw, GM_TRACE="1")
    ores = er.oracle_for(oracle, oix, "edge", rd, cfg) * tile
    base = base_run(("edge", cfg, form, "cap"), lambda: go(indexes[which], rd, kw, sw, tile))
    _compare(base["res"], ores, rd * tile)
    capfd.readouterr()
    for cap in (1, 2):
        o = go(indexes[which], rd, kw, dict(sw, GM_TEST_GRID_CAP=str(cap)), tile)
        n = len(rd) * tile
        assert n > 2 * 256 * cap and n % 256 != 0                   # k_prep_rows: a third, partial trip
        assert 2 * n // 4 > 256 * cap and (2 * n // 4) % 256 != 0   # k_heavy_collect (all reads, four read x strands a lane): a later, partial trip
        assert o["ctr"]["candidates"] > 256 * cap                   # k_scatter_hits
        err = capfd.readouterr().err
        if form == "wave":
            # k_vote_sparse lists every read x strand with more than 16 seeds or SA hits: at -m 10 -j 5 each 100-base strand has 18 seeds,
            # at most 19; so at least seeds_used / 19 read x strands are on the list
            mer = kw.get("mer", 10); jump = kw.get("jump", mer // 2)
            assert (100 - mer - 1) // jump + 1 > 16
            assert o["ctr"]["seeds_used"] // 19 > 2 * 4 * cap
        if form == "heavy":
            n_heavy = [int(x) for x in re.findall(r"(\d+) read x strands on the heavy path", err)]
            assert n_heavy and max(n_heavy) > 100, n_heavy
        assert o["path"] == base["path"]
        _compare(o["res"], ores, rd * tile)
        assert_same_run(o, base, (cfg, form, cap))


@pytest.mark.parametrize("cfg", ["base", "all", "no_nw"])
@pytest.mark.parametrize("block", ["kept", "mixed"])
@pytest.mark.parametrize("tag", list(pf.GROUPS))
def test_engineered_pair_blocks_in_one_workgroup(tag, block, cfg, pf_world, pf_index, oracle):
    """the engineered blocks of test_gpu_pair_filter.py (33 and 35 reads: 17 and 18 pairs) in ONE workgroup of two groups, the second
    a partial one: filter marks, the flagged read beside a kept one, against the oracle, GM_VOTE_PAIR=0 and the default geometry"""
    ix, poix = pf_index
    rd = pf_world.blocks[tag, block]
    L, jump = pf.GROUPS[tag]
    kw = dict(mer=pf.MER, jump=jump, **pf.CONFIGS[cfg])
    ores = pf.oracle_for(oracle, poix, pf_world, tag, block, cfg)
    base = base_run(("pf", tag, block, cfg), lambda: go(ix, rd, kw, er.BUCKET))
    off = go(ix, rd, kw, dict(er.BUCKET, GM_VOTE_PAIR="0"))
    assert f"vote=k_vote_pair<{tag}> + k_vote_bucket<" in base["path"] and "k_vote_pair" not in off["path"], (base["path"], off["path"])
    assert base["flagged"] == (2 if block == "mixed" else 0) and off["flagged"] == 0
    _compare(base["res"], ores, rd)
    for geo in PAIR_GEO[:1]:
        assert assert_pair_groups(len(rd), int(geo["GM_PAIR_CHUNK"])) == 2
        o = go(ix, rd, kw, dict(er.BUCKET, **geo))
        assert o["path"] == base["path"]
        _compare(o["res"], ores, rd)
        assert_same_run(o, base, (tag, block, cfg, geo))
        for a, b in zip(o["raw"], off["raw"]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("cfg", ["base", "all"])
@pytest.mark.parametrize("tag", list(pf.GROUPS))
def test_full_lds_candidate_list_then_a_next_group(tag, cfg, pf_world, pf_index, oracle):
    """more than 16 FURTHER candidates in one 16-pair group (the group's LDS list holds 16: the rest go to the shard by direct atomics),
    then two more groups in the same workgroup, whose lists have to start empty.  The block: the two reads of case 3 of
    test_gpu_pair_filter.py (a real second candidate on one strand, so one further candidate each) twenty times - the first group is 32
    of them -, then 25 kept reads; 65 reads, 33 pairs"""
    ix, poix = pf_index
    keep = pf_world.blocks[tag, "kept"]
    c3 = [r for r in keep if r[0].startswith("c3_")]
    assert len(c3) == 2
    rd = [(f"{n}#{k}", s_, q) for k in range(20) for n, s_, q in c3] + [r for r in keep if not r[0].startswith("c3_")][:25]
    assert len(rd) == 65
    L, jump = pf.GROUPS[tag]
    kw = dict(mer=pf.MER, jump=jump, **pf.CONFIGS[cfg])
    op = oracle.params(**kw)
    by_seq = {}
    for _, s_, q in rd:
        if s_ not in by_seq:
            by_seq[s_] = oracle.map_read(poix, op, oracle.pwm(s_, q), s_)
    ores = [by_seq[r[1]] for r in rd]
    if cfg == "all":                                                # (every candidate is accepted: the second one shows in the oracle)
        assert all(sum(len(h["pos"]) for h in by_seq[r[1]]["hits"]) >= 2 for r in c3)
    base = go(ix, rd, kw, er.BUCKET)
    off = go(ix, rd, kw, dict(er.BUCKET, GM_VOTE_PAIR="0"))
    assert f"vote=k_vote_pair<{tag}> + k_vote_bucket<" in base["path"] and "k_vote_pair" not in off["path"], (base["path"], off["path"])
    assert base["flagged"] == 0                                     # k_vote_pair itself voted for every read
    assert base["ctr"]["candidates"] >= 2 * 40 + 25                 # 32 further candidates in the first group: twice the LDS list
    _compare(base["res"], ores, rd)
    for geo in PAIR_GEO:
        assert assert_pair_groups(len(rd), int(geo["GM_PAIR_CHUNK"])) >= 2
        o = go(ix, rd, kw, dict(er.BUCKET, **geo))
        assert o["path"] == base["path"]
        _compare(o["res"], ores, rd)
        assert_same_run(o, base, (tag, cfg, geo))
        for x, y in zip(o["raw"], off["raw"]):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("cfg", sorted(PLANTED_CONFIGS))
def test_planted_repeats_with_several_groups_per_workgroup(cfg, planted, oracle, capfd):  # noqa: F811
    """the planted reads of test_gpu_pair_handoff.py: more than 16 further candidates in a group (the LDS list full: direct atomics), then a
    NEXT group in the same workgroup, whose list has to start empty; a shard overflows and the retry loop runs.  (What this case adds is
    the shard overflow and the retry under the multi-group geometry.  Shown once with a library built without the `n_x = 0u` after a
    flush: this case still passes - the further candidates of its kept reads evidently do not sit in a group that another group of the
    workgroup follows -, while test_full_lds_candidate_list_then_a_next_group and the engineered blocks fail, and the older pair tests pass)"""
    fa, rd = planted
    kw = PLANTED_CONFIGS[cfg]
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA)
    try:
        sw = dict(er.BUCKET, GM_TRACE="1")
        base = go(ix, rd, kw, sw)
        off = go(ix, rd, kw, dict(sw, GM_VOTE_PAIR="0"))
        assert "k_vote_pair<" in base["path"] and "k_vote_pair" not in off["path"], (base["path"], off["path"])
        ores = _oracle_results(oracle, oracle.index_load(fa), oracle.params(**kw), rd) if cfg == "m14_j7" else None
        capfd.readouterr()
        for geo in PAIR_GEO:
            assert_pair_groups(len(rd), int(geo["GM_PAIR_CHUNK"]))
            o = go(ix, rd, kw, dict(sw, **geo))
            trace = capfd.readouterr().err
            assert o["path"] == base["path"]
            assert_same_run(o, base, (cfg, geo))
            for a, b in zip(o["raw"], off["raw"]):
                np.testing.assert_array_equal(a, b)
            assert o["ctr"]["candidates"] > 0 and o["flagged"] > 0
            if "max_kmer_hits" not in kw:
                attempts = [int(a) for a in re.findall(r"vote done: \d+ candidates \(attempt (\d+)\)", trace)]
                assert attempts and max(attempts) >= 1, trace[-2000:]
            if ores is not None:
                _compare(o["res"], ores, rd)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------------ b. DP kernels
NW_FORMS = {
    "rows": ({}, r" nw=k_nw_rows/(pairs|cells)$"),
    "rows_cells": (dict(GM_NW_CELLS="b32"), r" nw=k_nw_rows/cells$"),
    "lane": (dict(GM_NW="lane"), r" nw=k_nw_lane<(13|19)>$"),
    "lane_streaming": (dict(GM_NW="lane", GM_NW_ROWS="0"), r" nw=k_nw_lane<0>$"),
    "lane_lds": (dict(GM_NW="lane", GM_NW_ROWS="2"), r" nw=k_nw_lane<(13|19),lds>$"),
}


def _dp_block(L, illumina, tile, syn_reads):
    """(reads, until) of one length, `tile` copies in a row: the 330 edge reads (100 bases) or the 40 reads of 150 bases of syn.fq.
    illumina: --illumina keeps Phred+64 for the reads before the first one that shows a quality below '@' and uses Phred+33 from that
    read on.  The reads before `until`, a little past the middle of the block, get Phred+64 qualities (every character shifted up
    by 31: none below '@'), the reads from `until` on keep Phred+33 ones with characters below '@' (edge.fq has only 'I': every seventh
    becomes '5').  The candidates of one 32-read group share a shard, so a lane's successive candidates come from both parts"""
    rd = er.block_reads("edge") if L == 100 else [r for r in syn_reads if len(r[1]) == 150]
    assert len(rd) >= 40 and all(len(r[1]) == L for r in rd)
    rd = [(f"{n}/{k}", s, q) for k in range(tile) for n, s, q in rd]
    if not illumina:
        return rd, 0
    until = len(rd) // 2 + 3
    low = lambda q: bytes(ord("5") if j % 7 == 3 else c for j, c in enumerate(q)) if min(q) >= 64 else q
    rd = [(n, s, bytes(min(126, c + 31) for c in q) if i < until else low(q)) for i, (n, s, q) in enumerate(rd)]
    assert all(min(q) >= 64 for _, _, q in rd[:until]) and all(min(q) < 64 for _, _, q in rd[until:])
    return rd, until


_DP_ORACLE = {}


def _dp_oracle(oracle, o_ix, rd, until):
    """the oracle read by read, each read with the Phred table --illumina gives it (tests/test_gpu_nw_rows.py); a read's answer is kept"""
    ops = (oracle.params(), oracle.params(illumina=1))
    out = []
    for i, (_, s, q) in enumerate(rd):
        t = 1 if i < until else 0
        key = (id(o_ix), s, q, t)
        if key not in _DP_ORACLE:
            _DP_ORACLE[key] = oracle.map_read(o_ix, ops[t], oracle.pwm(s, q, illumina=t), s)
        out.append(_DP_ORACLE[key])
    return out


@pytest.mark.parametrize("illumina", [0, 1])
@pytest.mark.parametrize("L", [100, 150])
@pytest.mark.parametrize("form", list(NW_FORMS))
def test_dp_lanes_take_several_candidates(form, L, illumina, indexes, syn_ix, oracle, oix, syn_oix, syn_reads):
    """GM_NW_GRID 1 and 2: every lane of k_nw_rows / k_nw_lane takes three candidates and more, the last trip partial.  The reads are
    repeated until the block has some 2400 candidates.  With one Phred table and with two (the first half of the block
    Phred+64, the rest Phred+33: a lane that kept an earlier candidate's table scores the next one wrong): against the oracle read by
    read, each read with its table, and against the default geometry"""
    ix, o_ix = (indexes["full"], oix) if L == 100 else (syn_ix, syn_oix)
    kw = dict(illumina=1) if illumina else {}
    sw, shows = NW_FORMS[form]
    one = base_run(("dp1", L), lambda: go(ix, _dp_block(L, 0, 1, syn_reads)[0], {}, {}))
    tile = 2400 // one["ctr"]["candidates"] + 1                       # (some 1200 candidates on either side of the switch of tables)
    rd, until = _dp_block(L, illumina, tile, syn_reads)
    base = base_run(("dp", form, L, illumina), lambda: go(ix, rd, kw, sw))
    assert re.search(shows, base["path"]), base["path"]
    if form == "rows" and L == 100 and not illumina:
        assert base["path"].endswith(" nw=k_nw_rows/pairs"), base["path"]      # (the pair table, not a second cells run: tests/test_gpu_nw_pairs.py)
    ores = _dp_oracle(oracle, o_ix, rd, until)
    _compare(base["res"], ores, rd)
    if illumina:
        # both tables are in use: accepted hits of reads on either side of the switch, more than a trip's worth each at grid 1
        reads_hit = base["raw"][0]["read"]
        assert 0 < until < len(rd) and (reads_hit < until).sum() > 256 and (reads_hit >= until).sum() > 256
    for grid in (1, 2):
        o = go(ix, rd, kw, dict(sw, GM_NW_GRID=str(grid)))
        assert o["ctr"]["candidates"] > 2 * 256 * grid and o["ctr"]["candidates"] % (256 * grid) != 0, o["ctr"]
        assert o["path"] == base["path"]
        _compare(o["res"], ores, rd)
        assert_same_run(o, base, (form, L, illumina, grid))
        assert len(o["raw"][0]) > 200


@pytest.mark.parametrize("L", [300, 600])
def test_capped_prep_tiles(L, indexes, oracle, oix, genome):
    """k_prep (rows above 152 bytes): tiles of 64 reads staged in LDS at 300 bases, of 256 reads read directly at 600; the 984 reads of
    test_gpu_edge_windows.py's probes of that length through one and two workgroups.  Status and self score bits (what k_prep
    computes) and the hits are the oracle's"""
    pr = ew.probes(oix, genome, L, False)
    rd = [(f"p{i}", s, q) for i, (s, q) in enumerate(zip(pr["reads"], pr["quals"]))]
    stride = (L + 7) // 8 * 8
    tr = 49152 // (2 * stride)
    per = 256 if tr >= 256 or tr < 64 else tr // 64 * 64                # gmk_prep: reads per tile
    assert per == (64 if L == 300 else 256)
    ores = ef.oracle_results(oracle, oix, oracle.params(), rd)
    assert sum(x["status"] == 0 for x in ores) > 300
    base = go(indexes["full"], rd, {}, {})
    _compare(base["res"], ores, rd)
    for cap in (1, 2):
        assert cdiv(len(rd), per) > cap and len(rd) % per != 0          # a workgroup takes a later tile, the last tile partial
        o = go(indexes["full"], rd, {}, dict(GM_TEST_GRID_CAP=str(cap)))
        assert o["path"] == base["path"]
        _compare(o["res"], ores, rd)
        assert_same_run(o, base, (L, cap))


_BAND_ORACLE = {}


@pytest.mark.parametrize("form", ["wave", "M1", "M5", "M7"])
def test_capped_wave_and_band_dp(form, indexes, oracle, oix):
    """k_nw (GM_NW=wave: 32 candidates a trip) and k_nw_band (128 lanes) under GM_TEST_GRID_CAP 1 and 2"""
    rd = er.block_reads("edge")
    kw, sw, per_trip, shows = (({}, dict(GM_NW="wave"), 32, " nw=k_nw") if form == "wave" else (dict(max_gap=int(form[1:])), {}, 128, " nw=k_nw_band"))
    if form not in _BAND_ORACLE:
        _BAND_ORACLE[form] = ef.oracle_results(oracle, oix, oracle.params(**kw), rd)
    ores = _BAND_ORACLE[form]
    base = go(indexes["full"], rd, kw, sw)
    assert base["path"].endswith(shows), base["path"]
    _compare(base["res"], ores, rd)
    for cap in (1, 2):
        o = go(indexes["full"], rd, kw, dict(sw, GM_TEST_GRID_CAP=str(cap)))
        assert o["ctr"]["candidates"] > 2 * per_trip * cap, o["ctr"]
        assert o["path"] == base["path"]
        _compare(o["res"], ores, rd)
        assert_same_run(o, base, (form, cap))


@pytest.mark.parametrize("form", ["rows", "band"])
def test_superseded_candidates_followed_by_live_ones(form, planted, oracle):  # noqa: F811
    """the overflow and retry fixture of test_gpu_nw_loads.py (-m 6 -j 1 on the planted repeats: the candidates emitted before a vote
    table overflowed are superseded): with one and two workgroups a lane's `continue` over such a candidate is followed by a live one"""
    fa, reads = planted
    reads = reads[:24] + [r for r in reads if r[0].startswith("e")][::6]
    kw = dict(mer=6, jump=1, **(dict(max_gap=5) if form == "band" else {}))
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA)
    try:
        ores = _oracle_results(oracle, oracle.index_load(fa), oracle.params(**kw), reads)
        base = go(ix, reads, kw, {})
        assert ("nw=k_nw_rows" if form == "rows" else "nw=k_nw_band") in base["path"], base["path"]
        assert base["ctr"]["vote_retries"] > 0, base["ctr"]
        _compare(base["res"], ores, reads)
        for cap in (1, 2):
            o = go(ix, reads, kw, dict(GM_TEST_GRID_CAP=str(cap), GM_NW_GRID=str(cap)))
            per_trip = 256 if form == "rows" else 128
            assert o["ctr"]["candidates"] > 2 * per_trip * cap and o["ctr"]["vote_retries"] > 0, o["ctr"]
            assert o["path"] == base["path"]
            _compare(o["res"], ores, reads)
            assert_same_run(o, base, (form, cap))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------------ c. output path
def _outputs(ix, rd, kw, sw):
    """gm_output_batch, _text and _bam of one block, each on a mapping of its own, all under the switches"""
    p = g.Params(**kw)
    names = [r[0].encode() for r in rd]; seqs = [r[1] for r in rd]; quals = [r[2][:len(r[1])] for r in rd]
    B, Q, Ln = g.pack_reads(seqs, quals)
    with switches(**sw):
        batch = g.Batch(ix, len(rd), B.shape[1])
        try:
            ix.coverage_reset(8)
            res = batch.map(p, B, Q, Ln)
            hits = {k: res[k].copy() for k in ("status", "self_score", "top_score", "denominator", "match_begin", "matches")}
            recs, cigars = batch.output(p, res)
            text, row_off = batch.output_text(p, batch.map(p, B, Q, Ln), names)
            bam = batch.output_bam(p, batch.map(p, B, Q, Ln), names, level=1)
            out = dict(res=res, hits=hits, recs=recs.copy(), cigars=cigars, text=text, row_off=row_off, bam=bam, raw_len=batch.bam_raw_len, n_recs=batch.bam_n_recs,
                       p=p, names=names, seqs=seqs, quals=quals)
        finally:
            ix.coverage_reset(8)
            batch.destroy()
    return out


def _check_models(ix, o):
    """what the existing tests ask of the three outputs: the rows are the formatter's of test_gpu_sam_text.py over the records, the BAM
    records the model's of tests/bam_model.py over the rows"""
    check_text(ix, o["p"], o["seqs"], o["quals"], o["names"], o["recs"], o["cigars"], o["text"], o["row_off"])
    members = bm.parse_bgzf(o["bam"])
    raw = b"".join(pl for pl, _, _ in members)
    assert o["raw_len"] == len(raw) and o["n_recs"] == len(o["recs"])
    check_records(bm.split_records(raw), bm.sam_to_bam_records(o["text"], [(c, 0) for c, _ in ix.contigs()]))


def _same_outputs(o, base, what):
    for k in base["hits"]:
        assert same_bytes(o["hits"][k], base["hits"][k]), (what, k)
    assert same_bytes(o["recs"], base["recs"]) and o["cigars"] == base["cigars"], what
    assert o["text"] == base["text"] and o["row_off"].tobytes() == base["row_off"].tobytes(), what
    assert o["bam"] == base["bam"], what


@pytest.mark.parametrize("kw_name", ["default", "M5", "group"])
@pytest.mark.parametrize("n_reads", [64, 330, 660])
def test_capped_output_of_the_edge_reads(n_reads, kw_name, indexes, oracle, oix):
    """records, SAM rows and BAM of 64 and 330 edge reads, and of the 330 twice, with one and two workgroups for every output kernel:
    k_out_text_rows and k_bam_rows (4 records a trip), k_traceback_lane<128>, k_traceback (GM_TRACEBACK=group) and k_traceback_band
    (-M 5: launches of 128 and 256 items; 128 items a trip or launch: what the 660 reads are for); records and CIGARs are the oracle's"""
    rd = er.block_reads("edge")
    rd = rd[133:133 + 64] if n_reads == 64 else rd if n_reads == 330 else rd + [(n + "_again", s_, q) for n, s_, q in rd]
    assert len(rd) == n_reads
    kw = dict(max_gap=5) if kw_name == "M5" else {}
    sw = dict(GM_TRACEBACK="group") if kw_name == "group" else {}
    ix = indexes["full"]
    base = _outputs(ix, rd, kw, sw)
    _check_models(ix, base)
    op = oracle.params(**kw)
    want = []
    for i, (name, seq, qual) in enumerate(rd):
        _, orecs, _ = oracle.read_output(oix, op, oracle.pwm(seq, qual), seq)
        want += [(i, r["contig"], r["chr_pos"], r["strand"], r["mapq"], r["cigar"]) for r in orecs]
    got = [(int(r["read"]), int(r["contig"]), int(r["chr_pos"]), int(r["strand"]), int(r["mapq"]), c) for r, c in zip(base["recs"], base["cigars"])]
    assert got == want
    for cap in (1, 2):
        o = _outputs(ix, rd, kw, dict(sw, GM_TEST_GRID_CAP=str(cap)))
        assert len(o["recs"]) > 2 * 4 * cap                          # k_out_text_rows, k_bam_rows: a third trip
        if n_reads == 660:                                           # the traceback kernel (128 items a trip, -M 5: a launch): a later, partial one
            assert len(o["recs"]) > 128 * cap and len(o["recs"]) % (128 * cap) != 0
        _same_outputs(o, base, (n_reads, kw_name, cap))
        _check_models(ix, o)


@pytest.mark.parametrize("form", ["default", "big", "all_pairs"])
def test_capped_grouping_and_output_of_the_repeat_reads(form, rep, oracle, capfd):
    """the repeat fixture: k_group_multi / k_group_big and their writers take one read per workgroup and trip; with one and two workgroups
    every listed read but the first ones is a later trip.  Hits byte for byte those of the default geometry and the oracle's; records,
    rows and BAM byte for byte"""
    ix, roix = rep
    rd = rf.all_reads()
    fsw = dict(dict(default={}, big=dict(GM_GROUP_BIG_MIN="1"), all_pairs=dict(GM_GROUP_BIG_MIN="1000000"))[form], GM_TRACE="1")
    base = base_run(("rep", form), lambda: _outputs(ix, rd, {}, fsw))
    if "ores" not in _BASE:
        _BASE["ores"] = rf.oracle_results(oracle, roix, oracle.params(), rd)
    assert repeat_compare(base["res"], _BASE["ores"], rd) > 500
    _check_models(ix, base)
    capfd.readouterr()
    for cap in (1, 2):
        o = _outputs(ix, rd, {}, dict(fsw, GM_TEST_GRID_CAP=str(cap)))
        counts = set(GROUP_TRACE.findall(capfd.readouterr().err))
        assert len(counts) == 1, counts
        n_multi, n_big = (int(x) for x in list(counts)[0][2:4])
        if form == "big":
            assert n_big > 2 * cap
        elif form == "all_pairs":
            assert n_multi > 2 * cap and n_big == 0
        else:
            assert n_multi > 2 * cap and n_big > 2 * cap, (n_multi, n_big)
        assert len(o["recs"]) > 2 * 4 * cap
        _same_outputs(o, base, (form, cap))
    repeat_compare(o["res"], _BASE["ores"], rd)


TB_CASES = {"lane128": ("default", 100, 128), "lane64": ("default", 300, 64), "group": ("group", 100, 32), "group_long": ("default", 600, 8), "band": ("M5", 100, 128)}


@pytest.mark.parametrize("case", list(TB_CASES))
def test_capped_traceback_forms(case, indexes, oracle, oix, genome, capfd):
    """gm_dev_traceback on the edge windows of test_gpu_edge_windows.py (some 1000 probes of a length) with one and two workgroups:
    k_traceback_lane<128> and <64>, k_traceback with 32 and with 8 items a trip, k_traceback_band in launches of 128 and 256 items
    (every launch but the first with i0 > 0).  Operations and CIGARs are the oracle's"""
    form, L, per_trip = TB_CASES[case]
    sw, kw, fasta = ew.TB_FORMS[form]
    shows = ew.tb_kernel(sw, kw, L, fasta)
    pr, o = ew.want(oracle, oix, genome, L, kw.get("max_gap", 3), fasta, True)
    B, Q, Ln = g.pack_reads(pr["reads"], pr["quals"])
    n = len(pr["ridx"]) - 5                                          # (all but the last five probes: the last trip of every form is a partial one)
    for cap in (1, 2):
        assert n > 2 * per_trip * cap and n % (per_trip * cap) != 0
        capfd.readouterr()
        with switches(GM_TRACE="1", GM_TEST_GRID_CAP=str(cap), **sw):
            ops = indexes["full"].dev_traceback(g.Params(**kw), B, Q, Ln, pr["ridx"][:n], pr["strand"][:n], pr["pos"][:n])
        assert re.findall(r"dev_traceback: \d+ probes, traceback=(\S+)", capfd.readouterr().err) == [shows]
        assert len(ops) == n
        for k, t in enumerate(o["tb"][:n]):
            where = (cap, int(pr["pos"][k]), int(pr["strand"][k]), k % 8)
            if t is None:
                assert len(ops[k]) == 0, where
            else:
                assert len(ops[k]) == t[0] and ew.rle(ops[k]) == t[1], (where, ew.rle(ops[k]), t[1])


@pytest.mark.parametrize("adaptor", [AD34, AD34[:6]], ids=["a34", "a6"])
def test_capped_adaptor_trim(adaptor, syn_ix):
    """k_adaptor_trim: four reads a trip; the 551 reads of syn_adapt.fq through one and two workgroups, against the model"""
    seqs = [r[1] for r in read_fastq(GOLDEN + "/syn_adapt.fq")]
    B, _, Ln = g.pack_reads(seqs, [b"I" * len(s) for s in seqs])
    want = kept_lengths(seqs, adaptor)
    assert (np.asarray(want) != Ln).sum() > 50                       # the adaptor is there to be found
    for cap in (1, 2):
        assert len(seqs) > 2 * 4 * cap and len(seqs) % (4 * cap) != 0
        with switches(GM_TEST_GRID_CAP=str(cap)):
            np.testing.assert_array_equal(syn_ix.adaptor_trim(B, Ln, adaptor), want)


# ------------------------------------------------------------------------------------------------------------------------ d. scans
def _scan_values(n, kind):
    rng = np.random.default_rng(1000 + n % 9973)
    if kind == "random":                                             # a sixteenth of them 2^32 - 1: any 17 of those pass 2^32
        v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        v[rng.random(n) < 1 / 16] = 0xFFFFFFFF
    elif kind == "zero_runs":                                        # whole blocks and whole threads' runs of zeros between the values
        v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        for lo in range(0, n, 5000):
            v[lo:lo + 3000] = 0
    else:                                                            # ones only in the last block of 1024
        v = np.zeros(n, np.uint32)
        v[max(0, (n - 1) // 1024 * 1024):] = 1
    return v


@pytest.mark.parametrize("kind", ["random", "zero_runs", "last_block"])
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 1025, 3 * 2 ** 20 + 5])
def test_scan_u32_against_numpy(n, kind, syn_ix):
    """gmk_scan_u32 (the scan behind entry, hit, match, record, CIGAR, row and BGZF offsets): blocks of 1024 values, then ONE workgroup
    whose threads take ceil(blocks / 1024) block sums each - one up to 2^20 values, two and four above"""
    v = _scan_values(n, kind)
    want = np.zeros(n + 1, np.uint64)
    np.cumsum(v, dtype=np.uint64, out=want[1:])
    got = syn_ix.dev_scan_u32(v)
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (n, kind, [(int(k), int(got[k]), int(want[k])) for k in bad[:4]])
    if kind == "random" and n >= 1023:
        assert int(want[-1]) > 1 << 32
    if n > 2 ** 20:
        assert cdiv(cdiv(n, 1024), 1024) >= 2                        # a thread of k_scan_sums adds several block sums


def _fastq_text(n_rec, L, blank_from=None, bad_at=None):
    """n_rec records of L bases (names r<i>); from record blank_from on, 1 .. 3 blank lines in front of every seventh record (the phase
    in which a tile is entered changes from tile to tile); record bad_at has no '+' line"""
    rng = np.random.default_rng(n_rec + L)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n_rec, L))]
    qual = (33 + rng.integers(0, 41, (n_rec, L))).astype(np.uint8)
    out = []
    for i in range(n_rec):
        if blank_from is not None and i >= blank_from and i % 7 == 0:
            out.append(b"\n" * (1 + i % 3))
        plus = b"-\n" if i == bad_at else b"+\n"
        out.append(b"@r%d\n" % i + seq[i].tobytes() + b"\n" + plus + qual[i].tobytes() + b"\n")
    return b"".join(out)


FASTQ_TEXTS = {
    # name: (records, bases, blank lines from, malformed record, tiles > 1024, line tiles > 1024)
    "both_above_ok": (70000, 26, 36000, None, True, True),
    "both_above_bad_record": (70000, 26, 36000, 61003, True, True),
    "bytes_just_under": (65700, 25, 35000, None, False, True),
    "lines_just_under": (63000, 30, 33000, None, True, False),
}


@pytest.mark.parametrize("name", list(FASTQ_TEXTS))
def test_fastq_rows_of_texts_beyond_one_item_per_scan_thread(name, syn_ix):
    """gm_dev_fastq_rows against fastq_text_model.py on texts of more than 1024 tiles of 4096 bytes and more than 1024 tiles of 256 lines:
    the single-workgroup scans (k_rt_scan, k_rt_phase_scan) give every thread two tiles; blank lines and a malformed record in the second
    half change the phase within one thread's run of tiles.  One text just under each threshold"""
    n_rec, L, blank_from, bad_at, many_tiles, many_lines = FASTQ_TEXTS[name]
    text = _fastq_text(n_rec, L, blank_from, bad_at)
    tile = g.lib().gm_dev_fastq_tile_bytes()
    n_lines = text.count(b"\n")
    if many_tiles:
        assert cdiv(len(text), tile) > 1024
    else:
        assert 960 < cdiv(len(text), tile) <= 1024
    if many_lines:
        assert cdiv(n_lines, 256) > 1024
    else:
        assert 1000 < cdiv(n_lines, 256) <= 1024
    want = check_probe(syn_ix, text, name)
    if bad_at is None:
        assert want["status"] == FM.OK and want["n"] == n_rec
    else:
        assert want["status"] == FM.MALFORMED and want["n"] == bad_at > n_rec // 2
