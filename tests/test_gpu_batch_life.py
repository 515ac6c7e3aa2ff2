"""A gm_batch's whole life: unlike blocks through ONE handle, each compared with the same block through a fresh handle.

A handle carries about a hundred device buffers that never shrink and come back uninitialised when they grow, and host state that
outlives a call (launch stamps, kernel-form flags, capacities, the resume key, the adaptor, the read format).  Every other GPU test
makes a fresh Batch or repeats one block; here the blocks of tests/batch_life.py - other sizes, strides, read lengths, parameters,
kernel forms, formats - follow one another in three orders, and block k's result must not depend on what blocks 1 .. k-1 were.
Equality with the fresh handle is exact (same_run); the oracle anchors the fresh results, so both sides are not wrong together.  Each
life asserts from its own path() / counters() that the transitions it exists for happened.

Also here: gm_batch_upload's parameters against gm_map_batch_device's (the map call's own -m / -j size the seed rows; `illumina` is
bound by the upload and a mismatch is refused by name), the launch stamp of k_vote_bucket's own slots at the edges of its 32 bits
(test switch GM_TEST_EPOCH), and the same life for the output calls and the coverage tracks."""
import numpy as np
import pytest

import bam_model as bm
import batch_life as bl
import gnumap_amd as g
import repeat_fixture as rf
from gnumap_amd import api
from sam_sort_model import sort_rows
from sam_text_model import check_text
from test_gpu_bam import check_records
from test_gpu_pair_handoff import planted  # noqa: F401  (the planted-repeat fixture)
from test_gpu_sam_text import same_track

pytestmark = pytest.mark.gpu
ORDERS = ["listed", "reversed", "shuffled"]
BUCKET = dict(GM_SEED_BUCKET="1")        # the full-SA life runs with the bucket table forced (tests/test_gpu_bucket.py)
_FRESH = {}


@pytest.fixture(scope="module")
def world(syn_fa, syn_reads, oracle):
    full = g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)
    sampled = g.Index(syn_fa, flags=0)
    blocks, groups = bl.syn_groups(full, syn_reads, pipeline=True)
    w = dict(full=dict(ix=full, opts=BUCKET, blocks=blocks, groups=groups),
             sampled=dict(ix=sampled, opts={}, blocks=blocks, groups=[grp for grp in groups if not any(b.name.startswith("pipeline") for b in grp)]),
             oix=oracle.index_load(syn_fa))
    yield w
    full.close(); sampled.close()


@pytest.fixture(scope="module")
def repeat_world(planted, oracle):  # noqa: F811
    fa, reads = planted
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA)
    blocks, groups = bl.planted_groups(reads)
    yield dict(ix=ix, opts={}, blocks=blocks, groups=groups, oix=oracle.index_load(fa))
    ix.close()


@pytest.fixture(scope="module")
def genome_world(tmp_path_factory, oracle):
    fa = rf.build_index(tmp_path_factory)
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA)
    blocks, groups = bl.repeat_groups(rf.all_reads(), rf.T_KEYS)
    yield dict(ix=ix, opts={}, blocks=blocks, groups=groups, oix=oracle.index_load(fa))
    ix.close()


def fresh(key, env, blk):
    """the block's result through a fresh handle on this index: computed once, never changed"""
    if (key, blk.name) not in _FRESH:
        _FRESH[(key, blk.name)] = bl.fresh_block(env["ix"], blk, env["opts"])
    return _FRESH[(key, blk.name)]


def live(key, env, order):
    """the life: every block of the order through one handle made for the largest of them, each call equal to its fresh result"""
    seq = bl.ordered(env["groups"], order)
    batch = g.Batch(env["ix"], max(b.n for b in seq), max(b.stride for b in seq))
    calls = []
    try:
        for k, blk in enumerate(seq):
            got = bl.run_block(batch, blk, env["opts"])
            print(f"{key} {order} call {k}: {blk.name} n={blk.n} stride={blk.stride} path: {got['path']} flagged={got['flagged']} ctr={got['ctr']}")
            bl.same_run(got, fresh(key, env, blk), (key, order, k, blk.name, "after " + (seq[k - 1].name if k else "nothing")))
            calls.append(got)
    finally:
        batch.destroy()
    return seq, calls


def has(calls, *parts):
    return any(all(p in c["path"] for p in parts) for c in calls)


def assert_common_transitions(seq, calls, what):
    paths = [c["path"] for c in calls]
    for form in ("nw=k_nw_rows/pairs", "nw=k_nw_rows/cells", "nw=k_nw_lane", "nw=k_nw_band"):
        assert has(calls, form), (what, form, paths)
    assert any(p.endswith("nw=k_nw") for p in paths), (what, "nw=k_nw", paths)
    assert any(paths[k - 1].startswith("reads=fastq") and paths[k].startswith("reads=fasta") and paths[k + 1].startswith("reads=fastq")
               for k in range(1, len(paths) - 1)), (what, "a FASTA block between two FASTQ blocks", paths)
    sizes = [b.n for b in seq]
    assert any(sizes[k] > max(sizes[:k]) for k in range(1, len(sizes))), (what, "a block with more rows than every block before it", sizes)
    # the narrow block behind the wide one is back on the pairs table (the quality range is this call's)
    k = next(k for k, b in enumerate(seq) if b.name == "narrow")
    assert "nw=k_nw_rows/pairs" in paths[k], (what, paths[k])


# ---- 2. a block's result does not depend on the handle's past ------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_life_on_the_full_sa_index(order, world):
    seq, calls = live("full", world["full"], order)
    what = ("full", order)
    assert_common_transitions(seq, calls, what)
    paths = [c["path"] for c in calls]
    assert has(calls, "vote=k_vote_pair<", "cands=shards"), (what, "k_vote_pair with the direct hand-off", paths)
    assert has(calls, "vote=k_vote_pair<", "cands=own-slots"), (what, "k_vote_pair with the gather hand-off", paths)
    assert has(calls, "vote=k_vote_bucket<", "cands=own-slots"), (what, "k_vote_bucket alone, stamped own slots", paths)
    assert any(("vote=k_vote_tiny" in p or "vote=k_vote_slots" in p) and "cands=own-slots" in p for p in paths), (what, "a count-array own-slots form", paths)
    assert has(calls, "cands=shards"), (what, paths)
    k = next(k for k, b in enumerate(seq) if b.name == "pipeline")
    assert paths[k] == "", (what, paths[k])             # the sub-batches mapped it to the end: the single-pass dispatch, which records its choice, never ran
    assert "seeds=bucket-table" in paths[k - 1] and "seeds=bucket-table" in paths[k + 1], (what, "a bucket-table block on either side of the pipeline", paths[k - 1:k + 2])
    assert calls[k]["ctr"]["candidates"] > 0 and calls[k]["ctr"]["seeds_used"] > 0
    t = next(k for k, b in enumerate(seq) if b.name == "pipeline_tiled")                        # the pipeline gave up, the single pass mapped the block
    assert "seeds=k_seed" in paths[t] and "cands=" in paths[t], (what, paths[t])
    assert "seeds=bucket-table" in paths[t - 1] and "seeds=bucket-table" in paths[t + 1], (what, paths[t - 1:t + 2])
    # the calls that failed (same_run held the block behind each to its fresh handle): a bucket-table block on one side, the GM_VOTE=wave
    # block on the other
    for name in ("bad_qual", "illumina_refused", "pipeline_bad_qual"):
        k = next(k for k, b in enumerate(seq) if b.name == name)
        assert "failed" in calls[k], (what, name)
        around = {seq[k - 1].name: paths[k - 1], seq[k + 1].name: paths[k + 1]}
        assert set(around) == {"small", "wave_vote"}, (what, name, list(around))
        assert "seeds=bucket-table" in around["small"] and "seeds=k_seed vote=sparse" in around["wave_vote"], (what, name, around)


@pytest.mark.parametrize("order", ORDERS)
def test_life_on_the_sampled_sa_index(order, world):
    seq, calls = live("sampled", world["sampled"], order)
    assert_common_transitions(seq, calls, ("sampled", order))
    paths = [c["path"] for c in calls]
    assert all("seeds=k_seed" in p and "locate=sampled-SA" in p for p, b in zip(paths, seq) if b.n and not b.fails), paths
    assert all(c["ctr"]["lf_steps"] > 0 for c, b in zip(calls, seq) if b.n and not b.fails)
    assert sum("failed" in c for c in calls) == 2                       # bad_qual and illumina_refused: the blocks behind them are their fresh handles' (same_run)


@pytest.mark.parametrize("order", ORDERS)
def test_life_on_the_planted_repeat_index(order, repeat_world):
    seq, calls = live("planted", repeat_world, order)
    what = ("planted", order)
    names = [b.name for b in seq]
    retries = [c["ctr"]["vote_retries"] for c in calls]
    k = names.index("quiet")
    assert retries[k] == 0 and retries[k - 1] > 0 and retries[k + 1] > 0, (what, "retry, quiet, retry on other reads", names, retries)
    assert {names[k - 1], names[k + 1]} == {"overflow_a", "overflow_b"}
    assert names[k + 2] == "lane_after" and "nw=k_nw_lane" in calls[k + 2]["path"] and calls[k + 2]["ctr"]["accepted"] > 300, (what, calls[k + 2]["path"])
    assert has(calls, "cands=shards") and has(calls, "vote=k_vote_pair<"), (what, [c["path"] for c in calls])
    assert retries[names.index("retry_split")] > 0 and retries[names.index("heavy")] >= 0
    # cand_cap grown by one call and inherited by a later, smaller one: that call's candidates alone exceed what the later block would
    # have been given (16 n + 64 x 1024)
    cands = [c["ctr"]["candidates"] for c in calls]
    assert any(cands[i] > 16 * seq[j].n + 64 * 1024 and seq[j].n < seq[i].n for i in range(len(seq)) for j in range(i + 1, len(seq))), \
        (what, "candidates above a later block's initial capacity", list(zip(names, [b.n for b in seq], cands)))
    sizes = [b.n for b in seq]
    assert any(sizes[k] > max(sizes[:k]) for k in range(1, len(sizes))), (what, sizes)


@pytest.mark.parametrize("order", ORDERS)
def test_life_on_the_repeat_genome(order, genome_world):
    """reads with up to 3001 accepted hits: the grouping workspace and the raw hits of one block are many times the next block's"""
    seq, calls = live("repeat", genome_world, order)
    accepted = [c["ctr"]["accepted"] for c in calls]
    assert max(accepted) > 20 * min(a for a, b in zip(accepted, seq) if b.name == "rep_few"), accepted
    assert any(accepted[k] < accepted[k - 1] // 20 for k in range(1, len(seq))), (order, "a small result directly behind a large one", accepted)
    k = [b.name for b in seq].index("rep_L100")
    assert "nw=k_nw_rows" in calls[k]["path"] and "nw=k_nw_lane" in calls[k - 1]["path"] and "nw=k_nw_lane" in calls[k + 1]["path"]


def test_fresh_repeat_block_is_the_oracles(genome_world, oracle):
    blk = genome_world["blocks"]["rep_all"]
    assert bl.hold_to_oracle(fresh("repeat", genome_world, blk), oracle, genome_world["oix"], ("repeat", blk.name), blk) == bl.ORACLE_SAMPLE


@pytest.mark.parametrize("name", bl.ORACLE_BLOCKS_SYN)
@pytest.mark.parametrize("key", ["full", "sampled"])
def test_fresh_results_are_the_oracles(key, name, world, oracle):
    """the anchor: the fresh result every life call is compared with is the oracle's, read by read (at most 200 reads of the block)"""
    env = world[key]
    blk = env["blocks"][name]
    assert bl.hold_to_oracle(fresh(key, env, blk), oracle, world["oix"], ("syn", name), blk) >= min(blk.n, 100)


def test_fresh_overflow_block_is_the_oracles(repeat_world, oracle):
    blk = repeat_world["blocks"]["overflow_a"]
    run = fresh("planted", repeat_world, blk)
    assert run["ctr"]["vote_retries"] > 0
    bl.hold_to_oracle(run, oracle, repeat_world["oix"], ("planted", blk.name), blk)


# ---- 4. gm_batch_upload's parameters against gm_map_batch_device's ---------------------------------------------------------------------
def device_run(batch, blk, p_up, p_map):
    batch.upload(p_up, blk.B, blk.Q, blk.Ln)
    batch.map_device(p_map)
    raw, status, self_score, top = batch.raw_hits()
    return dict(raw=np.sort(raw, order=["read", "pos", "strand"]), status=status, self_score=self_score, top=top, path=batch.path(), ctr=batch.counters())


@pytest.mark.parametrize("up,mp", [({}, dict(jump=1)), ({}, dict(mer=6, jump=1)), (dict(jump=1), {}), (dict(mer=14), {})],
                         ids=["default_then_j1", "default_then_m6_j1", "j1_then_default", "m14_then_default"])
def test_map_call_reads_its_own_mer_and_jump(up, mp, world, oracle):
    """upload(p1) then map_device(p2): the seed rows are sized and clipped by p2's -m / -j, not by what the upload saw.  Equal to a fresh
    handle doing upload(p2) + map_device(p2), seeds_used and path() included, and that one is the oracle's under p2.
    Before gm_map_batch_device sized the rows itself the upload's max_seeds (20 for these rows at -m 10 -j 5) was used as it stood: with
    -j 1 the one-wave k_vote_tiny was chosen for 20 clipped seeds where k_vote takes some 90 (another path(), other candidates); with
    -m 6 -j 1 the form choice let a one-wave kernel in whose lanes take up to 64 seeds against rows and step masks
    made for 20 - an illegal memory access on the device, not a clipped result."""
    ix = world["full"]["ix"]
    one = world["full"]["blocks"]["one_len"]
    blk = bl.Block("one_len/" + repr(sorted(mp.items())), one.reads, mp)
    batch = g.Batch(ix, blk.n, blk.stride)
    try:
        got = device_run(batch, blk, g.Params(**up), blk.p)
    finally:
        batch.destroy()
    fb = g.Batch(ix, blk.n, blk.stride)
    try:
        want = device_run(fb, blk, blk.p, blk.p)
    finally:
        fb.destroy()
    print("upload", up, "map", mp, "path:", got["path"], "seeds_used", got["ctr"]["seeds_used"], "fresh:", want["path"], want["ctr"]["seeds_used"])
    anchor = bl.fresh_block(ix, blk)                                         # the same block through gm_map_batch: the oracle's, read by read
    bl.hold_to_oracle(anchor, oracle, world["oix"], ("syn", blk.name), blk)
    assert anchor["path"] == want["path"] and anchor["ctr"] == want["ctr"]
    same_device_run(anchor, want, status=False)                              # (gm_map_batch's grouping goes on to write statuses of its own)
    assert got["ctr"]["seeds_used"] == want["ctr"]["seeds_used"] and got["path"] == want["path"], (got["path"], want["path"], got["ctr"], want["ctr"])
    assert got["ctr"] == want["ctr"]
    same_device_run(got, want)


def same_device_run(a, b, status=True):
    assert len(a["raw"]) == len(b["raw"]) and len(a["raw"]) > 400
    for f in ("read", "pos", "strand", "step"):
        assert np.array_equal(a["raw"][f], b["raw"][f]), f
    assert np.array_equal(a["raw"]["score"].view(np.uint32), b["raw"]["score"].view(np.uint32))
    assert np.array_equal(bl.bits(a["top"]), bl.bits(b["top"])) and np.array_equal(bl.bits(a["self_score"]), bl.bits(b["self_score"]))
    if status:
        assert np.array_equal(a["status"], b["status"])


def test_illumina_is_bound_by_the_upload(world):
    """the fallback scan of --illumina read the quality rows at upload: a map call with the other value is refused, naming the field - for
    rows from the host and for a text block; a FASTA block ignores the field in both calls"""
    ix = world["full"]["ix"]
    b = world["full"]["blocks"]
    blk = b["ill_on"]
    p0, p1 = g.Params(), g.Params(illumina=1)
    batch = g.Batch(ix, 600, 160)
    try:
        for up, mp in ((p1, p0), (p0, p1)):
            batch.upload(up, blk.B, blk.Q, blk.Ln)
            with pytest.raises(g.GnumapError) as e:
                batch.map_device(mp)
            assert e.value.code == -1 and "illumina" in str(e.value), str(e.value)
            batch.map_device(up)                                             # the value it was uploaded under still maps
            assert batch.counters()["candidates"] > 0
        assert batch.upload_text(p1, blk.text())["n"] == blk.n
        with pytest.raises(g.GnumapError) as e:
            batch.map_text(p0)
        assert e.value.code == -1 and "illumina" in str(e.value), str(e.value)
        assert len(batch.map_text(p1)["matches"]) > 0
        fa = b["fasta"]
        batch.upload(p1, fa.B, None, fa.Ln, fasta=True)
        batch.map_device(p0)
        assert batch.counters()["candidates"] > 0
    finally:
        batch.destroy()


# ---- 5. the launch stamp at its edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0xFFFFFFFD, 0x7F7FFFFE, 0x007FFFFE], ids=["wrap", "into_inf_nan", "denormal_to_normal"])
def test_launch_stamp_at_the_edges_of_its_bits(start, world):
    """k_vote_bucket / k_vote_pair (gather) stamp a read x strand's slot 0 with the launch number in the bits of a float field, and
    k_cand_gather takes the slots whose stamp is this launch's.  GM_TEST_EPOCH starts the counter where five own-slot calls cross the
    NaN patterns and the 32-bit wrap (0xFFFFFFFE, 0xFFFFFFFF, memset and 1, 2, 3), run from the largest finite float into inf / NaN,
    and from the denormals into the normals.  A small block behind a large one: the slots beyond its 2 n keep older stamps"""
    env = world["full"]
    b = env["blocks"]
    seq = [b["one_len"], b["nopair_small"], b["narrow"], b["gather_small"], b["one_len"]]
    batch = g.Batch(env["ix"], 600, 160)
    try:
        with bl.Switches(dict(GM_TEST_EPOCH=str(start))):
            for k, blk in enumerate(seq):
                got = bl.run_block(batch, blk, env["opts"])
                assert "cands=own-slots" in got["path"] and "seeds=bucket-table" in got["path"], got["path"]      # a stamped call
                bl.same_run(got, fresh("full", env, blk), (hex(start), k, blk.name))
                assert got["ctr"]["candidates"] > blk.n // 2
    finally:
        batch.destroy()


# ---- 3. the output half of the life ---------------------------------------------------------------------------------------------------------
SINKS = ["records", "text", "bam1", "bam_lz", "resident", "sorter"]


def run_sink(ix, batch, blk, sink, unmapped=False, names=None):
    """one (block, sink) step: the sink's bytes as a tuple of comparable pieces, and what the step's checks need"""
    names = names or blk.names
    batch.set_unmapped_rows(unmapped)
    with bl.Switches(blk.opts):
        batch.set_adaptor(blk.adaptor)
        info = {}
        if sink in ("resident", "resident_cap"):
            assert batch.upload_text(blk.p, blk.text())["n"] == blk.n
            res = batch.map_text(blk.p, mcap=1, pcap=1) if sink == "resident_cap" else batch.map_text(blk.p)
            info["map_calls"] = batch.map_calls
            text, row_off = batch.output_text_resident(blk.p, res)
            out = (text, row_off.tobytes())
        else:
            res = batch.map(blk.p, blk.B, blk.Q, blk.Ln, fasta=blk.fasta)
            if sink == "records":
                recs, cigars = batch.output(blk.p, res)
                info["recs"], info["cigars"] = recs, cigars
                out = tuple(np.ascontiguousarray(recs[f]).tobytes() for f in recs.dtype.names) + (tuple(cigars),)
            elif sink == "text":
                text, row_off = batch.output_text(blk.p, res, names, blk.tails())
                out = (text, row_off.tobytes())
            elif sink in ("bam1", "bam_lz"):
                out = (batch.output_bam(blk.p, res, names, blk.tails(), level=1, lz77=sink == "bam_lz"), batch.bam_raw_len, batch.bam_n_recs)
            else:
                s = api.SamSorter(ix)
                try:
                    s.add_block(batch, blk.p, res, 0, names=names, qual_tails=blk.tails())
                    out = (s.finish(), s.text())
                finally:
                    s.destroy()
        info["unmapped_rows"] = batch.unmapped_rows() if sink != "records" else 0
        info["n_matches"] = len(res["matches"])
    return out, info


@pytest.fixture(scope="module")
def output_life(world, syn_fa):
    """the fixed sequence of (block, sink) steps on one handle of the full-SA index, and the same steps through fresh handles on a
    second index object; both coverage tracks behind them"""
    ix = world["full"]["ix"]
    ix2 = g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)
    b = world["full"]["blocks"]
    rng = np.random.default_rng(9)
    none = bl.Block("none", [(b"none%d" % i, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)), b"I" * 100) for i in range(64)])
    pall = bl.Block("print_all", b["mixed"].reads, dict(print_all_sam=1))
    other = [b"other_%d_" % i + nm for i, nm in enumerate(b["mixed"].names)]
    steps = [("one_len", "records", {}), ("one_len", "text", {}),
             ("small", "resident", {}), ("mixed", "text", dict(names=other)), ("small", "resident", {}),      # a text block, the caller's names, a text block
             ("mixed", "text", dict(unmapped=True)), ("mixed", "text", {}),                                   # unmapped rows on for one call, off for the next
             ("one_len", "bam1", {}), ("none", "bam1", {}),                                                   # records, then none
             ("one_len", "text", {}), ("M5", "text", {}), ("one_len", "records", {}),                         # another traceback form between two default blocks
             ("print_all", "text", {}), ("mixed", "text", {}),                                                # print_all_sam 1, then 0
             ("small", "resident_cap", {}), ("mixed", "records", {}),                                         # GM_E_CAPACITY and its repeat, then another block
             ("bs", "text", {}), ("one_len", "bam_lz", {}), ("one_len", "sorter", {}), ("mixed", "sorter", {})]
    blocks = dict(b, none=none, print_all=pall)
    for i in (ix, ix2):
        i.coverage_reset(8)
        i.coverage_enable_nuc()
    batch = g.Batch(ix, 600, 160)
    life, alone = [], []
    try:
        with bl.Switches(BUCKET):
            for name, sink, kw in steps:
                life.append(run_sink(ix, batch, blocks[name], sink, **kw))
                fb = g.Batch(ix2, max(blocks[name].n, 1), blocks[name].stride)
                try:
                    alone.append(run_sink(ix2, fb, blocks[name], sink, **kw))
                finally:
                    fb.destroy()
    finally:
        batch.destroy()
    out = dict(ix=ix, steps=steps, blocks=blocks, life=life, alone=alone, cov=(ix.coverage_download(), ix2.coverage_download()),
               nuc=(ix.coverage_download_nuc(), ix2.coverage_download_nuc()), contigs=[(c, 0) for c, _ in ix.contigs()])
    ix2.close()
    return out


def step_of(o, name, sink, **kw):
    return next(k for k, s in enumerate(o["steps"]) if s == (name, sink, kw))


@pytest.mark.parametrize("sink", SINKS)
def test_output_life_every_step_equals_its_fresh_handle(sink, output_life):
    o = output_life
    mine = [k for k, (_, s, _) in enumerate(o["steps"]) if s == sink or (sink == "resident" and s == "resident_cap")]
    assert mine
    for k in mine:
        (got, gi), (want, wi) = o["life"][k], o["alone"][k]
        assert len(got) == len(want)
        for i, (x, y) in enumerate(zip(got, want)):
            assert x == y, (k, o["steps"][k], "piece", i)
        assert gi["unmapped_rows"] == wi["unmapped_rows"] and gi["n_matches"] == wi["n_matches"], (k, o["steps"][k])
        if o["steps"][k][1] == "resident_cap":                            # first capacities too small: the call was repeated, on both sides
            assert gi["map_calls"] == 2 and wi["map_calls"] == 2


def test_output_life_holds_what_it_is_for(output_life):
    o = output_life
    on, off = step_of(o, "mixed", "text", unmapped=True), step_of(o, "mixed", "text")
    assert off == on + 1
    assert o["life"][on][1]["unmapped_rows"] > 0 and o["life"][off][1]["unmapped_rows"] == 0
    assert o["life"][on][0][0] != o["life"][off][0][0] and b"\tYU:i:" in o["life"][on][0][0] and b"\tYU:i:" not in o["life"][off][0][0]
    k = step_of(o, "none", "bam1")
    assert o["life"][k][0] == (b"", 0, 0) and o["life"][k - 1][0][2] > 100                                  # records, then none
    k = step_of(o, "small", "resident_cap")
    assert o["steps"][k + 1][0] != "small" and o["life"][k + 1][1]["n_matches"] != o["life"][k][1]["n_matches"]      # the next block was mapped, not resumed
    a, pa = step_of(o, "mixed", "text"), step_of(o, "print_all", "text")
    assert len(o["life"][pa][0][0]) > len(o["life"][a][0][0])
    other = step_of(o, "mixed", "text", names=[b"other_%d_" % i + nm for i, nm in enumerate(o["blocks"]["mixed"].names)])
    assert o["life"][other][0][0].startswith(b"other_") and o["steps"][other - 1][1] == "resident" and o["steps"][other + 1][1] == "resident"
    assert o["life"][other - 1][0] == o["life"][other + 1][0]                                              # the text block again: its own names


def test_output_life_against_the_cpu_models(output_life):
    """once per sink: the text rows are sam_rows of the records, the BAM records those of the text rows, the resident rows the rows of
    the host-cut block, the sorter's text the sorted rows"""
    o = output_life
    ix = o["ix"]
    one, mixed, small = o["blocks"]["one_len"], o["blocks"]["mixed"], o["blocks"]["small"]
    recs = o["life"][step_of(o, "one_len", "records")][1]
    text, row_off = o["life"][step_of(o, "one_len", "text")][0]
    check_text(ix, one.p, one.seqs, one.quals, one.names, recs["recs"], recs["cigars"], text, np.frombuffer(row_off, np.uint64))
    assert len(recs["recs"]) > 300
    want = bm.sam_to_bam_records(text, o["contigs"])
    for sink in ("bam1", "bam_lz"):
        out, raw_len, n_recs = o["life"][step_of(o, "one_len", sink)][0]
        raw = bm.bgzf_payload(out)
        assert raw_len == len(raw) and n_recs == len(want) and len(out) < len(raw)
        check_records(bm.split_records(raw), want)
    assert o["life"][step_of(o, "one_len", "bam_lz")][0][0] != o["life"][step_of(o, "one_len", "bam1")][0][0]
    # the resident rows of `small`: those of gm_output_batch_text on the rows a host cuts (a fresh handle; the tracks were read already)
    fb = g.Batch(ix, small.n, small.stride)
    try:
        res = fb.map(small.p, small.B, small.Q, small.Ln)
        want_text, want_off = fb.output_text(small.p, res, small.names, small.tails())
        r2, c2 = fb.output(small.p, res)
    finally:
        fb.destroy()
    got_text, got_off = o["life"][step_of(o, "small", "resident")][0]
    assert got_text == want_text and got_off == want_off.tobytes() and len(r2) > 30
    check_text(ix, small.p, small.seqs, small.quals, small.names, r2, c2, got_text, want_off)
    contigs = [c for c, _ in ix.contigs()]
    for blk, name in ((one, "one_len"), (mixed, "mixed")):
        t, ro = o["life"][step_of(o, name, "text")][0]
        ro = np.frombuffer(ro, np.uint64)
        rows = [t[int(ro[i]):int(ro[i + 1])].decode("latin-1") for i in range(len(ro) - 1)]
        (n_rows, n_bytes), sorted_text = o["life"][step_of(o, name, "sorter")][0]
        assert n_rows == len(rows) and n_bytes == len(t)
        assert sorted_text == "".join(sort_rows(rows, contigs)).encode("latin-1")


def test_output_life_deposits_every_step_once(output_life):
    """the coverage track behind the whole sequence against the same steps through fresh handles on a second index: fp32 atomic order
    is the only difference allowed (same_track); a deposit made twice or not at all is far outside it.  `bs` is in the sequence: the
    nucleotide tracks too"""
    cov, ref = output_life["cov"]
    same_track(cov, ref)
    nuc, nref = output_life["nuc"]
    same_track(nuc, nref)
