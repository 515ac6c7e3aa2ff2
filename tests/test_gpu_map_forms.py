"""The path() string of those branches of the map step's form choice (map_choose_form and map_form_name in gm_api.cpp) that no other test
file asserts.  Taken stock of before this file: tests/test_gpu_edge_reads.py restates the dispatch rules and holds GM_VOTE=wave|block|big|
rounds, GM_VOTE_KERNEL=block, GM_VOTE_SPARSE=0, GM_VOTE_FIXED=0, GM_SLOTS_PIPE, GM_VOTE_SLOTS in every slot class with GM_SEED_FUSED=0 and
1, the sampled-SA index and more than 64 seeds per strand (-j 1) to the exact string, the three bucket-table forms to a pattern;
test_gpu_adaptor.py the adaptor's k_seed; test_gpu_index_tables.py k_vote_pair<4> / <7> and k_vote_bucket<2> / <4>; the lives of
test_gpu_batch_life.py every nw= form.  Left over, and here: GM_VOTE_KERNEL=slots, the bucket table's <6> and <8> instantiations and
k_vote_pair<8> as literals, -h with the bucket table forced and under GM_VOTE=wave, the default form under each of these gm_params, and
the empty block's own path.

Every string is the one the build before the map step was cut into named steps printed for the same block; the raw hits of each form
are those of the block under the same gm_params with no switch set (computed once per gm_params)."""
import numpy as np
import pytest

import batch_life as bl
import gnumap_amd as g

pytestmark = pytest.mark.gpu
BUCKET = dict(GM_SEED_BUCKET="1")
# name -> (gm_params keywords, switches, path())
FORMS = {
    "kernel_slots": ({}, dict(GM_VOTE="rounds", GM_VOTE_KERNEL="slots", GM_VOTE_SLOTS="14"),
                     "reads=fastq seeds=k_seed vote=k_vote_slots locate=full-SA cands=shards nw=k_nw_rows/pairs"),
    "bucket6": ({}, BUCKET, "reads=fastq seeds=bucket-table (in the vote kernel) vote=k_vote_bucket<6> locate=full-SA cands=own-slots nw=k_nw_rows/pairs"),
    "bucket8_j3": (dict(jump=3), BUCKET, "reads=fastq seeds=bucket-table (in the vote kernel) vote=k_vote_bucket<8> locate=full-SA cands=own-slots nw=k_nw_rows/pairs"),
    "pair8_j6": (dict(jump=6), BUCKET,
                 "reads=fastq seeds=bucket-table (in the vote kernel) vote=k_vote_pair<8> + k_vote_bucket<4> locate=full-SA cands=shards nw=k_nw_rows/pairs"),
    "h30_bucket": (dict(max_kmer_hits=30), BUCKET,
                   "reads=fastq seeds=bucket-table (in the vote kernel) vote=k_vote_bucket<6> locate=full-SA cands=own-slots nw=k_nw_rows/pairs"),
    "h30_wave": (dict(max_kmer_hits=30), dict(GM_VOTE="wave"), "reads=fastq seeds=k_seed vote=sparse locate=full-SA cands=shards nw=k_nw_rows/pairs"),
}
# the same gm_params with no switch set: what the raw hits are compared with, and its own string
DEFAULTS = {
    (): "reads=fastq seeds=k_seed vote=k_vote_tiny locate=full-SA cands=own-slots nw=k_nw_rows/pairs",
    (("jump", 3),): "reads=fastq seeds=k_seed vote=k_vote_tiny2 locate=full-SA cands=own-slots nw=k_nw_rows/pairs",
    (("jump", 6),): "reads=fastq seeds=k_seed vote=k_vote_tiny locate=full-SA cands=own-slots nw=k_nw_rows/pairs",
    (("max_kmer_hits", 30),): "reads=fastq seeds=k_seed vote=k_vote_tiny locate=full-SA cands=own-slots nw=k_nw_rows/pairs",
}
_DEFAULT = {}


@pytest.fixture(scope="module")
def full(syn_fa):
    ix = g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def reads(syn_reads):
    return [r for r in syn_reads if len(r[1]) == 100][:200]


def default_run(ix, reads, kw):
    key = tuple(sorted(kw.items()))
    if key not in _DEFAULT:
        _DEFAULT[key] = bl.fresh_block(ix, bl.Block("default/" + repr(key), reads, kw))
    return key, _DEFAULT[key]


@pytest.mark.parametrize("name", list(FORMS))
def test_path_of_the_form_and_the_default_forms_raw_hits(name, full, reads):
    kw, sw, path = FORMS[name]
    key, want = default_run(full, reads, kw)
    got = bl.fresh_block(full, bl.Block(name, reads, kw, sw))
    print(f"{name}: path: {got['path']} | default {key}: {want['path']} | raw {len(got['raw'])} / {len(want['raw'])}")
    assert got["path"] == path, (got["path"], path)
    assert want["path"] == DEFAULTS[key], (want["path"], DEFAULTS[key])
    assert len(got["raw"]) == len(want["raw"]) > len(reads) // 2
    for f in ("read", "pos", "strand", "step"):
        assert np.array_equal(got["raw"][f], want["raw"][f]), f
    assert np.array_equal(got["raw"]["score"].view(np.uint32), want["raw"]["score"].view(np.uint32))


def test_path_of_the_empty_block(full, reads):
    """no kernel runs and the path says so, behind a block that had one - and the next block's is its own again"""
    blk = bl.Block("bucket6", reads, {}, BUCKET)
    batch = g.Batch(full, len(reads), blk.stride)
    try:
        assert bl.run_block(batch, blk)["path"] == FORMS["bucket6"][2]
        got = bl.run_block(batch, bl.Block("empty", []))
        assert got["path"] == "reads=fastq (empty block: no kernel)" and len(got["raw"]) == 0
        assert bl.run_block(batch, blk)["path"] == FORMS["bucket6"][2]
    finally:
        batch.destroy()
