"""Shared by tests/test_gpu_batch_life.py: the block catalogue of a gm_batch's life, one call of a block through a handle, and the exact
comparison of two such calls.

A BLOCK is everything one call on a handle can differ in: the reads, the gm_params keywords, the run-time switches set (gm_set_option)
for that call only, the read format, the adaptor.  Blocks are built once per module and never changed; a block may stand in a life
more than once.  A life is a list of GROUPS - blocks that have to stay neighbours (a FASTA block between two FASTQ blocks, an
overflowing block, a quiet one, an overflowing one) - so that an order can be reversed or shuffled without losing the transitions the
life exists for."""
import os

import numpy as np
import pytest

import fasta_model as fm
import gnumap_amd as g
from conftest import GOLDEN, read_fastq
from test_gpu_parity import _compare
from test_gpu_read_text import same_hits

SHUFFLE_SEED = 5
ORACLE_SAMPLE = 200                      # reads of a block the oracle answers for (evenly spaced over the block)
PIPE = 4096                              # GM_PIPELINE's smallest sub-batch; the pipeline starts at three of them


class Block:
    def __init__(self, name, reads, kw=None, opts=None, fasta=False, adaptor=None, stride=None, fails=None, upload_kw=None):
        """reads: (name, sequence, quality line) triples; kw: gm_params keywords; opts: {switch: value} for this block's calls only.
        fails: (error code, a part of its text) - the block is uploaded (under upload_kw where the upload's gm_params differ from the map
        call's) and gm_map_batch_device has to return that error; the handle then goes on to the next block"""
        self.name, self.reads, self.kw, self.opts, self.fasta, self.adaptor = name, list(reads), dict(kw or {}), dict(opts or {}), fasta, adaptor
        self.fails, self.up = fails, g.Params(**(kw if upload_kw is None else upload_kw) or {})
        self.n = len(self.reads)
        self.names = [r[0] if isinstance(r[0], bytes) else str(r[0]).encode() for r in self.reads]
        self.seqs = [r[1] for r in self.reads]
        self.quals = None if fasta else [r[2] for r in self.reads]
        self.B, self.Q, self.Ln = g.pack_reads(self.seqs, None if fasta else [q[:len(s)] for s, q in zip(self.seqs, self.quals)], stride)
        self.stride = self.B.shape[1]
        self.p = g.Params(**self.kw)

    def tails(self):
        t = None if self.fasta else [q[len(s):] for s, q in zip(self.seqs, self.quals)]
        return t if t and any(t) else None

    def text(self):
        return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(self.names, self.seqs, self.quals))


class Switches:
    """the switches of one call, back to the environment's when the call is over"""

    def __init__(self, *dicts):
        self.opts = {}
        for d in dicts:
            self.opts.update(d)

    def __enter__(self):
        for k, v in self.opts.items():
            g.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            g.set_option(k, None)


def run_block(batch, blk, life_opts=None):
    """the block through this handle: gm_map_batch (upload + gm_map_batch_device + grouping), then what the handle says about the call"""
    with Switches(life_opts or {}, blk.opts):
        batch.set_adaptor(blk.adaptor)
        if blk.fails:
            return failed_call(batch, blk)
        res = batch.map(blk.p, blk.B, blk.Q, blk.Ln, fasta=blk.fasta)
        raw, status, self_score, top = batch.raw_hits()
        return dict(res=res, raw=np.sort(raw, order=["read", "pos", "strand"]), status=status, self_score=self_score, top=top, path=batch.path(),
                    flagged=batch.pair_flagged(), ctr=batch.counters(), n=blk.n, name=blk.name)


def failed_call(batch, blk):
    """a map call that returns an error is part of the life too: the upload goes through, gm_map_batch_device raises blk.fails - before
    its first launch (the `illumina` binding) or behind the vote kernels (a quality character below the offset) - and whatever it had
    set up by then is the next block's inheritance"""
    code, text = blk.fails
    batch.upload(blk.up, blk.B, blk.Q, blk.Ln, fasta=blk.fasta)
    with pytest.raises(g.GnumapError) as e:
        batch.map_device(blk.p)
    assert e.value.code == code and text in str(e.value), (blk.name, str(e.value))
    return dict(failed=str(e.value), path="(" + text + ")", flagged=0, ctr={}, n=blk.n, name=blk.name)


def fresh_block(ix, blk, life_opts=None):
    """the block through a handle that has seen nothing else, sized for this block alone"""
    batch = g.Batch(ix, max(blk.n, 1), blk.stride)
    try:
        return run_block(batch, blk, life_opts)
    finally:
        batch.destroy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_run(a, b, what):
    """exact: raw hits by (read, pos, strand) with their steps and score bits, status, self / top score bits, the path, the flagged reads,
    every counter, and the grouped result field by field (same_hits of test_gpu_read_text.py).  No counter is left out: gm_map_batch_device
    zeroes the work counters per call (the hipMemsetAsync of `counters` in front of k_prep, those of the fused seed search and of
    GMK_OVERFLOW_RS per attempt), the sub-batch pipeline sums its own per call, and an empty block reports zeros"""
    assert a["n"] == b["n"], what
    if "failed" in a or "failed" in b:                   # a refused call: refused in the same words on the fresh handle, and nothing else to compare
        assert a.get("failed") == b.get("failed"), (what, a.get("failed"), b.get("failed"))
        return
    assert len(a["raw"]) == len(b["raw"]), (what, len(a["raw"]), len(b["raw"]))
    for f in ("read", "pos", "strand", "step"):
        assert np.array_equal(a["raw"][f], b["raw"][f]), (what, "raw", f)
    assert np.array_equal(a["raw"]["score"].view(np.uint32), b["raw"]["score"].view(np.uint32)), (what, "raw score bits")
    assert np.array_equal(a["status"], b["status"]), (what, "status")
    assert np.array_equal(bits(a["self_score"]), bits(b["self_score"])), (what, "self score bits")
    assert np.array_equal(bits(a["top"]), bits(b["top"])), (what, "top score bits")
    assert a["path"] == b["path"], (what, a["path"], b["path"])
    assert a["flagged"] == b["flagged"], (what, "pair_flagged", a["flagged"], b["flagged"])
    assert a["ctr"] == b["ctr"], (what, a["ctr"], b["ctr"])
    same_hits(a["res"], b["res"], what)


# ---- the oracle as the anchor: both sides equal AND right --------------------------------------------------------------------------
def sample(n):
    return list(range(n)) if n <= ORACLE_SAMPLE else sorted(set(int(x) for x in np.linspace(0, n - 1, ORACLE_SAMPLE)))


def subset(res, idx):
    """the grouped result of the reads idx as a result of its own (positions stay where they are: matches index into them)"""
    mb = res["match_begin"]
    parts = [res["matches"][int(mb[i]):int(mb[i + 1])] for i in idx]
    nmb = np.zeros(len(idx) + 1, np.uint64)
    nmb[1:] = np.cumsum([len(x) for x in parts])
    return dict(status=res["status"][idx], self_score=res["self_score"][idx], top_score=res["top_score"][idx], denominator=res["denominator"][idx],
                match_begin=nmb, matches=np.concatenate(parts) if parts else res["matches"][:0], positions=res["positions"])


_ORACLE = {}


def oracle_answers(oracle, oix, key, blk, kept=None):
    """the oracle's results for the sampled reads of a block, computed once per (index, block).  kept: the lengths an adaptor trim left"""
    if key not in _ORACLE:
        op = oracle.params(**blk.kw)
        idx = sample(blk.n)
        out = []
        for i in idx:
            s = blk.seqs[i] if kept is None else blk.seqs[i][:int(kept[i])]
            if blk.fasta:
                P = fm.pwm_rows(s) if len(s) else np.zeros((1, 4), np.float32)
            else:
                P = oracle.pwm(s, blk.quals[i][:len(s)]) if len(s) else np.zeros((1, 4), np.float32)
            out.append(oracle.map_read(oix, op, P, s))
        _ORACLE[key] = (idx, out)
    return _ORACLE[key]


def hold_to_oracle(run, oracle, oix, key, blk):
    idx, ores = oracle_answers(oracle, oix, key, blk)
    _compare(subset(run["res"], idx), ores, [blk.reads[i] for i in idx])
    return len(idx)


# ---- orders --------------------------------------------------------------------------------------------------------------------------
def ordered(groups, order):
    """the blocks of a life: as listed, reversed (the whole list, so every neighbourhood is kept, the other way round), or the groups
    shuffled with a fixed seed"""
    if order == "listed":
        gs = groups
    elif order == "reversed":
        return [b for grp in groups for b in grp][::-1]
    else:
        gs = [groups[i] for i in np.random.default_rng(SHUFFLE_SEED).permutation(len(groups))]
    return [b for grp in gs for b in grp]


# ---- the catalogue on tests/golden/syn.fa -------------------------------------------------------------------------------------------------
def first_low_quality_read(reads):
    """--illumina's fallback point: the first read that shows a quality below '@' (SeqReader.cpp:1171-1180)"""
    for i, (_, s, q) in enumerate(reads):
        if any(c < 64 for c in q[:len(s)]):
            return i
    return len(reads)


def syn_groups(ix, syn_reads, pipeline):
    """pipeline: with the one block above 600 reads (3 x 4096 + 100, GM_PIPELINE's own threshold) - only the full-SA path cuts a block into
    sub-batches (`use_full && sub_n >= 4096` in gm_map_batch_device), so the sampled-SA life leaves it out"""
    from test_gpu_adaptor import AD34
    from test_gpu_nw_pairs import _reads_from_reference
    by_len = lambda L: [r for r in syn_reads if len(r[1]) == L]
    one = by_len(100)
    small = by_len(50)
    assert len(one) == 427 and len(syn_reads) == 551 and len(small) == 60
    b = {}
    b["one_len"] = Block("one_len", one)
    b["mixed"] = Block("mixed", syn_reads)
    b["small"] = Block("small", small)
    # one copy of `mixed` is all that fits below 600 reads: filled up from one_len, and a row stride no other block has
    b["grown"] = Block("grown", list(syn_reads) + one[:600 - len(syn_reads)], stride=b["mixed"].stride + 8)
    b["empty"] = Block("empty", [])
    wide = _reads_from_reference(ix, 300, 100, ord("@"), ord("h"), seed=65)                        # test_wide_two_table_block_falls_back_to_cells
    wide = wide[:100] + [(nm, s, bytes([ord("!")]) + q[1:-1] + b"~") for nm, s, q in wide[100:]]
    b["wide_qual"] = Block("wide_qual", wide, dict(illumina=1))
    b["narrow"] = Block("narrow", one[::-1])
    ill = read_fastq(os.path.join(GOLDEN, "syn_ill.fq"))
    cut = first_low_quality_read(ill)
    assert 0 < cut < len(ill) and len(ill) <= 600
    b["ill_on"] = Block("ill_on", ill[:cut], dict(illumina=1))
    b["ill_off"] = Block("ill_off", ill[cut:], dict(illumina=0))
    b["M5"] = Block("M5", syn_reads, dict(max_gap=5))
    b["no_nw"] = Block("no_nw", one, dict(nw=0))
    b["bs"] = Block("bs", syn_reads, dict(mode=1))
    b["m8_j5"] = Block("m8_j5", syn_reads, dict(mer=8, jump=5))
    b["u"] = Block("u", one, dict(unique_only=1, nw=0))
    fa = fm.parse_fasta(open(os.path.join(GOLDEN, "syn_reads_u100.fa"), "rb").read())
    b["fasta"] = Block("fasta", [(nm, s, b"") for nm, s in fa], fasta=True)
    ad = read_fastq(os.path.join(GOLDEN, "syn_adapt.fq"))
    assert len(ad) <= 600
    b["adaptor"] = Block("adaptor", ad, adaptor=AD34)
    b["adaptor_off"] = Block("adaptor_off", ad)
    b["lane"] = Block("lane", one, opts=dict(GM_NW="lane"))
    b["wave"] = Block("wave", one, opts=dict(GM_NW="wave"))
    # the switches of k_vote_pair on one_len as listed - its 100-base reads have 18 seed positions per strand, more than the 16 the pair
    # kernel takes (`max_reg <= 16`), so they run k_vote_bucket alone - and on `small` (8 positions), where the pair kernel runs
    b["gather"] = Block("gather", one, opts=dict(GM_PAIR_HANDOFF="gather"))
    b["fixed0"] = Block("fixed0", one, opts=dict(GM_VOTE_FIXED="0"))
    b["nopair"] = Block("nopair", one, opts=dict(GM_VOTE_PAIR="0"))
    b["gather_small"] = Block("gather_small", small, opts=dict(GM_PAIR_HANDOFF="gather"))
    b["nopair_small"] = Block("nopair_small", small, opts=dict(GM_VOTE_PAIR="0"))
    b["slots"] = Block("slots", one, opts=dict(GM_VOTE="block"))                                  # a count-array own-slots form beside the bucket table
    # calls that fail: behind the vote kernels (one quality character below the offset: "Invalid Fastq Character") and in front of every
    # launch (`illumina` other than the upload's).  Behind a bucket-table block and in front of a GM_VOTE=wave block of more reads: what the
    # failed or the earlier call chose - 2-bit read forms, own candidate slots, sized for 60 or 40 reads - is not the wave block's
    spoil = lambda reads, at: [(nm, s, q[:7] + b" " + q[8:]) if i == at else (nm, s, q) for i, (nm, s, q) in enumerate(reads)]
    b["bad_qual"] = Block("bad_qual", spoil(one[:40], 17), fails=(-8, "Invalid Fastq Character"))
    b["illumina_refused"] = Block("illumina_refused", one[:40], dict(illumina=1), upload_kw={}, fails=(-1, "illumina"))
    b["wave_vote"] = Block("wave_vote", one, opts=dict(GM_VOTE="wave"))
    groups = [[b["small"], b["bad_qual"], b["wave_vote"]], [b["small"], b["illumina_refused"], b["wave_vote"]]]
    groups += [[b["one_len"]], [b["mixed"]], [b["small"]], [b["grown"]], [b["empty"]], [b["wide_qual"], b["narrow"]], [b["ill_on"], b["ill_off"]],
              [b["M5"]], [b["bs"]], [b["m8_j5"]], [b["no_nw"], b["fasta"], b["u"]], [b["adaptor"], b["adaptor_off"]], [b["lane"]], [b["wave"]],
              [b["gather"]], [b["fixed0"]], [b["nopair"]], [b["gather_small"]], [b["nopair_small"]], [b["slots"]]]
    if pipeline:
        # one_len tiled: 29 copies of every read vote for the same places, one candidate shard of a sub-batch overflows, map_pipelined gives
        # up (returns 1) and the single pass maps the block - the fall-through behind a started pipeline.  Distinct reads cut from the
        # reference (the block of test_sub_batch_pipeline_pairs_against_cells) stay in the sub-batches to the end.
        reps = (3 * PIPE + 100 + len(one) - 1) // len(one)
        b["pipeline_tiled"] = Block("pipeline_tiled", (one * reps)[:3 * PIPE + 100], opts=dict(GM_PIPELINE=str(PIPE)))
        b["pipeline"] = Block("pipeline", _reads_from_reference(ix, 3 * PIPE + 100, 100, ord("#"), ord("F"), seed=11), opts=dict(GM_PIPELINE=str(PIPE)))
        groups.append([b["small"], b["pipeline"], b["small"], b["pipeline_tiled"], b["small"]])       # a bucket-table block on either side in every order
        # the bad quality character met by the sub-batches (map_pipelined's own check, in the first of them)
        b["pipeline_bad_qual"] = Block("pipeline_bad_qual", spoil(b["pipeline"].reads, 5), opts=dict(GM_PIPELINE=str(PIPE)), fails=(-8, "Invalid Fastq Character"))
        groups.append([b["small"], b["pipeline_bad_qual"], b["wave_vote"]])
    return b, groups


ORACLE_BLOCKS_SYN = ("one_len", "mixed", "M5", "bs", "m8_j5", "fasta")


# ---- the catalogue on the repeat genome of tests/repeat_fixture.py ---------------------------------------------------------------------------
def repeat_groups(reads, t_keys):
    """reads with 2 .. 3001 accepted hits each, of many lengths: the grouping workspace (g_*) and the raw-hit buffer grow and are
    reused at other sizes from block to block; the retry and heavy paths run on repeat families"""
    assert len(reads) <= 600
    L100 = [r for r in reads if len(r[1]) == 100]
    b = {}
    b["rep_all"] = Block("rep_all", reads)
    b["rep_odd"] = Block("rep_odd", reads[:0:-1])                                                  # the other way round, an odd count
    b["rep_L100"] = Block("rep_L100", L100)
    b["rep_T"] = Block("rep_T", reads, dict(max_matches=t_keys))
    b["rep_u_no_nw"] = Block("rep_u_no_nw", reads, dict(unique_only=1, nw=0))
    b["rep_overflow"] = Block("rep_overflow", reads[:40], dict(mer=6, jump=1))
    b["rep_heavy"] = Block("rep_heavy", reads, opts=dict(GM_HEAVY_MIN="8", GM_HEAVY_BUDGET="200000"))
    b["rep_few"] = Block("rep_few", reads[:12])                                                   # the two-copy family: two dozen hits
    groups = [[b["rep_few"], b["rep_all"], b["rep_few"]], [b["rep_overflow"], b["rep_L100"], b["rep_overflow"]], [b["rep_T"]], [b["rep_u_no_nw"], b["rep_odd"]],
              [b["rep_few"], b["rep_heavy"], b["rep_few"]]]
    return b, groups


# ---- the catalogue on the planted-repeat reference (tests/test_gpu_pair_handoff.py) ----------------------------------------------------
def planted_groups(reads):
    bucket14 = dict(GM_SEED_BUCKET="1", GM_KMER_TABLE="14")
    over = reads[:24] + [r for r in reads if r[0].startswith("e")][::6]                            # test_whole_path_with_and_without_superseded_candidates
    plain = [r for r in reads if r[0].startswith(("iid", "tail"))]
    repeats = reads[:24] + [r for r in reads if r[0].startswith("e")]
    assert len(reads) <= 600
    b = {}
    b["overflow_a"] = Block("overflow_a", over, dict(mer=6, jump=1))
    b["overflow_b"] = Block("overflow_b", over[::-1], dict(mer=6, jump=1))
    b["quiet"] = Block("quiet", plain, dict(mer=14, jump=7), bucket14)
    # k_nw_rows loads a flagged candidate's rs_overflow byte only when the retry or heavy path ran; k_nw_lane loads it always: the quiet
    # reads again under GM_NW=lane, behind the second overflowing block - a byte left at 1 passes a good candidate over
    b["lane_after"] = Block("lane_after", plain, dict(mer=14, jump=7), dict(bucket14, GM_NW="lane"))
    b["shard_grow"] = Block("shard_grow", reads, dict(mer=14, jump=7), bucket14)                  # test_direct_handoff_equals_gather[m14_j7]
    b["after_grow"] = Block("after_grow", plain[:40], dict(mer=14, jump=7), bucket14)
    b["heavy"] = Block("heavy", repeats, dict(mer=6, jump=1), dict(GM_HEAVY_MIN="8", GM_HEAVY_BUDGET="200000"))
    b["retry_split"] = Block("retry_split", over, dict(mer=6, jump=1), dict(GM_VOTE="block", GM_VOTE_KERNEL="block", GM_RETRY_BUDGET="16384"))
    groups = [[b["lane_after"], b["overflow_a"], b["quiet"], b["overflow_b"], b["lane_after"]], [b["shard_grow"], b["after_grow"]], [b["heavy"]],
              [b["retry_split"]]]
    return b, groups
