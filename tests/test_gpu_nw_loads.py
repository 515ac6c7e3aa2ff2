"""k_nw_rows' load group (gm_nw.hip): a candidate's read row (16-byte pieces, clamped into the row), its packed window (16-byte pieces,
clamped into the reference), its min_score and - only when the retry or heavy path ran - its rs_overflow byte are requested together,
before anything is tested.  These are the shapes at which the clamps and the piece arithmetic can go wrong: every row stride a length
can come with (padding that must never be read as data), a row that ends where the buffer does, windows at both ends of the reference
and beyond it, superseded candidates, FASTA rows.  Score bits are k_nw_lane's and the oracle's."""
import ctypes as C
import re

import numpy as np
import pytest

import gnumap_amd as g
from reflib import revcomp_pwm
from test_gpu_pair_handoff import CONFIGS, planted  # noqa: F401  (the planted-repeat fixture)
from test_gpu_parity import _compare, _oracle_results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ix_full(syn_fa):
    return g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)


@pytest.fixture(scope="module")
def oix(oracle, syn_fa):
    return oracle.index_load(syn_fa)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cut(syn_reads, L, n):
    return [(nm, s[:L], q[:L]) for nm, s, q in syn_reads if len(s) >= L][:n]


def _block(reads, L, stride):
    """the reads at this row stride, the padding of both arrays filled with 0xFF: padding read as data changes a score"""
    B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads], stride)
    B[:, L:] = 0xFF; Q[:, L:] = 0xFF
    return B, Q, Ln


def _score(ix, B, Q, Ln, ridx, strand, pos, lane=False, fasta=False, capfd=None):
    """gm_dev_nw_score with the default kernel choice (k_nw_rows, proved by the trace when capfd is given) or with GM_NW=lane"""
    if lane:
        g.set_option("GM_NW", "lane")
    if capfd is not None:
        capfd.readouterr()
        g.set_option("GM_TRACE", "1")
    try:
        out = ix.dev_nw_score(g.Params(), B, Q, Ln, ridx, strand, pos, fasta=fasta)
    finally:
        g.set_option("GM_NW", None)
        g.set_option("GM_TRACE", None)
    if capfd is not None:
        form = re.findall(r"dev_nw_score: \d+ probes, nw=(\S+)", capfd.readouterr().err)
        assert form and all(f.startswith("k_nw_lane" if lane else "k_nw_rows") for f in form), form
    return out


def _oracle_score(oracle, oix, op, read, strand, pos, L):
    P = oracle.pwm(read[1], read[2])
    if strand:
        P = revcomp_pwm(P)
    w = oracle.window(oix, int(pos), L)
    return np.float32(oracle.lib.gmo_nw_score(C.byref(op), np.ascontiguousarray(P, np.float32), L, w))


def _probes(n_reads, L, seed, per_read=16):
    """per read: consecutive starts (all 16 phases of the packed reference word), alternating strands"""
    rng = np.random.default_rng(seed)
    ridx, strand, pos = [], [], []
    for k in range(n_reads):
        base = int(rng.integers(0, 140000 - L))
        for d in range(per_read):
            ridx.append(k); strand.append((k + d) & 1); pos.append(base + d)
    return np.array(ridx, np.uint32), np.array(strand, np.uint8), np.array(pos, np.uint64)


WIDER = {L: (0, 8, 16, 48) for L in (24, 29, 33, 41, 56, 97, 100, 104)}
WIDER.update({L: (0, 8, 16) for L in (105, 113, 150)})


@pytest.mark.parametrize("L", sorted(WIDER))
def test_every_row_stride(L, ix_full, oracle, oix, syn_reads, capfd):
    """the same reads at the smallest stride (L rounded up to 8) and at wider ones: the last piece of a row is clamped to stride - 16,
    so where its chunks arrive depends on the stride; the padding (0xFF) is never data"""
    reads = _cut(syn_reads, L, 12)
    assert len(reads) == 12
    ridx, strand, pos = _probes(len(reads), L, L)
    s0 = (L + 7) // 8 * 8
    want, valid_lane = _score(ix_full, *_block(reads, L, s0), ridx, strand, pos, lane=True, capfd=capfd)
    assert valid_lane.all()
    op = oracle.params()
    for k in range(0, len(ridx), 5):
        assert bits(want[k]) == bits(_oracle_score(oracle, oix, op, reads[ridx[k]], strand[k], pos[k], L)), (L, k)
    for extra in WIDER[L]:
        score, valid = _score(ix_full, *_block(reads, L, s0 + extra), ridx, strand, pos, capfd=capfd)
        assert valid.all(), (L, extra)
        np.testing.assert_array_equal(bits(score), bits(want), err_msg=f"L={L} stride={s0 + extra}")


@pytest.mark.parametrize("L,stride", [(25, 32), (100, 104)])
def test_last_row_of_the_buffer(L, stride, ix_full, oracle, oix, syn_reads, capfd):
    """every candidate refers to the LAST read of the block: its row ends where the uploaded arrays end, on both strands.  (The device
    buffer is allocated with slack, so a read past the row would not fault here: what this pins is that nothing behind the row's L
    bytes - its 0xFF padding included - is taken as data when the last piece is clamped to stride - 16)"""
    reads = _cut(syn_reads, L, 9)
    B, Q, Ln = _block(reads, L, stride)
    last = len(reads) - 1
    starts = np.arange(5000, 5000 + 34, dtype=np.uint64)
    pos = np.concatenate([starts, starts]); strand = np.repeat(np.array([0, 1], np.uint8), len(starts)); ridx = np.full(len(pos), last, np.uint32)
    score, valid = _score(ix_full, B, Q, Ln, ridx, strand, pos, capfd=capfd)
    want, _ = _score(ix_full, B, Q, Ln, ridx, strand, pos, lane=True)
    assert valid.all()
    np.testing.assert_array_equal(bits(score), bits(want))
    op = oracle.params()
    for k in range(0, len(pos), 3):
        assert bits(score[k]) == bits(_oracle_score(oracle, oix, op, reads[last], strand[k], pos[k], L)), (L, k)


@pytest.mark.parametrize("L", [24, 100, 150])
def test_windows_at_the_ends_of_the_reference(L, ix_full, oracle, oix, syn_reads, capfd):
    """starts 0 .. 20 of the first contig (the window's words are clamped to word 0 and moved up), the last 20 valid starts of the last
    contig (its last word is the reference's last) and starts beyond: invalid, score 0, no load outside the packed reference"""
    reads = _cut(syn_reads, L, 6)
    B, Q, Ln = _block(reads, L, (L + 7) // 8 * 8 + 8)
    l_pac = int(ix_full.info.l_pac)
    offs = [int(o) for _, o in ix_full.contigs()] + [l_pac]
    inside = list(range(0, 21)) + list(range(l_pac - L - 19, l_pac - L + 1))
    beyond = [l_pac - L + 1, l_pac - L + 7, l_pac - 16, l_pac - 1, l_pac, l_pac + 12345, 2 ** 31, 2 ** 32 - L, 2 ** 32 - L + 1, 2 ** 32 - 1]
    ridx, strand, pos = [], [], []
    for k, s in enumerate(inside + beyond):
        for st in (0, 1):
            ridx.append((k + st) % len(reads)); strand.append(st); pos.append(s)
    ridx = np.array(ridx, np.uint32); strand = np.array(strand, np.uint8); pos = np.array(pos, np.uint64)
    one_contig = np.array([any(a <= int(s) and int(s) + L <= b for a, b in zip(offs, offs[1:])) for s in pos])
    assert one_contig.sum() == 2 * len(inside)
    score, valid = _score(ix_full, B, Q, Ln, ridx, strand, pos, capfd=capfd)
    want, valid_lane = _score(ix_full, B, Q, Ln, ridx, strand, pos, lane=True)
    np.testing.assert_array_equal(valid.astype(bool), one_contig)
    np.testing.assert_array_equal(valid, valid_lane)
    assert (bits(score[~one_contig]) == 0).all()
    np.testing.assert_array_equal(bits(score), bits(want))
    op = oracle.params()
    for k in np.flatnonzero(one_contig):
        assert bits(score[k]) == bits(_oracle_score(oracle, oix, op, reads[ridx[k]], strand[k], pos[k], L)), (L, int(pos[k]), int(strand[k]))


def _map_planted(ix, reads, kw, opts, capfd):
    p = g.Params(**kw)
    opts = dict(opts, GM_TRACE="1")
    capfd.readouterr()
    for k, v in opts.items():
        g.set_option(k, v)
    try:
        B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
        batch = g.Batch(ix, len(reads), B.shape[1])
        res = batch.map(p, B, Q, Ln)
        ctr, path = batch.counters(), batch.path()
        batch.destroy()
    finally:
        for k in opts:
            g.set_option(k, None)
    n_heavy = sum(int(x) for x in re.findall(r"(\d+) read x strands on the heavy path", capfd.readouterr().err))
    return res, ctr, path, n_heavy


@pytest.mark.parametrize("case", ["retry_kernel_ran", "nothing_superseded"])
def test_whole_path_with_and_without_superseded_candidates(case, planted, oracle, capfd):  # noqa: F811
    """the planted-repeat reference.  -m 6 -j 1: every read x strand collects some 2 000 SA hits, the LDS vote table of each overflows
    (rs_overflow = 1) and the retry kernel votes again, so the candidates emitted before the overflow are superseded: k_nw_rows reads
    a flagged candidate's rs_overflow byte inside its load group and passes over those.  One scored twice or passed over wrongly
    changes a read's hit count or denominator.  -m 14 -j 7 on the i.i.d. reads: neither path runs, no such byte is loaded.  Results
    are the oracle's read by read"""
    fa, reads = planted
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA)
    if case == "retry_kernel_ran":
        kw = dict(mer=6, jump=1)
        reads = reads[:24] + [r for r in reads if r[0].startswith("e")][::6]
        res, ctr, path, n_heavy = _map_planted(ix, reads, kw, {}, capfd)
        assert ctr["vote_retries"] > 0, ctr
    else:
        kw = CONFIGS["m14_j7"]
        reads = [r for r in reads if r[0].startswith(("iid", "tail"))]
        res, ctr, path, n_heavy = _map_planted(ix, reads, kw, dict(GM_SEED_BUCKET="1", GM_KMER_TABLE="14"), capfd)
        assert n_heavy == 0 and ctr["vote_retries"] == 0, (n_heavy, ctr)
    assert "nw=k_nw_rows" in path, path
    oix = oracle.index_load(fa)
    _compare(res, _oracle_results(oracle, oix, oracle.params(**kw), reads), reads)
    ix.close()


def test_fasta_block(ix_full, syn_reads, capfd):
    """a FASTA block (L = 50: four pieces, the last one half used) loads no quality rows; IUPAC letters take part"""
    L = 50
    rng = np.random.default_rng(50)
    seqs = []
    for _, s, _ in _cut(syn_reads, L, 16):
        s = bytearray(s)
        for j in rng.integers(0, L, 3):
            s[int(j)] = b"RYKMSWBDHVN"[int(rng.integers(0, 11))]
        seqs.append(bytes(s))
    B, _, Ln = g.pack_reads(seqs, None, 64)
    B[:, L:] = 0xFF
    ridx, strand, pos = _probes(len(seqs), L, 51)
    score, valid = _score(ix_full, B, None, Ln, ridx, strand, pos, fasta=True, capfd=capfd)
    want, valid_lane = _score(ix_full, B, None, Ln, ridx, strand, pos, lane=True, fasta=True)
    assert valid.all() and valid_lane.all()
    np.testing.assert_array_equal(bits(score), bits(want))
