"""k_nw_rows' two forms (gm_nw.hip): the pair table (two band cells per ds_read_b64, records only for the block's quality characters)
against the cells table (GM_NW_CELLS=b32, one ds_read_b32 per cell).  Raw hits and score bits must be the same for both, for every
length of both register shapes (<13> up to 104 bases, <19> above), both strands, reads with N bases, quality characters at the edges of
the block's range and both Phred tables; a block whose range would cost workgroups per CU keeps the cells table, and the path string
names the form that ran."""
import numpy as np
import pytest

import gnumap_amd as g

pytestmark = pytest.mark.gpu
LENGTHS = [24, 31, 33, 50, 64, 75, 97, 100, 104, 105, 113, 128, 136, 149, 150, 152]


@pytest.fixture(scope="module")
def ix_full(syn_fa):
    return g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)


def _reads_from_reference(ix, n, L, qlo, qhi, seed, n_rate=0.02, sub_rate=0.03):
    """n reads of L bases cut from the reference at random places (a few substitutions, some N bases, half of them reverse
    complemented), qualities drawn from [qlo, qhi] with both edge characters in every read"""
    rng = np.random.default_rng(seed)
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    out = []
    for k in range(n):
        b = int(rng.integers(0, 140000 - L))
        s = np.frombuffer(ix.window(b, L).upper(), np.uint8).copy()
        assert len(s) == L
        u = rng.random(L)
        sub = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]
        s = np.where(u < n_rate, ord("N"), np.where(u < n_rate + sub_rate, sub, s)).astype(np.uint8).tobytes()
        if k & 1:
            s = s.translate(comp)[::-1]
        q = bytearray(rng.integers(qlo, qhi + 1, L, dtype=np.int64).astype(np.uint8).tobytes())
        q[int(rng.integers(0, L))] = qlo
        q[int(rng.integers(0, L))] = qhi
        out.append((b, s, bytes(q)))
    return out


def _with_cells(fn):
    g.set_option("GM_NW_CELLS", "b32")
    try:
        return fn()
    finally:
        g.set_option("GM_NW_CELLS", None)


def _raw(batch, p, B, Q, Ln):
    batch.upload(p, B, Q, Ln)
    batch.map_device(p)
    hits, status, _, top = batch.raw_hits()
    hits = np.sort(hits, order=["read", "pos", "strand"])
    return hits, status, top, batch.path()


def _same_raw(a, b):
    assert len(a[0]) == len(b[0]) and len(a[0]) > 0
    for f in ("read", "pos", "strand", "step"):
        np.testing.assert_array_equal(a[0][f], b[0][f])
    np.testing.assert_array_equal(a[0]["score"].view(np.uint32), b[0]["score"].view(np.uint32))
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


@pytest.mark.parametrize("L", LENGTHS)
def test_score_bits_pairs_against_cells(L, ix_full):
    """function level (gm_dev_nw_score): reads with N bases and edge quality characters against 40 consecutive window starts around
    their origin (every phase of the packed reference word), both strands: the same fp32 bits from both forms"""
    reads = _reads_from_reference(ix_full, 16, L, ord("5"), ord("I"), seed=L)
    B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
    p = g.Params()
    ridx, strand, pos = [], [], []
    for k, (b, _, _) in enumerate(reads):
        for d in range(40):
            ridx.append(k); strand.append((k + d) & 1); pos.append(max(0, b - 20 + d))
    ridx = np.array(ridx, np.uint32); strand = np.array(strand, np.uint8); pos = np.array(pos, np.uint64)
    score, valid = ix_full.dev_nw_score(p, B, Q, Ln, ridx, strand, pos)
    score_c, valid_c = _with_cells(lambda: ix_full.dev_nw_score(p, B, Q, Ln, ridx, strand, pos))
    assert valid.all() and valid_c.all()
    assert (score > 0).any()
    np.testing.assert_array_equal(score.view(np.uint32), score_c.view(np.uint32))


@pytest.mark.parametrize("qrange", ["#J", "5I", "!~", "@@"])
def test_score_bits_at_range_edges(qrange, ix_full):
    """the narrowest range (one character), the benchmark's, a wide one and the whole printable range: every record of the table is
    reached from its first and last quality character"""
    qlo, qhi = ord(qrange[0]), ord(qrange[1])
    for L in (100, 150):
        reads = _reads_from_reference(ix_full, 24, L, qlo, qhi, seed=qlo * 1000 + L)
        B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
        p = g.Params()
        ridx = np.repeat(np.arange(len(reads), dtype=np.uint32), 8)
        strand = np.tile(np.array([0, 1], np.uint8), 4 * len(reads))
        pos = np.array([max(0, reads[i][0] - 3 + j % 8) for j, i in enumerate(ridx)], np.uint64)
        score, valid = ix_full.dev_nw_score(p, B, Q, Ln, ridx, strand, pos)
        score_c, valid_c = _with_cells(lambda: ix_full.dev_nw_score(p, B, Q, Ln, ridx, strand, pos))
        assert valid.all() and valid_c.all()
        np.testing.assert_array_equal(score.view(np.uint32), score_c.view(np.uint32))


@pytest.mark.parametrize("L", [50, 100, 104, 105, 150, 152])
def test_whole_path_raw_hits_pairs_against_cells(L, ix_full):
    """gm_map_batch_device on a block of one length: the path names the form, raw hits (positions, strands, steps, score bits), status
    and top scores are the same for both forms"""
    reads = _reads_from_reference(ix_full, 400, L, ord("5"), ord("I"), seed=7 * L)
    B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
    p = g.Params()
    batch = g.Batch(ix_full, len(reads), B.shape[1])
    a = _raw(batch, p, B, Q, Ln)
    assert "nw=k_nw_rows/pairs" in a[3], a[3]
    c = _with_cells(lambda: _raw(batch, p, B, Q, Ln))
    assert "nw=k_nw_rows/cells" in c[3], c[3]
    _same_raw(a, c)
    batch.destroy()


def test_sub_batch_pipeline_pairs_against_cells(ix_full):
    """the sub-batch pipeline (GM_PIPELINE, three sub-batches or more) reads each sub-batch's quality range from its own counters: same
    raw hits for both forms"""
    reads = _reads_from_reference(ix_full, 3 * 4096 + 100, 100, ord("#"), ord("F"), seed=11)
    B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
    p = g.Params()
    batch = g.Batch(ix_full, len(reads), B.shape[1])
    g.set_option("GM_PIPELINE", "4096")
    try:
        a = _raw(batch, p, B, Q, Ln)
        c = _with_cells(lambda: _raw(batch, p, B, Q, Ln))
    finally:
        g.set_option("GM_PIPELINE", None)
    _same_raw(a, c)
    batch.destroy()


def test_illumina_two_tables_pairs(ix_full):
    """--illumina with both Phred tables resident: a narrow range keeps the pair table (two tables of 18 characters), same hits as the
    cells form and as k_nw_lane"""
    reads = _reads_from_reference(ix_full, 300, 100, ord("@"), ord("P"), seed=64)
    reads = reads[:120] + [(b, s, bytes(c - 1 if c > ord("?") else c for c in q)) for b, s, q in reads[120:]]    # Phred+33 from read 120: a '?'
    B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
    p = g.Params(illumina=1)
    batch = g.Batch(ix_full, len(reads), B.shape[1])
    a = _raw(batch, p, B, Q, Ln)
    assert "nw=k_nw_rows/pairs" in a[3], a[3]
    c = _with_cells(lambda: _raw(batch, p, B, Q, Ln))
    assert "nw=k_nw_rows/cells" in c[3], c[3]
    _same_raw(a, c)
    g.set_option("GM_NW", "lane")
    try:
        d = _raw(batch, p, B, Q, Ln)
        assert "nw=k_nw_lane" in d[3], d[3]
    finally:
        g.set_option("GM_NW", None)
    _same_raw(a, d)
    batch.destroy()


def test_wide_two_table_block_falls_back_to_cells(ix_full):
    """two tables over '!' .. '~' would need 128 KB of pair records (fewer workgroups per CU than the 36 KB cells table): the cells form
    runs without being asked, with k_nw_lane's hits"""
    reads = _reads_from_reference(ix_full, 300, 100, ord("@"), ord("h"), seed=65)
    reads = reads[:100] + [(b, s, bytes([ord("!")]) + q[1:-1] + b"~") for b, s, q in reads[100:]]
    B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
    p = g.Params(illumina=1)
    batch = g.Batch(ix_full, len(reads), B.shape[1])
    a = _raw(batch, p, B, Q, Ln)
    assert "nw=k_nw_rows/cells" in a[3], a[3]
    g.set_option("GM_NW", "lane")
    try:
        d = _raw(batch, p, B, Q, Ln)
    finally:
        g.set_option("GM_NW", None)
    _same_raw(a, d)
    batch.destroy()
