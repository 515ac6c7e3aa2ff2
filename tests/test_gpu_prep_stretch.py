"""k_prep_rows (gm_prep.hip) fetches the 64 rows of a wavefront as one stretch of 16-byte pieces through LDS.  What can go wrong there is
at the edges: a stretch that starts 8 bytes off a 16-byte boundary (a sub-batch view that begins at an odd row), a last wavefront with
fewer than 64 rows, a last row that ends where its allocation ends, rows shorter than the stride, the <19> form, a block without
quality rows.  Every case runs the kernel alone (gm_dev_prep) and compares it array for array with the tile kernel (GM_PREP=tile):
status, the bits of self_score and min_score, the 2-bit rows, and the work counters (negative probabilities, characters above 127, the
quality range).  FASTQ cases are also compared with the oracle (status, self score)."""
import numpy as np
import pytest

import gnumap_amd as g

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
LOWER = np.frombuffer(b"acgt", np.uint8)
IUPAC = np.frombuffer(b"ACGTNRYKMSWBDHVacgtnrykm", np.uint8)
GRID_TRIPS_N = 5 * 256 * 20 + 3                                   # with GM_TEST_GRID_CAP=5: twenty trips per workgroup and a ragged end


@pytest.fixture(scope="module")
def ix(syn_fa):
    return g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)


@pytest.fixture(scope="module")
def oix(oracle, syn_fa):
    return oracle.index_load(syn_fa)


def _block(seed, n, stride, lens, fasta=False, qlo=40, qhi=73):
    """n rows: mostly ACGT, every 7th row with an N, every 5th with lower-case letters; the padding of a row is zero"""
    rng = np.random.default_rng(seed)
    lens = np.broadcast_to(np.asarray(lens, np.uint16), (n,)).copy()
    B = np.zeros((n, stride), np.uint8); Q = None if fasta else np.zeros((n, stride), np.uint8)
    for i in range(n):
        L = int(lens[i])
        row = (IUPAC if fasta else ACGT)[rng.integers(0, len(IUPAC) if fasta else 4, L)].copy()
        if not fasta and L:
            if i % 5 == 3:
                at = rng.integers(0, L, max(1, L // 4)); row[at] = LOWER[rng.integers(0, 4, len(at))]
            if i % 7 == 2:
                row[rng.integers(0, L, 1 + i % 3)] = ord("N")
            Q[i, :L] = rng.integers(qlo, qhi + 1, L)
        B[i, :L] = row
    return B, Q, lens


def _prep(ix, p, B, Q, Ln, form, grid_cap=None, **kw):
    g.set_option("GM_PREP", form)
    g.set_option("GM_TEST_GRID_CAP", None if grid_cap is None else str(grid_cap))
    try:
        return ix.dev_prep(p, B, Q, Ln, **kw)
    finally:
        g.set_option("GM_PREP", None); g.set_option("GM_TEST_GRID_CAP", None)


def _same(a, b, lo=0):
    np.testing.assert_array_equal(a["status"][lo:], b["status"][lo:])
    np.testing.assert_array_equal(a["self_score"][lo:].view(np.uint32), b["self_score"][lo:].view(np.uint32))
    np.testing.assert_array_equal(a["min_score"][lo:].view(np.uint64), b["min_score"][lo:].view(np.uint64))
    np.testing.assert_array_equal(a["pack"][lo:], b["pack"][lo:])
    for k in ("bad_qual", "high_qual", "qual_lo", "qual_hi"):
        assert a[k] == b[k], (k, a[k], b[k])


def _oracle_rows(oracle, oix, op, out, B, Q, Ln, rows, illumina_until=0):
    for i in rows:
        L = int(Ln[i])
        seq, qual = B[i, :L].tobytes(), Q[i, :L].tobytes()
        o = oracle.map_read(oix, op, oracle.pwm(seq, qual, 1 if i < illumina_until else 0) if L else np.zeros((1, 4), np.float32), seq)
        if o["status"] in (-2, -3):
            assert out["status"][i] == o["status"], (i, out["status"][i], o["status"])
        else:
            assert out["status"][i] == 0, (i, out["status"][i], o["status"])
        if o["status"] in (0, 1, 2):
            assert np.float32(out["self_score"][i]).view(np.uint32) == np.float32(o["self_score"]).view(np.uint32), i


def _edge_rows(n):
    """the rows at the ends of the block and on both sides of every wavefront edge of its first and last workgroup trips"""
    rows = set()
    for c in (0, 64, 128, 192, 256, n - n % 64, n):
        rows.update(r for r in range(c - 2, c + 2) if 0 <= r < n)
    return sorted(rows)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_read_counts(n, ix, oracle, oix):
    p = g.Params(mer=14)
    B, Q, Ln = _block(n, n, 104, 100)
    new, tile = _prep(ix, p, B, Q, Ln, None), _prep(ix, p, B, Q, Ln, "tile")
    _same(new, tile)
    assert new["bad_qual"] == 0 and new["high_qual"] == 0 and new["pack"].any()
    _oracle_rows(oracle, oix, oracle.params(mer=14), new, B, Q, Ln, _edge_rows(n))


def test_many_trips_per_workgroup(ix, oracle, oix):
    p = g.Params(mer=14)
    n = GRID_TRIPS_N
    B, Q, Ln = _block(11, n, 104, 100)
    new, tile = _prep(ix, p, B, Q, Ln, None, grid_cap=5), _prep(ix, p, B, Q, Ln, "tile", grid_cap=5)
    _same(new, tile)
    _same(new, _prep(ix, p, B, Q, Ln, None))                      # the launcher's own grid: one trip
    _oracle_rows(oracle, oix, oracle.params(mer=14), new, B, Q, Ln, _edge_rows(n) + list(range(5 * 256 - 2, 5 * 256 + 2)))


@pytest.mark.parametrize("stride,L", [(104, 24), (104, 97), (104, 100), (104, 103), (104, 104), (152, 105), (152, 150), (152, 152), (32, 24)])
def test_lengths_and_strides(stride, L, ix, oracle, oix):
    p = g.Params(mer=14)
    n = 2 * 256 + 64 + 7                                          # a second trip of the first workgroup's size, a whole wavefront and a short one
    B, Q, Ln = _block(stride * 1000 + L, n, stride, L)
    new, tile = _prep(ix, p, B, Q, Ln, None, grid_cap=1), _prep(ix, p, B, Q, Ln, "tile", grid_cap=1)
    _same(new, tile)
    _oracle_rows(oracle, oix, oracle.params(mer=14), new, B, Q, Ln, _edge_rows(n))


def test_mixed_lengths_and_a_read_shorter_than_the_seed(ix, oracle, oix):
    p = g.Params(mer=14)
    n = 333
    rng = np.random.default_rng(5)
    lens = rng.integers(14, 105, n)
    lens[[0, 63, 64, 200, n - 1]] = [13, 8, 1, 0, 9]               # shorter than -m: READ_TOO_SHORT (an empty row among them)
    B, Q, Ln = _block(6, n, 104, lens)
    new, tile = _prep(ix, p, B, Q, Ln, None), _prep(ix, p, B, Q, Ln, "tile")
    _same(new, tile)
    assert (new["status"][[0, 63, 64, 200, n - 1]] == -2).all() and (new["status"] == 0).sum() > 300
    _oracle_rows(oracle, oix, oracle.params(mer=14), new, B, Q, Ln, [r for r in range(n) if Ln[r]])


def test_quality_characters_above_127_take_the_direct_form(ix):
    """the first, a middle and the last read of a wavefront: the lane sums its read again from global memory"""
    p = g.Params(mer=14)
    n = 200
    B, Q, Ln = _block(8, n, 104, 100)
    for r, at in ((64, 0), (95, 50), (127, 99), (199, 7)):
        Q[r, at] = 200
    new, tile = _prep(ix, p, B, Q, Ln, None), _prep(ix, p, B, Q, Ln, "tile")
    _same(new, tile)
    assert new["high_qual"] > 0 and new["qual_hi"] == 200
    clean = Q.copy()
    clean[clean == 200] = 60
    ref = _prep(ix, p, B, clean, Ln, None)                       # the other reads are not touched by their neighbours' fallback
    keep = np.setdiff1d(np.arange(n), [64, 95, 127, 199])
    np.testing.assert_array_equal(new["self_score"][keep].view(np.uint32), ref["self_score"][keep].view(np.uint32))
    np.testing.assert_array_equal(new["pack"], ref["pack"])


def test_negative_probability_is_counted(ix):
    p = g.Params(mer=14)
    B, Q, Ln = _block(9, 130, 104, 100)
    Q[129, 3] = 30                                                 # Phred -3: 1 - 10^0.3 < 0
    new, tile = _prep(ix, p, B, Q, Ln, None), _prep(ix, p, B, Q, Ln, "tile")
    _same(new, tile)
    assert new["bad_qual"] > 0 and new["qual_lo"] == 30


def test_illumina_until_in_the_middle_of_a_wavefront(ix, oracle, oix):
    p = g.Params(mer=14, illumina=1)
    n, until = 192, 100
    B, Q, Ln = _block(10, n, 104, 100, qlo=66, qhi=104)
    Q[until, 17] = 53                                              # the first quality below '@': this read and all later ones are Phred+33
    new, tile = _prep(ix, p, B, Q, Ln, None), _prep(ix, p, B, Q, Ln, "tile")
    _same(new, tile)
    plain = _prep(ix, g.Params(mer=14), B, Q, Ln, None)
    assert (new["self_score"][:until] != plain["self_score"][:until]).any()
    np.testing.assert_array_equal(new["self_score"][until:].view(np.uint32), plain["self_score"][until:].view(np.uint32))
    _oracle_rows(oracle, oix, oracle.params(mer=14), new, B, Q, Ln, range(until - 4, until + 4), illumina_until=until)


def test_fasta_block_with_iupac_letters(ix):
    p = g.Params(mer=14)
    n = 256 + 70
    B, _, Ln = _block(12, n, 104, np.random.default_rng(12).integers(20, 105, n), fasta=True)
    new, tile = _prep(ix, p, B, None, Ln, None, fasta=True), _prep(ix, p, B, None, Ln, "tile", fasta=True)
    _same(new, tile)
    assert new["pack"].any() and np.isfinite(new["self_score"]).all()


@pytest.mark.parametrize("first_row", [1, 63, 65, 256 + 129])
def test_view_that_starts_at_an_odd_row(first_row, ix):
    """row r of a block of stride 104 starts at 104 r: 8 bytes off a 16-byte boundary when r is odd"""
    p = g.Params(mer=14)
    n = 3 * 256 + 100
    B, Q, Ln = _block(13, n, 104, 100)
    whole = _prep(ix, p, B, Q, Ln, None)
    view = _prep(ix, p, B, Q, Ln, None, first_row=first_row, grid_cap=1)
    np.testing.assert_array_equal(view["status"], whole["status"])
    np.testing.assert_array_equal(view["self_score"].view(np.uint32), whole["self_score"].view(np.uint32))
    np.testing.assert_array_equal(view["min_score"].view(np.uint64), whole["min_score"].view(np.uint64))
    np.testing.assert_array_equal(view["pack"][first_row:], whole["pack"][first_row:])
    assert not view["pack"][:first_row].any()
    _same(view, _prep(ix, p, B, Q, Ln, "tile", first_row=first_row, grid_cap=1), lo=first_row)


@pytest.mark.parametrize("n,stride,L", [(77, 104, 104), (64, 104, 100), (129, 152, 152), (3, 32, 24)])
def test_rows_that_end_with_their_allocation(n, stride, L, ix):
    p = g.Params(mer=14)
    B, Q, Ln = _block(14 + n, n, stride, L)
    _same(_prep(ix, p, B, Q, Ln, None, exact=True), _prep(ix, p, B, Q, Ln, None))
    _same(_prep(ix, p, B, Q, Ln, None, exact=True), _prep(ix, p, B, Q, Ln, "tile", exact=True))


def test_pipelined_map_equals_the_single_pass(ix, syn_reads):
    """GM_PIPELINE=4096 on 3 x 4096 + 100 reads: sub-batch views and a short last one.  4096 rows are a whole number of 16-byte pieces
    at any stride, so GM_PIPELINE=4097 runs too: its second view starts at an odd row, 8 bytes off a 16-byte boundary when the stride
    is an odd multiple of 8"""
    p = g.Params()
    reads = [syn_reads[i % len(syn_reads)] for i in range(3 * 4096 + 100)]
    rng = np.random.default_rng(3)
    seqs, quals = [], []
    for k, (_, s, q) in enumerate(reads):
        s = bytearray(s)
        if k >= len(syn_reads):
            s[int(rng.integers(0, len(s)))] = ACGT[rng.integers(0, 4)]
        seqs.append(bytes(s)); quals.append(q)
    B, Q, Ln = g.pack_reads(seqs, quals)
    out = {}
    for form in (None, "4096", "4097"):
        g.set_option("GM_PIPELINE", form)
        try:
            batch = g.Batch(ix, len(seqs), B.shape[1])
            res = batch.map(p, B, Q, Ln)
            out[form] = (res, batch.raw_hits(), batch.path())
            batch.destroy()
        finally:
            g.set_option("GM_PIPELINE", None)
    for form in ("4096", "4097"):
        for k in ("status", "self_score", "top_score", "denominator", "match_begin", "matches"):
            np.testing.assert_array_equal(out[form][0][k], out[None][0][k], err_msg=f"{form} {k}")
        for a, b in zip(out[form][1], out[None][1]):
            np.testing.assert_array_equal(a, b)
