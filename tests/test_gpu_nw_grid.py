"""k_nw_rows (gm_nw.hip) launched as one resident round of workgroups (the default) against the earlier grid of n_cands / 1024
workgroups, at least 2048 (GM_NW_GRID): the candidates are strided over the workgroups, every candidate's score is computed alone, so the
raw hits must be equal read by read - for blocks of one length through <13> and <19>, with one Phred table and with both (--illumina
switching off part way through the block)."""
import pytest

import gnumap_amd as g

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ix_full(syn_fa):
    return g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)


def _raw(ix, p, reads, grid):
    g.set_option("GM_NW_GRID", grid)
    try:
        B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
        batch = g.Batch(ix, len(reads), B.shape[1])
        try:
            batch.upload(p, B, Q, Ln)
            batch.map_device(p)
            hits, status, self_score, top = batch.raw_hits()
            return batch.path(), hits.copy(), status.copy(), self_score.copy(), top.copy()
        finally:
            batch.destroy()
    finally:
        g.set_option("GM_NW_GRID", None)


@pytest.mark.parametrize("illumina", [0, 1])
@pytest.mark.parametrize("L", [24, 63, 100, 104, 105, 150])
def test_resident_grid_equals_the_earlier_grid(L, illumina, ix_full, syn_reads):
    reads = [(n, s[:L], q[:L]) for n, s, q in syn_reads if len(s) >= L]
    if illumina:                                          # the first reads Phred+64: both tables are resident in the kernel
        reads = [(n, s, bytes(min(126, c + 31) for c in q) if i < 40 else q) for i, (n, s, q) in enumerate(reads)]
    p = g.Params(illumina=illumina)
    new = _raw(ix_full, p, reads, None)
    old = _raw(ix_full, p, reads, "2048")
    assert "k_nw_rows" in new[0] and "k_nw_rows" in old[0], new[0]
    for a, b in zip(new[1:], old[1:]):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert a.tobytes() == b.tobytes()
    assert len(new[1]) > 50                               # the comparison has hits to compare
