"""k_scatter_hits gives every accepted candidate of a read a slot of its own behind hit_begin[r], counted out by the read's cursor, which
k_prep zeroes at the start of every map call.  Reads planted with 0, 1, 2 and 5 accepted hits in a small repeat reference: the raw hits
(one per accepted candidate, grouped by read: hit_begin is their running count) and the results of Batch.map against the oracle, on a
handle that maps the block twice in a row - a cursor left over from the first call would move the second call's slots.  (Any form of the
kernel that treats reads with one hit apart has to pass this: one was measured and not kept)"""
import numpy as np
import pytest

import gnumap_amd as g
from test_gpu_parity import _compare, _oracle_results

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGT", np.uint8)
COPIES = (1, 2, 5)
KW = dict(mer=14, jump=7)


def _rand_seq(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


def _revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTN", b"TGCAN"))


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    rng = np.random.default_rng(21)
    elems = {k: [_rand_seq(rng, 100) for _ in range(6)] for k in COPIES}
    parts = []
    for k, es in elems.items():
        for e in es:
            for _ in range(k):
                parts.append(_rand_seq(rng, 700)); parts.append(e)
    parts.append(_rand_seq(rng, 30000))
    genome = b"".join(parts)
    d = tmp_path_factory.mktemp("scatter_single")
    fa = str(d / "planted.fa")
    with open(fa, "wb") as f:
        f.write(b">planted\n")
        for i in range(0, len(genome), 80):
            f.write(genome[i:i + 80] + b"\n")
    g.index_build(fa, g.GM_BUILD_HOST)
    reads, want = [], []                                         # want: accepted hits of the read
    def add(name, s, k):
        reads.append((name, _revcomp(s) if rng.random() < 0.5 else s, b"I" * len(s))); want.append(k)
    for rep in range(40):                                        # interleaved, so that a wavefront of the scatter kernel sees every kind
        for k, es in elems.items():
            add(f"e{k}_{rep}", es[rep % len(es)], k)
        add(f"none{rep}", _rand_seq(rng, 100), 0)
        p0 = len(genome) - 30000 + int(rng.integers(0, 29900))
        add(f"uniq{rep}", genome[p0:p0 + 100], 1)
    return fa, reads, np.array(want)


@pytest.fixture(scope="module")
def ix(planted):
    return g.Index(planted[0], flags=g.GM_INDEX_FULL_SA)


def _map_twice(ix, reads, **opts):
    p = g.Params(**KW)
    for k, v in opts.items():
        g.set_option(k, v)
    try:
        B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
        batch = g.Batch(ix, len(reads), B.shape[1])
        out = []
        for _ in range(2):
            res = batch.map(p, B, Q, Ln)
            out.append(dict(res=res, raw=batch.raw_hits(), ctr=batch.counters(), path=batch.path()))
        batch.destroy()
    finally:
        for k in opts:
            g.set_option(k, None)
    return out


def _check_raw(raw, want):
    hits, status, _, _ = raw
    n = len(want)
    counts = np.bincount(hits["read"], minlength=n)
    np.testing.assert_array_equal(counts, want)                  # (hit_begin = the running sum of these)
    assert (np.diff(hits["read"].astype(np.int64)) >= 0).all()   # grouped by read, every slot filled by its own read
    keys = set(zip(hits["read"].tolist(), hits["pos"].tolist(), hits["strand"].tolist()))
    assert len(keys) == len(hits)                                # no candidate twice, none lost to a shared slot
    assert np.isfinite(hits["score"]).all() and (hits["score"] != 0).all()


@pytest.mark.parametrize("opts", [dict(), dict(GM_SEED_BUCKET="1", GM_KMER_TABLE="14"), dict(GM_TEST_GRID_CAP="1")], ids=["default", "bucket", "one_workgroup"])
def test_reads_with_0_1_2_5_hits(opts, planted, ix, oracle):
    fa, reads, want = planted
    first, second = _map_twice(ix, reads, **opts)
    assert set(want.tolist()) == {0, 1, 2, 5}
    for o in (first, second):
        _check_raw(o["raw"], want)
        assert o["ctr"]["accepted"] == want.sum()
    for a, b in zip(first["raw"], second["raw"]):
        np.testing.assert_array_equal(a, b)
    for k in ("status", "self_score", "top_score", "denominator", "match_begin", "matches"):
        np.testing.assert_array_equal(first["res"][k], second["res"][k], err_msg=k)
    oix = oracle.index_load(fa)
    ores = _oracle_results(oracle, oix, oracle.params(**KW), reads)
    for i, o in enumerate(ores):                                 # the oracle's accepted places of a read = its raw hits
        assert sum(len(h["pos"]) for h in o["hits"]) == want[i], reads[i][0]
    _compare(second["res"], ores, reads)
