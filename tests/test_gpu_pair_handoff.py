"""k_vote_pair's hand-off (gm_pair.hip): by default each 16-pair flush appends its candidates straight to their shard and its flagged
reads to k_vote_bucket's list; GM_PAIR_HANDOFF=gather keeps the older form (own candidate slots + flag bytes, read back by
k_cand_gather / k_pair_collect / k_heavy_collect over all reads).  Both must give the same results and the same work counters.

The reference is i.i.d. with 100-bp elements planted 2, 8, 20 and 40 times: reads from those have several candidates on one strand
(the flush's LDS list of further candidates, and past its 16 entries the direct atomics), more than 16 second arrivals or more
than 384 SA hits on a strand (flagged), and enough candidates in one 16-pair group to overflow a shard (the retry loop of
gm_map_batch_device).  Reads with an N and -h caps flag more reads."""
import re

import numpy as np
import pytest

import gnumap_amd as g
from test_gpu_parity import _compare, _oracle_results

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGT", np.uint8)


def _rand_seq(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


def _revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTN", b"TGCAN"))


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    rng = np.random.default_rng(7)
    elems = {k: _rand_seq(rng, 100) for k in (2, 8, 20, 40)}
    parts = []
    for k, e in elems.items():
        for _ in range(k):
            parts.append(_rand_seq(rng, 1500))
            parts.append(e)
    parts.append(_rand_seq(rng, 60000))
    genome = b"".join(parts)
    d = tmp_path_factory.mktemp("pair_handoff")
    fa = str(d / "planted.fa")
    with open(fa, "wb") as f:
        f.write(b">planted\n")
        for i in range(0, len(genome), 80):
            f.write(genome[i:i + 80] + b"\n")
    g.index_build(fa, g.GM_BUILD_HOST)

    reads = []
    def add(name, s):
        if rng.random() < 0.5:
            s = _revcomp(s)
        reads.append((name, s, b"I" * len(s)))
    for i in range(300):                                         # i.i.d. reads with a few substitutions
        p = int(rng.integers(0, len(genome) - 100))
        s = bytearray(genome[p:p + 100])
        for _ in range(int(rng.integers(0, 3))):
            j = int(rng.integers(0, 100)); s[j] = BASES[(BASES.tolist().index(s[j]) + 1) % 4]
        add(f"iid{i}", bytes(s))
    for i in range(12):                                          # a non-ACGT base
        p = int(rng.integers(0, len(genome) - 100))
        s = bytearray(genome[p:p + 100]); s[int(rng.integers(0, 100))] = ord("N")
        add(f"n{i}", bytes(s))
    # consecutive: one 16-pair group holds many of them.  Two copies: two candidates on one strand and few enough second arrivals
    # that the read stays in k_vote_pair at -j 12 - more than 16 further candidates in a group (LDS list full: direct atomics)
    for k, cnt in ((2, 40), (8, 48), (20, 12), (40, 6)):
        for i in range(cnt):
            add(f"e{k}_{i}", elems[k])
    for i in range(40):
        p = int(rng.integers(0, len(genome) - 100))
        add(f"tail{i}", genome[p:p + 100])
    return fa, reads


CONFIGS = {
    "m14_j7": dict(mer=14, jump=7),                              # 13 seeds per strand -> k_vote_pair<7>
    "m10_j12": dict(mer=10, jump=12),                            # 8 seeds per strand -> k_vote_pair<4>
    "m8_j7_h4": dict(mer=8, jump=7, max_kmer_hits=4),            # many seeds above -h: flagged
}


@pytest.fixture(scope="module")
def ix(planted):
    return g.Index(planted[0], flags=g.GM_INDEX_FULL_SA)


def _map(ix, reads, kw, handoff, capfd=None):
    p = g.Params(**kw)
    g.set_option("GM_SEED_BUCKET", "1")
    g.set_option("GM_KMER_TABLE", str(p.mer))
    g.set_option("GM_PAIR_HANDOFF", handoff)
    g.set_option("GM_TRACE", "1")
    try:
        B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
        batch = g.Batch(ix, len(reads), B.shape[1])
        res = batch.map(p, B, Q, Ln)
        out = dict(res=res, raw=batch.raw_hits(), ctr=batch.counters(), path=batch.path())
        batch.destroy()
    finally:
        for k in ("GM_SEED_BUCKET", "GM_KMER_TABLE", "GM_PAIR_HANDOFF", "GM_TRACE"):
            g.set_option(k, None)
    if capfd is not None:
        out["trace"] = capfd.readouterr().err
    return out


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_direct_handoff_equals_gather(cfg, planted, ix, capfd):
    reads = planted[1]
    kw = CONFIGS[cfg]
    new = _map(ix, reads, kw, None, capfd)
    old = _map(ix, reads, kw, "gather", capfd)
    assert "k_vote_pair<" in new["path"], new["path"]
    assert "k_vote_pair<" in old["path"], old["path"]
    assert new["ctr"] == old["ctr"]
    assert new["ctr"]["candidates"] > 0 and new["ctr"]["seeds_used"] > 0
    for a, b in zip(new["raw"], old["raw"]):
        np.testing.assert_array_equal(a, b)
    for k in ("status", "self_score", "top_score", "denominator", "match_begin", "matches"):
        np.testing.assert_array_equal(new["res"][k], old["res"][k], err_msg=k)
    if "max_kmer_hits" in kw:                                    # (the capped element's reads are flagged: spread over the shards)
        return
    # the planted element's reads overflow a shard in the first attempt: the retry loop ran in both forms
    for o in (new, old):
        attempts = [int(a) for a in re.findall(r"vote done: \d+ candidates \(attempt (\d+)\)", o["trace"])]
        assert attempts and max(attempts) >= 1, o["trace"][-2000:]


def test_direct_handoff_matches_oracle(planted, ix, oracle):
    fa, reads = planted
    kw = CONFIGS["m14_j7"]
    new = _map(ix, reads, kw, None)
    assert "k_vote_pair<7>" in new["path"], new["path"]
    oix = oracle.index_load(fa)
    _compare(new["res"], _oracle_results(oracle, oix, oracle.params(**kw), reads), reads)
