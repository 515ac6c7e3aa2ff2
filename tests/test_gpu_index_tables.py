"""Every seed lookup of the device against the PLAIN reference of tests/index_edge_fixture.py (a sorted suffix array), at the record
edges of the five lookup structures: rank planes (gm_occ_plane), the memoised k-mer table and its extension, the compact table (count
bytes, empty-code bytes with the death depth, the escape flag - decoded in gm_seed_walk, gm_seed_rewalk_ool, gm_tiny_seeds<true> and
k_vote_slots_pp), the bucket records (1..28 positions inline, "more hits", "does not occur after d characters", "early position") and
the expanded suffix array.

Direct probes: gm_dev_sa_interval / gm_dev_locate on genomes whose length, granule count and primary sit on every edge (31 .. 3073
bases; primary at a granule's or a BWT block's first / last position, 1, seq_len; three contigs with an N run).  In bounds at the
smallest lengths: k_build_occ_planes writes occ_nblk = ceil(n / 96) + 1 granules into 4 * occ_nblk * 16 bytes; its gm_occ for the last
(never queried) granule and gm_inv_psi at k = primary = n read at most 15 words past the BWT, inside the 256 bytes every device buffer
is allocated with on top of its size; k_expand_full_sa writes full_sa[k] for ranks k <= n only into (n + 1) words.

Probe reads: two seeds each, -k 2 --no_nw, so that one wrong rank or count loses a position (the classed seed at offset 0, at offset
jump, and behind a prefix whose k-mer dies: the re-walk's decoder); compared with the oracle read by read
AND with the position sets computed in Python from the plain reference (tests/test_index_tables_cpu.py checks the guards and ties those
sets to the oracle).  One process: the switches go through gm_set_option and are cleared after every run."""
import numpy as np
import pytest

import gnumap_amd as g
import index_edge_fixture as xf
from test_gpu_edge_reads import run
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

NW_CFG = dict(mer=14, jump=7)                                       # NW on: the ordinary 100-base reads only
FUSED = dict(GM_VOTE="block", GM_SEED_FUSED="1", GM_KMER_TABLE="mer")
BUCKET = dict(GM_SEED_BUCKET="1", GM_KMER_TABLE="mer")
# name -> (switches, seed lookup batch.path() has to name, table length: 0, a number, "default" = min(mer, 12), "mer")
FORMS = {
    "kseed_T0": (dict(GM_KMER_TABLE="0"), "k_seed", 0),                                             # rank planes only
    "kseed_T6": (dict(GM_KMER_TABLE="6"), "k_seed", 6),
    "kseed_default": ({}, "k_seed", "default"),
    "kseed_default_nocompact": (dict(GM_KMER_COMPACT="0"), "k_seed", "default"),
    "kseed_mer": (dict(GM_KMER_TABLE="mer", GM_SEED_FUSED="0"), "k_seed", "mer"),
    "fused_big": (dict(FUSED, GM_VOTE="big"), "k-mer table (in the vote kernel)", "mer"),
    # without the compact table there is no fused form (gm_map_batch_device asks for it): the dispatch falls back to k_seed, and says so
    "fused_nocompact": (dict(FUSED, GM_VOTE_SLOTS="0", GM_KMER_COMPACT="0"), "k_seed", "mer"),
    "bucket": (dict(BUCKET, GM_VOTE_PAIR="0"), "bucket-table (in the vote kernel)", "mer"),
    "pair": (dict(BUCKET), "bucket-table (in the vote kernel)", "mer"),
    "pair_gather": (dict(BUCKET, GM_PAIR_HANDOFF="gather"), "bucket-table (in the vote kernel)", "mer"),
}
for _s in ("0", "-1", "40"):
    FORMS[f"fused_slots{_s}"] = (dict(FUSED, GM_VOTE_SLOTS=_s), "k-mer table (in the vote kernel)", "mer")
    FORMS[f"fused_slots{_s}_pipe"] = (dict(FUSED, GM_VOTE_SLOTS=_s, GM_SLOTS_PIPE="1"), "k-mer table (in the vote kernel)", "mer")


def expected_vote(form, max_len, kw):
    """the vote kernel gm_batch_path() has to name for the forms that force it (the rules of gm_map_batch_device), else None"""
    sw = FORMS[form][0]
    if form.startswith("fused"):
        dense = 2 if sw["GM_VOTE"] == "big" else 1
        pipe = int(sw.get("GM_SLOTS_PIPE", -1))
        pp = dense == 2 if pipe < 0 else pipe != 0
        if dense == 2:
            return "k_vote_slots_pp<64>" if pp else "k_vote_slots<64>"
        hint = int(sw["GM_VOTE_SLOTS"])
        return "k_vote_tiny" if hint == 0 else "k_vote_tiny2" if hint < 0 else "k_vote_slots_pp" if pp else "k_vote_slots"
    if form in ("bucket", "pair", "pair_gather"):
        reg = (max_len - kw["mer"] + kw["jump"] - 1) // kw["jump"]
        if form == "bucket":
            return "k_vote_bucket<2>" if reg <= 8 else "k_vote_bucket<4>"
        return "k_vote_pair<4> + k_vote_bucket<2>" if reg <= 8 else "k_vote_pair<7> + k_vote_bucket<4>"
    return None


@pytest.fixture(scope="module")
def built(tmp_path_factory, oracle):
    return xf.build_genomes(tmp_path_factory.mktemp("index_tables"), oracle)


@pytest.fixture(scope="module")
def dev(built):
    """ONE full-SA index per genome for every form, its tables of every length built here (the 14-mer bucket table is 34 GB per index)"""
    d = {w: g.Index(built[w][0], flags=g.GM_INDEX_FULL_SA) for w in "AB"}
    try:
        for ix in d.values():
            for mer, jump in ((14, 7), (10, 5)):
                p = g.Params(mer=mer, jump=jump, nw=0)
                for sw in ({}, dict(GM_KMER_TABLE="6"), dict(BUCKET, GM_KMER_TABLE=str(mer))):
                    for k, v in sw.items():
                        g.set_option(k, v)
                    try:
                        ix.prepare(p)
                    finally:
                        for k in sw:
                            g.set_option(k, None)
        yield d
    finally:
        for ix in d.values():
            ix.close()


# ------------------------------------------------------------------------------------------------ direct probes
def _check_direct(ix, nx, full):
    queries = xf.interval_queries(nx)
    xf.guard_interval_queries(nx, queries)
    n_found = 0
    for m, ks in queries.items():
        s, e = ix.dev_sa_interval(ks)
        want = np.array([nx.interval(k) for k in ks], np.uint64).reshape(-1, 2)
        bad = np.flatnonzero((s != want[:, 0]) | (e != want[:, 1]))
        assert len(bad) == 0, [(m, ks[i], int(s[i]), int(e[i]), tuple(want[i])) for i in bad[:5]]
        n_found += int((want[:, 1] > 0).sum())
    assert n_found > nx.n
    ranks = np.arange(1, nx.n + 1, dtype=np.uint64)
    want = np.array(nx.sa[1:], np.uint64)
    np.testing.assert_array_equal(ix.dev_locate(ranks, False), want)
    if full:
        np.testing.assert_array_equal(ix.dev_locate(ranks, True), want)


@pytest.mark.parametrize("flags", ["full", "sampled"])
@pytest.mark.parametrize("name", [n for n, _ in xf.sweep_genomes()])
def test_intervals_and_locate_on_the_sweep(name, flags, built):
    fa, oix, nx = built[name]
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA if flags == "full" else 0)
    try:
        assert ix.info.seq_len == nx.n
        _check_direct(ix, nx, flags == "full")
    finally:
        ix.close()


@pytest.mark.parametrize("flags", ["full", "sampled"])
@pytest.mark.parametrize("which", ["A", "B"])
def test_intervals_and_locate_on_the_probe_genomes(which, flags, built, dev):
    fa, oix, nx = built[which]
    ix = dev[which] if flags == "full" else g.Index(fa, flags=0)
    try:
        _check_direct(ix, nx, flags == "full")
    finally:
        if flags != "full":
            ix.close()


# ------------------------------------------------------------------------------------------------ every seed lookup on the probe reads
_READS, _ORACLE, _SEARCHED = {}, {}, {}


def _is_guard(r):
    return any(t[0] in ("cls", "rewalk") for t in r.get("tags", ()))


def block_reads(which, nx, cfg, shape):
    """"odd": the probe reads, depth probes and re-walk probes as they are, an odd number of them (k_vote_pair's tail pair); "tiled": three times over,
    the classed reads at the end of each copy - the block ends on special records, where the prefetch of the "next" read is clamped"""
    key = (which, cfg, shape)
    if key not in _READS:
        kw = NW_CFG if cfg == "nw" else xf.CONFIGS[cfg]
        bl = xf.blocks(which, nx, kw["mer"], kw["jump"], xf.genome_a()[1] if which == "A" else None)
        if cfg == "nw":
            rd = list(bl["ordinary"])
        else:
            rd = bl["probes"] + bl["depth"] + bl["rewalk"]
            if len(rd) % 2 == 0:
                rd = rd[:-1]                                        # (a depth probe of e = mer in the other orientation stays)
            if shape == "tiled":
                rd = ([r for r in rd if not _is_guard(r)] + [r for r in rd if _is_guard(r)]) * 3
                assert _is_guard(rd[-1])
            assert len(rd) % 2 == 1
        _READS[key] = rd
    return _READS[key]


def oracle_for(oracle, oix, which, cfg, rd):
    """the oracle's result of every read of the block, each computed once per (genome, configuration) and never changed"""
    kw = NW_CFG if cfg == "nw" else xf.CONFIGS[cfg]
    memo = _ORACLE.setdefault((which, cfg), {})
    op = oracle.params(**kw)
    for r in rd:
        if r["seq"] not in memo:
            memo[r["seq"]] = oracle.map_read(oix, op, oracle.pwm(r["seq"], b"I" * len(r["seq"])), r["seq"])
    return [memo[r["seq"]] for r in rd]


def _positions(res, i):
    mb = res["match_begin"]
    out = set()
    for m in res["matches"][int(mb[i]):int(mb[i + 1])]:
        out |= {(int(q["pos"]), int(q["strand"])) for q in res["positions"][m["pos_begin"]:m["pos_end"]]}
    return out


def _check_table_length(form, kw, ctr):
    """neither the path nor the trace names the table's length; the work counters do: a seed costs 2 (mer - T) rank queries after its
    table probe, none at T = mer, and no probe at all at T = 0"""
    T = FORMS[form][2]
    mer = kw["mer"]
    T = min(mer, 12) if T == "default" else mer if T == "mer" else T
    if T == 0:
        assert ctr["table_lookups"] == 0 and ctr["occ_calls"] >= 2 * mer * ctr["seeds_used"] > 0, ctr
    elif T == mer:
        assert ctr["occ_calls"] == 0 and ctr["table_lookups"] >= ctr["seeds_used"] > 0, ctr
    else:
        assert 2 * (mer - T) * ctr["seeds_used"] <= ctr["occ_calls"] <= 2 * (mer - T) * ctr["table_lookups"], ctr
        assert ctr["seeds_used"] > 0


@pytest.mark.parametrize("shape", ["odd", "tiled"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cfg", list(xf.CONFIGS))
@pytest.mark.parametrize("which", ["A", "B"])
def test_probe_reads_every_seed_lookup(which, cfg, form, shape, built, dev, oracle):
    fa, oix, nx = built[which]
    kw = xf.CONFIGS[cfg]
    rd = block_reads(which, nx, cfg, shape)
    ores = oracle_for(oracle, oix, which, cfg, rd)
    fq = xf.as_fastq(rd)
    sw, seeds, _ = FORMS[form]
    o = run(dev[which], fq, kw, sw)
    try:
        ctr = o["ctr"]
        print(which, cfg, form, shape, len(rd), o["path"], ctr)
        vote = expected_vote(form, max(len(r["seq"]) for r in rd), kw)
        assert f"seeds={seeds} vote={vote or ''}" in o["path"] and " locate=full-SA " in o["path"], o["path"]
        _compare(o["res"], ores, fq)
        want_seeds = want_hits = n_mapped = 0
        for i, r in enumerate(rd):
            want, ns, nh = xf.expected(nx, r["seq"], cfg)           # the plain reference's walk: never computed from the device
            want_seeds += ns; want_hits += nh
            assert _positions(o["res"], i) == want, r["name"]
            assert o["res"]["status"][i] == (0 if want else 2), r["name"]
            if "want" in r:                                          # depth probes: the walk resumed exactly at offset e
                assert want == r["want"], r["name"]
            n_mapped += bool(want)
        assert n_mapped > len(rd) // 2
        assert want_hits == sum(x["ctr"]["locates"] for x in ores)
        assert ctr["seeds_used"] == want_seeds and ctr["sa_hits"] == want_hits, (ctr, want_seeds, want_hits)
        if seeds == "k_seed":
            _check_table_length(form, kw, ctr)
        # k-mers searched: equal across the forms that walk one k-mer at a time and jump over a dead one (k_seed with any table, the
        # fused lookups and their re-walk - what test_fused_seed_lookup_counts_the_same_work compares).  The bucket forms are left out:
        # their walk asks about every position of a read at once (gm_bucket_rewalk) and counts the k-mers it drops, not the jumps.
        if not seeds.startswith("bucket"):
            first = _SEARCHED.setdefault((which, cfg, shape), (form, ctr["kmers_searched"]))
            assert ctr["kmers_searched"] == first[1], (form, ctr["kmers_searched"], first)
    finally:
        o["batch"].destroy()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("which", ["A", "B"])
def test_ordinary_reads_with_nw_every_seed_lookup(which, form, built, dev, oracle):
    fa, oix, nx = built[which]
    rd = block_reads(which, nx, "nw", "odd")
    ores = oracle_for(oracle, oix, which, "nw", rd)
    fq = xf.as_fastq(rd)
    sw, seeds, _ = FORMS[form]
    o = run(dev[which], fq, NW_CFG, sw)
    try:
        print(which, "nw", form, len(rd), o["path"], o["ctr"])
        vote = expected_vote(form, 100, NW_CFG)
        assert f"seeds={seeds} vote={vote or ''}" in o["path"] and " nw=k_nw_rows/" in o["path"], o["path"]
        _compare(o["res"], ores, fq)
        assert sum(x["status"] == 0 for x in ores) >= 50
        assert all(x["status"] != 1 for x in ores)                  # nobody stopped early at "too many": the oracle located every hit
        assert o["ctr"]["sa_hits"] == sum(x["ctr"]["locates"] for x in ores)
    finally:
        o["batch"].destroy()
