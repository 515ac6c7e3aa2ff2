"""The fixtures of tests/index_edge_fixture.py checked without a GPU: the GUARDS (computed from the plain reference alone: the generator
really reaches every record class, bucket count, early-flag edge and death depth it was built for), the oracle against the plain
reference (every interval query of the direct probes, every rank's located position), and the Python-computed position sets of the probe
reads against the oracle's map_read.  tests/test_gpu_index_tables.py runs the same queries and reads through every device form."""
import pytest

import index_edge_fixture as xf


@pytest.fixture(scope="module")
def built(tmp_path_factory, oracle):
    """{name: (fasta, oracle index, NaiveIndex)} of genome A, genome B and the sweep"""
    return xf.build_genomes(tmp_path_factory.mktemp("index_tables_cpu"), oracle)


def _oracle_positions(oracle, oix, seq, kw):
    o = oracle.map_read(oix, oracle.params(**kw), oracle.pwm(seq, b"I" * len(seq)), seq)
    assert o["status"] in (0, 2)                                  # --no_nw never says "too many"
    return o, {(int(p), int(s)) for h in o["hits"] for p, s in h["pos"]}


# ------------------------------------------------------------------------------------------------ the generator
def test_sweep_has_every_primary_position(built):
    by = {name: built[name][2] for name, _ in xf.primary_genomes()}
    assert by["p96_0"].primary % 96 == 0 and by["p96_1"].primary % 96 == 1 and by["p96_95"].primary % 96 == 95
    assert by["p128_0"].primary % 128 == 0 and by["p128_127"].primary % 128 == 127
    assert by["p_first"].primary == 1 and by["p_last"].primary == by["p_last"].n == 300
    for name, (fa, oix, nx) in built.items():
        assert nx.primary == int(oix.contents.primary), name     # the index under test has its $ where the plain sort puts it
    n3 = built["three_contigs_n"][2]
    assert len(n3.contigs) == 3 and n3.n == sum(n for _, n in xf.THREE_CONTIGS)


# what the committed generator gives on genome A (17 503 bases), per table length: records that escape because their intervals are not
# adjacent (the text's end sorts inside them), codes in records with a count >= 224, class c_lo and c_hi codes
REWALK_14_6_C_HI = 84                                               # two of them have no X that makes the first k-mer die
A_CLASSES = {
    14: dict(b_records=1, a_codes=2, c_lo=54, c_hi=179),
    12: dict(b_records=1, a_codes=2, c_lo=59, c_hi=209),
    10: dict(b_records=1, a_codes=3, c_lo=173, c_hi=614),
    6: dict(b_records=1, a_codes=8, c_lo=97, c_hi=379),
}
# mapped probe reads per class, genomes A and B together, per (seed length, table length): what the committed generator gives
PROBES = {
    (14, 14): dict(a_big=14, a_nb=4, b=8, c_lo=20, c_hi=34),
    (14, 12): dict(a_big=18, a_nb=4, b=8, c_lo=32, c_hi=58),
    (14, 6): dict(a_big=30, a_nb=16, b=20, c_lo=42, c_hi=86),
    (10, 10): dict(a_big=10, a_nb=8, b=8, c_lo=30, c_hi=34),
}


@pytest.mark.parametrize("T", sorted(A_CLASSES))
def test_genome_a_reaches_every_record_class(T, built):
    nx = built["A"][2]
    got = xf.class_summary(nx, T)
    print(T, got)
    assert got == A_CLASSES[T]
    cl = xf.classify(nx, T)
    W = nx.text[-13:-1]
    # the one non-adjacent record: W's tail + AG at sub-index 2, + CT at 7, the text's last T - 1 characters between them
    b = sorted((c & 7, w) for w, (c, _, k) in cl.items() if k == "b")
    if T >= 10:
        assert b == [(2, W[12 - (T - 2):] + b"AG"), (7, W[12 - (T - 2):] + b"CT")]
    else:
        assert len(b) == 8 and {w[:T - 2] for _, w in b} == {nx.text[-(T - 1):-1][:T - 2]}
    lower = [w for s, w in b if s <= 3][-1]
    assert nx.sa[cl[lower][1][1] + 1] == nx.n - (T - 1)          # the rank after the record's lower half: the text's last T - 1 characters


def test_dropping_the_text_end_loses_class_b():
    """the guard is alive: without W + C as the last 13 bases no record has non-adjacent intervals at T = 14"""
    text, _ = xf.genome_a(end_with_w=False)
    got = xf.class_summary(xf.NaiveIndex(text), 14)
    assert got["b_records"] == 0 and got["c_hi"] > 100


@pytest.fixture(scope="module")
def mapped(built, oracle):
    """{(genome, config): [(read dict, oracle result, oracle position set)]} of the probe reads and the depth probes"""
    out = {}
    for which in "AB":
        fa, oix, nx = built[which]
        marks = xf.genome_a()[1] if which == "A" else None
        for cfg, kw in xf.CONFIGS.items():
            bl = xf.blocks(which, nx, kw["mer"], kw["jump"], marks)
            out[which, cfg] = [(r,) + _oracle_positions(oracle, oix, r["seq"], kw) for r in bl["probes"] + bl["depth"] + bl["rewalk"]]
    return out


@pytest.mark.parametrize("m,T", xf.MT)
def test_guards_every_class_has_probe_reads(m, T, mapped):
    cfg = "m14_j7" if m == 14 else "m10_j5"
    n, again = {c: 0 for c in xf.CLASSES}, {c: 0 for c in xf.CLASSES}
    for which in "AB":
        for r, o, pos in mapped[which, cfg]:
            if o["status"] != 0:
                continue                                           # a read the oracle does not map proves nothing
            for c in xf.CLASSES:
                n[c] += ("cls", T, c) in r.get("tags", ())
                again[c] += ("rewalk", T, c) in r.get("tags", ())
    print((m, T), n, again)
    assert all(v >= 4 for v in n.values()), n
    assert all(v >= 4 for v in again.values()), again              # ... and as many that reach the classed seed in the re-walk
    assert n == PROBES[m, T]
    assert again == dict(PROBES[m, T], c_hi=REWALK_14_6_C_HI if (m, T) == (14, 6) else PROBES[m, T]["c_hi"])


def test_guards_bucket_counts_and_the_early_edge(mapped):
    tags = set()
    for r, o, pos in mapped["A", "m14_j7"]:
        if o["status"] == 0:
            tags |= r.get("tags", set())
    for c in xf.COUNTS + (">=224",):
        assert ("count", c) in tags, c
    assert ("seed_at", 4095) in tags and ("seed_at", 4096) in tags
    # -h 28: the 28-copy read keeps all 28 positions, the 29-copy read has no seed at all
    by_name = {r["name"]: (o, pos) for r, o, pos in mapped["A", "m14_j7_h28"]}
    _, marks = xf.genome_a()
    for c, want in ((28, 28), (29, 0), (30, 0)):
        o, pos = by_name[f"copies{c}_p{marks['planted'][c][0]}_o0_f"]
        assert len(pos) == want and o["status"] == (0 if want else 2) and o["ctr"]["locates"] == 2 * want


@pytest.mark.parametrize("mer", [14, 10])
def test_guards_every_death_depth_has_a_probe(mer, built, mapped):
    cfg = "m14_j7" if mer == 14 else "m10_j5"
    depths = {w: {r["depth"] for r, o, pos in mapped[w, cfg] if "depth" in r and o["status"] == 0} for w in "AB"}
    print(mer, depths)
    assert depths["B"] == set(range(1, mer + 1))
    assert depths["A"] == set(range(6, mer + 1))                  # every word of up to 5 characters occurs in 17 kbp of ACGT
    for w in "AB":
        for r, o, pos in mapped[w, cfg]:
            if "depth" in r:
                assert o["status"] == 0 and pos == r["want"], r["name"]


# ------------------------------------------------------------------------------------------------ the oracle against the plain reference
@pytest.mark.parametrize("name", xf.genome_names())
def test_oracle_intervals_and_locate_equal_the_plain_sort(name, built, oracle):
    fa, oix, nx = built[name]
    queries = xf.interval_queries(nx)
    xf.guard_interval_queries(nx, queries)
    for m, ks in queries.items():
        for k in ks:
            assert oracle.sa_interval(oix, k) == nx.interval(k), (m, k)
    for r in range(1, nx.n + 1):
        assert int(oracle.lib.gmo_locate(oix, r, None)) == nx.sa[r], r
    assert sorted(nx.sa) == list(range(nx.n + 1))


@pytest.mark.parametrize("cfg", sorted(xf.CONFIGS))
@pytest.mark.parametrize("which", ["A", "B"])
def test_probe_reads_position_sets_equal_the_oracle(which, cfg, built, mapped):
    nx = built[which][2]
    n_ok = 0
    for r, o, pos in mapped[which, cfg]:
        want, seeds, hits = xf.expected(nx, r["seq"], cfg)
        assert pos == want, r["name"]
        assert o["status"] == (0 if want else 2), r["name"]
        assert o["ctr"]["locates"] == hits, r["name"]
        n_ok += o["status"] == 0
    assert n_ok > 40
