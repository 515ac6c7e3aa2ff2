"""--snp (mode 5) at the edges, on the CPU: the oracle's restatement of SNPScoredSeq::score (src/SNPScoredSeq.cpp:25-109) - the pair HMM
of every kept sequence, its deposit at every place, places on the other strand through reverse_comp_cpy_phmm
(inc/SequenceOperations.h:164-181) - pinned to what the UNMODIFIED reference program writes with --snp
(tests/golden/ref_runs_snp_edge/, made by tests/golden/make_snp_edge_fixtures.py) for

    both    both.fa / both.fq: one 150-base segment on both strands of the genome, reads of 24 .. 150 bases cut from it in both
            orientations, a third of them with an N: other-strand places, the fifth (n) track, a segment that ends at l_pac
    edge    edge.fa / edge.fq: 100-bp reads at and across every contig start and end
    mixed   edge.fa / edge_mixed.fq: lengths 16 .. 150 one after the other

and the GUARDS of tests/edge_fixture.py that tests/test_gpu_snp_edges.py asserts again before it compares the device with the oracle."""
import json
import os

import pytest

import edge_fixture as ef
from conftest import GOLDEN

MANIFEST = json.load(open(os.path.join(ef.SNP_RUNS, "manifest.json")))


@pytest.fixture(scope="module")
def fastas(tmp_path_factory):
    return {"edge.fa": ef.build_index(tmp_path_factory), "both.fa": ef.build_index(tmp_path_factory, "both.fa")}


@pytest.fixture(scope="module")
def oixs(oracle, fastas):
    return {k: oracle.index_load(v) for k, v in fastas.items()}


_INFO = {}


def info_of(oracle, oixs, block):
    if block not in _INFO:
        _INFO[block] = ef.snp_info(oracle, oixs[ef.SNP_BLOCKS[block.replace("_plus", "")][0]], ef.snp_block_reads(block))
    return _INFO[block]


def test_both_genome_is_off_every_word_boundary(oixs):
    ctg, l_pac = ef.geometry(oixs["both.fa"])
    assert len(ctg) == 3 and all((e - b) % 16 for b, e in ctg) and all(b % 16 for b, _ in ctg[1:]) and l_pac % 16


@pytest.mark.parametrize("run", sorted(MANIFEST))
def test_oracle_snp_run_equals_reference_program(run, oracle, oixs, tmp_path):
    """gmo_run in mode 5: the SAM file of the reference program byte for byte (apart from @PG), and the first eight columns of its .gmp
    byte for byte - position, total and the five per-nucleotide sums of EVERY row, no row left out and no tolerance (the reference run
    has one thread and zeroed track arrays, tests/edge_ref_env.py; the oracle deposits in the same order).  The ninth column is the
    likelihood-ratio call, which the oracle does not restate (tests/test_snp_call_golden.py pins it)."""
    m = MANIFEST[run]
    out = str(tmp_path / "o")
    st = oracle.run(oixs[m["genome"]], oracle.params(mode=ef.GM_MODE_SNP), os.path.join(GOLDEN, m["fastq"]), out, threads=1)
    sam = b"".join(l for l in open(out + ".sam", "rb") if not l.startswith(b"@PG"))
    assert sam == ef.snp_ref_text(run, "sam"), run
    assert sam.count(b"\n") == m["sam_lines"] and st.n_records == m["sam_lines"] - 3
    ref = ef.snp_ref_text(run, "gmp").splitlines()
    assert len(ref) == m["gmp_rows"] > 500 and all(len(l.split(b"\t")) == 9 for l in ref)
    mine = open(out + ".gmp", "rb").read().splitlines()
    assert mine == [b"\t".join(l.split(b"\t")[:8]) for l in ref], run
    assert not os.path.exists(out + ".sgr")


def test_guards_both_strands_and_n(oracle, oixs):
    info = info_of(oracle, oixs, "both")
    assert ef.guard_snp_other_strand(info) >= 100
    assert ef.guard_snp_n_sequences(info) >= 20
    assert {k[4] for k in info["kept"]} == {150, 143, 100, 50, 36, 24}      # (offset 7 of the 150-base cut leaves 143)
    assert {k[1] for k in info["kept"]} == {0, 1}                       # kept sequences whose FIRST strand is the reverse one, too
    ef.guard_snp_deposits_touch(info, ef.snp_edge_positions(oixs["both.fa"], "both"))
    # the fifth track gets something: the posterior weight of a read's N goes to code 4 (bin_seq.cpp:222-241)
    cov, nuc = ef.snp_tracks(info, ef.geometry(oixs["both.fa"])[1] + 64, 1)
    assert nuc[4].sum() > 10.0 and nuc[:4].sum() > 0.9 * cov.sum() - nuc[4].sum()


def test_guards_more_than_one_chunk_of_kept_sequences(oracle, oixs):
    """GM_SNP_CHUNK=64 gives chunks of 128 kept sequences: edge.fq has to fill more than one of them, edge_mixed.fq more than three"""
    assert ef.guard_snp_kept(info_of(oracle, oixs, "edge"), 128) > 128
    mixed = info_of(oracle, oixs, "mixed")
    assert ef.guard_snp_kept(mixed, 384) > 384
    assert len(ef.guard_snp_lengths(mixed)) >= 5
    assert sum(1 for k in mixed["kept"] if k[2] > 1) >= 20             # sequences with several places


@pytest.mark.parametrize("block", ["edge", "mixed"])
def test_guard_deposits_touch_every_edge(block, oracle, oixs):
    oix = oixs["edge.fa"]
    pos = ef.snp_edge_positions(oix, block)
    ctg, l_pac = ef.geometry(oix)
    assert pos[:2] == [0, l_pac - 1] and len(pos) == 6
    ef.guard_snp_deposits_touch(info_of(oracle, oixs, block), pos)


def test_guard_exact_bins(oracle, oixs):
    """the counts tests/test_gpu_snp_edges.py fixes for its bit-exact comparisons.  edge.fq and edge_mixed.fq alone have no bin that one
    place covers - every read stands beside its reverse complement on the same window - so the blocks compared exactly carry the interior
    reads of ef.snp_interior_reads() around them: at least 1000 exact bins (41 reads x 100 bases), and none of them lost to a chance hit"""
    _, l_pac = ef.geometry(oixs["edge.fa"])
    assert len(ef.snp_exact_bins(info_of(oracle, oixs, "edge"), l_pac + 64)[0]) == 0
    inner = ef.snp_interior_reads()
    assert len(inner) == 41 and sum(b"N" in r[1] for r in inner) >= 8 and sum(r[0].endswith("_r") for r in inner) == 20
    for block in ("edge_plus", "mixed_plus"):
        info = info_of(oracle, oixs, block)
        n, _ = ef.guard_snp_exact_bins(info, l_pac + 64, 1000)
        assert n == 4100, n
        first, last = info["kept"][0], info["kept"][-1]
        n_reads = len(ef.snp_block_reads(block))
        assert first[0] == 0 and last[0] == n_reads - 1                  # exact bins from the first and from the last kept sequence
        assert len(info["kept"]) > (128 if block == "edge_plus" else 384)
    # the bins under an other-strand place: six reads of both.fq mapped one at a time
    rd = ef.snp_single_reads(ef.reads("both.fq"))
    assert len(rd) == 6 and sum(b"N" in r[1] for r in rd) == 1
    _, l_pac = ef.geometry(oixs["both.fa"])
    n_other = n_all = 0
    for r in rd:
        info = ef.snp_info(oracle, oixs["both.fa"], [r])
        bins, cov, nuc, other = ef.snp_exact_bins(info, l_pac + 64)
        assert len(bins) == sum(p[2] for p in info["places"])          # its places do not overlap: every covered bin is exact
        n_other += int(other.sum()); n_all += len(bins)
    assert n_other >= 300 and n_all - n_other >= 300, (n_other, n_all)
