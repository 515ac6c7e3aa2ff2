"""The oracle's unique map on repeat-rich reads, pinned to the UNMODIFIED reference program: process_hits' groups, their std::map order,
the position sets and the -T / -u exits (inc/align_seq2_raw.cpp:102-165, :299-306) where a read has 2 .. 3001 accepted hits in one key or
in thousands.  Fixtures: tests/golden/make_repeat_fixtures.py (rep.fa.gz, rep.fq.gz, rep_limit.fq, ref_runs_repeat/).  The guards of
tests/repeat_fixture.py are asserted here on the oracle; tests/test_gpu_repeat_groups.py asserts them again before it compares the
device with the oracle."""
import os
import shutil
import subprocess

import pytest

import repeat_fixture as rf
from conftest import ROOT


@pytest.fixture(scope="module")
def rep_fa(tmp_path_factory):
    return rf.build_index(tmp_path_factory)


@pytest.fixture(scope="module")
def oix(oracle, rep_fa):
    return oracle.index_load(rep_fa)


@pytest.fixture(scope="module")
def rd():
    return rf.reads()


@pytest.fixture(scope="module")
def ores(oracle, oix, rd):
    return rf.oracle_results(oracle, oix, oracle.params(), rd)


def test_geometry_is_off_every_word_boundary(oix):
    assert rf.check_geometry(oix) > 500000


@pytest.mark.parametrize("mode", sorted(rf.MANIFEST))
def test_oracle_run_equals_reference_program(mode, oracle, oix, rep_fa, tmp_path):
    m = rf.MANIFEST[mode]
    out = str(tmp_path / "o")
    st = oracle.run(oix, oracle.params(**m["params"]), rf.fastq_path(rep_fa, m["fastq"]), out, threads=1)
    sam = b"".join(l for l in open(out + ".sam", "rb") if not l.startswith(b"@PG"))
    assert sam == rf.ref_text(mode, "sam"), mode                   # record order included
    assert sam.count(b"\n") == m["sam_lines"]
    assert m["tracks"] == ["sgr"] and not os.path.exists(out + ".gmp")
    assert open(out + ".sgr", "rb").read() == rf.ref_text(mode, "sgr"), mode
    assert st.n_records == m["sam_lines"] - 3                      # 3 @SQ lines


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gnumap_ref")), reason="reference program only exists in the build container")
@pytest.mark.parametrize("mode", ["default", "u_no_nw", "limit_T3001"])
def test_fixtures_are_what_the_reference_program_writes_now(mode, rep_fa, tmp_path):
    """the committed fixtures are reproducible: the reference program indexes rep.fa itself, runs, and writes the same bytes"""
    m = rf.MANIFEST[mode]
    for f in ("rep.fa", m["fastq"]):
        shutil.copy(rf.fastq_path(rep_fa, f), tmp_path)
    r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gnumap_ref"), "-g", "rep.fa", "-o", "r", "-a", "0.9", "-c", "1"] + m["argv"] + [m["fastq"]],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300, env=dict(os.environ, **rf.REF_MALLOC_ENV))
    assert r.returncode == 0, r.stderr[-800:]
    sam = b"".join(l for l in open(tmp_path / "r.sam", "rb") if not l.startswith(b"@PG"))
    assert sam == rf.ref_text(mode, "sam")
    assert open(tmp_path / "r.sgr", "rb").read() == rf.ref_text(mode, "sgr")


def test_guard_hit_counts_at_every_boundary(rd, ores):
    got = rf.guard_hit_counts(rd, ores)
    print("accepted hits -> reads:", got)


def test_guard_same_key_reads_have_one_key(rd, ores):
    rf.guard_one_key(rd, ores)


def test_guard_keys_that_tie_on_their_first_word(rd, ores):
    print(rf.guard_tie_family(rd, ores))


def test_guard_keys_that_differ_in_their_first_word(rd, ores):
    rf.guard_first_word_family(rd, ores)


def test_guard_long_keys_differ_beyond_word_18(rd, ores):
    rf.guard_long_keys(rd, ores)


def test_guard_groups_with_both_strands(rd, ores):
    print("groups with both strands, first hit not the lowest place:", rf.guard_both_strand_groups(rd, ores))


def test_guard_palindrome_holds_both_strands_of_every_copy(rd, ores):
    rf.guard_palindrome(rd, ores)


def test_guard_set_limit_reads(oracle, oix):
    assert rf.guard_set_limit(oracle, oix) == (3000, 3001)


def test_guard_T_met_exactly_and_missed_by_one(oracle, oix, rd):
    rf.guard_T_pair(oracle, oix, rd)


def test_guard_denominator_depends_on_processing_order(oracle, oix, rd, ores):
    print("reads whose denominator changes with the order of the additions:", len(rf.guard_order_sensitive(oracle, oix, rd, ores)))
