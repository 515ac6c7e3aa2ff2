"""The oracle at the edges of the reference, pinned to the UNMODIFIED reference program: the clamped window start b = max(0, c - i)
(inc/align_seq2_raw.cpp:267, the only position one seed can vote for twice), contigs that begin and end inside a 16-base word and
inside a pac byte, the last partial coverage bin.  Fixtures: tests/golden/make_edge_fixtures.py (edge.fa, edge.fq, edge_mixed.fq,
ref_runs_edge/).  The guards of tests/edge_fixture.py are asserted here on the oracle; the GPU tests assert them again before they
compare the device with the oracle."""
import os
import shutil
import subprocess

import pytest

import edge_fixture as ef
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def edge_fa(tmp_path_factory):
    return ef.build_index(tmp_path_factory)


@pytest.fixture(scope="module")
def oix(oracle, edge_fa):
    return oracle.index_load(edge_fa)


@pytest.fixture(scope="module")
def rd():
    return ef.reads()


def test_geometry_is_off_every_word_boundary(oix):
    ef.check_geometry(oix)


@pytest.mark.parametrize("mode", sorted(ef.MANIFEST))
def test_oracle_run_equals_reference_program(mode, oracle, oix, tmp_path):
    m = ef.MANIFEST[mode]
    out = str(tmp_path / "o")
    st = oracle.run(oix, oracle.params(**m["params"]), os.path.join(GOLDEN, m["fastq"]), out, threads=1)
    sam = b"".join(l for l in open(out + ".sam", "rb") if not l.startswith(b"@PG"))
    assert sam == ef.ref_text(mode, "sam"), mode
    assert sam.count(b"\n") == m["sam_lines"]
    for ext in ("sgr", "gmp"):
        if ext in m["tracks"]:
            assert open(out + "." + ext, "rb").read() == ef.ref_text(mode, ext), (mode, ext)
        else:
            assert not os.path.exists(out + "." + ext)
    assert st.n_records == m["sam_lines"] - 3           # 3 @SQ lines


def test_bin1_track_has_the_first_and_last_base_of_every_contig(oix):
    """what the bin-size-1 mode is for: rows for position 1 and for the last position of every contig"""
    ctg, _ = ef.geometry(oix)
    rows = {(f[0], int(f[1])) for f in (l.split(b"\t") for l in ef.ref_text("bin1", "sgr").splitlines())}
    names = sorted({c for c, _ in rows})
    assert len(names) == 3
    for name, (b, e) in zip([oix.contents.contigs[i].name for i in range(3)], ctg):
        assert (name, 1) in rows and (name, e - b) in rows, name


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gnumap_ref")), reason="reference program only exists in the build container")
@pytest.mark.parametrize("mode", ["default", "m14_j7_no_nw", "bs", "mixed"])
def test_fixtures_are_what_the_reference_program_writes_now(mode, tmp_path):
    """the committed fixtures are reproducible: the reference program indexes edge.fa itself, runs, and writes the same bytes"""
    m = ef.MANIFEST[mode]
    for f in ("edge.fa", m["fastq"]):
        shutil.copy(os.path.join(GOLDEN, f), tmp_path)
    r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gnumap_ref"), "-g", "edge.fa", "-o", "r", "-a", "0.9", "-c", "1"] + m["argv"] + [m["fastq"]],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300, env=dict(os.environ, **ef.REF_MALLOC_ENV))
    assert r.returncode == 0, r.stderr[-800:]
    sam = b"".join(l for l in open(tmp_path / "r.sam", "rb") if not l.startswith(b"@PG"))
    assert sam == ef.ref_text(mode, "sam")
    for ext in m["tracks"]:
        assert open(tmp_path / f"r.{ext}", "rb").read() == ef.ref_text(mode, ext)


def test_guard_one_seed_votes_twice_for_the_clamped_start(oracle, oix, rd):
    ores = ef.oracle_results(oracle, oix, oracle.params(mer=14, jump=7, nw=0), rd)
    found = ef.guard_double_vote(oracle, oix, rd, ores)
    assert {ef.parse(rd[i][0])[1] for i in found} >= {20, 23, 40, 60}
    assert {ef.parse(rd[i][0])[4] for i in found} == {"f", "r"}


def test_guards_on_default_parameters(oracle, oix, rd):
    ores = ef.oracle_results(oracle, oix, oracle.params(), rd)
    ef.guard_position_zero(rd, ores)
    ef.guard_contig_ends(oix, rd, ores)
    ef.guard_no_hit_across_a_start(oix, rd, ores)


def test_guard_no_window_across_a_boundary_without_nw(oracle, oix, rd):
    """with votes alone (--no_nw) nothing but the contig test stands between the seeds of a read that hangs off a contig and a hit whose
    window lies across the boundary (a chance hit of a 10-mer elsewhere in the previous contig is a hit like any other)"""
    ores = ef.oracle_results(oracle, oix, oracle.params(nw=0), rd)
    ef.guard_windows_inside_one_contig(oix, rd, ores)
    ef.guard_contig_ends(oix, rd, ores)


def test_guard_single_votes_do_not_map(oracle, oix, rd):
    ef.guard_single_votes(oracle, oix, oracle.params(mer=14, nw=0), rd)
