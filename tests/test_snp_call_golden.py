"""CPU side of the SNP-call column (--snp's ninth .gmp column, GenomeBwt::PrintSNPCall src/GenomeBwt.cpp:1011-1090): the ABI declares and
exports its three entry points, they refuse tracks they cannot work on, and the NumPy / math restatement of the statistic
(tests/snpcall_model.py: closed-form chi-square CDFs, log likelihood ratios) agrees with what the UNMODIFIED reference function, linked
against the reference's own GSL 1.9, returned for tests/golden/ref_vectors_snpcall.npz.  That agreement is what fixes the numbers of the
comparison rule before any GPU run: the device kernel is then held to the same vectors under twice the figures measured here."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import gnumap_amd as g
from gnumap_amd import api
from conftest import GOLDEN, ROOT
import snpcall_model as M

NEW = ["gm_snp_calls", "gm_dev_snp_stat", "gm_coverage_write_gmp_calls"]
GM_E_ARG, GM_E_NO_DEVICE = -1, -3


def test_abi_declares_and_exports_the_snp_call_entry_points():
    src = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = g.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in api.EXPORTS, name
    assert "gm_snp_rec" in src and api.SNP_DTYPE.itemsize == 64
    assert [api.SNP_DTYPE.fields[k][1] for k in ("pos", "contig", "chr_pos", "total", "nuc", "p_val", "ref", "alt1", "alt2", "diploid")] == \
        [0, 8, 16, 24, 28, 48, 56, 57, 58, 59]


def test_entry_points_refuse_unusable_tracks(syn_fa, tmp_path):
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    calls = (lambda: ix.snp_calls(), lambda: ix.coverage_write_gmp_calls(str(tmp_path / "x.gmp")))
    for f in calls:                                     # no track at all
        with pytest.raises(g.GnumapError) as e:
            f()
        assert e.value.code == GM_E_ARG
    ix.coverage_reset(8)                                # bin size other than 1
    for f in calls:
        with pytest.raises(g.GnumapError, match="bin size 1") as e:
            f()
        assert e.value.code == GM_E_ARG
    ix.coverage_reset(1)                                # the right geometry, but nothing to compute on: no quiet host path
    for f in calls + (lambda: ix.dev_snp_stat(np.ones((3, 5), np.float32)),):
        with pytest.raises(g.GnumapError) as e:
            f()
        assert e.value.code == GM_E_NO_DEVICE
    L = g.lib()
    assert L.gm_snp_calls(None, 0.001, 0, None, 0, None, None) == GM_E_ARG
    assert L.gm_dev_snp_stat(ix.h, None, 1, 0, None, None, None, None) == GM_E_ARG
    assert L.gm_coverage_write_gmp_calls(ix.h, 0.001, 0, None, 0) == GM_E_ARG
    assert not os.path.exists(tmp_path / "x.gmp")


def _vectors():
    v = np.load(os.path.join(GOLDEN, "ref_vectors_snpcall.npz"))
    return v, v["counts"].view(np.float32)


def test_vector_set_covers_what_it_should():
    v, cnt = _vectors()
    tot = cnt.astype(np.float64).sum(1)
    p = v["p_dip"].view(np.float64)
    assert len(cnt) > 1000 and tot.max() <= 400.5 and (tot < 0.01).any() and (tot > 300).any()
    assert (v["dip"] == 1).sum() > 100 and (v["pos2_dip"] == -1).sum() > 100 and (v["pos1_dip"] == 4).sum() > 10
    assert (p == 0).sum() > 20 and ((p > 0) & (p < 1e-13)).sum() > 5 and ((p > 1e-9) & (p < 1e-3)).sum() > 50 and (p > 0.01).sum() > 50
    s = np.sort(cnt, 1)
    assert (s[:, 4] == s[:, 3]).sum() >= 40                                             # ties between the maxima
    with np.errstate(divide="ignore", invalid="ignore"):
        r = s[:, 4] / s[:, 3]
    assert ((r > 2.99) & (r < 3.0)).sum() > 50 and ((r > 3.0) & (r < 3.01)).sum() > 50


@pytest.mark.parametrize("monop", [False, True], ids=["diploid", "monop"])
def test_restatement_agrees_with_the_reference_function(monop):
    v, cnt = _vectors()
    p_ref = (v["p_monop"] if monop else v["p_dip"]).view(np.float64)
    skipped = 0
    worst_rel = worst_abs = 0.0
    for i, c in enumerate(cnt):
        p, p1, p2, dip = M.is_snp(c, monop)
        if monop:
            same = p1 == v["pos1_monop"][i] and not dip
        else:
            same = (p1, p2, int(dip)) == (v["pos1_dip"][i], v["pos2_dip"][i], v["dip"][i])
        if not same:
            assert M.on_decision_point(c, p_ref[i], 0.001, monop, M.P_REL), (i, c, (p, p1, p2, dip))
            skipped += 1
            continue
        worst_abs = max(worst_abs, abs(p - p_ref[i]))
        if p_ref[i] > 1e-9:
            worst_rel = max(worst_rel, abs(p - p_ref[i]) / p_ref[i])
        assert M.p_close(p, p_ref[i], M.P_REL), (i, c, p, p_ref[i])
    print(f"monop={monop}: largest relative difference {worst_rel:.3g} (p_ref > 1e-9), largest absolute {worst_abs:.3g}, {skipped} rows left out")
    assert skipped <= M.MAX_SKIPPED_SHARE * len(cnt)
    # the constants are the measurement, not a guess above it
    assert worst_rel <= M.MEASURED_REL * 1.001 and worst_abs <= M.MEASURED_ABS * 1.001


def test_restatement_reproduces_the_reference_runs():
    """the ninth column of the reference program's own files from the counts it printed next to it (five decimals, so lossy: the p-value
    under the run tolerance; letters exact except where the two largest sums are equal at printed precision or a decision point is within
    the band - the text cannot decide those rows, so they are counted and reported, not capped: the cap belongs to the GPU tests)"""
    man = json.load(open(os.path.join(GOLDEN, "ref_runs_snp", "manifest.json")))["runs"]
    for name, m in sorted(man.items()):
        rows = [l.split("\t") for l in gzip.open(os.path.join(GOLDEN, "ref_runs_snp", name + ".gmp.gz"), "rt").read().splitlines()]
        assert len(rows) == m["rows"] and all(len(r) == 9 for r in rows)
        n_call = skipped = n_y1 = n_y2 = 0
        for r in rows:
            cnt = np.array([float(x) for x in r[3:8]], np.float32)
            ref_base = "acgt".index(r[8][2]) if r[8] != "N" else None
            if ref_base is None:
                p, p1, p2, dip = M.is_snp(cnt, m["monop"])
                top2 = np.sort(cnt)[-2:]
                assert not dip or abs(top2[1] - top2[0]) <= 2e-5 or M.on_decision_point(cnt, p, m["pval"], m["monop"], M.RUN_REL, ratio_rel=1e-4), r
                continue
            n_call += 1
            want, p_ref = M.parse_call(r[8])
            n_y1 += want[0] == "Y" and want[3] is None; n_y2 += want[0] == "Y" and want[3] is not None
            got = M.parse_call(M.call_text(cnt, ref_base, m["pval"], m["monop"]))
            top2 = np.sort(cnt)[-2:]
            if got is None or got[0] != want:
                assert abs(top2[1] - top2[0]) <= 2e-5 or M.on_decision_point(cnt, p_ref, m["pval"], m["monop"], M.RUN_REL, ratio_rel=1e-4), (name, r, got)
                skipped += 1
                continue
            assert M.p_close(got[1], p_ref, M.RUN_REL), (name, r, got)
        print(f"{name}: {n_call} rows with a call, {skipped} undecidable from the printed counts")
        assert n_call == m["calls"]
        if m["fastq"] == "syn_snp.fq":
            assert n_y1 >= 1 and (m["monop"] or n_y2 >= 1)
