"""The SNP-call column of --snp's .gmp on the device (k_snp_call, gnumap_amd/csrc/gm_snpcall.hip) = GenomeBwt::PrintSNPCall
(src/GenomeBwt.cpp:1011-1090) with is_snp / LRT / dipLRT behind it, through the C ABI and the driver binary:

  1. gm_dev_snp_stat against what the UNMODIFIED reference function (with the reference's own GSL 1.9) returned for
     tests/golden/ref_vectors_snpcall.npz, both ploidy settings;
  2. synthetic tracks written straight into the HBM tracks: gm_coverage_write_gmp_calls against a Python formatter over the same arrays
     (tests/snpcall_model.py, itself pinned to the reference function by tests/test_snp_call_golden.py), its first eight columns against
     gm_coverage_write_gmp's bytes, gm_snp_calls against the file's 'Y' rows;
  3. the driver with --snp --snp_calls (and --snp_monop, --snp_pval=0.05) on tests/golden/syn_snp.fq against the nine-column files the
     unmodified reference PROGRAM wrote (tests/golden/ref_runs_snp/).

Comparison rule of the ninth column: letters exact; p-values |p - p_ref| <= rel * p_ref + floor with the measured constants of
snpcall_model.py; a row may be left out of the letter comparison only on a decision point (or, in 3, where the deposited sums differ
enough between the two programs to move it across), and such rows are capped at 0.5 % of the rows that carry a call."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
from gnumap_amd import api
from conftest import GOLDEN, ROOT
from test_gpu_driver_golden import compare_tracks
import snpcall_model as M

pytestmark = pytest.mark.gpu
GM_MODE_SNP = 5
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
RUNS = os.path.join(GOLDEN, "ref_runs_snp")


@pytest.fixture(scope="module")
def ix_full(syn_fa):
    return g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("monop", [False, True], ids=["diploid", "monop"])
def test_dev_snp_stat_against_the_reference_function(ix_full, monop):
    v = np.load(os.path.join(GOLDEN, "ref_vectors_snpcall.npz"))
    cnt = v["counts"].view(np.float32)
    p_ref = (v["p_monop"] if monop else v["p_dip"]).view(np.float64)
    p, p1, p2, dip = ix_full.dev_snp_stat(cnt, monop)
    skipped = 0
    worst_rel = worst_abs = 0.0
    for i in range(len(cnt)):
        if monop:
            same = p1[i] == v["pos1_monop"][i] and p2[i] == -1 and dip[i] == 0
        else:
            same = (p1[i], p2[i], dip[i]) == (v["pos1_dip"][i], v["pos2_dip"][i], v["dip"][i])
        if not same:
            assert M.on_decision_point(cnt[i], p_ref[i], 0.001, monop, M.P_REL), (i, cnt[i], (p[i], p1[i], p2[i], dip[i]))
            skipped += 1
            continue
        worst_abs = max(worst_abs, abs(p[i] - p_ref[i]))
        if p_ref[i] > 1e-9:
            worst_rel = max(worst_rel, abs(p[i] - p_ref[i]) / p_ref[i])
    print(f"monop={monop}: device vs reference function: largest relative difference {worst_rel:.3g} (p_ref > 1e-9), largest absolute {worst_abs:.3g}, "
          f"{skipped} rows left out; allowed {M.P_REL:.3g} / {M.P_FLOOR:.3g}")
    for i in range(len(cnt)):
        assert M.p_close(p[i], p_ref[i], M.P_REL) or M.on_decision_point(cnt[i], p_ref[i], 0.001, monop, M.P_REL), (i, cnt[i], p[i], p_ref[i])
    assert skipped <= M.MAX_SKIPPED_SHARE * len(cnt)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def _synthetic_tracks(bins, l_pac, contigs):
    """seeded: cov[bins], nuc[5, bins] with covered runs on both sides of every contig boundary, at the first and the last position, totals
    from 0.002 to 5000, the print threshold from both sides, every kind of composition"""
    rng = np.random.default_rng(11)
    cov = np.zeros(bins, np.float32); nuc = np.zeros((5, bins), np.float32)
    where = [np.arange(0, 40), np.arange(l_pac - 40, l_pac)]
    for _, off in contigs[1:]:
        where.append(np.arange(off - 60, off + 60))
    where.append(rng.choice(l_pac, 6000, replace=False))
    pos = np.unique(np.concatenate(where))
    for k in pos:
        kind = rng.integers(6)
        total = float(np.exp(rng.uniform(np.log(0.002), np.log(400))))
        if kind == 0:
            c = rng.dirichlet(np.full(5, 0.3)) * total
        elif kind == 1:
            e = rng.uniform(0, 0.03); c = np.array([1 - e, e / 2, e / 4, e / 4, 0])[rng.permutation(5)] * total
        elif kind == 2:
            f = rng.choice([0.5, 0.6, 0.7, 0.74, 0.76]); c = np.array([f, 0.99 - f, 0.005, 0.005, 0])[rng.permutation(5)] * total
        elif kind == 3:
            total = float(rng.choice([1000.0, 5000.0])) * rng.uniform(0.9, 1.1)
            f = rng.choice([1.0, 0.5, 0.7, 0.97]); c = np.array([f, 1 - f, 0, 0, 0])[rng.permutation(5)] * total
        elif kind == 4:
            a = total / 2.1; c = np.array([a, a, 0.1 * a, 0, 0])[rng.permutation(5)]
        else:
            c = np.array([0.02, 0.02, 0.03, 0.03, 0.9]) * total
        nuc[:, k] = c.astype(np.float32)
        cov[k] = np.float32(nuc[:, k].astype(np.float64).sum())
    thr = np.float32(0.001)
    edge = pos[100:106]
    cov[edge[0]] = np.nextafter(thr, np.float32(0)); cov[edge[1]] = thr; cov[edge[2]] = np.nextafter(thr, np.float32(1))      # only the last one prints
    cov[edge[3]] = 1000.0; nuc[:, edge[3]] = [0, 1000.0, 0, 0, 0]
    cov[edge[4]] = 5000.0; nuc[:, edge[4]] = [2500.0, 0, 2400.0, 100.0, 0]
    cov[edge[5]] = 5000.0; nuc[:, edge[5]] = [0, 0, 0, 5000.0, 0]
    cov[l_pac:] = 7.0; nuc[:, l_pac:] = 1.0            # the tail past the reference never prints
    return cov, nuc


def _upload(ix, cov, nuc):
    import torch
    from gnumap_amd import dist as gd
    dev = torch.device("cuda", 0)
    gd.DeviceTrack(ix.coverage_device_ptr(), len(cov)).tensor(dev).copy_(torch.from_numpy(cov))
    gd.DeviceTrack(ix.coverage_nuc_device_ptr(), 5 * len(cov)).tensor(dev).copy_(torch.from_numpy(nuc.reshape(-1)))
    torch.cuda.synchronize()


def _expected_rows(cov, nuc, l_pac, contigs, genome, pval, monop):
    """[(contig, pos, [six %.5f strings], call text or 'N', letters, p as a double, counts)] for every printed position"""
    rows = []
    offs = [o for _, o in contigs] + [l_pac]
    for k in np.nonzero(cov[:l_pac] > np.float32(0.001))[0]:
        ci = int(np.searchsorted(offs, k, side="right")) - 1
        cnt = nuc[:, k]
        ref_base = "acgt".index(chr(genome[k]))
        p, p1, p2, dip = M.is_snp(cnt, monop)
        text = M.call_text(cnt, ref_base, pval, monop)
        rows.append((contigs[ci][0], int(k - offs[ci] + 1), ["%.5f" % cov[k]] + ["%.5f" % x for x in cnt], text, M.parse_call(text), p, cnt, int(k), ci, ref_base))
    return rows


@pytest.mark.parametrize("monop,pval", [(False, 0.001), (True, 0.001), (False, 0.05)], ids=["diploid", "monop", "pval05"])
def test_writer_and_call_list_on_synthetic_tracks(ix_full, syn_fa, tmp_path, monop, pval):
    L = g.lib()
    l_pac = int(ix_full.info.l_pac); contigs = ix_full.contigs()
    pac = np.fromfile(syn_fa + ".gnumap.pac", np.uint8)                                  # 2 bits per base, four per byte, first base highest
    genome = bytes(b"acgt"[(pac[k >> 2] >> ((~k & 3) << 1)) & 3] for k in range(l_pac))
    assert genome[150000:150040] == ix_full.window(150000, 40)
    ix_full.coverage_reset(1); ix_full.coverage_enable_nuc()
    bins = ix_full.coverage_bins()
    cov, nuc = _synthetic_tracks(bins, l_pac, contigs)
    _upload(ix_full, cov, nuc)
    want = _expected_rows(cov, nuc, l_pac, contigs, genome, pval, monop)
    n_y = sum(1 for w in want if w[4] and w[4][0][0] == "Y"); n_ydip = sum(1 for w in want if w[4] and w[4][0][0] == "Y" and w[4][0][3])
    assert len(want) > 6000 and n_y > 1000 and (monop or n_ydip > 500) and sum(1 for w in want if w[3] == "N") > 300       # the inputs are worth the run
    # the eight-column file of the same arrays
    eight = str(tmp_path / "eight.gmp")
    p5 = g.Params(mode=GM_MODE_SNP)
    assert L.gm_coverage_write_gmp(ix_full.h, C.byref(p5.c), cov.ctypes.data, np.ascontiguousarray(nuc).ctypes.data, eight.encode(), 0) == 0
    eight_lines = open(eight).read().splitlines()
    texts = []
    try:
        for slice_bins in (None, b"4096", b"7001"):            # 7001 x threads does not divide the 280000 positions
            assert L.gm_set_option(b"GM_TRACK_SLICE", slice_bins) == 0
            out = str(tmp_path / "nine.gmp")
            ix_full.coverage_write_gmp_calls(out, pval, monop)
            texts.append(open(out).read())
            calls = ix_full.snp_calls(pval, monop)
            _check_file_and_calls(texts[-1], eight_lines, want, calls, pval, monop, contigs)
    finally:
        assert L.gm_set_option(b"GM_TRACK_SLICE", None) == 0
    assert texts[0] == texts[1] == texts[2]                   # the text does not depend on the slicing
    # capacity protocol of gm_snp_calls
    n_y = sum(1 for l in texts[0].splitlines() if l.split("\t")[8].startswith("Y"))
    got = C.c_uint64(); one = np.zeros(1, api.SNP_DTYPE)
    assert L.gm_snp_calls(ix_full.h, pval, int(monop), one.ctypes.data, 1, C.byref(got), None) == api.GM_E_CAPACITY and got.value == n_y > 1
    assert L.gm_snp_calls(ix_full.h, pval, int(monop), None, 0, C.byref(got), None) == api.GM_E_CAPACITY and got.value == n_y
    ix_full.coverage_reset(8)


def _check_file_and_calls(text, eight_lines, want, calls, pval, monop, contigs):
    lines = text.splitlines()
    assert len(lines) == len(want) == len(eight_lines)
    skipped = n_call = 0
    y_rows = []
    for line, e8, w in zip(lines, eight_lines, want):
        f = line.split("\t")
        assert len(f) == 9 and "\t".join(f[:8]) == e8, (line, e8)                       # gm_coverage_write_gmp's bytes
        assert f[0] == w[0] and int(f[1]) == w[1] and f[2:8] == w[2], (line, w)
        mine = M.parse_call(f[8])
        n_call += w[4] is not None
        total = float(f[2])
        if mine is not None and total > 400:
            assert np.isfinite(mine[1]) and 0.0 <= mine[1] <= 1.0, line
        if mine is not None and mine[0][0] == "Y":
            y_rows.append((f, mine, w))
        if (mine is None) != (w[4] is None) or (mine is not None and mine[0] != w[4][0]):
            assert M.on_decision_point(w[6], w[5], pval, monop, M.P_REL), (line, w[3])
            skipped += 1
            continue
        if mine is not None:
            assert M.p_close(mine[1], w[4][1], M.TEXT_REL), (line, w[3])
    assert skipped <= M.MAX_SKIPPED_SHARE * n_call, (skipped, n_call)
    # gm_snp_calls: exactly the file's 'Y' rows, in order
    assert len(calls) == len(y_rows) > 100
    assert (np.diff(calls["pos"].astype(np.int64)) > 0).all()
    for r, (f, mine, w) in zip(calls, y_rows):
        assert contigs[int(r["contig"])][0] == f[0] and int(r["chr_pos"]) == int(f[1]) and int(r["pos"]) == w[7]
        assert ["%.5f" % r["total"]] + ["%.5f" % x for x in r["nuc"]] == f[2:8]
        letters = ("Y", "acgt"[r["ref"]], "acgtn"[r["alt1"]], "acgtn"[r["alt2"]] if r["diploid"] else None)
        assert letters == mine[0] and (r["alt2"] == 255) == (not r["diploid"]), (r, f)
        assert "%.2e" % r["p_val"] == f[8].split("p_val=")[1] and 0.0 <= r["p_val"] < float(np.float32(pval))


def test_p_values_above_a_total_of_400_are_finite(ix_full):
    """beyond the reference's reach (its pow() underflows to 0 / 0 from a total of about 440): finite, in [0, 1], and monotone in the evidence"""
    rng = np.random.default_rng(3)
    tot = np.exp(rng.uniform(np.log(400), np.log(2e5), 4000))
    shares = rng.dirichlet(np.full(5, 0.4), 4000)
    cnt = (shares * tot[:, None]).astype(np.float32)
    for monop in (False, True):
        p, p1, p2, dip = ix_full.dev_snp_stat(cnt, monop)
        assert np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all()
        assert (p1 == cnt.argmax(1)).all()
    hom = np.zeros((6, 5), np.float32); hom[:, 2] = [10, 100, 440, 470, 5000, 1e6]
    p, _, _, dip = ix_full.dev_snp_stat(hom, False)
    assert (np.diff(p) <= 0).all() and p[0] > 0 and p[2] == 0 and p[-1] == 0 and not dip.any()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def _gmp_rows(text):
    d = {}
    for line in text.splitlines():
        f = line.split("\t")
        assert len(f) == 9, line
        d[(f[0], int(f[1]))] = f
    return d


def _allowance(x):
    return 1e-4 * max(1.0, abs(x)) + 2e-5            # compare_tracks' per-number tolerance


@pytest.mark.parametrize("name", ["snp", "snp_monop", "snp_pval05", "snp_synfq"])
def test_cli_snp_calls_against_the_reference_program(name, tmp_path, syn_fa):
    m = json.load(open(os.path.join(RUNS, "manifest.json")))["runs"][name]
    ref_text = gzip.open(os.path.join(RUNS, name + ".gmp.gz"), "rt").read()
    ref = _gmp_rows(ref_text)
    ref_calls = [M.parse_call(f[8]) for f in ref.values() if f[8] != "N"]
    if m["fastq"] == "syn_snp.fq":      # the test cannot pass on an all-N file
        assert any(c[0][0] == "Y" and c[0][3] is None for c in ref_calls) and (m["monop"] or any(c[0][0] == "Y" and c[0][3] for c in ref_calls))
    out = str(tmp_path / "mine")
    r = subprocess.run([EXE, "-g", syn_fa, "-o", out, "-a", "0.9"] + m["argv"] + ["--snp_calls", os.path.join(GOLDEN, m["fastq"])], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-1500:]
    sam = "".join(l for l in open(out + ".sam") if not l.startswith("@PG"))
    sam_ref = os.path.join(RUNS, "snp.sam.gz") if m["fastq"] == "syn_snp.fq" else os.path.join(GOLDEN, "ref_runs", "default.sam.gz")
    assert sam == gzip.open(sam_ref, "rt").read()
    assert not os.path.exists(out + ".sgr")
    mine_text = open(out + ".gmp").read()
    mine = _gmp_rows(mine_text)
    strip = lambda rows: "".join("\t".join(f[:8]) + "\n" for f in rows.values())
    compare_tracks(strip(mine), strip(ref), 8)
    skipped = n_call = 0
    for k in set(mine) & set(ref):
        a, b = mine[k], ref[k]
        ca, cb = M.parse_call(a[8]), M.parse_call(b[8])
        n_call += cb is not None
        cnt = np.array([float(x) for x in b[3:8]], np.float32)
        if (ca is None) != (cb is None) or (ca is not None and ca[0] != cb[0]):
            top = np.sort(cnt)[-2:]
            p_ref = cb[1] if cb is not None else M.is_snp(cnt, m["monop"])[0]
            tie = abs(float(top[1]) - float(top[0])) <= _allowance(top[1]) + _allowance(top[0])
            ratio_rel = 2 * (_allowance(top[1]) / max(float(top[1]), 1e-30) + _allowance(top[0]) / max(float(top[0]), 1e-30))
            assert tie or M.on_decision_point(cnt, p_ref, m["pval"], m["monop"], M.RUN_REL, ratio_rel=ratio_rel), (a, b)
            skipped += 1
            continue
        if cb is not None:
            assert M.p_close(ca[1], cb[1], M.RUN_REL), (a, b)
    print(f"{name}: {n_call} rows with a call, {skipped} left out of the letter comparison")
    assert n_call > 50 and skipped <= M.MAX_SKIPPED_SHARE * n_call, (skipped, n_call)


def test_cli_flags_without_snp_calls_change_nothing(tmp_path, syn_fa):
    """--snp alone still writes eight columns; --snp_pval / --snp_monop are accepted and, as in a reference run, change only the column
    that is not there"""
    fq = os.path.join(GOLDEN, "syn_snp.fq")
    outs = []
    for i, extra in enumerate(([], ["--snp_pval=0.05", "--snp_monop"])):
        out = str(tmp_path / f"o{i}")
        r = subprocess.run([EXE, "-g", syn_fa, "-o", out, "-a", "0.9", "--snp"] + extra + [fq], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-1500:]
        outs.append(open(out + ".gmp").read())
        assert all(len(l.split("\t")) == 8 for l in outs[-1].splitlines()) and len(outs[-1].splitlines()) > 5000
    compare_tracks(outs[0], outs[1], 8)
    ref = gzip.open(os.path.join(RUNS, "snp.gmp.gz"), "rt").read()
    compare_tracks(outs[0], "".join("\t".join(l.split("\t")[:8]) + "\n" for l in ref.splitlines()), 8)
    r = subprocess.run([EXE, "-g", syn_fa, "-o", str(tmp_path / "bad"), "--snp", "--snp_pval=abc", fq], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "snp_pval" in r.stderr
