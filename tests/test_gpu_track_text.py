"""<out>.sgr and the eight-column <out>.gmp formatted on the device (k_track_sizes / k_track_rows, gnumap_amd/csrc/gm_tracktext.hip;
gm_coverage_write_sgr_device, gm_coverage_write_gmp_device, gm_coverage_text) against the host writers' bytes (gm_coverage_write_sgr /
_gmp, pinned to printf by tests/test_track_text.py and to the reference program by tests/test_gpu_driver_golden.py):

  1. .sgr on syn.fa, bin sizes 8, 1 and 3 (bins straddle the contig boundaries), three slab sizes, append mode;
  2. .gmp in the modes BS, BS2, ATOG, ATOG2 and SNP: the base filter on the 2-bit reference, "%f" of the total, both thresholds;
  3. gm_coverage_text on ranges: whole, empty, inside a tile, one bin on each side of every contig boundary; the capacity protocol;
  4. values only snprintf prints (>= 1e9, inf, negative, NaN): their slabs - and no other - are formatted by the host emitters;
  5. generated genomes with a 37-base contig under a 200-character name and names longer than a tile's LDS window.  With contig
     lengths 1000, 37, 5000 bin 16 of size 64 starts at 1024, inside the short contig, which so gets one row; with 1030, 37, 5000 no bin
     of size 64 starts in [1030, 1067) and the contig gets no row, exactly as with the host writer;
  6. the driver with --track_text=device against the reference program's files.

Fixed tracks are written straight into the HBM tracks, so 1-5 compare bytes.  Every value of 1, 2, 3 and 5 lies in [0, 1e9): there
host_slabs must be 0 - a host-formatted slab would hide the kernel."""
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

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
GM_E_ARG, GM_E_CAPACITY = -1, -5
MODES = {"bs": 1, "b2": 2, "atog": 3, "atog2": 4, "snp": 5}
SLICES = (None, 4096, 7001)
DEFAULT_SLICE = 1 << 24


def _values(n, rng):
    """the recipe of tests/test_track_text.py: decimal ties at 5 and 6 places, the thresholds and their neighbours, zeros"""
    v = rng.random(n).astype(np.float32) * np.float32(40.0)
    v[::7] = (rng.integers(0, 1 << 20, len(v[::7])) / np.float32(1 << 14)).astype(np.float32)
    v[::11] = np.float32(0.001)
    v[1::11] = np.nextafter(np.float32(0.001), np.float32(1))
    v[2::11] = np.float32(0.0)
    v[3::11] = np.float32(0.015625); v[4::11] = np.float32(2.5e-6); v[5::11] = np.float32(123456.789); v[6::11] = np.float32(8.0)
    v[7::11] = np.float32(0.000015); v[8::11] = np.float32(99999.995)
    return v


def _upload(ix, cov, nuc=None):
    import torch
    from gnumap_amd import dist as gd
    dev = torch.device("cuda", 0)
    gd.DeviceTrack(ix.coverage_device_ptr(), len(cov)).tensor(dev).copy_(torch.from_numpy(cov))
    if nuc is not None:
        gd.DeviceTrack(ix.coverage_nuc_device_ptr(), 5 * len(cov)).tensor(dev).copy_(torch.from_numpy(nuc.reshape(-1)))
    torch.cuda.synchronize()


def _tracks(ix, bs, seed, with_nuc):
    """fresh tracks of this bin size in HBM, filled from the recipe; returns (cov, nuc or None)"""
    ix.coverage_reset(bs)
    if with_nuc:
        ix.coverage_enable_nuc()
    bins = ix.coverage_bins()
    rng = np.random.default_rng(seed)
    cov = _values(bins, rng)
    nuc = _values(5 * bins, rng) if with_nuc else None
    _upload(ix, cov, nuc)
    return cov, nuc


def _host_file(ix, p, cov, nuc, path):
    L = g.lib()
    L.gm_coverage_write_sgr.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    L.gm_coverage_write_gmp.argtypes = [C.c_void_p, C.POINTER(api.gm_params), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    if p is None:
        assert L.gm_coverage_write_sgr(ix.h, cov.ctypes.data, os.fsencode(path), 0) == 0
    else:
        assert L.gm_coverage_write_gmp(ix.h, C.byref(p.c), cov.ctypes.data, nuc.ctypes.data, os.fsencode(path), 0) == 0
    return open(path, "rb").read()


def _device_file(ix, p, path, append=False):
    if p is None:
        ix.coverage_write_sgr_device(path, append)
    else:
        ix.coverage_write_gmp_device(p.c, path, append)
    return open(path, "rb").read()


def ix_fa(ix):
    return os.path.join(GOLDEN, "syn.fa")


def _n_printed_bins(ix, bs):
    return (ix.info.l_pac + bs - 1) // bs


def _every_slab_size(ix, p, bs, want, tmp_path):
    """the device file under the three slab sizes: the host writer's bytes each time, and not one slab formatted by the host"""
    nbk = _n_printed_bins(ix, bs)
    for sl in SLICES:
        g.set_option("GM_TRACK_SLICE", sl)
        try:
            got = _device_file(ix, p, str(tmp_path / f"dev{sl}"))
            st = ix.coverage_text_stats()
        finally:
            g.set_option("GM_TRACK_SLICE", None)
        assert got == want, (sl, len(got), len(want))
        per = sl or DEFAULT_SLICE
        assert st["host_slabs"] == 0, st
        assert st["slabs"] == (nbk + per - 1) // per and st["bytes"] == len(want) and st["rows"] == want.count(b"\n"), st
        assert st["launches"] == 3 * st["slabs"] and st["kernel_ms"] > 0, st


@pytest.fixture(scope="module")
def ix(syn_fa):
    x = g.Index(syn_fa)
    yield x
    x.close()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [8, 1, 3])
def test_sgr_equals_the_host_writer(ix, bs, tmp_path):
    cov, _ = _tracks(ix, bs, 100 + bs, False)
    down = ix.coverage_download()
    assert np.array_equal(down.view(np.uint32), cov.view(np.uint32))
    want = _host_file(ix, None, down, None, str(tmp_path / "host.sgr"))
    contigs = ix.contigs()
    offs = np.array([o for _, o in contigs], np.int64)
    count = np.arange(_n_printed_bins(ix, bs), dtype=np.int64) * bs
    ci = np.searchsorted(offs, count, side="right") - 1
    py = "".join("%s\t%d\t%.5f\n" % (contigs[ci[k]][0], count[k] - offs[ci[k]] + 1, float(cov[k])) for k in range(len(count)) if float(cov[k]) > 0.001)
    assert want == py.encode() and want.count(b"\n") > 1000
    if bs == 3:          # some bin starts in one contig and ends in the next
        assert any(o % 3 for o in offs[1:])
    _every_slab_size(ix, None, bs, want, tmp_path)
    out = str(tmp_path / "twice.sgr")
    for sl in (None, 4096):
        g.set_option("GM_TRACK_SLICE", sl)
        try:
            assert _device_file(ix, None, out) == want
            assert _device_file(ix, None, out, append=True) == 2 * want
        finally:
            g.set_option("GM_TRACK_SLICE", None)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,bs", [("bs", 1), ("b2", 1), ("atog", 1), ("atog2", 1), ("snp", 1), ("bs", 3)])
def test_gmp_equals_the_host_writer(ix, mode, bs, tmp_path):
    p = g.Params(mode=MODES[mode])
    cov, nuc = _tracks(ix, bs, 200 + MODES[mode] + bs, True)
    want = _host_file(ix, p, cov, nuc, str(tmp_path / "host.gmp"))
    rows = want.split(b"\n")[:-1]
    assert len(rows) > 10000 and all(r.count(b"\t") == 7 for r in rows[:2000])
    if mode == "snp":    # 0.001f itself is not above the threshold, its successor is; "%.5f" of the total
        assert len(rows) == int((cov[:_n_printed_bins(ix, bs)] > np.float32(0.001)).sum())
    else:                # every positive total at a position of the mode's base; "%f" of the total
        totals = {r.split(b"\t")[2] for r in rows}
        assert totals & {b"0.000002", b"0.000003"} and b"0.001000" in totals
    _every_slab_size(ix, p, bs, want, tmp_path)
    assert _device_file(ix, p, str(tmp_path / "dev4096"), append=True) == 2 * want


def test_gmp_device_needs_the_mode_and_the_nucleotide_tracks(syn_fa, tmp_path):
    x = g.Index(syn_fa)
    try:
        L = g.lib()
        L.gm_last_error.restype = C.c_char_p
        x.coverage_reset(1)
        out = os.fsencode(str(tmp_path / "o.gmp"))
        assert L.gm_coverage_write_gmp_device(x.h, C.byref(g.Params(mode=5).c), out, 0) == GM_E_ARG           # no gm_coverage_enable_nuc
        assert b"gm_coverage_write_gmp_device" in L.gm_last_error()
        got = C.c_uint64()
        assert L.gm_coverage_text(x.h, C.byref(g.Params(mode=1).c), 0, 10, None, 0, C.byref(got)) == GM_E_ARG
        assert b"gm_coverage_text" in L.gm_last_error()
        x.coverage_enable_nuc()
        assert L.gm_coverage_write_gmp_device(x.h, C.byref(g.Params().c), out, 0) == GM_E_ARG                 # normal mode writes an .sgr
        assert not os.path.exists(out)
    finally:
        x.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def _lines_per_bin(whole, printed):
    """text of every bin: the lines of `whole` dealt to the bins that print, in order"""
    lines = whole.split(b"\n")[:-1]
    assert len(lines) == int(printed.sum())
    per = [b""] * len(printed)
    for k, ln in zip(np.nonzero(printed)[0], lines):
        per[k] = ln + b"\n"
    return per


@pytest.mark.parametrize("mode,bs", [(None, 3), ("snp", 1), ("atog", 1)])
def test_coverage_text_ranges(ix, mode, bs, tmp_path):
    p = g.Params(mode=MODES[mode]) if mode else None
    cov, nuc = _tracks(ix, bs, 300 + bs, mode is not None)
    firsts = [(o + bs - 1) // bs for _, o in ix.contigs()[1:]]          # the first bin that starts in a contig
    for kb in firsts:                                                    # a total that prints on both sides of every boundary
        cov[kb - 1] = np.float32(7.25); cov[kb] = np.float32(0.5)
    _upload(ix, cov, nuc)
    whole = _host_file(ix, p, cov, nuc, str(tmp_path / "host"))
    bins, nbk = ix.coverage_bins(), _n_printed_bins(ix, bs)
    assert ix.coverage_text(p, 0, bins) == whole and ix.coverage_text(p) == whole
    assert ix.coverage_text_stats()["host_slabs"] == 0
    if mode is None:
        printed = cov[:nbk].astype(np.float64) > 0.001
    elif mode == "snp":
        printed = cov[:nbk] > np.float32(0.001)
    else:
        pac = np.fromfile(ix_fa(ix) + ".gnumap.pac", np.uint8)
        k = np.arange(nbk, dtype=np.int64)
        printed = (((pac[k >> 2] >> ((~k & 3) << 1)) & 3) == "acgt".index("a")) & (cov[:nbk] > np.float32(0.0))
    per = _lines_per_bin(whole, printed)
    ranges = [(1000, 1000), (0, 0), (bins, bins), (77, 203), (131, 1500), (nbk - 1, nbk), (nbk, bins), (nbk - 300, bins)]
    for kb in firsts:
        ranges += [(kb - 1, kb), (kb, kb + 1), (kb - 1, kb + 1), (kb - 257, kb + 257)]
    for sl in (None, 4096):
        g.set_option("GM_TRACK_SLICE", sl)
        try:
            for lo, hi in ranges:
                assert ix.coverage_text(p, lo, hi) == b"".join(per[lo:min(hi, nbk)]), (sl, lo, hi)
        finally:
            g.set_option("GM_TRACK_SLICE", None)
    assert ix.coverage_text(p, 1000, 1000) == b"" and (mode == "atog" or all(per[kb - 1] and per[kb] for kb in firsts))
    # the capacity protocol of gm_snp_calls: the size first, and nothing behind cap is touched
    L = g.lib()
    pp = C.byref(p.c) if p else None
    lo, hi = 131, 1500
    want = b"".join(per[lo:hi])
    got = C.c_uint64()
    assert L.gm_coverage_text(ix.h, pp, lo, hi, None, 0, C.byref(got)) == GM_E_CAPACITY and got.value == len(want)
    buf = np.full(len(want) + 64, 0xAA, np.uint8)
    assert L.gm_coverage_text(ix.h, pp, lo, hi, buf.ctypes.data, len(want) - 1, C.byref(got)) == GM_E_CAPACITY and got.value == len(want)
    assert buf[:len(want) - 1].tobytes() == want[:-1] and (buf[len(want) - 1:] == 0xAA).all()
    assert L.gm_coverage_text(ix.h, pp, lo, hi, buf.ctypes.data, len(want), C.byref(got)) == 0 and got.value == len(want)
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
    g.set_option("GM_TRACK_SLICE", 512)            # the buffer ends in the middle of a later slab
    try:
        buf[:] = 0xAA
        cap = len(want) * 2 // 3
        assert L.gm_coverage_text(ix.h, pp, lo, hi, buf.ctypes.data, cap, C.byref(got)) == GM_E_CAPACITY and got.value == len(want)
        assert buf[:cap].tobytes() == want[:cap] and (buf[cap:] == 0xAA).all()
    finally:
        g.set_option("GM_TRACK_SLICE", None)
    assert L.gm_coverage_text(ix.h, pp, 5, 4, None, 0, C.byref(got)) == GM_E_ARG
    assert L.gm_coverage_text(ix.h, pp, 0, bins + 1, None, 0, C.byref(got)) == GM_E_ARG


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_values_only_snprintf_prints_send_their_slab_to_the_host(ix, tmp_path):
    per = 4096
    p = g.Params(mode=MODES["snp"])
    ix.coverage_reset(1); ix.coverage_enable_nuc()
    bins = ix.coverage_bins()
    rng = np.random.default_rng(41)
    cov = _values(bins, rng); nuc = _values(5 * bins, rng).reshape(5, bins)
    at = lambda slab: slab * per + 1001
    cov[at(0)] = 1e9; cov[at(1)] = 3e9; cov[at(2)] = np.inf                    # the first value put_fixed hands to snprintf, a larger one, inf
    for slab in range(3, 9):
        cov[at(slab)] = 5.0
    nuc[0, at(3)] = -1.0; nuc[2, at(4)] = np.nan; nuc[4, at(5)] = np.inf; nuc[3, at(6)] = -np.inf
    nuc[1, at(7)] = -0.0                                                       # prints as 0.00000 on both sides: no host slab
    cov[at(8)] = np.nextafter(np.float32(1e9), np.float32(0))                  # the largest value the device prints itself
    cov[at(9)] = 0.0; nuc[1, at(9)] = -3.0; cov[at(10)] = np.nan; cov[at(11)] = -7.0       # rows that are not printed flag nothing
    _upload(ix, cov, nuc)
    want = _host_file(ix, p, cov, nuc.reshape(-1), str(tmp_path / "host.gmp"))
    for token in (b"\t1000000000.00000\t", b"\t3000000000.00000\t", b"\tinf\t", b"\t-1.00000\t", b"\tnan\t", b"\t-inf\t", b"\t999999936.00000\t"):
        assert token in want, token
    g.set_option("GM_TRACK_SLICE", per)
    try:
        got = _device_file(ix, p, str(tmp_path / "dev.gmp"))
        st = ix.coverage_text_stats()
        assert got == want
        assert st["host_slabs"] == 7 and st["slabs"] == (ix.info.l_pac + per - 1) // per and st["rows"] == want.count(b"\n"), st
        assert st["launches"] == 3 * st["slabs"] - 7            # no rows pass for a slab the host formats
        per_bin = _lines_per_bin(want, cov[:ix.info.l_pac] > np.float32(0.001))
        assert ix.coverage_text(p, at(6) - 5, at(8) + 5) == b"".join(per_bin[at(6) - 5:at(8) + 5])
    finally:
        g.set_option("GM_TRACK_SLICE", None)
    assert _device_file(ix, p, str(tmp_path / "dev1.gmp")) == want and ix.coverage_text_stats()["host_slabs"] == 1      # one slab: all of it on the host
    # the .sgr: the same three totals
    ix.coverage_reset(8)
    bins = ix.coverage_bins()
    cov = _values(bins, rng)
    cov[5] = 1e9; cov[4096 + 5] = np.inf; cov[2 * 4096 + 5] = -1.0; cov[3 * 4096 + 5] = np.nan      # the last two print no row
    _upload(ix, cov)
    want = _host_file(ix, None, cov, None, str(tmp_path / "host.sgr"))
    g.set_option("GM_TRACK_SLICE", per)
    try:
        assert _device_file(ix, None, str(tmp_path / "dev.sgr")) == want and b"\tinf\n" in want
        assert ix.coverage_text_stats()["host_slabs"] == 2
    finally:
        g.set_option("GM_TRACK_SLICE", None)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
GEO = {"1000_37_5000": ((1000, 37, 5000), {1: 37, 8: 5, 64: 1}), "1030_37_5000": ((1030, 37, 5000), {1: 37, 8: 5, 64: 0})}


@pytest.fixture(scope="module", params=list(GEO))
def geo_ix(request, tmp_path_factory):
    lengths, short_rows = GEO[request.param]
    rng = np.random.default_rng(5)
    d = tmp_path_factory.mktemp("geo")
    fa = str(d / "geo.fa")
    names = ["first", "m" * 200, "third_" + "x" * 144]          # 256 rows under the third name do not fit one LDS window
    with open(fa, "w") as f:
        for name, n in zip(names, lengths):
            seq = "".join("ACGT"[i] for i in rng.integers(0, 4, n))
            f.write(">%s\n" % name + "".join(seq[i:i + 60] + "\n" for i in range(0, n, 60)))
    g.index_build(fa, g.GM_BUILD_HOST)
    x = g.Index(fa)
    yield x, names, lengths, short_rows
    x.close()


@pytest.mark.parametrize("bs", [1, 8, 64])
def test_geometry_short_contig_and_long_names(geo_ix, bs, tmp_path):
    x, names, lengths, short_rows = geo_ix
    o1, o2, l_pac = lengths[0], lengths[0] + lengths[1], sum(lengths)
    assert [n for n, _ in x.contigs()] == names and [o for _, o in x.contigs()] == [0, o1, o2] and x.info.l_pac == l_pac
    for mode in (None, "snp", "b2"):
        p = g.Params(mode=MODES[mode]) if mode else None
        x.coverage_reset(bs)
        if mode:
            x.coverage_enable_nuc()
        bins = x.coverage_bins()
        rng = np.random.default_rng(500 + bs)
        cov = (rng.random(bins).astype(np.float32) + np.float32(0.5)) * np.float32(30.0)      # every bin prints
        nuc = _values(5 * bins, rng) if mode else None
        _upload(x, cov, nuc)
        want = _host_file(x, p, cov, nuc, str(tmp_path / "host"))
        rows_of = lambda name: sum(1 for l in want.split(b"\n")[:-1] if l.split(b"\t")[0] == name.encode())
        if mode != "b2":
            # a contig gets a row for every bin that starts in it: none for the short one where no multiple of 64 falls into it
            assert rows_of(names[1]) == short_rows[bs] == (o2 + bs - 1) // bs - (o1 + bs - 1) // bs
            assert rows_of(names[0]) == (o1 + bs - 1) // bs and rows_of(names[2]) == (l_pac + bs - 1) // bs - (o2 + bs - 1) // bs
        for sl in (None, 300):
            g.set_option("GM_TRACK_SLICE", sl)
            try:
                assert _device_file(x, p, str(tmp_path / "dev")) == want, (mode, sl)
                assert x.coverage_text_stats()["host_slabs"] == 0
                assert x.coverage_text(p) == want
            finally:
                g.set_option("GM_TRACK_SLICE", None)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def track(text, ncol):
    d = {}
    for line in text.splitlines():
        f = line.split("\t")
        assert len(f) == ncol, line
        d[(f[0], int(f[1]))] = [float(x) for x in f[2:]]
    return d


def compare_tracks(mine, ref, ncol):
    """the comparison tests/test_gpu_driver_golden.py applies to the host path (two runs differ in the order of the fp32 atomic adds)"""
    a, b = track(mine, ncol), track(ref, ncol)
    assert len(b) > 100 or not b
    # a bin whose fp32-atomic sum is a rounding error away from the 0.001 print threshold may differ in presence only
    for k in set(a) ^ set(b):
        assert (a.get(k) or b.get(k))[0] < 2e-3, k
    for k in set(a) & set(b):
        for x, y in zip(a[k], b[k]):
            assert abs(x - y) <= 1e-4 * max(1.0, abs(y)) + 2e-5, (k, x, y)


def _golden(mode):
    """(argv, fastq, SAM text, track text of eight or three columns, extension) of a run of the reference program"""
    if mode == "snp":
        runs = os.path.join(GOLDEN, "ref_runs_snp")
        gmp = gzip.open(os.path.join(runs, "snp.gmp.gz"), "rt").read()
        return (["--snp"], "syn_snp.fq", gzip.open(os.path.join(runs, "snp.sam.gz"), "rt").read(),
                "".join("\t".join(l.split("\t")[:8]) + "\n" for l in gmp.splitlines()), "gmp")
    runs = os.path.join(GOLDEN, "ref_runs")
    m = json.load(open(os.path.join(runs, "manifest.json")))[mode]
    ext = "sgr" if "sgr" in m["tracks"] else "gmp"
    return (m["argv"], m["fastq"], gzip.open(os.path.join(runs, f"{mode}.sam.gz"), "rt").read(), gzip.open(os.path.join(runs, f"{mode}.{ext}.gz"), "rt").read(), ext)


@pytest.mark.parametrize("mode", ["default", "bs_all", "b2", "atog", "snp"])
def test_cli_with_track_text_device(mode, tmp_path):
    argv, fastq, sam_ref, track_ref, ext = _golden(mode)
    out = str(tmp_path / "mine")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "-a", "0.9"] + argv + ["--track_text=device", os.path.join(GOLDEN, fastq)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, GM_TRACK_SLICE="50000"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "track text on the device:" in r.stderr and "(0 formatted by the host)" in r.stderr, r.stderr[-1500:]
    assert "".join(l for l in open(out + ".sam") if not l.startswith("@PG")) == sam_ref
    assert not os.path.exists(out + (".gmp" if ext == "sgr" else ".sgr"))
    compare_tracks(open(out + "." + ext).read(), track_ref, 3 if ext == "sgr" else 8)
