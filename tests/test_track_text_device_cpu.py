"""The device track writers (gm_coverage_write_sgr_device / _gmp_device / gm_coverage_text, gnumap_amd/csrc/gm_tracktext.hip) where there
is no device: a host-only index answers GM_E_NO_DEVICE and names the call, bad arguments answer GM_E_ARG before a device is looked
for, and the driver refuses an unknown --track_text value before it opens anything.  CPU only."""
import ctypes as C
import os
import subprocess

import pytest

import gnumap_amd as g
from gnumap_amd import api
from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
GM_E_ARG, GM_E_NO_DEVICE = -1, -3
u64 = C.c_uint64


@pytest.fixture()
def host_ix(syn_fa):
    h = C.c_void_p()
    L = g.lib()
    assert L.gm_index_open(os.fsencode(syn_fa), 0, api.GM_INDEX_HOST_ONLY, C.byref(h)) == 0
    L.gm_last_error.restype = C.c_char_p
    yield L, h
    L.gm_index_close(h)


def _text(L, h, p, lo, hi, cap=0):
    got = u64(12345)
    buf = C.create_string_buffer(max(cap, 1))
    rc = L.gm_coverage_text(h, p, lo, hi, buf, cap, C.byref(got))
    return rc, got.value


def test_host_only_index_has_no_device_path(host_ix, tmp_path):
    L, h = host_ix
    assert L.gm_coverage_reset(h, 8) == 0
    bins = L.gm_coverage_bins(h)
    out = str(tmp_path / "t.sgr").encode()
    assert L.gm_coverage_write_sgr_device(h, out, 0) == GM_E_NO_DEVICE
    assert b"gm_coverage_write_sgr_device" in L.gm_last_error()
    p = g.Params(mode=1)
    assert L.gm_coverage_write_gmp_device(h, C.byref(p.c), str(tmp_path / "t.gmp").encode(), 0) == GM_E_NO_DEVICE
    assert b"gm_coverage_write_gmp_device" in L.gm_last_error()
    rc, _ = _text(L, h, None, 0, bins)
    assert rc == GM_E_NO_DEVICE and b"gm_coverage_text" in L.gm_last_error()
    rc, _ = _text(L, h, C.byref(p.c), 0, bins)
    assert rc == GM_E_NO_DEVICE and b"gm_coverage_text" in L.gm_last_error()
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "t.gmp"))      # refused before a file was opened


def test_argument_errors(host_ix, tmp_path):
    L, h = host_ix
    out = str(tmp_path / "t.sgr").encode()
    p = g.Params(mode=1)
    # no coverage track yet
    assert L.gm_coverage_write_sgr_device(h, out, 0) == GM_E_ARG and b"gm_coverage_write_sgr_device" in L.gm_last_error()
    assert L.gm_coverage_write_gmp_device(h, C.byref(p.c), out, 0) == GM_E_ARG and b"gm_coverage_write_gmp_device" in L.gm_last_error()
    rc, _ = _text(L, h, None, 0, 0)
    assert rc == GM_E_ARG and b"gm_coverage_text" in L.gm_last_error()
    assert L.gm_coverage_reset(h, 8) == 0
    bins = L.gm_coverage_bins(h)
    # ranges
    rc, _ = _text(L, h, None, 5, 4)
    assert rc == GM_E_ARG and b"gm_coverage_text" in L.gm_last_error()
    rc, _ = _text(L, h, None, 0, bins + 1)
    assert rc == GM_E_ARG and b"gm_coverage_text" in L.gm_last_error()
    # a .gmp in normal mode
    assert L.gm_coverage_write_gmp_device(h, C.byref(g.Params().c), out, 0) == GM_E_ARG
    assert b"gm_coverage_write_gmp_device" in L.gm_last_error()
    # null pointers
    assert L.gm_coverage_write_sgr_device(h, None, 0) == GM_E_ARG
    assert L.gm_coverage_write_gmp_device(h, None, out, 0) == GM_E_ARG
    assert L.gm_coverage_text(h, None, 0, bins, None, 0, None) == GM_E_ARG
    assert L.gm_coverage_text_stats(h, None) == GM_E_ARG
    assert not os.path.exists(out)
    st = api.gm_track_text_stats()
    assert L.gm_coverage_text_stats(h, C.byref(st)) == 0 and st.slabs == 0 and st.rows == 0


def test_driver_refuses_an_unknown_track_text_value(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "--track_text=bogus", os.path.join(GOLDEN, "syn.fq")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "Error: --track_text takes host or device, not: bogus" in r.stderr
    assert os.listdir(tmp_path) == []
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--track_text=host|device" in r.stderr
