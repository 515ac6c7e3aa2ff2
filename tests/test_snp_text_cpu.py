"""The result of --snp as text (gm_coverage_write_gmp_calls_device, gm_coverage_calls_text, gm_coverage_write_vcf, gm_dev_fmt_e2) where
there is no device: the symbols are exported and wrapped, a host-only index answers GM_E_NO_DEVICE and names the call, bad arguments
answer GM_E_ARG before a device is looked for, and the driver knows --vcf and refuses it without --snp before it opens anything.
CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
from gnumap_amd import api
from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
GM_E_ARG, GM_E_NO_DEVICE = -1, -3
u64 = C.c_uint64
NEW = ("gm_dev_fmt_e2", "gm_coverage_write_gmp_calls_device", "gm_coverage_calls_text", "gm_coverage_write_vcf")


@pytest.fixture()
def host_ix(syn_fa):
    h = C.c_void_p()
    L = g.lib()
    assert L.gm_index_open(os.fsencode(syn_fa), 0, api.GM_INDEX_HOST_ONLY, C.byref(h)) == 0
    L.gm_last_error.restype = C.c_char_p
    yield L, h
    L.gm_index_close(h)


def _calls_text(L, h, lo, hi, cap=0):
    got = u64(12345)
    buf = C.create_string_buffer(max(cap, 1))
    return L.gm_coverage_calls_text(h, 0.001, 0, lo, hi, buf, cap, C.byref(got)), got.value


def test_symbols_are_exported_declared_and_wrapped():
    L = g.lib()
    header = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    for name in NEW:
        assert name in api.EXPORTS and getattr(L, name).argtypes is not None and ("int " + name + "(") in header, name
    for name in ("dev_fmt_e2", "coverage_write_gmp_calls_device", "coverage_calls_text", "coverage_write_vcf"):
        assert callable(getattr(g.Index, name)), name


def test_host_only_index_has_no_device_path(host_ix, tmp_path):
    L, h = host_ix
    assert L.gm_coverage_reset(h, 1) == 0
    bins = L.gm_coverage_bins(h)
    gmp, vcf = str(tmp_path / "t.gmp").encode(), str(tmp_path / "t.vcf").encode()
    assert L.gm_coverage_write_gmp_calls_device(h, 0.001, 0, gmp, 0) == GM_E_NO_DEVICE
    assert b"gm_coverage_write_gmp_calls_device" in L.gm_last_error()
    rc, _ = _calls_text(L, h, 0, bins)
    assert rc == GM_E_NO_DEVICE and b"gm_coverage_calls_text" in L.gm_last_error()
    assert L.gm_coverage_write_vcf(h, 0.001, 0, vcf, 0) == GM_E_NO_DEVICE
    assert b"gm_coverage_write_vcf" in L.gm_last_error()
    v = np.array([0.5]); out = np.zeros(16, np.uint8); ln = np.zeros(1, np.uint8)
    assert L.gm_dev_fmt_e2(h, v.ctypes.data, 1, out.ctypes.data, ln.ctypes.data) == GM_E_NO_DEVICE
    assert os.listdir(tmp_path) == []                  # refused before a file was opened


def test_argument_errors(host_ix, tmp_path):
    L, h = host_ix
    gmp, vcf = str(tmp_path / "t.gmp").encode(), str(tmp_path / "t.vcf").encode()
    # no coverage track yet
    assert L.gm_coverage_write_gmp_calls_device(h, 0.001, 0, gmp, 0) == GM_E_ARG and b"gm_coverage_write_gmp_calls_device" in L.gm_last_error()
    assert L.gm_coverage_write_vcf(h, 0.001, 0, vcf, 0) == GM_E_ARG and b"gm_coverage_write_vcf" in L.gm_last_error()
    rc, _ = _calls_text(L, h, 0, 0)
    assert rc == GM_E_ARG and b"gm_coverage_calls_text" in L.gm_last_error()
    # a bin size other than 1
    assert L.gm_coverage_reset(h, 8) == 0
    bins = L.gm_coverage_bins(h)
    assert L.gm_coverage_write_gmp_calls_device(h, 0.001, 0, gmp, 0) == GM_E_ARG and b"bin size 1" in L.gm_last_error()
    assert L.gm_coverage_write_vcf(h, 0.001, 0, vcf, 0) == GM_E_ARG and b"bin size 1" in L.gm_last_error()
    rc, _ = _calls_text(L, h, 0, bins)
    assert rc == GM_E_ARG and b"bin size 1" in L.gm_last_error()
    # ranges
    assert L.gm_coverage_reset(h, 1) == 0
    bins = L.gm_coverage_bins(h)
    rc, _ = _calls_text(L, h, 5, 4)
    assert rc == GM_E_ARG and b"gm_coverage_calls_text" in L.gm_last_error()
    rc, _ = _calls_text(L, h, 0, bins + 1)
    assert rc == GM_E_ARG and b"gm_coverage_calls_text" in L.gm_last_error()
    # null pointers
    assert L.gm_coverage_write_gmp_calls_device(h, 0.001, 0, None, 0) == GM_E_ARG
    assert L.gm_coverage_write_vcf(h, 0.001, 0, None, 0) == GM_E_ARG
    assert L.gm_coverage_calls_text(h, 0.001, 0, 0, bins, None, 0, None) == GM_E_ARG
    assert L.gm_coverage_calls_text(h, 0.001, 0, 0, bins, None, 10, C.byref(u64())) == GM_E_ARG
    assert L.gm_coverage_write_gmp_calls_device(None, 0.001, 0, gmp, 0) == GM_E_ARG
    assert L.gm_dev_fmt_e2(h, None, 3, None, None) == GM_E_ARG
    assert os.listdir(tmp_path) == []


def test_driver_refuses_vcf_without_snp(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "--vcf", os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--vcf" in r.stderr and "--snp" in r.stderr and "No matching arg" not in r.stderr
    assert os.listdir(tmp_path) == []
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "-b", "--vcf", os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--vcf" in r.stderr and "--snp" in r.stderr and os.listdir(tmp_path) == []


def test_driver_knows_vcf():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--vcf" in r.stderr
    # the flag is parsed: with --snp the complaint is about what comes next (no read file), not about the flag
    r = subprocess.run([EXE, "--snp", "--vcf"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "No matching arg" not in r.stderr
