"""SAM text on the device, the parts that need no device: the two entry points are exported and refuse a host-only index with
GM_E_NO_DEVICE; the driver rejects bad --sam_shards / --sam_text values before it opens an index."""
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


def test_text_entry_points_are_exported_and_declared():
    lib = g.load_library()
    header = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    for name in ("gm_output_batch_text", "gm_dev_fmt_g6"):
        assert hasattr(lib, name), name
        assert name in api.EXPORTS and f"int {name}(" in header
    for struct in ("gm_read_text", "gm_sam_text"):
        assert f"}} {struct};" in header
    # the mirrors: four pointers; pointer + 3 x u64 + pointer + u64
    assert C.sizeof(api.gm_read_text) == 32 and C.sizeof(api.gm_sam_text) == 48
    assert api.gm_sam_text.text_len.offset == 16 and api.gm_sam_text.n_recs.offset == 24 and api.gm_sam_text.row_off.offset == 32


def test_text_calls_refuse_a_host_only_index(syn_fa):
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    lib = g.lib()
    p = g.Params()
    reads = api.gm_reads(); rt = api.gm_read_text(); hits = api.gm_hits(); out = api.gm_sam_text()
    rc = lib.gm_output_batch_text(ix.h, C.byref(p.c), None, C.byref(reads), C.byref(rt), C.byref(hits), C.byref(out), None)
    assert rc == GM_E_NO_DEVICE and b"no usable HIP device" in lib.gm_last_error()
    with pytest.raises(g.GnumapError) as e:
        ix.dev_fmt_g6(np.array([1.5, 2.5e-7]))
    assert e.value.code == GM_E_NO_DEVICE
    assert lib.gm_output_batch_text(None, C.byref(p.c), None, C.byref(reads), C.byref(rt), C.byref(hits), C.byref(out), None) == GM_E_ARG
    ix.close()


def test_records_call_refuses_a_host_only_index(syn_fa):
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    lib = g.lib()
    p = g.Params()
    reads = api.gm_reads(); hits = api.gm_hits(); out = api.gm_sam_out()
    rc = lib.gm_output_batch(ix.h, C.byref(p.c), None, C.byref(reads), C.byref(hits), C.byref(out), None)
    assert rc == GM_E_NO_DEVICE and b"no usable HIP device" in lib.gm_last_error()
    assert lib.gm_output_batch(None, C.byref(p.c), None, C.byref(reads), C.byref(hits), C.byref(out), None) == GM_E_ARG
    ix.close()


@pytest.mark.parametrize("flag, word", [("--sam_shards=0", "sam_shards"), ("--sam_shards=65", "sam_shards"), ("--sam_shards=-3", "sam_shards"),
                                        ("--sam_shards=two", "sam_shards"), ("--sam_text=bogus", "sam_text")])
def test_driver_rejects_bad_values_before_touching_a_device(flag, word, tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, flag, os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and word in r.stderr
    assert "HIP device" not in r.stderr                                  # the argument error comes first, with or without a GPU
    assert not os.path.exists(out + ".sam") and not os.path.exists(out + ".0.sam")


def test_usage_documents_the_two_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--sam_text=host|device" in r.stderr and "--sam_shards=K" in r.stderr
