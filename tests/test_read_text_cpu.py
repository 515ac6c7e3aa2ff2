"""FASTQ text cut on the device, the parts that need no device: the entry points are declared, exported and wrapped, they refuse a
host-only index with GM_E_NO_DEVICE and name themselves, the driver documents --read_text and rejects what it cannot take before it
opens an index; and the model of fastq_text_model.py agrees with itself on the texts of read_text_cases.py, so that the device tests
cannot be wrong about their own expectations."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fastq_text_model as M
import gnumap_amd as g
import read_text_cases as cases
from conftest import GOLDEN, ROOT
from gnumap_amd import api

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
GM_E_ARG, GM_E_NO_DEVICE = -1, -3
NEW = ("gm_batch_upload_text", "gm_map_batch_text", "gm_output_batch_text_resident", "gm_dev_fastq_rows")


def test_entry_points_are_declared_exported_and_wrapped():
    lib = g.load_library()
    header = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in api.EXPORTS and f"int {name}(" in header, name
    assert hasattr(lib, "gm_dev_fastq_tile_bytes") and "uint32_t gm_dev_fastq_tile_bytes(void);" in header and "gm_dev_fastq_tile_bytes" in api.EXPORTS
    for struct in ("gm_text_info", "gm_text_rec"):
        assert f"}} {struct};" in header
    for method in ("upload_text", "map_text", "output_text_resident"):
        assert callable(getattr(g.Batch, method))
    assert callable(g.Index.dev_fastq_rows)
    # the mirrors: 3 x u32 + i32 + u64; 6 x u32, and the numpy record of the same layout
    assert C.sizeof(api.gm_text_info) == 24 and api.gm_text_info.status.offset == 12 and api.gm_text_info.bad_at.offset == 16
    assert C.sizeof(api.gm_text_rec) == 24 == api.TEXT_REC_DTYPE.itemsize == M.REC_DTYPE.itemsize
    assert [f for f, _ in api.gm_text_rec._fields_] == list(api.TEXT_REC_DTYPE.names) == list(M.REC_DTYPE.names)
    assert (api.GM_TEXT_OK, api.GM_TEXT_MALFORMED, api.GM_TEXT_TOO_LONG) == (M.OK, M.MALFORMED, M.TOO_LONG)
    assert lib.gm_dev_fastq_tile_bytes() == cases.TILE               # needs no device: a constant of the kernels


def test_compute_entry_points_refuse_a_host_only_index_by_name(syn_fa):
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    lib = g.lib()
    p = g.Params()
    hits = api.gm_hits(); out = api.gm_sam_text(); info = api.gm_text_info()
    text = np.frombuffer(cases.SMALL, np.uint8)
    calls = {
        "gm_map_batch_text": lambda h: lib.gm_map_batch_text(h, C.byref(p.c), None, C.byref(hits), None),
        "gm_output_batch_text_resident": lambda h: lib.gm_output_batch_text_resident(h, C.byref(p.c), None, C.byref(hits), C.byref(out), None),
        "gm_dev_fastq_rows": lambda h: lib.gm_dev_fastq_rows(h, text.ctypes.data, len(text), C.byref(info), None, None, None, None, 0),
    }
    for name, call in calls.items():
        assert call(ix.h) == GM_E_NO_DEVICE, name
        err = lib.gm_last_error().decode()
        assert name in err and "no usable HIP device" in err, err
        assert call(None) == GM_E_ARG, name
    with pytest.raises(g.GnumapError) as e:
        ix.dev_fastq_rows(cases.SMALL)
    assert e.value.code == GM_E_NO_DEVICE
    # gm_batch_upload_text takes a batch, and there is none without a device
    with pytest.raises(g.GnumapError) as e:
        g.Batch(ix, 16, 64)
    assert e.value.code == GM_E_NO_DEVICE
    assert lib.gm_batch_upload_text(None, C.byref(p.c), text.ctypes.data, len(text), C.byref(info), None, 0, None) == GM_E_ARG
    ix.close()


def test_usage_documents_the_flag():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--read_text=host|device" in r.stderr and "FASTQ only" in r.stderr


def test_driver_rejects_a_bad_value_before_touching_a_device(tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "--read_text=bogus", os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "read_text" in r.stderr and "bogus" in r.stderr
    assert "HIP device" not in r.stderr and not os.path.exists(out + ".sam")


def test_driver_refuses_the_flag_with_fasta_reads(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b">r0\nACGTACGTACGTACGTACGTACGTACGTACGT\n>r1\nTTGACCATGACCATGACCATGGGGTTTACGTAA\n")
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "--read_text=device", str(fa)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "FASTQ only" in r.stderr and "--read_text=device" in r.stderr
    assert "HIP device" not in r.stderr and not os.path.exists(out + ".sam")


# ---- the model against itself --------------------------------------------------------------------------------------------------------
def reference_scan(text):
    """the same rule written the way the host parser is: a cursor, one memchr per line.  (n, status, bad_at, [(name, seq, qual)])"""
    cur, limit, out = 0, len(text), []

    def line():
        nonlocal cur
        if cur >= limit:
            return None
        e = text.find(b"\n", cur)
        s = cur
        if e < 0:
            cur = limit
            return s, text[s:]
        cur = e + 1
        return s, text[s:e]
    while True:
        nm = line()
        while nm is not None and len(nm[1]) == 0:
            nm = line()
        if nm is None:
            return len(out), M.OK, 0, out
        sq, pl, ql = line(), line(), line()
        if sq is None or pl is None or ql is None or nm[1][:1] != b"@" or len(pl[1]) == 0 or pl[1][:1] != b"+" or len(sq[1]) > len(ql[1]):
            return len(out), M.MALFORMED, nm[0], out
        if len(sq[1]) > 2048:
            return len(out), M.TOO_LONG, nm[0], out
        out.append((nm[1][1:], sq[1], ql[1]))


ALL_TEXTS = {**cases.good_texts(), **{"bad_" + k: v for k, v in cases.bad_texts().items()},
             **{f"prefix_{k}": b"\n" * k + cases.SMALL for k in (0, 1, 15, 16, 17, cases.TILE - 1, cases.TILE, cases.TILE + 1)}}


@pytest.mark.parametrize("case", sorted(ALL_TEXTS))
def test_model_agrees_with_itself(case):
    text = ALL_TEXTS[case]
    m = M.model(text)
    n, status, bad_at, reads = reference_scan(text)
    assert (m["n"], m["status"]) == (n, status)
    if status != M.OK:
        assert m["bad_at"] == bad_at
    assert case.startswith("bad_") == (status != M.OK)
    assert m["stride"] % 8 == 0 and m["stride"] >= max(8, m["max_len"]) and (m["stride"] - m["max_len"] < 8 or m["stride"] == 8)
    # rows rebuilt from the gm_text_rec offsets are the rows the model returns, and what the cursor scan read
    for i, (r, (name, seq, qual)) in enumerate(zip(m["recs"], reads)):
        L = int(r["seq_len"])
        assert text[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])] == name and text[int(r["name_off"]) - 1:int(r["name_off"])] == b"@"
        assert text[int(r["seq_off"]):int(r["seq_off"]) + L] == seq == m["bases"][i, :L].tobytes()
        assert text[int(r["qual_off"]):int(r["qual_off"]) + int(r["qual_len"])] == qual
        assert m["quals"][i, :L].tobytes() == qual[:L] and not m["bases"][i, L:].any() and not m["quals"][i, L:].any()
        assert m["len"][i] == L and m["names"][i] == name[:1023] and m["tails"][i] == qual[L:]


def test_the_cases_hold_what_their_names_say():
    t = cases.good_texts()
    assert M.parse(t["stride_follows_the_maximum"])["recs"]["seq_len"].tolist() == [1, 7, 8, 9, 63, 64, 65, 2047, 2048]
    assert M.parse(t["length_zero_reads"])["recs"]["seq_len"].tolist() == [0, 9, 0, 0]
    assert max(len(x) for x in M.model(t["name_1500_bytes"])["names"]) == 1023 and int(M.parse(t["name_1500_bytes"])["recs"]["name_len"].max()) == 1500
    assert int(M.parse(t["name_is_only_at"])["recs"]["name_len"][0]) == 0
    assert b"\r" in M.model(t["crlf"])["bases"].tobytes() and b"\0" in M.model(t["nul_in_name"])["names"][0]
    assert any(M.model(t["quality_longer_than_sequence"])["tails"]) and len(t["many_records"]) > 8 * cases.TILE
    assert M.parse(t["blank_runs_70"])["n"] == 3 and M.parse(t["only_blank_lines"])["n"] == 0
    b = cases.bad_texts()
    two = M.parse(b["two_bad_first_wins"])
    assert two["n"] == 20 and two["bad_at"] < cases.TILE < len(b["two_bad_first_wins"]) - 20 and len(M.lines_of(b["two_bad_first_wins"])) > 256 + 80
    assert M.parse(b["too_long_before_malformed"])["status"] == M.TOO_LONG and M.parse(b["too_long_after_malformed"])["status"] == M.MALFORMED
    assert M.parse(b["too_long_and_short_quality"])["status"] == M.MALFORMED
    ks = cases.prefix_lengths()
    for m in (16, 64, 128, 1024, cases.TILE, 2 * cases.TILE):
        assert {m - 1, m, m + 1} <= set(ks)


def test_illumina_until_of_the_model():
    Q = np.full((4, 8), 70, np.uint8)
    assert M.illumina_until(Q, [8, 8, 8, 8]) == 4
    Q[2, 5] = 63
    assert M.illumina_until(Q, [8, 8, 8, 8]) == 2 and M.illumina_until(Q, [8, 8, 5, 8]) == 4
    Q[3, 0] = 200                                                    # a signed char: negative
    assert M.illumina_until(Q, [8, 8, 5, 8]) == 3
