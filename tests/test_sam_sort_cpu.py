"""--sam_sort=coordinate without a device: the model the GPU tests compare with (tests/sam_sort_model.py) on the SAM files of the
reference program under tests/golden/, the driver's usage text and its refusals, and the ABI calls on a host-only index."""
import ctypes as C
import glob
import gzip
import os
import subprocess

import pytest

import gnumap_amd as g
from conftest import GOLDEN, ROOT
from sam_sort_model import HD, sam_sort_model, sort_rows

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
SAMS = [os.path.join("ref_runs", "default.sam.gz"), os.path.join("ref_runs", "all.sam.gz"), os.path.join("ref_runs", "bs_all.sam.gz"),
        os.path.join("ref_runs_repeat", "all.sam.gz"), os.path.join("ref_runs_edge", "default.sam.gz"), os.path.join("celgen", "default.sam.gz")]


def split(text):
    lines = text.splitlines(keepends=True)
    return [l for l in lines if l.startswith("@")], [l for l in lines if not l.startswith("@")]


def keys_of(header, rows):
    rank = {f[3:].rstrip("\n"): None for l in header if l.startswith("@SQ") for f in l.split("\t") if f.startswith("SN:")}
    rank = {c: i for i, c in enumerate(rank)}
    return [(len(rank), 0) if r.split("\t")[2] == "*" else (rank[r.split("\t")[2]], int(r.split("\t")[3])) for r in rows]


@pytest.mark.parametrize("rel", SAMS)
def test_model_on_the_reference_programs_sam_files(rel):
    path = os.path.join(GOLDEN, rel)
    assert os.path.exists(path), sorted(glob.glob(os.path.join(GOLDEN, "*", "*.sam.gz")))[:50]
    text = gzip.open(path, "rt").read()
    header, rows = split(text)
    assert len(rows) > 100 and header and all(l.startswith("@SQ") for l in header)
    out = sam_sort_model(text)
    oh, orows = split(out)
    assert oh == [HD] + header                                              # header lines in place behind the @HD line
    assert sorted(orows) == sorted(rows) and len(orows) == len(rows)        # a permutation of the rows
    keys = keys_of(header, orows)
    assert all(a <= b for a, b in zip(keys, keys[1:]))                      # non-decreasing keys
    assert len(set(keys_of(header, rows))) < len(rows) or rel.startswith("celgen")      # (equal keys exist: stability is put to the test)
    # input order among equal keys: duplicates of a whole row are told apart by a serial number put in front of every row
    tagged = [f"{i:08d}|{r}" for i, r in enumerate(rows)]
    th, trows = split(sam_sort_model("".join(header) + "".join(t.split("|", 1)[1].replace("\t", f"|{t[:8]}\t", 1) for t in tagged)))
    last = {}
    tkeys = keys_of(header, trows)
    for k, r in zip(tkeys, trows):
        serial = int(r.split("\t")[0].rsplit("|", 1)[1])
        assert last.get(k, -1) < serial, (k, serial)
        last[k] = serial
    assert sam_sort_model(out) == out                                       # applied twice: unchanged
    assert sam_sort_model(text.encode()) == out.encode()                    # bytes in, bytes out


def test_model_puts_rows_without_a_contig_last_in_input_order():
    header = "@SQ\tSN:b\tLN:10\n@SQ\tSN:a\tLN:10\n@PG\tID:x\n"
    rows = ["r0\t512\t*\t0\t0\t*\n", "r1\t0\ta\t5\t1\tM\n", "r2\t0\tb\t7\t1\tM\n", "r3\t512\t*\t0\t0\t*\n", "r4\t16\tb\t7\t1\tM\n", "r5\t0\tb\t10\t1\tM\n",
            "r6\t0\tb\t9\t1\tM\n", "r7\t0\ta\t1\t1\tM\n"]
    out = sam_sort_model(header + "".join(rows))
    assert out == HD + header + "".join(rows[i] for i in (2, 4, 6, 5, 7, 1, 0, 3))          # @SQ order, not name order; 10 after 9
    assert sort_rows([r.rstrip("\n") for r in rows], ["b", "a"]) == [rows[i].rstrip("\n") for i in (2, 4, 6, 5, 7, 1, 0, 3)]


def run(args, tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out] + args + [os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=600)
    return r, out


def test_usage_names_the_option():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--sam_sort=none|coordinate" in r.stderr and "@HD" in r.stderr and "SO:coordinate" in r.stderr


@pytest.mark.parametrize("args, message", [
    (["--sam_sort=bogus"], "--sam_sort takes none or coordinate, not: bogus"),
    (["--sam_sort=coordinate", "--sam_text=host"], "cannot be combined with --sam_text=host"),
    (["--sam_text=host", "--sam_sort=coordinate"], "cannot be combined with --sam_text=host"),
    (["--sam_sort=coordinate", "--sam_shards=2"], "cannot be combined with --sam_shards above 1"),
    (["--sam_sort=coordinate", "--gpus=2"], "cannot be combined with --gpus above 1"),
], ids=["bogus", "text_host", "text_host_first", "shards", "gpus"])
def test_refusals_before_a_device_is_opened(args, message, tmp_path):
    r, out = run(args, tmp_path)
    assert r.returncode == 1 and message in r.stderr, r.stderr[-1000:]
    assert "No matching arg" not in r.stderr and "no usable HIP device" not in r.stderr
    assert os.listdir(tmp_path) == []                                       # no file written


@pytest.mark.parametrize("args", [["--sam_sort=coordinate"], ["--sam_sort=coordinate", "--sam_text=device", "--sam_shards=1", "--gpus=1"], ["--sam_sort=none", "--sam_text=host"]],
                         ids=["coordinate", "coordinate_spelled_out", "none"])
def test_the_option_reaches_the_device(args, tmp_path):
    import torch
    r, out = run(args + ["-a", "0.9"], tmp_path)
    assert "No matching arg" not in r.stderr and "--sam_sort" not in r.stderr
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr[-1500:]
        first = open(out + ".sam").readline()
        assert (first == HD) == ("--sam_sort=coordinate" in args)
    else:
        assert r.returncode != 0 and "no usable HIP device" in r.stderr      # GM_E_NO_DEVICE, not a parse error


def test_abi_on_a_host_only_index(syn_fa):
    from gnumap_amd import api
    L = g.lib()
    for name in ("gm_sam_sorter_create", "gm_sam_sorter_destroy", "gm_output_batch_sorted", "gm_output_batch_sorted_resident", "gm_sam_sorter_finish",
                 "gm_sam_sorter_read", "gm_sam_sorter_stats", "gm_sam_sorter_add_rows"):
        assert hasattr(L, name) and name in api.EXPORTS
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    h = C.c_void_p()
    assert L.gm_sam_sorter_create(ix.h, C.byref(h)) == -3 and not h.value   # GM_E_NO_DEVICE
    assert "no usable HIP device" in L.gm_last_error().decode()
    with pytest.raises(g.GnumapError) as e:
        api.SamSorter(ix)
    assert e.value.code == -3
    p = g.Params()
    hits = api.gm_hits(); reads = api.gm_reads(); rt = api.gm_read_text()
    assert L.gm_output_batch_sorted(ix.h, C.byref(p.c), None, C.byref(reads), C.byref(rt), C.byref(hits), None, 0, None) == -3
    assert L.gm_output_batch_sorted_resident(ix.h, C.byref(p.c), None, C.byref(hits), None, 0, None) == -3
    n = C.c_uint64(7)
    assert L.gm_sam_sorter_create(None, C.byref(h)) == -1                   # GM_E_ARG
    assert L.gm_sam_sorter_finish(None, C.byref(n), C.byref(n), None) == -1
    assert L.gm_sam_sorter_read(None, None, 0, C.byref(n), None) == -1
    assert L.gm_sam_sorter_add_rows(None, 0, None, None, None, None, 0, None) == -1
    L.gm_sam_sorter_destroy(None)
    ix.close()
