"""FASTQ text cut into read rows on the device (gm_batch_upload_text: the k_rt_* kernels of gm_readtext.hip) and --read_text=device.

* gm_dev_fastq_rows against the model of fastq_text_model.py, byte for byte, on the texts of read_text_cases.py: line, lane, wave and
  tile edges, blank-line runs, empty reads, long names, bytes that look special and are not, the first bad record of either kind;
* the ABI end to end: upload_text + map_text + output_text_resident against map + output_text of the same reads cut by the model,
  with an adaptor, with --illumina's fallback, the capacity resumes, GM_TEST_MAX_BLOCK;
* the driver with --read_text=device against the outputs of the UNMODIFIED reference program (tests/golden/ref_runs)."""
import os

import numpy as np
import pytest

import fastq_text_model as M
import gnumap_amd as g
import read_text_cases as cases
from conftest import GOLDEN
from gnumap_amd import api
from test_gpu_sam_text import BATCHING_MODES, MANIFEST, check_against_reference, ref_text, assert_same_sam, run_driver, same_track

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ix(syn_fa):
    x = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    yield x
    x.close()


def check_probe(ix, text, what):
    want = M.model(text)
    got = ix.dev_fastq_rows(text)
    for k in ("n", "max_len", "stride", "status"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    if want["status"] != M.OK:
        assert got["bad_at"] == want["bad_at"], (what, got["bad_at"], want["bad_at"])
    for f in M.REC_DTYPE.names:
        assert np.array_equal(got["recs"][f], want["recs"][f]), (what, f)
    assert np.array_equal(got["len"], want["len"]), what
    assert got["bases"].shape == want["bases"].shape and np.array_equal(got["bases"], want["bases"]), what
    assert np.array_equal(got["quals"], want["quals"]), what
    return want


# ---- probe parity --------------------------------------------------------------------------------------------------------------------
def test_the_tile_size_the_cases_were_built_for():
    assert g.lib().gm_dev_fastq_tile_bytes() == cases.TILE


@pytest.mark.parametrize("case", sorted(cases.good_texts()))
def test_probe_equals_model_on_well_formed_text(ix, case):
    want = check_probe(ix, cases.good_texts()[case], case)
    assert want["status"] == M.OK


def test_probe_equals_model_behind_every_prefix_of_blank_lines(ix):
    """the same four records behind k blank lines: every line of a record on either side of a lane, wave and tile edge"""
    ks = cases.prefix_lengths(g.lib().gm_dev_fastq_tile_bytes())
    assert len(ks) > 70
    for k in ks:
        want = check_probe(ix, b"\n" * k + cases.SMALL, f"prefix {k}")
        assert want["n"] == 4 and int(want["recs"]["name_off"][0]) == k + 1


def test_probe_equals_model_with_text_in_front_of_every_edge(ix):
    """the same, the prefix being records (not blank lines): the phase of a line at a tile's start is 0, 1, 2 and 3 in turn"""
    one = [M.fastq([cases.rec(i, 11 + i % 5)]) for i in range(400)]
    ends = np.cumsum([len(x) for x in one])
    filler = b"".join(one)
    tile = g.lib().gm_dev_fastq_tile_bytes()
    for cut in (tile - 40, tile - 20, tile - 1, tile, tile + 1, tile + 13, 2 * tile - 7, 2 * tile, 2 * tile + 30):
        at = int(ends[ends <= cut][-1])                            # whole records up to about `cut`
        for pad in range(0, 48, 5):
            check_probe(ix, filler[:at] + b"\n" * pad + cases.SMALL, f"cut {cut} pad {pad}")


@pytest.mark.parametrize("case", sorted(cases.bad_texts()))
def test_probe_stops_at_the_first_bad_record(ix, case):
    want = check_probe(ix, cases.bad_texts()[case], case)          # n, status, bad_at as the model's; the rows of the n good records intact
    assert want["status"] != M.OK


def test_probe_limits(ix):
    info = api.gm_text_info()
    buf = np.zeros(16, np.uint8)
    import ctypes as C
    rc = g.lib().gm_dev_fastq_rows(ix.h, buf.ctypes.data, 1 << 32, C.byref(info), None, None, None, None, 0)
    assert rc == -1 and "2^32" in g.lib().gm_last_error().decode()


# ---- the ABI end to end --------------------------------------------------------------------------------------------------------------
def syn_text(reads):
    return M.fastq([(r[0].encode(), r[1], r[2]) for r in reads])


HITS = ("status", "self_score", "top_score", "denominator", "match_begin")


def same_hits(a, b, what):
    for k in HITS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)
    assert len(a["matches"]) == len(b["matches"]), what
    for f in a["matches"].dtype.names:                              # field by field: the records carry padding bytes
        assert np.ascontiguousarray(a["matches"][f]).tobytes() == np.ascontiguousarray(b["matches"][f]).tobytes(), (what, f)
    n_p = int(a["matches"]["pos_end"].max()) if len(a["matches"]) else 0
    for f in ("pos", "strand"):
        assert np.array_equal(a["positions"][f][:n_p], b["positions"][f][:n_p]), (what, f)


def run_host_cut(ix, p, text, adaptor=None, bin_size=8):
    """map + output_text on the rows the model cuts: (hits, SAM text, coverage, trimmed lengths, fallback-free)"""
    m = M.model(text)
    batch = g.Batch(ix, max(m["n"], 1), m["stride"])
    batch.set_adaptor(adaptor)
    ix.coverage_reset(bin_size)
    res = batch.map(p, m["bases"], m["quals"], m["len"])
    tails = m["tails"] if any(m["tails"]) else None
    sam, row_off = batch.output_text(p, res, m["names"], tails)
    cov = ix.coverage_download()
    kept = batch.trimmed_len()
    batch.destroy()
    return res, sam, row_off, cov, kept


def run_device_cut(ix, p, text, adaptor=None, bin_size=8, mcap=None, pcap=None, text_cap=None):
    batch = g.Batch(ix, 4096, 2048)
    batch.set_adaptor(adaptor)
    ix.coverage_reset(bin_size)
    info = batch.upload_text(p, text)
    res = batch.map_text(p, mcap=mcap, pcap=pcap)
    map_calls = batch.map_calls
    sam, row_off = batch.output_text_resident(p, res, text_cap=text_cap)
    cov = ix.coverage_download()
    kept = batch.trimmed_len()
    calls = (map_calls, batch.text_calls)
    batch.destroy()
    return info, res, sam, row_off, cov, kept, calls


def with_tails(reads):
    """some quality lines longer than their sequences, one name beyond 1023 bytes"""
    out = []
    for i, r in enumerate(reads):
        q = r[2] + (b"#t%d" % i if i % 9 == 0 else b"")
        out.append(((r[0] + "_") * 90 if i % 20 == 5 else r[0], r[1], q))
    return out


@pytest.mark.parametrize("adaptor", [None, b"ACGTTGCAAC"], ids=["plain", "adaptor"])
@pytest.mark.parametrize("kw", [{}, {"print_all_sam": 1}], ids=["default", "print_all"])
def test_abi_text_block_equals_host_cut_block(ix, syn_reads, kw, adaptor):
    p = g.Params(**kw)
    text = syn_text(with_tails(syn_reads[:300]))
    res, sam, row_off, cov, kept = run_host_cut(ix, p, text, adaptor)
    info, res2, sam2, row_off2, cov2, kept2, _ = run_device_cut(ix, p, text, adaptor)
    m = M.parse(text)
    assert info["n"] == m["n"] == 300 and info["status"] == M.OK and info["stride"] == m["stride"]
    for f in M.REC_DTYPE.names:
        assert np.array_equal(info["recs"][f], m["recs"][f]), f
    assert np.array_equal(kept, kept2)
    if adaptor:
        assert int((kept.astype(int) != m["recs"]["seq_len"].astype(int)).sum()) == m["n"]       # FixReads2 shortens every read
    same_hits(res, res2, "hits")
    assert len(res["matches"]) > 100
    assert sam2 == sam and np.array_equal(row_off, row_off2)
    assert sam.count(b"#t") >= 1                                    # quality tails were printed
    if not adaptor:                                                 # (trimmed, the reads with the long names need not map)
        assert max(len(l.split(b"\t")[0]) for l in sam.splitlines()) == 1023
    same_track(cov2, cov)                                           # deposited once: not twice, not never


@pytest.mark.parametrize("adaptor", [None, b"ACGTTGCAAC"], ids=["plain", "adaptor"])
@pytest.mark.parametrize("where", ["first", "middle", "last", "nowhere"])
def test_abi_text_block_illumina_fallback(ix, syn_reads, where, adaptor):
    """--illumina: Phred+64 up to the first read with a quality below '@' in its kept length, Phred+33 from there on"""
    p = g.Params(illumina=1)
    n = 120
    low = {"first": 0, "middle": 61, "last": n - 1, "nowhere": None}[where]
    reads = []
    for i, r in enumerate(syn_reads[:n]):
        q = bytearray(min(126, c + 31) for c in r[2])             # Phred+64 characters, none below 64
        if i == low:
            q[3] = 40
        if i == 7 and adaptor:
            q[-1] = 35                                              # FixReads2 cuts this one off (every read loses at least 4 bases): no fallback from it
        reads.append((r[0], r[1], bytes(q)))
    text = syn_text(reads)
    res, sam, _, cov, kept = run_host_cut(ix, p, text, adaptor)
    info, res2, sam2, _, cov2, kept2, _ = run_device_cut(ix, p, text, adaptor)
    assert np.array_equal(kept, kept2) and int(kept.min()) > 3
    m = M.model(text)
    assert M.illumina_until(m["quals"], kept) == (n if low is None else low)      # the inputs are what the case says they are
    same_hits(res, res2, where)
    assert sam2 == sam
    same_track(cov2, cov)


def test_abi_text_block_capacity_resumes(ix, syn_reads):
    p = g.Params()
    text = syn_text(syn_reads[:200])
    res, sam, row_off, cov, _ = run_host_cut(ix, p, text)
    info, res2, sam2, row_off2, cov2, _, calls = run_device_cut(ix, p, text, mcap=3, pcap=2, text_cap=16)
    assert calls == (2, 2)                                          # GM_E_CAPACITY with the sizes needed, then the call that only copies / only then deposits
    same_hits(res, res2, "resume")
    assert sam2 == sam
    same_track(cov2, cov)


def test_abi_text_block_records_and_small_cases(ix, syn_reads):
    import ctypes as C
    p = g.Params()
    batch = g.Batch(ix, 64, 2048)
    h = api.gm_hits()
    # nothing from upload_text resident: map_text is an argument error
    assert g.lib().gm_map_batch_text(ix.h, C.byref(p.c), batch.h, C.byref(h), None) == -1
    info = batch.upload_text(p, b"")
    assert info["n"] == 0 and info["status"] == M.OK and info["stride"] == 8
    res = batch.map_text(p)
    assert len(res["matches"]) == 0
    # more records than the batch takes; nothing is left resident
    with pytest.raises(g.GnumapError) as e:
        batch.upload_text(p, syn_text(syn_reads[:65]))
    assert e.value.code == -1 and "max_reads" in str(e.value)
    assert g.lib().gm_map_batch_text(ix.h, C.byref(p.c), batch.h, C.byref(h), None) == -1
    # a table too small: the number needed comes back
    text = syn_text(syn_reads[:40])
    buf = np.frombuffer(text + b"\0", np.uint8)
    ti = api.gm_text_info(); small = np.zeros(8, api.TEXT_REC_DTYPE)
    rc = g.lib().gm_batch_upload_text(batch.h, C.byref(p.c), buf.ctypes.data, len(text), C.byref(ti), small.ctypes.data, 8, None)
    assert rc == api.GM_E_CAPACITY and ti.n == 40
    # a FASTA batch
    assert g.lib().gm_batch_set_read_format(batch.h, api.GM_READS_FASTA) == 0
    rc = g.lib().gm_batch_upload_text(batch.h, C.byref(p.c), buf.ctypes.data, len(text), C.byref(ti), None, 0, None)
    assert rc == -6 and "FASTA" in g.lib().gm_last_error().decode()
    # gm_output_batch on a text block, with a gm_reads that carries n and stride
    info = batch.upload_text(p, text)
    res = batch.map_text(p)
    recs, cigars = batch.output(p, res)
    m = M.model(text)
    b2 = g.Batch(ix, 64, m["stride"])
    recs2, cigars2 = b2.output(p, b2.map(p, m["bases"], m["quals"], m["len"]))
    assert recs.tobytes() == recs2.tobytes() and cigars == cigars2 and len(recs) > 20
    b2.destroy(); batch.destroy()


def test_abi_text_block_treated_as_too_large(ix, syn_reads):
    import ctypes as C
    p = g.Params()
    batch = g.Batch(ix, 256, 2048)
    batch.upload_text(p, syn_text(syn_reads[:100]))
    g.set_option("GM_TEST_MAX_BLOCK", 60)
    try:
        with pytest.raises(g.GnumapError) as e:
            batch.map_text(p)
        assert e.value.code == api.GM_E_BATCH_TOO_LARGE
    finally:
        g.set_option("GM_TEST_MAX_BLOCK", None)
    assert len(batch.map_text(p)["matches"]) > 30                   # the block is still resident
    batch.destroy()


# ---- the driver against the reference program's outputs ----------------------------------------------------------------------------------
FILE_ORDER = [m for m in sorted(MANIFEST) if "--illumina" in MANIFEST[m]["argv"]]


@pytest.mark.parametrize("mode", sorted(MANIFEST))
def test_cli_read_text_device_equals_reference_program(mode, tmp_path):
    out = str(tmp_path / "mine")
    r = run_driver(mode, ["--read_text=device"], out)
    check_against_reference(mode, out)
    stage = [l for l in r.stderr.splitlines() if l.startswith("stage seconds")]
    assert len(stage) == 1
    if mode in FILE_ORDER:                                          # --illumina: file order, cut by the host as without the flag
        assert "gm_map_batch_text" not in stage[0] and "pack" in stage[0]
    else:
        assert "gm_map_batch_text" in stage[0] and " stage " in stage[0] and "pack" not in stage[0]


@pytest.mark.parametrize("mode", BATCHING_MODES)
def test_cli_read_text_device_with_device_sam_text_in_small_chunks(mode, tmp_path):
    out = str(tmp_path / "mine")
    r = run_driver(mode, ["--read_text=device", "--sam_text=device", "--chunk_reads=37", "--workers=3"], out)
    check_against_reference(mode, out)
    assert ("gm_map_batch_text" in r.stderr) == (mode not in FILE_ORDER)
    assert "gm_output_batch_text" in r.stderr and "SAM format" not in r.stderr


def test_cli_read_text_device_file_order_blocks_are_cut_by_the_host(tmp_path):
    out = str(tmp_path / "mine")
    r = run_driver("default", ["--read_text=device", "--batch=64"], out)
    check_against_reference("default", out)
    assert "gm_map_batch_text" not in r.stderr


@pytest.mark.parametrize("mode", ["malformed", "malformed_tail"])
@pytest.mark.parametrize("text", ["host", "device"])
def test_cli_read_text_device_malformed_prefix_on_the_device_rest_by_the_host(mode, text, tmp_path):
    out = str(tmp_path / "mine")
    r = run_driver(mode, ["--read_text=device", f"--sam_text={text}", "--chunk_reads=16"], out)
    check_against_reference(mode, out)
    assert "gm_map_batch_text" in r.stderr and "--Found error" in r.stderr         # the reference's recovery ran on the rest, in file order


@pytest.mark.parametrize("text", ["host", "device"])
def test_cli_read_text_device_block_mapped_in_halves(text, tmp_path):
    out = str(tmp_path / "mine")
    r = run_driver("default", ["--read_text=device", f"--sam_text={text}"], out, env=dict(os.environ, GM_TEST_MAX_BLOCK="60"))
    assert "mapped in halves" in r.stderr
    check_against_reference("default", out)


def test_cli_read_text_device_shards_concatenate_to_the_single_file(tmp_path):
    out = str(tmp_path / "mine")
    run_driver("default", ["--read_text=device", "--sam_text=device", "--sam_shards=4", "--chunk_reads=37", "--workers=3"], out)
    shards = [open(f"{out}.{k}.sam").read() for k in range(4)]
    assert sum(1 for s in shards if any(not l.startswith("@") for l in s.splitlines())) >= 2
    assert_same_sam("".join(l + "\n" for l in "".join(shards).splitlines() if not l.startswith("@PG")), ref_text("default", "sam"), "shards")


def test_cli_read_text_device_too_long_read(tmp_path):
    import subprocess
    from test_gpu_sam_text import EXE
    fq = tmp_path / "long.fq"
    lines = open(os.path.join(GOLDEN, "syn.fq"), "rb").read().splitlines(keepends=True)
    fq.write_bytes(b"".join(lines[:40]) + M.fastq([(b"the_long_one", b"ACGT" * 513, b"I" * 2052)]) + b"".join(lines[40:]))
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", str(tmp_path / "mine"), "--read_text=device", str(fq)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "ERROR: read @the_long_one is longer than 2048 bases" in r.stderr
