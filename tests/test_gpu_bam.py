"""--sam_format=bam: BAM records written on the device (k_bam_sizes / k_bam_rows, gm_bam.hip) inside BGZF blocks, against
tests/bam_model.py applied to the SAM rows the text path prints for the same records.

* the ABI: gm_output_batch_bam on blocks of 64 reads - names of about 900 bytes (cut to 254), a 2048-base read beside fifty 900-base reads
  with an insertion or a deletion on both strands (records of more than 65280 bytes: one spans two BGZF blocks), random reads (nothing
  maps: len = 0) - at both levels, the resident form, a FASTA block, the deposits, and GM_E_CAPACITY;
* the driver: <out>.bam against the model of the default run's <out>.sam, its header, its end marker, the tracks; sorted BAM;
* gnumap_amd.api.SamSorter(rows="bam"): read and read_bgzf.

The four value bytes of XA and XP are compared by value against the printed "%g" field: |v - t| <= 5.1e-6 |t| (six digits plus float
rounding); a field that prints nan has to hold a NaN."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

import gnumap_amd as g
import bam_model as bm
from conftest import GOLDEN
from gnumap_amd import api
from reflib import revcomp_str
from sam_sort_model import sam_sort_model, sort_rows
from test_gpu_driver_golden import compare_tracks
from test_gpu_sam_sort import SORTED, drive, edge_run, no_pg  # noqa: F401  (edge_run is a fixture)
from test_gpu_sam_text import same_track

pytestmark = pytest.mark.gpu


def rc(s):
    s = revcomp_str(s)
    return (s.encode() if isinstance(s, str) else s).upper()


def check_records(got, want):
    """bm.records_equal, with a printed nan standing for any NaN"""
    fixed, model = [], []
    for a, b in zip(got, want):
        if len(a) == len(b):
            a, b = bytearray(a), bytearray(b)
            for o in bm.float_tag_offsets(bytes(b)):
                if math.isnan(struct.unpack_from("<f", b, o)[0]):
                    assert math.isnan(struct.unpack_from("<f", a, o)[0])
                    a[o:o + 4] = b[o:o + 4] = struct.pack("<f", 1.0)          # (compared: both are NaN)
            a, b = bytes(a), bytes(b)
        fixed.append(a); model.append(b)
    fixed += got[len(fixed):]; model += want[len(model):]
    why = bm.records_equal(fixed, model)
    assert why is None, why


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def abi(syn_fa, syn_reads):
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    genome = b"".join(l.strip() for l in open(syn_fa, "rb") if not l.startswith(b">")).upper()
    rng = np.random.default_rng(21)
    blocks = []
    for k in range(3):
        rd = syn_reads[64 * k:64 * (k + 1)]
        names = [r[0].encode() for r in rd]; seqs = [r[1] for r in rd]; quals = [r[2][:len(r[1])] for r in rd]
        if k == 1:
            names = [(nm + b"_") * 45 for nm in names]
        if k == 2:
            names[0] = b"long2048"; seqs[0] = genome[1000:3048]; quals[0] = b"I" * 2048
            for j in range(50):                                              # 900 bases with one base inserted or deleted in the middle, on either strand
                at = 4000 + 3100 * j
                s = genome[at:at + 900]
                s = s[:450] + (b"ACGT"[j & 3:(j & 3) + 1] + s[450:899] if j % 3 == 1 else s[451:] + genome[at + 900:at + 901] if j % 3 == 2 else s[450:])
                assert len(s) == 900
                names[1 + j] = b"long900_%d" % j; seqs[1 + j] = rc(s) if j & 1 else s
                quals[1 + j] = bytes((33 + rng.integers(25, 41, 900)).astype(np.uint8))
        blocks.append((names, seqs, quals))
    blocks.append(([b"none%d" % i for i in range(64)], [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)) for _ in range(64)], [b"I" * 100] * 64))
    packed = [g.pack_reads(s, q) for _, s, q in blocks]
    batches = [g.Batch(ix, 64, B.shape[1]) for B, _, _ in packed]
    ix.coverage_reset(8)
    rows, recs = [], []
    for (names, _, _), (B, Q, Ln), batch in zip(blocks, packed, batches):
        text, row_off = batch.output_text(p, batch.map(p, B, Q, Ln), names)
        rows.append([text[int(row_off[i]):int(row_off[i + 1])] for i in range(len(row_off) - 1)])
    cov = ix.coverage_download()
    for (B, Q, Ln), batch in zip(packed, batches):
        recs.append(batch.output(p, batch.map(p, B, Q, Ln))[0])
    contigs = [(c, 0) for c, _ in ix.contigs()]
    want = [bm.sam_to_bam_records(b"".join(r), contigs) for r in rows]
    yield dict(ix=ix, p=p, blocks=blocks, packed=packed, batches=batches, rows=rows, recs=recs, cov=cov, contigs=contigs, want=want)
    for b in batches:
        b.destroy()
    ix.close()


def test_fixture_holds_what_the_encoder_has_to_get_right(abi):
    rows = [r.split(b"\t") for blk in abi["rows"] for r in blk]
    assert [len(r) > 40 for r in abi["rows"]] == [True, True, True, False]
    rev_indel = [r for r in rows if r[1] == b"16" and (b"I" in r[5] or b"D" in r[5])]
    fwd_indel = [r for r in rows if r[1] == b"0" and (b"I" in r[5] or b"D" in r[5])]
    assert len(rev_indel) >= 5 and len(fwd_indel) >= 5
    assert any(b"I" in r[5] for r in rev_indel) and any(b"D" in r[5] for r in rev_indel)
    assert any(len(r[0]) > 254 for r in rows) and any(len(r[9]) == 2048 for r in rows)
    sizes = np.cumsum([len(x) for x in abi["want"][2]])
    assert sizes[-1] > bm.PAYLOAD and bm.PAYLOAD not in sizes                 # a record of block 2 spans two BGZF blocks


@pytest.mark.parametrize("level", [0, 1])
def test_output_bam_equals_the_model_of_the_text_rows(abi, level):
    ix, p = abi["ix"], abi["p"]
    ix.coverage_reset(8)
    for k, ((names, _, _), (B, Q, Ln), batch) in enumerate(zip(abi["blocks"], abi["packed"], abi["batches"])):
        out = batch.output_bam(p, batch.map(p, B, Q, Ln), names, level=level)
        want = abi["want"][k]
        if not want:
            assert out == b"" and batch.bam_raw_len == 0 and batch.bam_n_recs == 0
            continue
        members = bm.parse_bgzf(out)
        raw = b"".join(pl for pl, _, _ in members)
        assert batch.bam_raw_len == len(raw) and batch.bam_n_recs == len(want) and len(members) == (len(raw) + bm.PAYLOAD - 1) // bm.PAYLOAD
        assert all(bt == (0 if level == 0 else 2) for _, bt, _ in members)
        got = bm.split_records(raw)
        check_records(got, want)
        for rec, r in zip(got, abi["recs"][k]):                               # XP: post_prob's own bits
            _, xp = bm.float_tag_offsets(rec)
            assert rec[xp:xp + 4] == np.float32(r["post_prob"]).tobytes()
        if level == 1:
            assert len(out) < len(raw)
    cov = ix.coverage_download()
    nan = np.isnan(abi["cov"])                                               # (the 2048-base read's posterior is NaN in the reference's arithmetic)
    assert np.array_equal(np.isnan(cov), nan)
    same_track(cov[~nan], abi["cov"][~nan])


def test_nothing_is_deposited_on_capacity(abi):
    ix, p = abi["ix"], abi["p"]
    (names, _, _), (B, Q, Ln), batch = abi["blocks"][0], abi["packed"][0], abi["batches"][0]
    ix.coverage_reset(8)
    once = batch.output_bam(p, batch.map(p, B, Q, Ln), names)
    ref = ix.coverage_download()
    L = g.lib()
    res = batch.map(p, B, Q, Ln)
    rt, keep = api._pack_read_text(names, None, 64)
    buf = np.full(len(once) + 16, 0xAA, np.uint8)
    bo = api.gm_bam_out(); bo.data = buf.ctypes.data; bo.cap = len(once) - 1; bo.level = 1
    ix.coverage_reset(8)
    assert L.gm_output_batch_bam(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(bo), None) == api.GM_E_CAPACITY
    assert bo.cap == len(once) and bo.len == 0 and (buf == 0xAA).all()
    assert float(ix.coverage_download().sum()) == 0.0
    assert L.gm_output_batch_bam(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(bo), None) == 0
    assert bytes(buf[:bo.len]) == once and (buf[bo.len:] == 0xAA).all()
    same_track(ix.coverage_download(), ref)
    bo.level = 3
    assert L.gm_output_batch_bam(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(bo), None) == -1
    del keep


@pytest.mark.parametrize("level", [0, 1])
def test_resident_form_on_a_text_block(abi, syn_fq, level):
    ix, p = abi["ix"], abi["p"]
    lines = open(syn_fq, "rb").read().splitlines(keepends=True)
    batch = g.Batch(ix, 64, 2048)
    for k in range(2):
        t = b"".join(lines[4 * 64 * k:4 * 64 * (k + 1)])
        assert batch.upload_text(p, t, want_recs=False)["n"] == 64
        text, _ = batch.output_text_resident(p, batch.map_text(p))
        out = batch.output_bam_resident(p, batch.map_text(p), level=level)
        want = bm.sam_to_bam_records(text, abi["contigs"])
        assert len(want) > 40
        check_records(bm.split_records(bm.bgzf_payload(out)), want)
    batch.destroy()


def test_fasta_block_with_iupac_letters_on_both_strands(abi):
    ix, p = abi["ix"], abi["p"]
    names, seqs = [], []
    for l in open(os.path.join(GOLDEN, "syn_reads.fa"), "rb"):
        if l.startswith(b">"):
            names.append(l[1:].strip()); seqs.append(b"")
        else:
            seqs[-1] += l.strip()
    iupac = [i for i, s in enumerate(seqs) if any(c not in b"ACGTNacgtn" for c in s)]
    pick = (iupac + [i for i in range(len(seqs)) if i not in iupac])[:64]
    names, seqs = [names[i] for i in pick], [seqs[i] for i in pick]
    B, Q, Ln = g.pack_reads(seqs, None)
    batch = g.Batch(ix, 64, B.shape[1])
    text, _ = batch.output_text(p, batch.map(p, B, None, Ln, fasta=True), names)
    rows = [r.split(b"\t") for r in text.splitlines()]
    odd = lambda r: any(c not in b"ACGTNacgtn" for c in r[9])
    assert any(r[1] == b"0" and odd(r) for r in rows) and any(r[1] == b"16" and b"n" in r[9] for r in rows), "IUPAC letters on both strands"
    for level in (0, 1):
        out = batch.output_bam(p, batch.map(p, B, None, Ln, fasta=True), names, level=level)
        check_records(bm.split_records(bm.bgzf_payload(out)), bm.sam_to_bam_records(text, abi["contigs"]))
    batch.destroy()


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def check_bam_file(bam_path, sam_path, sort=False):
    """<out>.bam against the SAM file of the default run: header lines (the @PG line aside), records = the model of the rows, end marker"""
    data = open(bam_path, "rb").read()
    assert data.endswith(bm.EOF) and not data[:-28].endswith(bm.EOF)
    members = bm.parse_bgzf(data)
    assert members[-1][0] == b"" and all(pl for pl, _, _ in members[:-1])
    payload = b"".join(pl for pl, _, _ in members)
    text, refs, at = bm.parse_header(payload)
    sam = open(sam_path, "rb").read()
    if sort:
        sam = sam_sort_model(sam)
    head = b"".join(l for l in sam.splitlines(keepends=True) if l.startswith(b"@"))
    assert no_pg(text) == no_pg(head) and b"@PG" in text and b"--sam_format=bam" in text
    assert [f"@SQ\tSN:{c}\tLN:{n}\n".encode() for c, n in refs] == [l for l in head.splitlines(keepends=True) if l.startswith(b"@SQ")]
    got = bm.split_records(payload[at:])
    want = bm.sam_to_bam_records(sam, refs)
    assert len(want) > 100
    check_records(got, want)
    return members, got


@pytest.fixture(scope="module")
def syn_run(tmp_path_factory, syn_fa, syn_fq):
    out = str(tmp_path_factory.mktemp("synbam") / "plain")
    drive(syn_fa, syn_fq, out, [])
    return out


CASES = [([], None), (["--bam_level=0"], None), (["--read_text=device"], None), (["--chunk_reads=64", "--workers=3"], None),
         (["--chunk_reads=500", "--workers=2"], {"GM_TEST_MAX_OUT_BLOCK": "60"})]
IDS = ["default", "level_0", "read_text_device", "small_blocks", "written_in_halves"]


@pytest.mark.parametrize("extra, env", CASES, ids=IDS)
def test_cli_bam_on_the_edge_genome(extra, env, edge_run, tmp_path):
    fa, fq, ctg, rd, plain = edge_run
    out = str(tmp_path / "o")
    r = drive(fa, fq, out, ["--sam_format=bam"] + extra, env=dict(os.environ, **env) if env else None)
    if env:
        assert "written in halves" in r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if not f.endswith(".sgr")) == ["o.bam"]      # no <out>.sam
    members, got = check_bam_file(out + ".bam", plain + ".sam")
    assert f"{len(got)} SAM records" in r.stderr
    assert all(bt == (0 if "--bam_level=0" in extra else 2) for _, bt, _ in members[:-1])
    compare_tracks(open(out + ".sgr").read(), open(plain + ".sgr").read(), 3)


@pytest.mark.parametrize("extra", [[], ["--bam_level=0", "--read_text=device", "--track_text=device"]], ids=["default", "level_0_device_text"])
def test_cli_bam_on_syn_fq(extra, syn_run, syn_fa, syn_fq, tmp_path):
    out = str(tmp_path / "o")
    drive(syn_fa, syn_fq, out, ["--sam_format=bam"] + extra)
    assert not os.path.exists(out + ".sam")
    check_bam_file(out + ".bam", syn_run + ".sam")
    compare_tracks(open(out + ".sgr").read(), open(syn_run + ".sgr").read(), 3)


@pytest.mark.parametrize("env", [None, {"GM_SORT_PIECE": "65536"}], ids=["one_piece", "small_pieces"])
def test_cli_sorted_bam(env, edge_run, tmp_path):
    fa, fq, ctg, rd, plain = edge_run
    out = str(tmp_path / "o")
    r = drive(fa, fq, out, ["--sam_format=bam"] + SORTED, env=dict(os.environ, **env) if env else None)
    if env:
        assert "pieces of 65536 bytes" in r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if not f.endswith(".sgr")) == ["o.bam"]
    members, got = check_bam_file(out + ".bam", plain + ".sam", sort=True)
    keys = [struct.unpack_from("<ii", x, 4) for x in got]
    assert keys == sorted(keys) and len(set(keys)) < len(keys)
    compare_tracks(open(out + ".sgr").read(), open(plain + ".sgr").read(), 3)


# ---- the sorter with BAM records ---------------------------------------------------------------------------------------------------
def bam_sorter(abi):
    g.set_option("GM_SORT_PIECE", 65536)
    try:
        s = api.SamSorter(abi["ix"], rows="bam")
    finally:
        g.set_option("GM_SORT_PIECE", None)
    for k in (3, 2, 1, 0):                                                    # added in reverse
        B, Q, Ln = abi["packed"][k]
        batch = abi["batches"][k]
        s.add_block(batch, abi["p"], batch.map(abi["p"], B, Q, Ln), 10 * k, names=abi["blocks"][k][0])
    return s


def sorted_model(abi):
    rows = [r.decode("latin-1") for k in range(4) for r in abi["rows"][k]]
    return bm.sam_to_bam_records("".join(sort_rows(rows, [c for c, _ in abi["contigs"]])).encode("latin-1"), abi["contigs"])


def test_sorter_with_bam_rows_reads_whole_records_in_model_order(abi):
    want = sorted_model(abi)
    s = bam_sorter(abi)
    with pytest.raises(g.GnumapError) as e:
        s.set_rows("text")                                                    # after an add
    assert e.value.code == -1
    n_rows, n_bytes = s.finish()
    assert n_rows == len(want) and n_bytes == sum(len(x) for x in want)
    slabs = []
    while True:
        t = s.read(20000)
        if not t:
            break
        assert len(t) <= 20000 and sum(len(x) for x in bm.split_records(t)) == len(t)      # whole records
        slabs.append(t)
    assert len(slabs) > 5
    check_records(bm.split_records(b"".join(slabs)), want)
    s.destroy()


@pytest.mark.parametrize("level", [0, 1])
def test_sorter_read_bgzf_returns_whole_blocks(abi, level):
    want = sorted_model(abi)
    s = bam_sorter(abi)
    s.finish()
    runs = []
    while True:
        t = s.read_bgzf(70000, level=level)
        if not t:
            break
        members = bm.parse_bgzf(t)                                            # whole blocks
        raw = b"".join(pl for pl, _, _ in members)
        assert len(t) <= 70000 and len(raw) + 31 * len(members) <= 70000 and sum(len(x) for x in bm.split_records(raw)) == len(raw)
        runs.append(raw)
    assert len(runs) >= 2
    check_records(bm.split_records(b"".join(runs)), want)
    with pytest.raises(g.GnumapError) as e:
        api.SamSorter(abi["ix"]).read_bgzf(70000, level=2)
    assert e.value.code == -1
    s.destroy()


# ---- a caller's own hits (stamp 0: validated and uploaded again) through every sink -------------------------------------------------
def test_a_callers_own_hits_give_what_the_resident_hits_give_through_every_sink(syn_fa, syn_reads, syn_fq):
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    rd = syn_reads[:300]
    names = [r[0].encode() for r in rd]
    B, Q, Ln = g.pack_reads([r[1] for r in rd], [r[2][:len(r[1])] for r in rd])
    batch = g.Batch(ix, len(rd), B.shape[1])

    def own(res):
        h = api.gm_hits()
        C.memmove(C.byref(h), C.byref(res["_struct"]), C.sizeof(h))
        assert h.stamp != 0
        h.stamp = 0
        return dict(res, _struct=h)

    def sorted_rows(res, rows, names):
        s = api.SamSorter(ix, rows=rows)
        s.add_block(batch, p, res, 0, names=names)
        n_rows, n_bytes = s.finish()
        out = s.text()
        s.destroy()
        return n_rows, n_bytes, out

    def every_sink(res, names):
        """(what each sink returned, the track after each); names None: the resident forms"""
        sinks = [lambda: batch.output_text(p, res, names) if names else batch.output_text_resident(p, res),
                 lambda: batch.output_bam(p, res, names, level=0) if names else batch.output_bam_resident(p, res, level=0),
                 lambda: batch.output_bam(p, res, names, level=1) if names else batch.output_bam_resident(p, res, level=1),
                 lambda: sorted_rows(res, "text", names), lambda: sorted_rows(res, "bam", names)]
        got, cov = [], []
        for sink in sinks:
            ix.coverage_reset(8)
            got.append(sink())
            cov.append(ix.coverage_download())
        return got, cov

    res = batch.map(p, B, Q, Ln)
    want, want_cov = every_sink(res, names)                                   # the resident hits first: a caller's version takes their place
    got, got_cov = every_sink(own(res), names)
    text, row_off = want[0]
    assert text.count(b"\n") > 150 and len(row_off) == text.count(b"\n") + 1
    assert got[0][0] == text and np.array_equal(got[0][1], row_off)
    assert got[1:] == want[1:]
    assert len(want[1]) > len(want[2]) > 28 and want[3][0] == want[4][0] == len(row_off) - 1 and want[3][2] != want[4][2]
    for a, b in zip(got_cov, want_cov):
        same_track(a, b)
    batch.destroy()

    # the pools of gm_batch_upload_text with a caller's own hits
    lines = open(syn_fq, "rb").read().splitlines(keepends=True)
    batch = g.Batch(ix, 300, 2048)
    assert batch.upload_text(p, b"".join(lines[:4 * 300]), want_recs=False)["n"] == 300
    res = batch.map_text(p)
    ix.coverage_reset(8)
    want = batch.output_text_resident(p, res)
    want_cov = ix.coverage_download()
    ix.coverage_reset(8)
    got = batch.output_text_resident(p, own(res))
    assert want[0].count(b"\n") > 150 and got[0] == want[0] and np.array_equal(got[1], want[1])
    same_track(ix.coverage_download(), want_cov)
    batch.destroy(); ix.close()
