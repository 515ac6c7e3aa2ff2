"""Every egress kernel at human-size coordinates: the world of tests/wide_fixture.py (a 100 Mbp contig and 41 short ones behind it,
positions of one to nine digits, BAM bins of every level, indels beside bin boundaries, ties and reads that map nowhere) through

    records     gm_output_batch                       = the oracle's records and CIGARs, field for field
    text rows   gm_output_batch_text                  = sam_text_model.sam_rows of the ORACLE's records; with unmapped rows, unmapped_model.merge
    BAM         gm_output_batch_bam, levels 0 / 1 / 1 + LZ77 = bam_model's records of those rows; refID, pos and bin against the table's literals
    sorter      gm_sam_sorter, text and BAM rows      = sam_sort_model's order of the model rows
    .bai        gm_sam_sorter_bai                     = bai_model.build_bai of the file; every planted place is reached through it
    tracks      k_track_sizes / k_track_rows          = the host writer's file and a formatter in Python, at bin sizes 8 and 1; -b rows of ranges
    driver      --sam_text / --track_text =device, sorted BAM with its index and --sam_unmapped

The fixture asserts from the oracle's records that the world holds what it was planted for (wide_fixture.self_check) before any test
looks at the device.  It prints its build time; nothing is asserted about it."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import gnumap_amd as g
import bai_model as bai
import bam_model as bm
import unmapped_model as um
import wide_fixture as wf                   # puts tools/ on the path
import scale_check
from conftest import ROOT
from gnumap_amd import api
from sam_text_model import sam_rows
from test_gpu_sam_text import same_track

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
ARGV = ["-a", "0.9", "-m", "14", "-j", "7"]
HD = b"@HD\tVN:1.0\tSO:coordinate\n"


class Block:
    """a block of the world's reads, mapped once; the oracle's records of it (read = index in the block) and the model's rows"""

    def __init__(self, env, reads, orecs):
        self.reads = reads
        self.names = [r.name for r in reads]; self.seqs = [r.seq for r in reads]; self.quals = [r.qual for r in reads]
        self.status = [st for st, _ in orecs]
        self.orecs = [dict(q, read=i) for i, (_, recs) in enumerate(orecs) for q in recs]
        self.ocigars = [q["cigar"] for q in self.orecs]
        self.rows = sam_rows(self.orecs, self.ocigars, self.names, self.seqs, self.quals, env["names"], env["p"].adjust)
        self.merged, self.new = um.merge(self.rows, [q["read"] for q in self.orecs], self.names, self.seqs, self.quals, self.status)
        self.B, self.Q, self.Ln = g.pack_reads(self.seqs, self.quals)
        self.batch = g.Batch(env["ix"], len(reads), self.B.shape[1])
        self.res = self.batch.map(env["p"], self.B, self.Q, self.Ln)

    def place_of_row(self, k):
        return wf.PLACES[self.reads[self.orecs[k]["read"]].place]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from reflib import OracleLib
    t0 = time.time()
    d = tmp_path_factory.mktemp("wide")
    w = wf.World(d, g.index_build)
    t1 = time.time()
    ix = g.Index(w.fa, device=0, flags=g.GM_INDEX_FULL_SA)
    t2 = time.time()
    orecs = wf.oracle_records(w, OracleLib())
    counts = wf.self_check(w, orecs)
    p = g.Params(**wf.KW)
    assert [(n, o) for n, o in ix.contigs()] == [(n, o) for (n, _), o in zip(w.contigs, w.offs)] and ix.info.l_pac == w.offs[-1]
    env = dict(w=w, ix=ix, p=p, orecs=orecs, names=[n for n, _ in w.contigs], contigs=w.contigs, dir=d)
    ix.coverage_reset(8)
    env["blocks"] = [Block(env, w.reads[lo:hi], orecs[lo:hi]) for lo, hi in w.blocks]
    print(f"\nwide world: FASTA + index build {t1 - t0:.1f} s, index load {t2 - t1:.1f} s, oracle + mapping {time.time() - t2:.1f} s, "
          f"{time.time() - t0:.1f} s in all; oracle records per class {counts}")
    yield env
    for b in env["blocks"]:
        b.batch.destroy()
    ix.close()
    shutil.rmtree(d, ignore_errors=True)


def test_world_is_three_unequal_blocks_with_every_class(world):
    blocks = world["blocks"]
    assert len({len(b.reads) for b in blocks}) == 3 and sum(len(b.reads) for b in blocks) == 170
    assert sum(len(b.rows) for b in blocks) == 154 and sum(sum(b.new) for b in blocks) == wf.N_NOWHERE
    for b in blocks:
        assert any(b.new) and {wf.PLACES[r.place].cls for r in b.reads if r.place is not None} >= {"digits", "bins", "indels", "short"}


# ---- records ----------------------------------------------------------------------------------------------------------------------
def test_records_equal_the_oracles_field_for_field(world):
    bits = lambda x: int(np.float32(x).view(np.uint32))
    for b in world["blocks"]:
        recs, cigars = b.batch.output(world["p"], b.res)
        got = [(int(r["read"]), int(r["pos"]), int(r["contig"]), int(r["chr_pos"]), int(r["strand"]), int(r["mapq"]), c, bits(r["a_score"]), bits(r["post_prob"]),
                int(r["sim_matches"])) for r, c in zip(recs, cigars)]
        want = [(q["read"], int(q["pos"]), int(q["contig"]), int(q["chr_pos"]), int(q["strand"]), int(q["mapq"]), q["cigar"], bits(q["a_score"]), bits(q["post_prob"]),
                 int(q["sim_matches"])) for q in b.orecs]
        assert got == want
        assert [int(s) for s in b.res["status"]] == b.status


# ---- text rows --------------------------------------------------------------------------------------------------------------------
def check_rows(text, row_off, want):
    assert len(row_off) == len(want) + 1 and int(row_off[0]) == 0 and int(row_off[-1]) == len(text)
    got = [text[int(row_off[k]):int(row_off[k + 1])] for k in range(len(want))]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
    assert text == b"".join(want)
    assert all(r.endswith(b"\n") and r.count(b"\n") == 1 for r in got)


def test_text_rows_equal_the_formatter_fed_with_the_oracles_records(world):
    digits = set()
    for b in world["blocks"]:
        b.batch.set_unmapped_rows(False)
        text, row_off = b.batch.output_text(world["p"], b.res, b.names, text_cap=16)
        assert b.batch.text_calls == 2                              # 16 bytes: GM_E_CAPACITY with the needed size, then that size
        check_rows(text, row_off, b.rows)
        digits |= {len(r.split(b"\t")[3]) for r in b.rows}
    assert digits == set(range(1, 10))


def test_text_capacity_answer_is_the_needed_size(world):
    import ctypes as C
    b = world["blocks"][1]
    b.batch.set_unmapped_rows(False)
    rt, keep = api._pack_read_text(b.names, None, len(b.names))
    small = np.zeros(16, np.uint8)
    st = api.gm_sam_text(); st.text = small.ctypes.data; st.text_cap = 16
    rc = g.lib().gm_output_batch_text(world["ix"].h, C.byref(world["p"].c), b.batch.h, C.byref(b.res["_reads"]), C.byref(rt), C.byref(b.res["_struct"]), C.byref(st), None)
    assert rc == api.GM_E_CAPACITY and st.text_cap == st.text_len == len(b"".join(b.rows)) and st.n_recs == len(b.rows)
    del keep


def test_text_with_unmapped_rows_equals_the_models_merge(world):
    for b in world["blocks"]:
        b.batch.set_unmapped_rows(True)
        try:
            text, row_off = b.batch.output_text(world["p"], b.res, b.names, text_cap=16)
            assert b.batch.unmapped_rows() == sum(b.new)
        finally:
            b.batch.set_unmapped_rows(False)
        check_rows(text, row_off, b.merged)


# ---- BAM --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,lz77", [(0, False), (1, False), (1, True)], ids=["stored", "huffman", "lz77"])
def test_bam_records_equal_the_model_and_the_tables_literals(world, level, lz77):
    seen = set()
    for b in world["blocks"]:
        b.batch.set_unmapped_rows(False)
        got = bm.split_records(bm.bgzf_payload(b.batch.output_bam(world["p"], b.res, b.names, level=level, lz77=lz77)))
        want = bm.sam_to_bam_records(b"".join(b.rows), world["contigs"])
        why = bm.records_equal(got, want)
        assert why is None, why
        for k, rec in enumerate(got):
            f = um.fixed_fields(rec)
            pl = b.place_of_row(k)
            assert (f[0], f[1], f[4]) == (pl.contig, pl.start, pl.bin), (pl, f)          # refID, 0-based pos, bin
            seen.add(f[4])
    assert set(wf.BIN_LITERALS) <= seen and {0, 1, 9, 73, 585, 1097, 5291, 10784} <= seen


# ---- the sorter and the .bai ------------------------------------------------------------------------------------------------------
SEQS = (20, 30, 10)                                   # the blocks arrive as 0, 1, 2 and are numbered so that they count as 2, 0, 1


def sorter_with(world, rows, seqs):
    s = api.SamSorter(world["ix"], rows=rows)
    for b, seq in zip(world["blocks"], seqs):
        b.batch.set_unmapped_rows(True)
        try:
            s.add_block(b.batch, world["p"], b.res, seq, names=b.names)
        finally:
            b.batch.set_unmapped_rows(False)
    order = sorted(range(len(seqs)), key=lambda k: seqs[k])
    merged = [r for k in order for r in world["blocks"][k].merged]
    new = [x for k in order for x in world["blocks"][k].new]
    want = um.sort_rows(merged, world["names"])
    assert s.finish()[0] == len(want) == 170
    tail = [r for r, x in zip(merged, new) if x]
    assert len(tail) == wf.N_NOWHERE and want[-len(tail):] == tail                # rows without a contig last, in input order
    return s, want


def sorted_bam(world, s, level, lz77=False):
    ix = world["ix"]
    head = ix.bgzf_compress(ix.bam_header(HD), level=level)
    s.index_begin(len(head))
    slabs = []
    while True:
        t = s.read_bgzf(20000, level=level, lz77=lz77)
        if not t:
            break
        slabs.append(t)
    assert len(slabs) >= 2
    return head + b"".join(slabs) + api.bgzf_eof()


def test_sorter_text_rows_in_the_models_order(world):
    s, want = sorter_with(world, "text", SEQS)
    assert s.text(cap=9000) == b"".join(want)
    dup = [r.split(b"\t")[0] for r in want if r.startswith(b"ties:dup:")]
    order = sorted(range(3), key=lambda k: SEQS[k])
    assert dup == [r.name for k in order for r in world["blocks"][k].reads if r.name.startswith(b"ties:dup:")] and len(dup) == 2 * wf.N_DUP      # ties in input order
    keys = [(world["names"].index(f[2].decode()), int(f[3])) for f in (r.split(b"\t") for r in want[:-wf.N_NOWHERE])]
    assert keys == sorted(keys) and keys[-1][0] == 41 and max(k[1] for k in keys) == 100_000_901
    s.destroy()


def planted_regions(world):
    """(refID, beg, end) of every planted place, and the windows around every boundary"""
    out = [(pl.contig, pl.start, pl.start + wf.SPANS[pl.kind]) for pl in wf.PLACES]
    for B, _, _ in wf.BOUNDARIES:
        out += [(0, B - 1, B), (0, B, B + 1), (0, B - 200, B + 200)]
    out += [(0, 0, 1 << 29), (41, 0, 1 << 29), (0, 99_999_000, 100_001_000)]
    return out


@pytest.mark.parametrize("level,lz77", [(0, False), (1, False), (1, True)], ids=["stored", "huffman", "lz77"])
def test_sorter_bam_rows_and_the_index(world, level, lz77):
    s, want = sorter_with(world, "bam", SEQS)
    data = sorted_bam(world, s, level, lz77)
    sc = bai.scan(data)
    why = um.records_differ([bytes(x) for x in sc["recs"]], um.to_records(want, world["contigs"]))
    assert why is None, why
    got = s.bai()
    assert got == bai.build_bai(data)
    parsed = bai.parse_bai(got)
    assert parsed["n_no_coor"] == wf.N_NOWHERE == int((sc["ref"] < 0).sum())
    regions = planted_regions(world)
    assert bai.check_queries(data, got, regions) >= 154 + len(wf.PLACES)
    for pl in wf.PLACES:                                                          # the record of the place itself, by its literal bin
        mine = [k for k in range(len(sc["recs"])) if sc["ref"][k] == pl.contig and sc["pos"][k] == pl.start and um.fixed_fields(sc["recs"][k])[4] == pl.bin
                and sc["end"][k] == pl.start + wf.SPANS[pl.kind]]
        assert len(mine) >= 2, pl
        hit = bai.records_in_chunks(data, bai.query(parsed, pl.contig, pl.start, pl.start + 1))
        assert set(mine) <= hit, pl
        assert any(c for c in parsed["refs"][pl.contig]["bins"].get(pl.bin, ())), pl
    assert {0, 1, 9, 73, 585, 1097} <= set(parsed["refs"][0]["bins"])
    s.destroy()


# ---- tracks -----------------------------------------------------------------------------------------------------------------------
def deposit(world, bs, p=None, nuc=False, text=False):
    """fresh tracks of this bin size with every block's deposits, through gm_output_batch or gm_output_batch_text"""
    ix = world["ix"]
    ix.coverage_reset(bs)
    if nuc:
        ix.coverage_enable_nuc()
    for b in world["blocks"]:
        if p is None:
            batch, res, pp = b.batch, b.res, world["p"]
        else:
            batch = g.Batch(ix, len(b.reads), b.B.shape[1]); pp = p
            res = batch.map(pp, b.B, b.Q, b.Ln)
        if text:
            batch.output_text(pp, res, b.names)
        else:
            batch.output(pp, res)
        if p is not None:
            batch.destroy()


def sgr_rows(world, cov, bs, lo, hi):
    """PrintFinalSGR's rows of the bins [lo, hi) in Python (tools/scale_check.track_rows: the formatter of
    test_gpu_track_text.py::test_sgr_equals_the_host_writer, on the bins that are not 0)"""
    return b"".join(r for _, r in scale_check.track_rows(world["names"], np.array(world["w"].offs[:-1], np.int64), None, 0, bs, lo, cov[lo:hi], None))


def track_ranges(world, bs):
    """bin ranges: over the 7-to-8 and the 8-to-9 digit change, chrW's end and the next contig's start, the 150-base contig, the last bin"""
    o = world["w"].offs
    nbk = (o[-1] + bs - 1) // bs
    at = lambda pos: pos // bs
    return dict(digits_7_8=(at(9_999_900), at(10_000_100) + 1), digits_8_9=(at(99_999_900), at(100_000_100) + 1), chrW_end=(at(o[1] - 120), at(o[1] + 120) + 1),
                contig_150=(at(o[2] - 16), at(o[3] + 16) + 1), genome_end=(nbk - at(120) - 1, nbk), beyond_the_end=(nbk - 3, nbk + 64))


@pytest.mark.parametrize("bs", [8, 1])
def test_sgr_device_file_host_file_and_formatter_agree(world, bs, tmp_path):
    ix = world["ix"]
    deposit(world, bs)
    cov = ix.coverage_download()
    nbk = (ix.info.l_pac + bs - 1) // bs
    assert ix.coverage_bins() == ix.info.l_pac // bs + 64
    host, dev = str(tmp_path / "host.sgr"), str(tmp_path / "dev.sgr")
    ix.coverage_write_sgr(cov, host)
    ix.coverage_write_sgr_device(dev)
    want = open(host, "rb").read()
    assert open(dev, "rb").read() == want
    assert ix.coverage_text_stats()["host_slabs"] == 0
    assert want == sgr_rows(world, cov, bs, 0, nbk) and want.count(b"\n") > 3000 // bs
    assert {len(l.split(b"\t")[1]) for l in want.splitlines()} == set(range(1, 10))          # every digit count is printed
    for what, (lo, hi) in track_ranges(world, bs).items():
        got = ix.coverage_text(None, lo, min(hi, ix.coverage_bins()))
        assert got == sgr_rows(world, cov, bs, lo, min(hi, nbk)), what
        assert got.count(b"\n") >= 100 // bs or what == "beyond_the_end", what
    r78 = ix.coverage_text(None, *track_ranges(world, bs)["digits_7_8"]); r89 = ix.coverage_text(None, *track_ranges(world, bs)["digits_8_9"])
    assert {len(l.split(b"\t")[1]) for l in r78.splitlines()} == {7, 8} and {len(l.split(b"\t")[1]) for l in r89.splitlines()} == {8, 9}
    edge = ix.coverage_text(None, *track_ranges(world, bs)["chrW_end"]).splitlines()
    assert {l.split(b"\t")[0] for l in edge} == {b"chrW", b"s01"} and any(l.startswith(b"s01\t1\t") for l in edge)
    small = ix.coverage_text(None, *track_ranges(world, bs)["contig_150"]).splitlines()
    assert {l.split(b"\t")[0] for l in small} == {b"s01", b"s02"}
    last = ix.coverage_text(None, *track_ranges(world, bs)["genome_end"]).splitlines()[-1].split(b"\t")
    assert last[0] == b"s41" and int(last[1]) == (nbk - 1) * bs - world["w"].offs[41] + 1


def gmp_rows(world, pac, cov, nuc, lo, hi):
    """PrintFinalBisulfite's rows of the positions [lo, hi) from the tracks' values of that range (cov[hi - lo], nuc[5][hi - lo])"""
    return b"".join(r for _, r in scale_check.track_rows(world["names"], np.array(world["w"].offs[:-1], np.int64), pac, 1, 1, lo, cov, nuc))


def test_bisulfite_rows_on_both_sides_of_10_8(world):
    """-b: coverage_text of ranges around planted places against the formatter fed with the DEVICE's own bins of those ranges (the values
    are checked elsewhere: the text kernel is under test), and those bins against a second deposit through gm_output_batch_text"""
    import torch
    from gnumap_amd import dist as gd
    ix, o = world["ix"], world["w"].offs
    p1 = g.Params(mode=1, **wf.KW)
    l_pac = o[-1]
    ranges = [(9_999_900, 10_000_150), (99_999_850, 100_000_250), (o[1] - 150, o[1] + 150), (o[2] - 10, o[3] + 10), (o[10] - 50, o[10] + 150), (l_pac - 150, l_pac)]
    pac = np.fromfile(world["w"].fa + ".gnumap.pac", np.uint8)
    dev = torch.device("cuda", 0)

    def views():
        bins = ix.coverage_bins()
        track = gd.DeviceTrack(ix.coverage_device_ptr(), bins).tensor(dev)
        nt = gd.DeviceTrack(ix.coverage_nuc_device_ptr(), 5 * bins).tensor(dev)
        return [(track[lo:hi].cpu().numpy(), [nt[q * bins + lo:q * bins + hi].cpu().numpy() for q in range(5)]) for lo, hi in ranges]

    deposit(world, 1, p1, nuc=True)
    vals = views()
    rows = 0
    for (lo, hi), (cov, nuc) in zip(ranges, vals):
        got = ix.coverage_text(p1, lo, hi)
        assert got == gmp_rows(world, pac, cov, nuc, lo, hi), (lo, hi)
        rows += got.count(b"\n")
        assert got.count(b"\n") >= 10, (lo, hi)
    assert ix.coverage_text_stats()["host_slabs"] == 0 and rows > 150
    # only positions whose reference base is c print, and one planted position has 7 (8) digits beside the change: the longer count is there
    assert 8 in {len(l.split(b"\t")[1]) for l in ix.coverage_text(p1, *ranges[0]).splitlines()}
    assert 9 in {len(l.split(b"\t")[1]) for l in ix.coverage_text(p1, *ranges[1]).splitlines()}
    assert {l.split(b"\t")[0] for l in ix.coverage_text(p1, *ranges[4]).splitlines()} == {b"Z", b"L" + b"x" * 199}          # the 1- and the 200-character name
    deposit(world, 1, p1, nuc=True, text=True)
    again = views()
    same_track(np.concatenate([c for c, _ in again]), np.concatenate([c for c, _ in vals]))
    same_track(np.concatenate([x for _, n in again for x in n]), np.concatenate([x for _, n in vals for x in n]))


# ---- the driver -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fq(world):
    path = str(world["dir"] / "wide.fq")
    with open(path, "wb") as f:
        f.write(world["w"].fastq())
    return path


def drive(world, fq, out, extra):
    r = subprocess.run([EXE, "-g", world["w"].fa, "-o", out] + ARGV + extra + [fq], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def rows_of(path):
    return [l for l in open(path, "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]


def test_cli_device_text_and_track_text_equal_the_host_paths(world, fq, tmp_path):
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    drive(world, fq, host, ["--sam_text=host", "--track_text=host"])
    r = drive(world, fq, dev, ["--sam_text=device", "--track_text=device"])
    assert "gm_output_batch_text" in r.stderr and "track text on the device:" in r.stderr and "(0 formatted by the host)" in r.stderr
    strip = lambda path: b"".join(l for l in open(path, "rb").read().splitlines(keepends=True) if not l.startswith(b"@PG"))
    assert strip(dev + ".sam") == strip(host + ".sam")
    assert rows_of(dev + ".sam") == [r for b in world["blocks"] for r in b.rows]
    sq = [l for l in open(dev + ".sam", "rb").read().splitlines() if l.startswith(b"@SQ")]
    assert len(sq) == 42 and sq[0] == b"@SQ\tSN:chrW\tLN:100001000"
    sgr = open(dev + ".sgr", "rb").read()
    assert sgr == open(host + ".sgr", "rb").read() and sgr.count(b"\n") > 300
    assert {len(l.split(b"\t")[1]) for l in sgr.splitlines()} == set(range(1, 10))


def test_cli_sorted_bam_with_index_and_unmapped_rows(world, fq, tmp_path):
    out = str(tmp_path / "o")
    drive(world, fq, out, ["--sam_sort=coordinate", "--sam_format=bam", "--bam_index", "--sam_unmapped"])
    data, index = open(out + ".bam", "rb").read(), open(out + ".bam.bai", "rb").read()
    sc = bai.scan(data)
    s, want = sorter_with(world, "bam", (0, 1, 2))                  # the ABI-level sorter on the blocks in file order
    abi = bai.scan(sorted_bam(world, s, 1))
    s.destroy()
    assert [bytes(x) for x in sc["recs"]] == [bytes(x) for x in abi["recs"]]
    why = um.records_differ([bytes(x) for x in sc["recs"]], um.to_records(want, world["contigs"]))
    assert why is None, why
    assert index == bai.build_bai(data)
    parsed = bai.parse_bai(index)
    assert parsed["n_no_coor"] == wf.N_NOWHERE
    assert bai.check_queries(data, index, planted_regions(world)) >= 154 + len(wf.PLACES)
