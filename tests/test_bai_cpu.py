"""--bam_index without a device: tests/bai_model.py against a .bai written out by hand for a BAM of twelve hand-placed records in
hand-sized BGZF blocks (bins from SAMv1 section 5.3, offsets from the blocks' sizes), the specification's query on every fixture the GPU
tests use, the driver's refusals and usage line, and the ABI's refusals that need no GPU.

The fixture builders of tests/test_gpu_bai.py live here, so that what they build is checked on the model before a device sees it."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gnumap_amd as g
import bai_model as bai
import bam_model as bm
from conftest import GOLDEN, ROOT
from gnumap_amd import api

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
NEW = ("gm_sam_sorter_index_begin", "gm_sam_sorter_bai")


# ---- building blocks -------------------------------------------------------------------------------------------------------------
def row(name, flag, rname, pos0, cigar, L=23):
    """a SAM row: pos0 is 0-based; L bases"""
    return b"\t".join([name, b"%d" % flag, rname, b"%d" % (pos0 + 1), b"30", cigar, b"*", b"0", b"0", b"A" * L, b"I" * L, b"XA:f:1", b"XP:f:1", b"X0:i:1"])


def unplaced(rec):
    """the record with refID = pos = -1"""
    return rec[:4] + struct.pack("<ii", -1, -1) + rec[12:]


def bgzf_block(payload, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(payload), len(payload)))


def slabs_of(recs, cap=200000):
    """the records cut as gm_sam_sorter_read_bgzf(cap) cuts them: as many whole records as are sure to fit cap as stored blocks"""
    per = bm.PAYLOAD + 31
    room = cap // per * bm.PAYLOAD + max(cap % per - 31, 0)
    out, cur, size = [], [], 0
    for r in recs:
        if cur and size + len(r) > room:
            out.append(cur); cur, size = [], 0
        cur.append(r); size += len(r)
    if cur:
        out.append(cur)
    return out


def assemble(header, recs, cap=200000, level=1):
    """the file the driver writes: the header's blocks, every slab's blocks of 65280 bytes, the end marker"""
    out = [bgzf_block(header[a:a + bm.PAYLOAD], level) for a in range(0, len(header), bm.PAYLOAD)]
    for slab in slabs_of(recs, cap):
        raw = b"".join(slab)
        out += [bgzf_block(raw[a:a + bm.PAYLOAD], level) for a in range(0, len(raw), bm.PAYLOAD)]
    return b"".join(out) + bm.EOF


# ---- the fixture of the GPU tests ------------------------------------------------------------------------------------------------
BIG_CONTIGS = [("f%d" % i, 300) for i in range(7)]


def big_fixture(contigs=BIG_CONTIGS):
    """(records in coordinate order, their (contig, chr_pos) keys): what test_fixture_holds_what_the_index_has_to_get_right lists"""
    rows = []                                    # (ref, pos0, flag, cigar)

    def add(ref, pos0, cigar=b"120M", flag=0):
        rows.append((ref, pos0, flag, cigar))

    # f0: no record.  f1: windows 0 .. 2 empty, 300 records in window 3, windows 4 and 5 empty, a record over windows 6 and 7
    for i in range(300):
        add(1, 3 * 16384 + 7 * i)
    add(1, 7 * 16384 - 60)
    # f2: the bin levels.  Ends exactly on 2^14 (leaf bin), spans 2^14 (bin 585), no CIGAR, > 70 KB of leaf records, 585 again (a second
    # chunk), leaf records, 585 twice more close by (merged), then one record across each higher boundary, up to bin 0
    add(2, 16384 - 120)
    add(2, 16384 - 60)
    add(2, 20000, b"*")
    for i in range(300):
        add(2, 20010 + 5 * i)
    add(2, 2 * 16384 - 60)
    add(2, 2 * 16384 + 10); add(2, 2 * 16384 + 20)
    add(2, 3 * 16384 - 60)
    add(2, 3 * 16384 + 10)
    add(2, 4 * 16384 - 60)
    for shift in (17, 20, 23, 26):
        add(2, (1 << shift) - 60)
    add(2, (1 << 26) + 100, flag=4)              # placed, flag 0x4: unmapped in the pseudo-bin
    # f3: no record.  f4, f5: the bulk.  f6: no record
    for i in range(600):
        add(4, 100 + 3 * i, b"60M2D58M" if i % 7 == 3 else b"50M3I67M" if i % 7 == 5 else b"120M")
    for i in range(500):
        add(5, 1 + 5 * i, flag=16 if i & 1 else 0)
    names = [c for c, _ in contigs]
    text = [row(b"q%05d" % i, flag, names[ref].encode(), pos0, cigar, 120) for i, (ref, pos0, flag, cigar) in enumerate(rows)]
    text += [row(b"u%05d" % i, 4, names[0].encode(), 0, b"*", 120) for i in range(5)]
    recs = bm.sam_to_bam_records(b"\n".join(text), contigs)
    recs[-5:] = [unplaced(r) for r in recs[-5:]]
    keys = [(ref, pos0 + 1) for ref, pos0, _, _ in rows] + [(len(contigs), 0)] * 5
    # one read name padded so that a record of the first slab ends exactly on byte 65280 of its payload
    ends = np.cumsum([len(r) for r in recs])
    k = int(np.searchsorted(ends, bm.PAYLOAD))                               # the first record that ends at or behind the boundary
    if ends[k] != bm.PAYLOAD:
        pad = bm.PAYLOAD - int(ends[k - 1])
        assert 0 < pad < 240
        f = text[k - 1].split(b"\t")
        f[0] += b"x" * pad
        recs[k - 1] = bm.sam_to_bam_records(b"\t".join(f), contigs)[0]
    return recs, keys


def small_fixtures(contigs):
    """{name: records} of the other cases of tests/test_gpu_bai.py, on an index with these contigs"""
    c0 = contigs[0][0].encode()
    one = bm.sam_to_bam_records(row(b"only", 0, c0, 77, b"23M"), contigs)
    at_limit = bm.sam_to_bam_records(row(b"edge", 0, c0, (1 << 29) - 23, b"23M"), contigs)
    return {"one_row": one, "end_2_29": at_limit}


# ---- the model against an index written out by hand --------------------------------------------------------------------------------
def vo(coffset, uoffset):
    return coffset << 16 | uoffset


def hand_bam():
    contigs = [("c0", 1000), ("c1", 100000), ("c2", 50000), ("c3", 10)]
    header = bm.header_bytes(b"", contigs)
    assert len(header) == 12 + 4 * 11                                         # 56 bytes: a stored block of 87
    rows = [row(b"r00", 0, b"c1", 100, b"23M"),                               # [100, 123): window 0, bin 4681
            row(b"r01", 0, b"c1", 16380, b"23M"),                             # [16380, 16403): windows 0 and 1, bin 585
            row(b"r02", 0, b"c1", 16390, b"23M"),                             # window 1, bin 4682
            row(b"r03", 0, b"c1", 32760, b"23M"),                             # [32760, 32783): windows 1 and 2, bin 585 again
            row(b"r04", 4, b"c1", 32770, b"23M"),                             # window 2, bin 4683, flag 0x4
            row(b"r05", 0, b"c1", 40000, b"23M"),                             # window 2, bin 4683
            row(b"r06", 0, b"c1", 49150, b"23M"),                             # [49150, 49173): windows 2 and 3, bin 585
            row(b"r07", 0, b"c1", 90000, b"23M"),                             # window 5, bin 4686; window 4 stays empty
            row(b"r08", 0, b"c2", 20000, b"23M"),                             # window 1, bin 4682: window 0 is a leading empty one
            row(b"r09", 0, b"c2", 20010, b"*"),                               # no CIGAR: [20010, 20011); 96 bytes
            row(b"r10", 16, b"c2", 20020, b"23M"),
            row(b"r11", 4, b"c0", 0, b"23M")]
    recs = bm.sam_to_bam_records(b"\n".join(rows), contigs)
    recs[11] = unplaced(recs[11])
    assert [len(r) for r in recs] == [100] * 9 + [96, 100, 100]
    raw = b"".join(recs)
    # stored blocks: payload + 31 bytes.  Block 1 holds r00 .. r03 and half of r04, block 2 its other half and r05 (which ends on the payload's end), block 3 the rest
    data = bgzf_block(header, 0) + bgzf_block(raw[:450], 0) + bgzf_block(raw[450:600], 0) + bgzf_block(raw[600:], 0) + bm.EOF
    assert len(data) == 87 + 481 + 181 + 627 + 28
    return data


def test_model_equals_an_index_written_out_by_hand():
    data = hand_bam()
    B1, B2, B3, END = 87, 568, 749, 1376
    want = b"BAI\x01" + struct.pack("<i", 4)
    want += struct.pack("<ii", 0, 0)                                          # c0: no record
    want += struct.pack("<i", 6)                                              # c1: five bins and the pseudo-bin
    want += struct.pack("<Ii", 585, 2) + struct.pack("<QQQQ", vo(B1, 100), vo(B1, 400), vo(B3, 0), vo(B3, 100))   # r01 + r03 merged (both in block 1), r06
    want += struct.pack("<Ii", 4681, 1) + struct.pack("<QQ", vo(B1, 0), vo(B1, 100))
    want += struct.pack("<Ii", 4682, 1) + struct.pack("<QQ", vo(B1, 200), vo(B1, 300))
    want += struct.pack("<Ii", 4683, 1) + struct.pack("<QQ", vo(B1, 400), vo(B3, 0))            # r04 (straddles blocks 1 and 2) and r05, which ends on a payload's end
    want += struct.pack("<Ii", 4686, 1) + struct.pack("<QQ", vo(B3, 100), vo(B3, 200))
    want += struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", vo(B1, 0), vo(B3, 200), 7, 1)
    want += struct.pack("<i", 6) + struct.pack("<6Q", vo(B1, 0), vo(B1, 100), vo(B1, 300), vo(B3, 0), vo(B3, 0), vo(B3, 100))
    want += struct.pack("<i", 2)                                              # c2
    want += struct.pack("<Ii", 4682, 1) + struct.pack("<QQ", vo(B3, 200), vo(B3, 496))
    want += struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", vo(B3, 200), vo(B3, 496), 3, 0)
    want += struct.pack("<i", 2) + struct.pack("<2Q", 0, vo(B3, 200))
    want += struct.pack("<ii", 0, 0)                                          # c3
    want += struct.pack("<Q", 1)                                              # r11
    got = bai.build_bai(data)
    assert got == want
    s = bai.scan(data)
    assert s["vbeg"][4] == vo(B1, 400) and s["vend"][4] == vo(B2, 50) and s["vend"][5] == vo(B3, 0) and s["vend"][11] == vo(END, 0)
    p = bai.parse_bai(got)
    assert p["n_no_coor"] == 1 and [r["order"] for r in p["refs"]] == [[], [585, 4681, 4682, 4683, 4686, 37450], [4682, 37450], []]
    assert p["refs"][1]["pseudo"] == (vo(B1, 0), vo(B3, 200), 7, 1) and p["refs"][2]["lin"] == [0, vo(B3, 200)]


def test_reader_on_the_hand_written_index():
    data = hand_bam()
    p = bai.parse_bai(bai.build_bai(data))
    assert bai.reg2bins(0, 1 << 29) == list(range(37449))
    assert bai.reg2bins(16384, 16385) == [0, 1, 9, 73, 585, 4682]
    hit = lambda ref, a, b: bai.records_in_chunks(data, bai.query(p, ref, a, b))
    assert bai.overlapping(data, 1, 16384, 16390) == {1} and 1 in hit(1, 16384, 16390)
    assert bai.overlapping(data, 1, 32768, 32769) == {3} and 3 in hit(1, 32768, 32769)
    assert hit(1, 90000, 90001) == {7}                                        # the linear index drops the chunks of bin 585 in front of r07
    assert hit(1, 70000, 80000) <= {6} and hit(0, 0, 1000) == set() and hit(3, 0, 10) == set()
    assert bai.overlapping(data, 2, 20010, 20011) == {8, 9} and bai.overlapping(data, 2, 20011, 20012) == {8}   # no CIGAR: one base
    assert bai.check_queries(data, bai.build_bai(data), bai.regions_of(data)) > 100
    with pytest.raises(AssertionError):
        bai.records_in_chunks(data, [(vo(87, 50), vo(87, 100))])              # a chunk that starts inside a record
    with pytest.raises(AssertionError):
        bai.parse_bai(bai.build_bai(data) + b"\0")


def test_model_refuses_what_the_device_refuses():
    contigs = [("c0", 1000)]
    header = bm.header_bytes(b"", contigs)
    ok, over = (bm.sam_to_bam_records(row(b"r", 0, b"c0", (1 << 29) - 23 + d, b"23M"), contigs) for d in (0, 1))
    got = bai.parse_bai(bai.build_bai(assemble(header, ok)))
    assert got["refs"][0]["order"] == [0 + 4681 + 32767, 37450] and len(got["refs"][0]["lin"]) == 32768
    with pytest.raises(ValueError):
        bai.build_bai(assemble(header, over))
    a, b = (bm.sam_to_bam_records(row(b"r", 0, b"c0", p, b"23M"), contigs)[0] for p in (10, 9))
    with pytest.raises(ValueError):
        bai.build_bai(assemble(header, [a, b]))


# ---- the fixtures of the GPU tests, on the model's own index -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_file():
    recs, keys = big_fixture()
    return assemble(bm.header_bytes(b"", BIG_CONTIGS), recs), recs, keys


def check_big_fixture(data, recs):
    """what the fixture has to contain, read from the model of the file `data` (header, slabs of cap 200000, end marker)"""
    s = bai.scan(data)
    n = len(recs)
    assert 1500 < n < 2000 and len(slabs_of(recs)) >= 3
    u_beg, u_end = s["vbeg"] & 0xFFFF, s["vend"] & 0xFFFF
    c_beg, c_end = s["vbeg"] >> 16, s["vend"] >> 16
    sizes = np.array([len(r) for r in recs])
    first_slab = np.cumsum(sizes[:len(slabs_of(recs)[0])])
    assert bm.PAYLOAD in first_slab                                          # a record ends exactly on byte 65280 of a payload ...
    k = int(np.nonzero(first_slab == bm.PAYLOAD)[0][0])
    assert u_end[k] == 0 and c_end[k] == c_beg[k + 1] and u_beg[k + 1] == 0 and c_end[k] > c_beg[k]      # ... its end is (the next block, 0), where a record starts
    assert any(c_end[i] > c_beg[i] and u_end[i] > 0 for i in range(n))       # a record straddles two blocks
    # the last record of a slab whose last block is short: its end is the next slab's first block, not a payload's end
    last = np.cumsum([len(x) for x in slabs_of(recs)])[:-1] - 1
    assert any(u_end[i] == 0 and (u_beg[i] + sizes[i]) % bm.PAYLOAD != 0 for i in last)
    ref, pos, end = s["ref"], s["pos"], s["end"]
    bins = [bm.reg2bin(int(a), int(b)) for a, b in zip(pos, end)]
    for shift, b in ((14, 585), (17, 73), (20, 9), (23, 1), (26, 0)):
        assert any(bins[i] == b and pos[i] < 1 << shift < end[i] for i in range(n) if ref[i] == 2), shift
    assert any(end[i] == 1 << 14 and bins[i] == 4681 for i in range(n))      # ends on 2^14: stays in the leaf
    assert any(struct.unpack_from("<H", recs[i], 16)[0] == 0 and end[i] == pos[i] + 1 and ref[i] >= 0 for i in range(n))     # no CIGAR
    p = bai.parse_bai(bai.build_bai(data))
    lin1 = p["refs"][1]["lin"]
    assert lin1[:3] == [0, 0, 0] and lin1[3] != 0 and lin1[4] == lin1[5] == lin1[3] and lin1[6] == lin1[7] != lin1[3]      # empty windows in front and between; one record over two windows
    runs585 = sum(1 for i in range(n) if ref[i] == 2 and bins[i] == 585 and not (i and ref[i - 1] == 2 and bins[i - 1] == 585))
    chunks585 = p["refs"][2]["bins"][585]
    assert runs585 == 4 and len(chunks585) == 2                              # left and re-entered inside one block: merged; after > 70 KB: a second chunk
    assert (chunks585[1][0] >> 16) > (chunks585[0][1] >> 16)
    assert [bool(r["order"]) for r in p["refs"]] == [False, True, True, False, True, True, False]
    assert p["n_no_coor"] == 5
    assert p["refs"][2]["pseudo"][3] == 1 and any(s["flag"][i] & 4 and ref[i] == 2 for i in range(n))
    return p


def test_big_fixture_holds_what_the_index_has_to_get_right(big_file):
    data, recs, keys = big_file
    check_big_fixture(data, recs)
    assert keys == sorted(keys) and len(keys) == len(recs)


def test_query_property_on_the_model_of_every_gpu_fixture(big_file):
    data, recs, _ = big_file
    assert bai.check_queries(data, bai.build_bai(data), bai.regions_of(data)) > 5000
    header = bm.header_bytes(b"", BIG_CONTIGS)
    for name, small in small_fixtures(BIG_CONTIGS).items():
        f = assemble(header, small)
        regions = bai.regions_of(f, n_random=20) if name != "end_2_29" else [(0, w << 14, (w + 1) << 14) for w in (0, 32766, 32767)] + [(0, 0, 1 << 29)]
        assert bai.check_queries(f, bai.build_bai(f), regions) >= 1, name
    empty = bai.build_bai(assemble(header, []))
    assert empty == b"BAI\x01" + struct.pack("<i", 7) + b"\0" * 56 + b"\0" * 8 and len(empty) == 8 + 8 * 7 + 8


# ---- the driver and the ABI without a device ---------------------------------------------------------------------------------------
def run(args, tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out] + args + [os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=600)
    return r, out


@pytest.mark.parametrize("args, missing", [
    (["--bam_index"], "--sam_format=bam"),
    (["--bam_index", "--sam_format=bam"], "--sam_sort=coordinate"),
    (["--bam_index", "--sam_sort=coordinate"], "--sam_format=bam"),
], ids=["alone", "no_sort", "no_bam"])
def test_bam_index_is_refused_before_a_device_is_opened(args, missing, tmp_path):
    r, out = run(args, tmp_path)
    assert r.returncode == 1 and r.stderr.startswith("Error: --bam_index") and f"give {missing}" in r.stderr, r.stderr[-1000:]
    assert "No matching arg" not in r.stderr and "no usable HIP device" not in r.stderr
    assert os.listdir(tmp_path) == []                                       # no file written


def test_usage_names_the_flag():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--bam_index " in r.stderr and "<out>.bam.bai" in r.stderr
    assert "--sam_format=sam|bam" in r.stderr and "--bam_level=0|1" in r.stderr       # the lines that were there stay


def test_entry_points_are_exported_declared_and_refuse_null(syn_fa):
    L = g.lib()
    header = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in api.EXPORTS and f"int {name}(" in header, name
    assert hasattr(api.SamSorter, "index_begin") and hasattr(api.SamSorter, "bai")
    fields = [k for k, _ in api.gm_sam_sort_stats._fields_]
    assert fields[-3:] == ["bai_ms", "bai_bytes", "bai_chunks"] and fields[:9] == ["rows", "text_bytes", "pieces", "piece_bytes", "add_s", "sort_s", "gather_ms", "gather_bytes", "download_s"]
    n = C.c_uint64(7)
    assert L.gm_sam_sorter_index_begin(None, 0) == -1
    assert L.gm_sam_sorter_bai(None, None, 0, C.byref(n), None) == -1
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    with pytest.raises(g.GnumapError) as e:
        api.SamSorter(ix, rows="bam")                                        # no sorter, so no index, without a device
    assert e.value.code == -3
    ix.close()
