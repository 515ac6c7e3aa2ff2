"""--sam_format=bam without a device: the reader and model the GPU tests compare with (tests/bam_model.py) against records written out
by hand from SAMv1 section 4.2, reg2bin at its level boundaries, gm_bam_header and gm_bgzf_eof (host code), the ABI's refusals on a
host-only index, and the driver's usage text and refusals."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import gnumap_amd as g
import bam_model as bm
from conftest import GOLDEN, ROOT
from gnumap_amd import api

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
NEW = ("gm_bam_header", "gm_bgzf_compress", "gm_bgzf_eof", "gm_output_batch_bam", "gm_output_batch_bam_resident", "gm_sam_sorter_set_rows",
       "gm_sam_sorter_read_bgzf")
CONTIGS = [("chrA", 1000), ("chrB", 70000)]


def test_model_on_a_forward_row_written_out_by_hand():
    row = b"r1\t0\tchrB\t16385\t30\t5M\t*\t0\t0\tACGTN\tI5!+~\tXA:f:0.5\tXP:f:1\tX0:i:3\n"
    want = b"".join([
        struct.pack("<i", 1), struct.pack("<i", 16384),                     # refID, pos (0-based)
        bytes([3, 30]), struct.pack("<H", 4681 + 1),                        # l_read_name, mapq, bin: [16384, 16389) lies in the second 16 KiB window
        struct.pack("<H", 1), struct.pack("<H", 0), struct.pack("<i", 5),   # n_cigar_op, flag, l_seq
        struct.pack("<iii", -1, -1, 0),                                     # next_refID, next_pos, tlen
        b"r1\0", struct.pack("<I", 5 << 4 | 0),                             # read_name, 5M
        bytes([0x12, 0x48, 0xF0]),                                          # A C | G T | N pad
        bytes([40, 20, 0, 10, 93]),                                         # I 5 ! + ~ minus 33
        b"XAf", struct.pack("<f", 0.5), b"XPf", struct.pack("<f", 1.0), b"X0i", struct.pack("<i", 3)])
    want = struct.pack("<i", len(want)) + want
    assert bm.sam_to_bam_records(b"@SQ\tSN:chrA\tLN:1000\n" + row, CONTIGS) == [want]
    assert bm.split_records(want + want) == [want, want]
    assert bm.float_tag_offsets(want) == (len(want) - 18, len(want) - 11)
    assert bm.records_equal([want], [want]) is None


def test_model_on_a_reverse_row_with_an_insertion_and_a_deletion():
    # as the SAM row prints it: the CIGAR already in reversed token order, SEQ reverse-complemented (a non-ACGT letter became n)
    row = b"name/2\t16\tchrA\t101\t0\t2M1I3M2D4M\t*\t0\t0\tacgtnACGTa\tABCDEFGHIJKL\tXA:f:-1.25e-05\tXP:f:0.333333\tX0:i:-2"
    ops = [(2, 0), (1, 1), (3, 0), (2, 2), (4, 0)]
    want = b"".join([
        struct.pack("<i", 0), struct.pack("<i", 100), bytes([7, 0]), struct.pack("<H", 4681), struct.pack("<H", 5), struct.pack("<H", 16),
        struct.pack("<i", 10), struct.pack("<iii", -1, -1, 0), b"name/2\0",
        b"".join(struct.pack("<I", n << 4 | o) for n, o in ops),
        bytes([0x12, 0x48, 0xF1, 0x24, 0x81]),                              # a c | g t | n A | C G | T a
        bytes(c - 33 for c in b"ABCDEFGHIJ"),                               # the first l_seq characters of a longer quality line
        b"XAf", struct.pack("<f", -1.25e-05), b"XPf", struct.pack("<f", 0.333333), b"X0i", struct.pack("<i", -2)])
    want = struct.pack("<i", len(want)) + want
    assert bm.sam_to_bam_records(row, CONTIGS) == [want]
    # the reference span of the CIGAR is M + D = 11: [100, 111)
    assert struct.unpack_from("<H", want, 14)[0] == bm.reg2bin(100, 111)
    near = bytearray(want)
    xa, _ = bm.float_tag_offsets(want)
    near[xa:xa + 4] = struct.pack("<f", -1.25e-05 * (1 + 4e-6))
    assert bm.records_equal([bytes(near)], [want]) is None
    near[xa:xa + 4] = struct.pack("<f", -1.25e-05 * (1 + 8e-6))
    assert "float tag" in bm.records_equal([bytes(near)], [want])
    other = bytearray(want); other[40] ^= 1
    assert "differs at byte 40" in bm.records_equal([bytes(other)], [want])


def test_model_cuts_names_and_counts_no_operation():
    row = b"n" * 300 + b"\t0\tchrA\t1\t300\t*\t*\t0\t0\tA\t \tXA:f:1\tXP:f:1\tX0:i:1"
    rec = bm.sam_to_bam_records(row, CONTIGS)[0]
    assert rec[12] == 255 and rec[36:36 + 255] == b"n" * 254 + b"\0" and rec[13] == 255          # l_read_name is one byte; mapq clamped
    assert struct.unpack_from("<H", rec, 16)[0] == 0 and struct.unpack_from("<H", rec, 14)[0] == bm.reg2bin(0, 1)     # no operation: a span of 1
    assert rec[36 + 255:36 + 255 + 2] == bytes([0x10, 0])                    # one base, one quality below '!' floored at 0


def test_reg2bin_at_the_level_boundaries():
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        edge = 1 << shift
        assert bm.reg2bin(0, edge) == first                                  # ends at the boundary: the first window of that size
        assert bm.reg2bin(edge, 2 * edge) == first + 1                       # starts at it: the second
        assert bm.reg2bin(edge - 10, edge) == 4681 + (edge >> 14) - 1 and bm.reg2bin(edge, edge + 10) == 4681 + (edge >> 14)      # short spans beside it stay in 16 KiB windows
        up = {14: 585, 17: 73, 20: 9, 23: 1, 26: 0}[shift]
        assert bm.reg2bin(edge - 1, edge + 1) == up                          # across it: one level up
    assert bm.reg2bin(0, 1) == 4681 and bm.reg2bin(0, 1 << 29) == 0


def test_bam_header_on_a_host_only_index(syn_fa):
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    contigs = []
    for l in open(syn_fa):
        if l.startswith(">"):
            contigs.append([l[1:].split()[0], 0])
        else:
            contigs[-1][1] += len(l.strip())
    assert contigs and [c for c, _ in contigs] == [c for c, _ in ix.contigs()]
    text = b"@HD\tVN:1.0\tSO:coordinate\n" + b"".join(f"@SQ\tSN:{c}\tLN:{n}\n".encode() for c, n in contigs)
    want = bm.header_bytes(text, contigs)
    assert ix.bam_header(text) == want
    assert ix.bam_header(b"") == bm.header_bytes(b"", contigs)
    assert bm.parse_header(want) == (text, [(c, n) for c, n in contigs], len(want))
    L = g.lib()
    buf = (C.c_uint8 * (len(want) + 8))(*([0xAA] * (len(want) + 8)))
    need = C.c_uint64(0)
    assert L.gm_bam_header(ix.h, text, len(text), buf, len(want) - 1, C.byref(need)) == api.GM_E_CAPACITY      # one byte short
    assert need.value == len(want) and bytes(buf) == b"\xAA" * (len(want) + 8)
    assert L.gm_bam_header(ix.h, text, len(text), buf, len(want), C.byref(need)) == 0
    assert bytes(buf) == want + b"\xAA" * 8
    ix.close()


def test_entry_points_are_exported_declared_and_refuse_a_host_only_index(syn_fa):
    L = g.lib()
    header = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in api.EXPORTS and f"int {name}(" in header, name
    assert "GM_ROWS_TEXT = 0, GM_ROWS_BAM = 1" in header and (api.GM_ROWS_TEXT, api.GM_ROWS_BAM) == (0, 1)
    for name in ("output_bam", "output_bam_resident"):
        assert hasattr(api.Batch, name)
    assert hasattr(api.Index, "bam_header") and hasattr(api.Index, "bgzf_compress") and hasattr(api.SamSorter, "read_bgzf") and hasattr(api, "bgzf_eof")
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    n = C.c_uint64(7)
    out = (C.c_uint8 * 64)()
    assert L.gm_bgzf_compress(ix.h, b"abc", 3, 1, out, 64, C.byref(n), None) == -3 and "no usable HIP device" in L.gm_last_error().decode()
    assert L.gm_bgzf_compress(ix.h, b"abc", 3, 2, out, 64, C.byref(n), None) == -1          # GM_E_ARG: the level
    with pytest.raises(g.GnumapError) as e:
        ix.bgzf_compress(b"abc")
    assert e.value.code == -3
    p = g.Params()
    hits = api.gm_hits(); reads = api.gm_reads(); rt = api.gm_read_text(); bo = api.gm_bam_out()
    assert L.gm_output_batch_bam(ix.h, C.byref(p.c), None, C.byref(reads), C.byref(rt), C.byref(hits), C.byref(bo), None) == -3
    assert L.gm_output_batch_bam_resident(ix.h, C.byref(p.c), None, C.byref(hits), C.byref(bo), None) == -3
    assert L.gm_sam_sorter_set_rows(None, 1) == -1 and L.gm_sam_sorter_read_bgzf(None, 1, None, 0, C.byref(n), None) == -1
    ix.close()


def test_the_end_marker():
    spec = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert api.bgzf_eof() == spec == bm.EOF
    assert bm.parse_bgzf(spec) == [(b"", 1, 28)]                            # an empty payload in one fixed-Huffman block
    assert bm.parse_bgzf(spec + spec) == [(b"", 1, 28)] * 2
    with pytest.raises(AssertionError):
        bm.parse_bgzf(spec[:-1] + b"\x01")                                   # ISIZE
    with pytest.raises(AssertionError):
        bm.parse_bgzf(spec[:16] + b"\x1c" + spec[17:] + b"\0")               # BSIZE past the trailer: the stream must end at it


def test_huffman_lengths():
    assert bm.huffman_lengths([5, 0, 1, 1]) == {0: 1, 2: 2, 3: 2}
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) == 46367 and max(bm.huffman_lengths(fib).values()) == 21


def run(args, tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out] + args + [os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=600)
    return r, out


@pytest.mark.parametrize("args, flag", [
    (["--sam_format=cram"], "--sam_format"),
    (["--bam_level=2", "--sam_format=bam"], "--bam_level"),
    (["--bam_level=1"], "--bam_level"),
    (["--sam_format=bam", "--sam_text=host"], "--sam_text=host"),
    (["--sam_format=bam", "--sam_shards=2"], "--sam_shards"),
], ids=["cram", "level_2", "level_alone", "text_host", "shards"])
def test_refusals_before_a_device_is_opened(args, flag, tmp_path):
    r, out = run(args, tmp_path)
    assert r.returncode == 1 and flag in r.stderr and r.stderr.startswith("Error: "), r.stderr[-1000:]
    assert "No matching arg" not in r.stderr and "no usable HIP device" not in r.stderr
    assert os.listdir(tmp_path) == []                                       # no file written


def test_level_2_alone_is_refused_for_its_value(tmp_path):
    r, out = run(["--bam_level=2"], tmp_path)
    assert r.returncode == 1 and "--bam_level takes 0 or 1, not: 2" in r.stderr and os.listdir(tmp_path) == []


def test_usage_names_both_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--sam_format=sam|bam" in r.stderr and "--bam_level=0|1" in r.stderr and "<out>.bam" in r.stderr
