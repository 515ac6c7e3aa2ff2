"""BGZF on the device (k_bgzf_deflate / k_bgzf_compact, gm_bam.hip) through gm_bgzf_compress, on bytes of the test's own: every output is
walked member by member by tests/bam_model.parse_bgzf (magic, BC subfield, BSIZE, raw inflate up to the trailer, CRC-32, ISIZE), has to
inflate to the input, has to come out the same twice, and has to equal byte for byte what tests/bgzf_lz_model.py writes without matches.

Sizes around the payload cut (65280), a payload of one byte value, one that cannot be compressed (stored, and never larger than stored),
Fibonacci histograms whose unlimited Huffman code is deeper than deflate's 15 bits, and BAM-like records, whose Huffman form is
measured against zlib's Z_HUFFMAN_ONLY raw deflate of the same payloads."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import gnumap_amd as g
import bam_model as bm
import bgzf_lz_model as lzm
from conftest import GOLDEN, read_fastq
from gnumap_amd import api

pytestmark = pytest.mark.gpu
P = bm.PAYLOAD


@pytest.fixture(scope="module")
def ix():
    i = g.Index(os.path.join(GOLDEN, "syn.fa"), device=0)
    yield i
    i.close()


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def shuffled(counts, first=65, seed=5):
    data = np.concatenate([np.full(c, first + i, np.uint8) for i, c in enumerate(counts)])
    np.random.default_rng(seed).shuffle(data)
    return data.tobytes()


def bam_like(n_bytes=200_000):
    """records the model builds from syn.fq's reads: names, packed bases, qualities and tags as a BAM file holds them"""
    reads = read_fastq(os.path.join(GOLDEN, "syn.fq"))
    rng = np.random.default_rng(11)
    rows = []
    for k, (name, seq, qual) in enumerate(reads + reads):                    # (syn.fq alone gives 123 KB: every read at two places)
        pos = int(rng.integers(1, 180000))
        rows.append(b"\t".join([name.encode() + (b"" if k < len(reads) else b"/b"), b"16" if k & 1 else b"0", b"chr1", str(pos).encode(), b"30", f"{len(seq)}M".encode(), b"*", b"0", b"0", seq, qual,
                                f"XA:f:{0.9 + 0.0001 * (k % 97):g}".encode(), b"XP:f:1", b"X0:i:1"]))
    raw = b"".join(bm.sam_to_bam_records(b"\n".join(rows), [("chr1", 200000)]))
    assert len(raw) >= n_bytes, len(raw)
    return raw[:n_bytes]


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(3)
    text = bytes(rng.choice(np.frombuffer(b"ACGTNacgtn\t\n0123456789IIIIIIII##", np.uint8), 2 * P + 1))
    cases = {f"size_{n}": text[:n] for n in (1, P - 1, P, P + 1, 2 * P + 1)}
    cases["one_value"] = b"\x07" * 5000
    cases["uniform"] = bytes(np.random.default_rng(4).permutation(np.tile(np.arange(256, dtype=np.uint8), 64)))      # 16384 bytes, every value 64 times
    cases["fib22"] = shuffled(fib(22))                                       # 46367 bytes, counts F(1) .. F(22)
    cases["fib21_eob"] = shuffled(fib(22)[1:])                               # 46366 bytes, counts F(2) .. F(22): with the end-of-block symbol's 1, F(1) .. F(22)
    cases["bam_like"] = bam_like()
    return cases


@pytest.fixture(scope="module")
def outputs(ix, inputs):
    """every case compressed once at both levels; shared by the tests below"""
    return {(k, lv): ix.bgzf_compress(v, level=lv) for k, v in inputs.items() for lv in (0, 1)}


def test_the_fibonacci_inputs_need_the_length_limit(inputs):
    """asserted on the test's own Huffman build, before anything of the device's is looked at.  Over its 22 literals alone the code of
    fib22 is 21 bits deep; a deflate block also codes the end-of-block symbol once, and with that 23rd count of 1 the optimal code of fib22
    is only 12 deep - so fib21_eob is the input in which the block's own 22 counts are F(1) .. F(22) and its code 21 deep."""
    h = np.bincount(np.frombuffer(inputs["fib22"], np.uint8), minlength=256).tolist()
    assert len(inputs["fib22"]) == 46367 and sorted(c for c in h if c) == fib(22)
    assert max(bm.huffman_lengths(h).values()) == 21
    h = np.bincount(np.frombuffer(inputs["fib21_eob"], np.uint8), minlength=256).tolist() + [1]
    assert sorted(c for c in h if c) == fib(22) and max(bm.huffman_lengths(h).values()) == 21


def test_empty_input(ix):
    assert ix.bgzf_compress(b"", level=0) == b"" and ix.bgzf_compress(b"", level=1) == b""
    with pytest.raises(g.GnumapError) as e:
        ix.bgzf_compress(b"abc", level=2)
    assert e.value.code == -1


@pytest.mark.parametrize("level", [0, 1])
def test_every_output_parses_and_inflates_to_its_input(inputs, outputs, level):
    for k, data in inputs.items():
        out = outputs[k, level]
        members = bm.parse_bgzf(out)
        n_blocks = (len(data) + P - 1) // P
        assert len(members) == n_blocks, k
        assert [len(p) for p, _, _ in members] == [min(P, len(data) - i * P) for i in range(n_blocks)], k          # every ISIZE
        assert b"".join(p for p, _, _ in members) == data, k
        assert gzip.decompress(out) == data, k
        for (p, btype, size) in members:
            assert size <= len(p) + 31, (k, size, len(p))                     # no block is larger than its stored form
            if level == 0:
                assert btype == 0 and size == len(p) + 31, k


def test_a_second_call_gives_identical_bytes(ix, inputs, outputs):
    for k in ("size_%d" % (2 * P + 1), "fib21_eob", "bam_like", "uniform"):
        for lv in (0, 1):
            assert ix.bgzf_compress(inputs[k], level=lv) == outputs[k, lv], (k, lv)


def test_block_types_at_level_1(inputs, outputs):
    assert [b for _, b, _ in bm.parse_bgzf(outputs["uniform", 1])] == [0]     # nothing to gain: stored
    assert outputs["uniform", 1] == outputs["uniform", 0]
    for k in ("one_value", "fib22", "fib21_eob", "size_%d" % P):
        assert all(b == 2 for _, b, _ in bm.parse_bgzf(outputs[k, 1])), k
        assert len(outputs[k, 1]) < len(outputs[k, 0]), k
    assert len(outputs["one_value", 1]) < 18 + 8 + 140 + 5000 // 8 + 8         # one bit per byte behind the code lengths
    assert [b for _, b, _ in bm.parse_bgzf(outputs["size_1", 1])] == [0]      # a Huffman block cannot beat 6 bytes


def test_level_1_bytes_equal_the_model(inputs, outputs):
    """byte for byte: level 1 against tests/bgzf_lz_model.py without matches (the code builder, the header, the bit stream, the rule
    for the stored block, CRC-32 and ISIZE), level 0 against stored members built here"""
    for k, data in inputs.items():
        assert outputs[k, 1] == lzm.compress(data, matches=False), k
        stored = b""
        for at in range(0, len(data), P):
            d = data[at:at + P]
            stored += (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 30) + b"\x01" + struct.pack("<HH", len(d), len(d) ^ 0xFFFF) + d +
                       struct.pack("<II", zlib.crc32(d), len(d)))
        assert outputs[k, 0] == stored, k


def test_capacity_one_byte_short(ix, inputs, outputs):
    for lv in (0, 1):
        want = outputs["bam_like", lv]
        with pytest.raises(g.GnumapError) as e:
            ix.bgzf_compress(inputs["bam_like"], level=lv, cap=len(want) - 1)
        assert e.value.code == api.GM_E_CAPACITY and e.value.needed == len(want)
        assert not e.value.buffer[len(want) - 1:].any()                       # nothing past cap
        assert ix.bgzf_compress(inputs["bam_like"], level=lv, cap=len(want)) == want


def test_size_against_zlib_huffman_only(inputs, outputs):
    """the deflate streams of the BAM-like input at level 1 against zlib's Z_HUFFMAN_ONLY raw deflate of the same 65280-byte payloads.  An
    optimal single-tree code behind the plain code-length header is within 0.1 % of zlib's (which run-length codes its header); the 1 %
    is room for the length-limit heuristic and nothing else."""
    data = inputs["bam_like"]
    members = bm.parse_bgzf(outputs["bam_like", 1])
    assert len(members) == 4 and all(b == 2 for _, b, _ in members)           # BTYPE=10 in every block
    mine = sum(size - 26 for _, _, size in members)
    ref = bm.zlib_huffman_only(data)
    print(f"deflate bytes of {len(data)} BAM-like bytes: device {mine}, zlib Z_HUFFMAN_ONLY {ref} ({100.0 * (mine / ref - 1):+.2f} %)")
    assert len(outputs["bam_like", 1]) < len(outputs["bam_like", 0])
    assert mine <= 1.01 * ref
