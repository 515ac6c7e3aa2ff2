"""--bam_lz77 / GM_BGZF_LZ77 without a device: the token-keeping inflate the GPU tests read the device's blocks with
(tests/deflate_model.py) against zlib's own output and against hand-made streams it has to refuse, the restatement of k_bgzf_deflate_lz
(tests/bgzf_lz_model.py) against both, the level word at the ABI of a host-only index, the constant and the keywords of the binding, and
the driver's usage text and refusals."""
import ctypes as C
import gzip
import inspect
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import gnumap_amd as g
import bam_model as bm
import bgzf_lz_model as lzm
import deflate_model as dm
from conftest import GOLDEN, ROOT
from gnumap_amd import api

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
GM_E_ARG, GM_E_NO_DEVICE = -1, -3


def golden_records(name="default"):
    """the BAM records bam_model makes of a golden SAM file"""
    text = gzip.open(os.path.join(GOLDEN, "ref_runs", name + ".sam.gz")).read()
    contigs = [(f[1][3:].decode(), int(f[2][3:])) for f in (l.split(b"\t") for l in text.splitlines() if l.startswith(b"@SQ"))]
    return b"".join(bm.sam_to_bam_records(text, contigs))


@pytest.fixture(scope="module")
def payloads():
    return {"records": golden_records()[:bm.PAYLOAD], "random": np.random.default_rng(2).integers(0, 256, 20000, dtype=np.uint8).tobytes()}


class Bits:
    """a hand-made stream, first bit lowest"""
    def __init__(self):
        self.v = self.n = 0

    def put(self, v, n):
        self.v |= v << self.n; self.n += n
        return self

    def code(self, v, n):                                # a Huffman code: most significant bit first
        return self.put(int(format(v, f"0{n}b")[::-1], 2), n)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8 + 1, "little")


ZLIB_FORMS = {"level_1": (1, zlib.Z_DEFAULT_STRATEGY), "level_6": (6, zlib.Z_DEFAULT_STRATEGY), "huffman_only": (6, zlib.Z_HUFFMAN_ONLY),
              "fixed": (6, zlib.Z_FIXED), "level_0": (0, zlib.Z_DEFAULT_STRATEGY)}


@pytest.mark.parametrize("form", list(ZLIB_FORMS))
@pytest.mark.parametrize("what", ["records", "random"])
def test_model_inflates_what_zlib_wrote(payloads, what, form):
    data = payloads[what]
    level, strategy = ZLIB_FORMS[form]
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    stream = c.compress(data) + c.flush()
    r = dm.inflate(stream)
    assert r.out == zlib.decompress(stream, -15) == data and r.used == len(stream)
    assert dm.expand(r.tokens) == data
    assert all(t[0] == "L" or (3 <= t[1] <= 258 and 1 <= t[2] <= 32768) for t in r.tokens)
    if form in ("huffman_only", "level_0"):
        assert all(t[0] == "L" for t in r.tokens)
    elif what == "records":
        assert any(t[0] == "M" for t in r.tokens)
    want = {("records", "fixed"): {1}, ("records", "level_0"): {0}, ("random", "level_0"): {0}, ("records", "level_6"): {2}}.get((what, form))
    if want:
        assert {b["btype"] for b in r.blocks} == want
    for b in r.blocks:
        if b["btype"] == 2:
            assert len(b["lit_lengths"]) == b["hlit"] and len(b["dist_lengths"]) == b["hdist"] and b["lit_lengths"][256]


def fixed_block():
    return Bits().put(1, 1).put(1, 2)


def dynamic_block(lit, dist):
    """a final dynamic block whose code lengths (at most 7) are sent as three bits each under a flat 3-bit code-length code"""
    b = Bits().put(1, 1).put(2, 2).put(len(lit) - 257, 5).put(len(dist) - 1, 5).put(15, 4)
    sent = {0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 6: 3, 7: 3}
    for s in dm.CL_ORDER:
        b.put(sent.get(s, 0), 3)
    for l in list(lit) + list(dist):
        b.code(l, 3)
    return b


def test_model_reads_hand_made_blocks():
    # fixed code: 'a' (0x30 + 97, 8 bits), length 3 (symbol 257: 0000001), distance 1 (00000), end of block (0000000)
    s = fixed_block().code(0x30 + 97, 8).code(1, 7).code(0, 5).code(0, 7).bytes()
    r = dm.inflate(s)
    assert r.out == b"aaaa" == zlib.decompress(s, -15) and r.tokens == [("L", 97), ("M", 3, 1)]
    # dynamic: literals 'a' and 'b' and the end of block at two bits, length symbol 257 at two; one distance symbol (0) at one bit
    lit = [0] * 258
    lit[97] = lit[98] = lit[256] = lit[257] = 2
    s = dynamic_block(lit, [1]).code(0, 2).code(1, 2).code(3, 2).code(0, 1).code(2, 2).bytes()
    r = dm.inflate(s)
    assert r.out == b"abbbb" == zlib.decompress(s, -15) and r.tokens == [("L", 97), ("L", 98), ("M", 3, 1)]
    assert r.blocks[0]["hlit"] == 258 and r.blocks[0]["hdist"] == 1 and r.blocks[0]["dist_lengths"] == [1]
    assert dm.length_symbol(3) == 257 and dm.length_symbol(258) == 285 and dm.length_symbol(257) == 284 and dm.length_symbol(10) == 264
    assert dm.distance_symbol(1) == 0 and dm.distance_symbol(32768) == 29 and dm.distance_symbol(24576) == 28 and dm.distance_symbol(5) == 4


def refusal_streams():
    lit = [0] * 258
    lit[97] = lit[98] = lit[256] = lit[257] = 2
    over = list(lit); over[99] = 2
    under = list(lit); under[257] = 0
    no_eob = list(lit); no_eob[256] = 0; no_eob[99] = 2
    return {
        "distance_beyond_the_output": (fixed_block().code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7), "distance 2 with 1 bytes"),
        "length_symbol_286": (fixed_block().code(0x30 + 97, 8).code(0xC0 + 6, 8).code(0, 5).code(0, 7), "length symbol 286"),
        "distance_symbol_30": (fixed_block().code(0x30 + 97, 8).code(1, 7).code(30, 5).code(0, 7), "distance symbol 30"),
        "over_subscribed": (dynamic_block(over, [1]), "over-subscribed"),
        "incomplete": (dynamic_block(under, [1]), "incomplete"),
        "incomplete_distance_code": (dynamic_block(lit, [2]), "incomplete"),
        "no_end_of_block_code": (dynamic_block(no_eob, [1]), "no end-of-block"),
        "stream_ends_early": (fixed_block().code(0x30 + 97, 8), "ends inside"),
        "stored_nlen": (Bits().put(1, 1).put(0, 2).put(0, 5).put(3, 16).put(3, 16).put(0x616161, 24), "NLEN"),
        "block_type_3": (Bits().put(1, 1).put(3, 2), "block type 3"),
    }


@pytest.mark.parametrize("case", list(refusal_streams()))
def test_model_refuses(case):
    bits, message = refusal_streams()[case]
    stream = bits.bytes() if case != "stream_ends_early" else bits.bytes()[:-1]
    with pytest.raises(AssertionError, match=re.escape(message)):
        dm.inflate(stream)
    if case != "incomplete_distance_code":               # (zlib lets any single distance code pass)
        with pytest.raises(zlib.error):
            d = zlib.decompressobj(-15)
            d.decompress(stream)
            if not d.eof:
                raise zlib.error("the stream ends early")


def model_cases(payloads):
    rng = np.random.default_rng(9)
    rep = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    return [b"a", b"abcabc", bytes(5000), (rep * 30)[:7000], payloads["records"], payloads["random"][:3000]]


def test_restated_kernel_writes_valid_members_with_the_tokens_it_found(payloads):
    """tests/bgzf_lz_model.py is what the GPU tests hold the device's bytes against: here it is held against zlib and the token model"""
    cases = model_cases(payloads)
    for data in cases:
        z = lzm.compress(data)
        (payload, btype, size), = bm.parse_bgzf(z)
        assert payload == data and size == len(z)
        r = dm.inflate(z[18:-8])
        assert r.out == data and r.tokens == [("L", t) if not isinstance(t, tuple) else ("M",) + t for t in lzm.tokens(data)] or btype == 0
    sizes = {len(d): len(lzm.compress(d)) for d in cases}
    assert sizes[1] == 32 and sizes[3000] == 3031                                                 # stored
    assert sizes[5000] < 300 and sizes[7000] < 1024
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    z1 = len(c.compress(payloads["records"]) + c.flush())
    huff = bm.zlib_huffman_only(payloads["records"])
    assert sizes[bm.PAYLOAD] - 26 <= (huff + z1) // 2, (sizes[bm.PAYLOAD], huff, z1)


def test_restated_level_1_writes_literal_blocks_or_stored_ones(payloads):
    """matches=False is k_bgzf_deflate at level 1 (tests/test_gpu_bgzf.py holds the device's bytes against it): one block over the bytes
    alone, never larger than stored, and the very block the matched form falls back to where matches do not pay"""
    for data in model_cases(payloads):
        z = lzm.compress(data, matches=False)
        (payload, btype, size), = bm.parse_bgzf(z)
        assert payload == data and size == len(z) and size <= len(data) + 31
        assert zlib.decompress(z[18:-8], -15) == data
        if btype != 0:
            r = dm.inflate(z[18:-8])
            assert r.out == data and r.tokens == [("L", b) for b in data]
            assert [(b["btype"], b["hlit"], b["hdist"]) for b in r.blocks] == [(2, 257, 1)]
        zm = lzm.compress(data)
        bl = dm.inflate(zm[18:-8]).blocks
        if bl[0].get("hlit") == 257:
            assert zm == z, len(data)
    assert len(lzm.compress(b"a", matches=False)) == 32                     # stored
    assert lzm.compress(payloads["records"], matches=False) != lzm.compress(payloads["records"])      # (the matched form does find matches there)


def test_level_word_on_a_host_only_index(syn_fa):
    L = g.lib()
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    n = C.c_uint64(7)
    out = (C.c_uint8 * 64)()
    assert L.gm_bgzf_compress(ix.h, b"abc", 3, 0x101, out, 64, C.byref(n), None) == GM_E_NO_DEVICE          # the level was accepted
    for level in (0x100, 0x102, 0x201, 0x10001):
        assert L.gm_bgzf_compress(ix.h, b"abc", 3, level, out, 64, C.byref(n), None) == GM_E_ARG, hex(level)
        text = L.gm_last_error().decode()
        assert "GM_BGZF_LZ77" in text and str(level) in text, text
    with pytest.raises(g.GnumapError) as e:
        ix.bgzf_compress(b"abc", level=1, lz77=True)
    assert e.value.code == GM_E_NO_DEVICE
    with pytest.raises(g.GnumapError) as e:
        ix.bgzf_compress(b"abc", level=0, lz77=True)
    assert e.value.code == GM_E_ARG
    assert L.gm_sam_sorter_read_bgzf(None, 0x101, None, 0, C.byref(n), None) == GM_E_ARG
    ix.close()


def test_constant_and_keywords():
    header = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    m = re.search(r"enum \{ GM_BGZF_LZ77 = (0x[0-9a-fA-F]+) \};", header)
    assert m and int(m.group(1), 16) == api.GM_BGZF_LZ77 == 0x100
    for f in (api.Index.bgzf_compress, api.Batch.output_bam, api.Batch.output_bam_resident, api.SamSorter.read_bgzf):
        p = inspect.signature(f).parameters
        assert p["lz77"].default is False and p["level"].default == 1, f


def run(args, tmp_path):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out] + args + [os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=600)
    return r, out


@pytest.mark.parametrize("args", [["--bam_lz77"], ["--bam_lz77", "--sam_format=bam", "--bam_level=0"]], ids=["alone", "level_0"])
def test_flag_is_refused_before_a_device_is_opened(args, tmp_path):
    r, out = run(args, tmp_path)
    assert r.returncode == 1 and "--bam_lz77" in r.stderr and r.stderr.startswith("Error: "), r.stderr[-1000:]
    assert "No matching arg" not in r.stderr and "no usable HIP device" not in r.stderr
    assert os.listdir(tmp_path) == []                                       # no file written


def test_usage_names_the_flag():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--bam_lz77" in r.stderr and "--bam_level=0|1" in r.stderr


def test_flag_gets_past_option_parsing(tmp_path):
    import torch
    r, out = run(["--sam_format=bam", "--bam_lz77"], tmp_path)
    assert "No matching arg" not in r.stderr and "--bam_lz77" not in r.stderr
    if torch.cuda.is_available():
        assert r.returncode == 0 and bm.parse_bgzf(open(out + ".bam", "rb").read()), r.stderr[-1500:]
    else:
        assert r.returncode != 0 and "no usable HIP device" in r.stderr      # GM_E_NO_DEVICE, not a parse error
