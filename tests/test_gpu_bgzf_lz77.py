"""BGZF with LZ77 matches on the device (k_bgzf_deflate_lz, gm_bam.hip; level 1 | GM_BGZF_LZ77, --bam_lz77).  Every output is walked
member by member by tests/bam_model.parse_bgzf (zlib inflates it; CRC-32, ISIZE, BSIZE) AND read by tests/deflate_model.inflate, which
keeps the tokens and asserts on everything RFC 1951 forbids; and it has to equal, byte for byte, what tests/bgzf_lz_model.py - the
kernel's scheme in plain Python - writes for the same input, which pins WHICH matches the device finds and that nothing in it depends
on timing.

What the matcher cannot reach and the tests therefore do not ask for: a match of length 3 (a match counts from
4 bytes: length symbol 257 is never used), and a source in the same tile of 256 positions as the match.

Two cases the tests do not have.  A source that is not 16-byte aligned: every caller of gm_bgzf_device passes the start of an allocation
and payloads begin at multiples of 65280, so no entry point reaches the kernel's byte-wise load.  An input on which the 15-bit limit
acts on a code of the matched form: with matches taken out, the Fibonacci inputs of tests/test_gpu_bgzf.py no longer give a code deeper
than 15 (13 for the one used here); the limit itself is asserted, and the builder (bz_build_code) is the one level 1 runs, where fib21_eob reaches the limit."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import gnumap_amd as g
import bai_model as bai
import bam_model as bm
import bgzf_lz_model as lzm
import deflate_model as dm
from conftest import GOLDEN
from gnumap_amd import api
from test_gpu_bam import abi, bam_sorter, check_records, sorted_model  # noqa: F401  (abi is a fixture)
from test_bgzf_lz77_cpu import golden_records
from test_gpu_bgzf import fib, shuffled
from test_gpu_sam_sort import SORTED, drive, no_pg

pytestmark = pytest.mark.gpu
P = bm.PAYLOAD
LENGTHS = (3, 4, 10, 257, 258, 259, 300, 600)
DISTANCES = sorted({e for b, x in zip(dm.DIST_BASE, dm.DIST_EXTRA) for e in (b, b + (1 << x) - 1)} | {32769, 50000})
PERIODS = (1, 2, 3, 4, 5, 8, 31, 32, 255, 256, 257, 300)


def rnd(n, seed, lo=0):
    return np.random.default_rng(seed).integers(lo, 256, n, dtype=np.uint8).tobytes()


def text(n, seed=3):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"ACGTNacgtn\t\n0123456789IIIIIIII##", np.uint8), n))


def planted(length, distance=1000):
    """64 byte values at random - six bits each, so the block is not stored - with bytes [2000, 2000 + length) copied from 1000 back"""
    d = bytearray(b & 63 for b in rnd(3000, 100 + length))
    d[2000:2000 + length] = d[2000 - distance:2000 - distance + length]
    return bytes(d)


def repeat_at(d):
    """a 64-byte random string again at distance d, zeros between (random bytes there would have the block stored, and a few byte values at
    random have it written as level 1 writes it: one match does not pay for the lengths of two codes); below 64, a d-byte string
    repeated to 512 bytes"""
    if d < 64:
        return (rnd(d, 200 + d) * 512)[:512]
    s = rnd(64, 200 + d, lo=1)
    return s + bytes(d - 64) + s


def de_bruijn(k, n):
    """the k-ary de Bruijn sequence of order n (every n-gram once, cyclically), as bytes 0 .. k - 1"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(seq)


def every_symbol():
    """zeros, and for every distance symbol a string again at that symbol's first distance, in a length of a length symbol (258 .. 285 in
    turn: 257 is a length of 3).  The second copy starts a tile, so its source lies in an earlier one; its first byte is no zero, so
    the match over the zeros in front of it ends where it begins; the byte behind it differs from the one behind its source"""
    d = bytearray(P)
    rng = np.random.default_rng(77)
    want = []
    for i, dist in enumerate(dm.DIST_BASE):
        length = dm.LEN_BASE[1 + i % 28]
        free = lambda a, b: a >= 0 and b <= P and not any(d[a:b])
        at = next(a for a in range(256 * ((dist + 511) // 256), P, 256)              # the first tile start with room for both copies
                  if free(a - dist - 8, a - dist + min(dist, length) + 8) and free(a - 8 if dist > 8 else a, a + length + 8))
        src = at - dist
        d[src:src + min(dist, length)] = rng.integers(1, 255, min(dist, length), dtype=np.uint8).tobytes()
        for j in range(length):
            d[at + j] = d[src + j]
        d[at + length] = 255 if d[src + length] != 255 else 254
        want.append((length, dist))
    return bytes(d), want


def build_cases():
    c = {f"n{n}": text(n) for n in (1, 2, 3, 4, 5)}
    c["abc2"] = b"abc" * 2
    c.update({f"size_{n}": text(n) for n in (P - 1, P, P + 1, 2 * P + 17)})
    c.update({f"len_{n}": planted(n) for n in LENGTHS})
    c.update({f"dist_{d}": repeat_at(d) for d in DISTANCES})
    c.update({f"period_{d}": (rnd(d, 400 + d) * 4096)[:4096] for d in PERIODS})
    c["equal"] = b"\x07" * P
    c["period_300_full"] = (rnd(300, 500) * 300)[:P]
    c["random"] = rnd(20000, 600)
    c["one_distance"] = bytes(np.random.default_rng(601).permutation(256).astype(np.uint8)) * 16
    c["no_repeat"] = de_bruijn(16, 3) + b"\0\0"
    f = shuffled(fib(22))
    c["fib_tail"] = f + f[-18000:]
    c["every_symbol"] = every_symbol()[0]
    c["records"] = golden_records()[:2 * P + 17]
    return c


def read_members(out):
    """[(payload, BTYPE, size, deflate_model's reading of the member's stream)]; both readers have to agree"""
    res, at = [], 0
    for payload, btype, size in bm.parse_bgzf(out):
        r = dm.inflate(out[at + 18:at + size - 8])
        assert r.out == payload and dm.expand(r.tokens) == payload and r.used == size - 26 and len(r.blocks) == 1 and r.blocks[0]["btype"] == btype
        assert all(t[0] == "L" or (3 <= t[1] <= 258 and 1 <= t[2] <= 32768) for t in r.tokens)
        res.append((payload, btype, size, r))
        at += size
    return res


def matches(members):
    return [t for m in members for t in m[3].tokens if t[0] == "M"]


@pytest.fixture(scope="module")
def ix():
    i = g.Index(os.path.join(GOLDEN, "syn.fa"), device=0)
    yield i
    i.close()


@pytest.fixture(scope="module")
def cases():
    return build_cases()


@pytest.fixture(scope="module")
def outputs(ix, cases):
    """every case compressed once, shared by the tests below"""
    return {k: ix.bgzf_compress(v, level=1, lz77=True) for k, v in cases.items()}


@pytest.fixture(scope="module")
def members(cases, outputs):
    """every output read once by both readers: it inflates to its input, member by member"""
    res = {}
    for k, data in cases.items():
        res[k] = read_members(outputs[k])
        assert [len(m[0]) for m in res[k]] == [min(P, len(data) - at) for at in range(0, len(data), P)], k
        assert b"".join(m[0] for m in res[k]) == data, k
        assert all(m[2] <= len(m[0]) + 31 for m in res[k]), k               # no block is larger than its stored form
    return res


def test_sizes(cases, members):
    for n in (1, 2, 3, 4, 5):
        assert [(m[1], m[2]) for m in members[f"n{n}"]] == [(0, n + 31)]     # nothing to gain: stored
    assert len(members["abc2"]) == 1 and not matches(members["abc2"])         # (its one match has length 3)
    for n in (P - 1, P, P + 1, 2 * P + 17):
        ms = members[f"size_{n}"]
        assert len(ms) == (n + P - 1) // P and ms[0][1] == 2
    one = members[f"size_{P + 1}"][1]
    assert one[0] == cases[f"size_{P + 1}"][P:] and one[3].tokens == [("L", one[0][0])]        # nothing refers across the boundary
    assert not matches(members[f"size_{2 * P + 17}"][2:])                     # 17 bytes
    ms = members["records"]
    assert [m[1] for m in ms] == [2, 2, 0] and all(len(matches([m])) > 1000 for m in ms[:2])
    huff, z1 = deflate_sizes(cases["records"][:2 * P])
    assert sum(m[2] - 26 for m in ms[:2]) <= (huff + z1) / 2                  # at least half of what zlib -1 gains over Huffman alone


def test_planted_lengths(members):
    for n in LENGTHS:
        ms = matches(members[f"len_{n}"])
        assert all(3 <= t[1] <= 258 for t in ms)
        if n >= 257:                                     # found, cut at 258 (another candidate of the same hash may hide its first bytes);
                                                         # a short one does not pay for its two codes' lengths: level 1's block is written
            assert min(n, 258) - 4 <= max(t[1] for t in ms if t[2] == 1000) <= min(n + 2, 258), (n, ms)


def test_distances(members):
    found = set()
    for d in DISTANCES:
        ms = matches(members[f"dist_{d}"])
        assert all(t[2] <= 32768 for t in ms)
        # validity is what is asked for; all the same the repeat is found wherever its source lies in an earlier tile of 256 positions
        # (512 bytes of a period near 64 are written stored: 256 literals and the code lengths leave nothing to gain)
        if 256 <= d <= 32768 or (d < 64 and members[f"dist_{d}"][0][1] == 2):
            assert any(t[2] == d and t[1] >= 60 for t in ms), d


def test_the_matcher_works(cases, members):
    """at worst the period + a few literals, two matches per 255 bytes at 48 bits at most, a header of at most 170 bytes"""
    for d in PERIODS:
        (m,) = members[f"period_{d}"]
        assert m[2] < 1024 and matches([m]), d
    assert members["equal"][0][2] < 2048 and matches(members["equal"])
    assert members["period_300_full"][0][2] < P // 8 and matches(members["period_300_full"])


def test_code_edges(cases, members):
    (m,) = members["random"]
    assert m[1] == 0 and m[2] == 20000 + 31                                  # stored
    (m,) = members["one_distance"]
    ms = matches([m])
    assert m[1] == 2 and len(ms) > 10 and {t[2] for t in ms} == {256}
    dl = m[3].blocks[0]["dist_lengths"]
    assert sorted(dl) == [0] * (len(dl) - 1) + [1] and dl[dm.distance_symbol(256)] == 1       # one distance symbol, a one-bit code
    (m,) = members["no_repeat"]
    assert m[1] == 2 and not matches([m]) and m[3].blocks[0]["dist_lengths"] == [1] and m[3].blocks[0]["hlit"] == 257
    (m,) = members["fib_tail"]
    b = m[3].blocks[0]
    assert m[1] == 2 and matches([m]) and max(b["lit_lengths"]) <= 15 and max(b["dist_lengths"]) <= 15


def test_every_symbol_within_reach(members):
    (m,) = members["every_symbol"]
    ms = matches([m])
    want = every_symbol()[1]
    assert len(set(want) & {(t[1], t[2]) for t in ms}) >= 20                  # found as planted, where no neighbour got in the way
    assert {dm.length_symbol(t[1]) for t in ms} == set(range(258, 286))       # 257 stands for a length of 3: below the matcher's 4
    assert {dm.distance_symbol(t[2]) for t in ms} == set(range(30))
    b = m[3].blocks[0]
    assert b["hlit"] == 286 and b["hdist"] == 30


def test_bytes_equal_the_restated_kernel(cases, outputs):
    for k, data in cases.items():
        if len(data) <= 8192 or k in ("every_symbol", "fib_tail", "size_%d" % (P + 1)):
            assert outputs[k] == lzm.compress(data), k


def test_determinism(ix, cases, outputs):
    for k in ("size_%d" % (2 * P + 17), "every_symbol", "fib_tail"):
        for _ in range(2):
            assert ix.bgzf_compress(cases[k], level=1, lz77=True) == outputs[k], k
    big = text(5 * P + 100, seed=8)                                          # a larger input in between: the token areas are used again
    z = ix.bgzf_compress(big, level=1, lz77=True)
    assert b"".join(m[0] for m in read_members(z)) == big
    for k in ("size_%d" % P, "period_300_full", "n1"):
        assert ix.bgzf_compress(cases[k], level=1, lz77=True) == outputs[k], k


def test_many_payloads_through_a_grid_smaller_than_their_number(ix):
    """more payloads than the device has compute units, so that workgroups take a second and a third payload"""
    unit = text(P, seed=12)
    n = 600
    data = b"".join(struct.pack("<I", i) + unit[4:] for i in range(n))
    z = ix.bgzf_compress(data, level=1, lz77=True)
    first = lzm.member(data[:P])
    ms = bm.parse_bgzf(z)
    assert len(ms) == n and b"".join(p for p, _, _ in ms) == data
    assert z[:len(first)] == first
    assert len({s for _, _, s in ms}) < 40 and all(s < P * 5 // 8 for _, _, s in ms)      # alike but for four bytes; 32 byte values: five bits a byte at most


def test_levels_without_the_flag_are_unchanged(ix, cases, outputs):
    data = cases["size_%d" % (2 * P + 17)]
    z0, z1 = ix.bgzf_compress(data, level=0), ix.bgzf_compress(data, level=1)
    assert [(b, s) for _, b, s in bm.parse_bgzf(z0)] == [(0, P + 31), (0, P + 31), (0, 17 + 31)]
    m1 = bm.parse_bgzf(z1)
    assert [b for _, b, _ in m1] == [2, 2, 0] and b"".join(p for p, _, _ in m1) == data
    for (p, b, s), r in zip(m1[:2], read_members(z1)[:2]):
        assert all(t[0] == "L" for t in r[3].tokens) and r[3].blocks[0]["hlit"] == 257 and r[3].blocks[0]["hdist"] == 1
    mine, ref = sum(s - 26 for _, _, s in m1[:2]), bm.zlib_huffman_only(data[:2 * P])
    assert mine <= 1.01 * ref
    # random text has nothing but short far matches, which cost more than their literals: the matched form falls back to level 1's block
    assert outputs["size_%d" % (2 * P + 17)] == z1 and len(z1) < len(z0)
    for k in ("equal", "fib_tail", "every_symbol", "random", "no_repeat", "len_10", "dist_4097", "n5"):
        assert len(outputs[k]) <= len(ix.bgzf_compress(cases[k], level=1)), k                  # never larger than level 1
    for level in (0x100, 2, 0x102, 0x201):
        with pytest.raises(g.GnumapError) as e:
            ix.bgzf_compress(data, level=level)
        assert e.value.code == -1
    want = outputs["size_%d" % P]
    with pytest.raises(g.GnumapError) as e:
        ix.bgzf_compress(cases["size_%d" % P], level=1, lz77=True, cap=len(want) - 1)
    assert e.value.code == api.GM_E_CAPACITY and e.value.needed == len(want)
    assert ix.bgzf_compress(cases["size_%d" % P], level=1, lz77=True, cap=len(want)) == want


# ---- records -----------------------------------------------------------------------------------------------------------------------
def deflate_sizes(raw):
    """zlib's Z_HUFFMAN_ONLY and level 1 raw deflate of raw's payloads of 65280 bytes"""
    z1 = 0
    for at in range(0, len(raw), P):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z1 += len(c.compress(raw[at:at + P]) + c.flush())
    return bm.zlib_huffman_only(raw), z1


def test_output_bam_with_matches(abi):
    ix, p = abi["ix"], abi["p"]
    for k in (0, 2):
        (names, _, _), (B, Q, Ln), batch = abi["blocks"][k], abi["packed"][k], abi["batches"][k]
        plain = batch.output_bam(p, batch.map(p, B, Q, Ln), names, level=1)
        stats = batch.bam_raw_len, batch.bam_n_recs
        out = batch.output_bam(p, batch.map(p, B, Q, Ln), names, level=1, lz77=True)
        assert (batch.bam_raw_len, batch.bam_n_recs) == stats
        ms = read_members(out)
        raw = b"".join(m[0] for m in ms)
        assert raw == bm.bgzf_payload(plain) and len(out) < len(plain) and matches(ms)
        check_records(bm.split_records(raw), abi["want"][k])
        huff, z1 = deflate_sizes(raw)
        mine = sum(m[2] - 26 for m in ms)
        print(f"block {k}: {len(raw)} bytes of records: device {mine}, zlib Z_HUFFMAN_ONLY {huff}, zlib -1 {z1}")
        assert mine <= (huff + z1) / 2                                       # at least half of what zlib -1 gains over Huffman alone
        assert out == lzm.compress(raw)


def test_resident_form_with_matches(abi, syn_fq):
    ix, p = abi["ix"], abi["p"]
    lines = open(syn_fq, "rb").read().splitlines(keepends=True)
    batch = g.Batch(ix, 64, 2048)
    assert batch.upload_text(p, b"".join(lines[:4 * 64]), want_recs=False)["n"] == 64
    plain = batch.output_bam_resident(p, batch.map_text(p), level=1)
    stats = batch.bam_raw_len, batch.bam_n_recs
    out = batch.output_bam_resident(p, batch.map_text(p), level=1, lz77=True)
    assert (batch.bam_raw_len, batch.bam_n_recs) == stats and len(out) < len(plain)
    ms = read_members(out)
    assert b"".join(m[0] for m in ms) == bm.bgzf_payload(plain) and matches(ms)
    batch.destroy()


def test_level_word_and_capacity_at_the_abi(abi):
    ix, p = abi["ix"], abi["p"]
    (names, _, _), (B, Q, Ln), batch = abi["blocks"][0], abi["packed"][0], abi["batches"][0]
    once = batch.output_bam(p, batch.map(p, B, Q, Ln), names, lz77=True)
    L = g.lib()
    res = batch.map(p, B, Q, Ln)
    rt, keep = api._pack_read_text(names, None, 64)
    buf = np.full(len(once) + 16, 0xAA, np.uint8)
    bo = api.gm_bam_out(); bo.data = buf.ctypes.data; bo.cap = len(once) + 16; bo.level = api.GM_BGZF_LZ77
    call = lambda: L.gm_output_batch_bam(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(bo), None)
    ix.coverage_reset(8)
    assert call() == -1 and "GM_BGZF_LZ77" in L.gm_last_error().decode()      # 0 | GM_BGZF_LZ77
    assert (buf == 0xAA).all() and float(ix.coverage_download().sum()) == 0.0    # nothing written, nothing deposited
    bo.level = 1 | api.GM_BGZF_LZ77; bo.cap = len(once) - 1
    assert call() == api.GM_E_CAPACITY
    assert bo.cap == len(once) and bo.len == 0 and (buf == 0xAA).all() and float(ix.coverage_download().sum()) == 0.0
    assert call() == 0
    assert bytes(buf[:bo.len]) == once and (buf[bo.len:] == 0xAA).all() and float(ix.coverage_download().sum()) > 0
    del keep


# ---- sorter and index --------------------------------------------------------------------------------------------------------------
def test_sorter_read_bgzf_with_matches(abi):
    want = sorted_model(abi)
    runs = {}
    for lz in (False, True):
        s = bam_sorter(abi)
        s.finish()
        runs[lz] = []
        while True:
            t = s.read_bgzf(70000, level=1, lz77=lz)
            if not t:
                break
            ms = read_members(t) if lz else [(pl,) for pl, _, _ in bm.parse_bgzf(t)]      # whole members
            raw = b"".join(m[0] for m in ms)
            assert len(t) <= 70000 and sum(len(x) for x in bm.split_records(raw)) == len(raw)
            runs[lz].append((raw, len(t)))
        s.destroy()
    assert len(runs[True]) >= 3 and [r for r, _ in runs[True]] == [r for r, _ in runs[False]]
    assert sum(n for _, n in runs[True]) < sum(n for _, n in runs[False])
    check_records(bm.split_records(b"".join(r for r, _ in runs[True])), want)


def test_index_of_the_smaller_file(abi):
    ix = abi["ix"]
    s = bam_sorter(abi)
    s.finish()
    head = ix.bgzf_compress(ix.bam_header(b"@HD\tVN:1.0\tSO:coordinate\n"), level=1, lz77=True)
    s.index_begin(len(head))
    slabs = [s.read_bgzf(70000, level=1, lz77=True)]
    with pytest.raises(g.GnumapError) as e:
        s.read_bgzf(70000, level=1)                                          # one indexed file, one level word
    assert e.value.code == -1 and "one level" in str(e.value)
    while slabs[-1]:
        slabs.append(s.read_bgzf(70000, level=1, lz77=True))
    assert len(slabs) > 3
    data = head + b"".join(slabs) + api.bgzf_eof()
    read_members(data[:-28])
    got = s.bai()
    assert got == bai.build_bai(data)
    assert bai.check_queries(data, got, bai.regions_of(data, n_random=50)) > 100
    s.destroy()


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def bam_parts(path):
    data = open(path, "rb").read()
    assert data.endswith(bm.EOF)
    ms = read_members(data[:-28])
    payload = b"".join(m[0] for m in ms)
    head, refs, at = bm.parse_header(payload)
    return data, ms, head, payload[at:]


@pytest.mark.parametrize("extra", [[], SORTED], ids=["input_order", "sorted_and_indexed"])
def test_cli_bam_lz77(extra, syn_fa, syn_fq, tmp_path):
    out = str(tmp_path / "o")
    drive(syn_fa, syn_fq, out, ["--sam_format=bam"] + extra)
    plain = bam_parts(out + ".bam")
    os.remove(out + ".bam")
    drive(syn_fa, syn_fq, out, ["--sam_format=bam", "--bam_lz77"] + extra)
    data, ms, head, recs = bam_parts(out + ".bam")
    assert recs == plain[3] and len(bm.split_records(recs)) > 100
    assert no_pg(head) == no_pg(plain[2]) and b"--bam_lz77" in head and b"--bam_lz77" not in plain[2]
    assert len(data) < len(plain[0]) and matches(ms)
    huff, z1 = deflate_sizes(recs)
    print(f"{len(recs)} bytes of records: file {len(data)} bytes against {len(plain[0])}; zlib Z_HUFFMAN_ONLY {huff}, zlib -1 {z1}")
    if extra:
        os.remove(out + ".bam")
        drive(syn_fa, syn_fq, out, ["--sam_format=bam", "--bam_lz77", "--bam_index"] + extra)
        assert sorted(f for f in os.listdir(tmp_path) if not f.endswith(".sgr")) == ["o.bam", "o.bam.bai"]
        again, index = open(out + ".bam", "rb").read(), open(out + ".bam.bai", "rb").read()
        assert again == data                                                 # byte for byte the file of the run without --bam_index
        assert index == bai.build_bai(data)
        assert bai.check_queries(data, index, bai.regions_of(data, n_random=50)) > 100
