"""k_bgzf_deflate_lz (gm_bam.hip) restated in plain Python: which matches the device finds and the member it writes
for a payload, byte for byte.  tests/test_bgzf_lz77_cpu.py holds its output against zlib and tests/deflate_model.py;
tests/test_gpu_bgzf_lz77.py holds the device's bytes against it.

tokens(payload)  the greedy parse: [byte | (length, distance)].  Tiles of 256 positions; a position's one candidate is the largest
                 position of an EARLIER tile whose 4 bytes have the same hash; a match counts from 4 bytes, within 32768
member(payload)  the BGZF member: one dynamic-Huffman block over the tokens (both codes by Huffman's algorithm on the sorted counts,
                 halved until no code is longer than 15 bits; code lengths sent as 4 bits each), or level 1's block over the bytes
                 where that is not larger, or a stored block where that is not larger
matches=False    (deflate, member, compress) what k_bgzf_deflate writes at level 1: the block over the bytes, or the stored block
"""
import struct
import zlib

import numpy as np

from deflate_model import DIST_EXTRA, LEN_EXTRA, distance_symbol, length_symbol

TILE, HEAD, MIN, MAX, WINDOW, PAYLOAD = 256, 8192, 4, 258, 32768, 65280


def _hashes(d):
    """the hash of the 4 bytes at every position that has 4"""
    a = np.frombuffer(bytes(d), np.uint8).astype(np.uint32)
    if len(a) < MIN:
        return []
    v = a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24
    return ((v * np.uint32(0x9E3779B1)) >> 19).tolist()


def tokens(d):
    n, head, out, start = len(d), [0] * HEAD, [], 0
    hs = _hashes(d)
    for tb in range(0, n, TILE):
        te = min(tb + TILE, n)
        found = {}
        for p in range(max(tb, start), min(te, len(hs))):
            c1 = head[hs[p]]
            if c1 and p - (c1 - 1) <= WINDOW:
                c, l, mx = c1 - 1, 0, min(n - p, MAX)
                while l < mx and d[c + l] == d[p + l]:
                    l += 1
                if l >= MIN:
                    found[p] = (l, p - c)
        for p in range(tb, min(te, len(hs))):
            head[hs[p]] = p + 1                              # (the largest so far: positions ascend)
        p = max(tb, start)
        while p < te:
            if p in found:
                out.append(found[p]); p += found[p][0]
            else:
                out.append(d[p]); p += 1
        start = max(start, p)
    return out


def _code(hist):
    """{symbol: (length, code as sent, first bit lowest)} as bz_build_code makes it"""
    order = sorted((c, s) for s, c in enumerate(hist) if c)
    m = len(order)
    if m == 0:
        return {}
    if m == 1:
        return {order[0][1]: (1, 0)}
    wt = [c for c, _ in order]
    while True:
        w, par = wt + [0] * (m - 1), [0] * (2 * m - 1)
        li, ni, nn = 0, m, m
        while nn < 2 * m - 1:
            pick = []
            for _ in range(2):
                if li < m and (ni >= nn or w[li] <= w[ni]):
                    pick.append(li); li += 1
                else:
                    pick.append(ni); ni += 1
            w[nn] = w[pick[0]] + w[pick[1]]
            par[pick[0]] = par[pick[1]] = nn
            nn += 1
        dep = [0] * (2 * m - 1)
        for i in range(2 * m - 3, -1, -1):
            dep[i] = dep[par[i]] + 1
        if max(dep[:m]) <= 15:
            break
        wt = [(x + 1) >> 1 for x in wt]
    length = {s: dep[i] for i, (_, s) in enumerate(order)}
    count = [0] * 16
    for l in length.values():
        count[l] += 1
    nxt, code = [0] * 16, 0
    for k in range(1, 16):
        code = (code + count[k - 1]) << 1
        nxt[k] = code
    out = {}
    for s in sorted(length):
        l = length[s]
        out[s] = (l, int(format(nxt[l], f"0{l}b")[::-1], 2))
        nxt[l] += 1
    return out


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):
        self.v |= v << self.n; self.n += n

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _header(w, lc, dc):
    nl, nd = max(max(lc) + 1, 257), max(dc) + 1 if dc else 1
    w.put(1, 1); w.put(2, 2); w.put(nl - 257, 5); w.put(nd - 1, 5); w.put(15, 4)
    for k in range(19):
        w.put(0 if k < 3 else 4, 3)
    rev4 = lambda l: int(format(l, "04b")[::-1], 2)
    for s in range(nl):
        w.put(rev4(lc[s][0] if s in lc else 0), 4)
    if dc:
        for s in range(nd):
            w.put(rev4(dc[s][0] if s in dc else 0), 4)
    else:
        w.put(rev4(1), 4)


def deflate(d, matches=True):
    """the raw deflate stream of one payload: the smallest of the matched form, level 1's block over the bytes, and the stored block.
    matches=False: what k_bgzf_deflate writes at level 1 - the block over the bytes, or the stored block where that is not larger"""
    toks = tokens(d) if matches else []
    lh, dh, bh = [0] * 286, [0] * 30, [0] * 257
    lh[256] = bh[256] = 1
    for t in toks:
        if isinstance(t, tuple):
            lh[length_symbol(t[0])] += 1; dh[distance_symbol(t[1])] += 1
        else:
            lh[t] += 1
    for b in d:
        bh[b] += 1
    lc, dc, bc = _code(lh), _code(dh), _code(bh)
    w = _Bits()
    _header(w, lc, dc)
    for t in toks:
        if isinstance(t, tuple):
            s = length_symbol(t[0]); w.put(lc[s][1], lc[s][0]); w.put((t[0] - 3) & ((1 << LEN_EXTRA[s - 257]) - 1), LEN_EXTRA[s - 257])
            s = distance_symbol(t[1]); w.put(dc[s][1], dc[s][0]); w.put((t[1] - 1) & ((1 << DIST_EXTRA[s]) - 1), DIST_EXTRA[s])
        else:
            w.put(lc[t][1], lc[t][0])
    w.put(lc[256][1], lc[256][0])
    plain = _Bits()
    _header(plain, bc, {})
    for b in d:
        plain.put(bc[b][1], bc[b][0])
    plain.put(bc[256][1], bc[256][0])
    if not matches or plain.n <= w.n:                        # ties go to the simpler form
        w = plain
    body = w.bytes()
    if len(body) >= len(d) + 5:
        body = b"\x01" + struct.pack("<HH", len(d), len(d) ^ 0xFFFF) + bytes(d)
    return body


def member(d, matches=True):
    body = deflate(d, matches)
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(d), len(d)))


def compress(data, matches=True):
    return b"".join(member(data[at:at + PAYLOAD], matches) for at in range(0, len(data), PAYLOAD))
