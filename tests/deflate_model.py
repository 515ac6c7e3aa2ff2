"""A small inflate for raw deflate streams (RFC 1951: stored, fixed and dynamic blocks) in plain Python that keeps what zlib throws away:
the tokens.  tests/test_bgzf_lz77_cpu.py holds it against zlib's own output, tests/test_gpu_bgzf_lz77.py reads the device's blocks
with it.

inflate(data) -> Inflated: .out the bytes, .tokens [('L', byte) | ('M', length, distance)] over all blocks, .blocks one dict per block
(btype; for a dynamic block hlit, hdist, lit_lengths, dist_lengths), .used the bytes of `data` the stream takes.

It asserts on everything the RFC forbids: a distance beyond the bytes produced so far, length symbols 286 / 287, distance symbols
30 / 31, an over-subscribed or incomplete code (other than the single one-bit distance code, section 3.2.7), a block without an
end-of-block code, a stored block whose NLEN is not the complement of LEN, block type 3, a stream that ends early.
"""
from collections import namedtuple

Inflated = namedtuple("Inflated", "out tokens blocks used")

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_symbol(length):
    """the length symbol (257 .. 285) of a match length 3 .. 258"""
    assert 3 <= length <= 258
    return 257 + max(i for i, b in enumerate(LEN_BASE) if b <= length)


def distance_symbol(distance):
    assert 1 <= distance <= 32768
    return max(i for i, b in enumerate(DIST_BASE) if b <= distance)


class _Bits:
    def __init__(self, data):
        self.data, self.at = data, 0                     # at: in bits

    def take(self, n):
        v = 0
        for k in range(n):
            assert self.at < 8 * len(self.data), "the stream ends inside a block"
            v |= ((self.data[self.at >> 3] >> (self.at & 7)) & 1) << k
            self.at += 1
        return v


def _decoder(lengths, what, one_bit_code_allowed=False):
    """{(length, code): symbol} of the canonical code (section 3.2.2); asserts that the code is complete"""
    used = [l for l in lengths if l]
    assert used, f"{what}: no code at all"
    assert max(used) <= 15
    space = sum(1 << (15 - l) for l in used)
    assert space <= 1 << 15, f"{what}: over-subscribed code"
    if space < 1 << 15:
        assert one_bit_code_allowed and used == [1], f"{what}: incomplete code {sorted(used)}"
    count = [0] * 16
    for l in used:
        count[l] += 1
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


def _symbol(bits, table, what):
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.take(1)                  # Huffman codes arrive most significant bit first
        if (l, code) in table:
            return table[(l, code)]
    raise AssertionError(f"{what}: a code of no symbol")


def inflate(data):
    bits = _Bits(bytes(data))
    out, tokens, blocks = bytearray(), [], []
    while True:
        final, btype = bits.take(1), bits.take(2)
        assert btype != 3, "block type 3"
        block = dict(btype=btype)
        if btype == 0:
            bits.at = (bits.at + 7) & ~7
            ln, nln = bits.take(16), bits.take(16)
            assert ln ^ nln == 0xFFFF, "stored block: NLEN is not the complement of LEN"
            at = bits.at >> 3
            assert at + ln <= len(bits.data), "the stream ends inside a stored block"
            out += bits.data[at:at + ln]
            tokens += [("L", b) for b in bits.data[at:at + ln]]
            bits.at += 8 * ln
        else:
            if btype == 1:
                lit = _decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, "fixed literal/length code")
                dist = _decoder([5] * 32, "fixed distance code")
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                assert hlit <= 286, f"HLIT {hlit}"
                assert hdist <= 30, f"HDIST {hdist}"
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits.take(3)
                cl_table = _decoder(cl, "code-length code")
                lengths = []
                while len(lengths) < hlit + hdist:
                    s = _symbol(bits, cl_table, "code-length code")
                    if s < 16:
                        lengths.append(s)
                    elif s == 16:
                        assert lengths, "repeat with no length before it"
                        lengths += [lengths[-1]] * (3 + bits.take(2))
                    else:
                        lengths += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
                assert len(lengths) == hlit + hdist, "a repeat runs past HLIT + HDIST"
                ll, dl = lengths[:hlit], lengths[hlit:]
                assert ll[256], "no end-of-block code"
                lit = _decoder(ll, "literal/length code")
                dist = _decoder(dl, "distance code", one_bit_code_allowed=True) if any(dl) else {}
                block.update(hlit=hlit, hdist=hdist, lit_lengths=ll, dist_lengths=dl)
            while True:
                s = _symbol(bits, lit, "literal/length code")
                if s < 256:
                    out.append(s); tokens.append(("L", s))
                elif s == 256:
                    break
                else:
                    assert s <= 285, f"length symbol {s}"
                    length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                    assert dist, "a match in a block with no distance code"
                    d = _symbol(bits, dist, "distance code")
                    assert d <= 29, f"distance symbol {d}"
                    distance = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                    assert distance <= len(out), f"distance {distance} with {len(out)} bytes produced"
                    for _ in range(length):
                        out.append(out[-distance])
                    tokens.append(("M", length, distance))
        blocks.append(block)
        if final:
            break
    return Inflated(bytes(out), tokens, blocks, (bits.at + 7) >> 3)


def expand(tokens):
    """the bytes a token list stands for"""
    out = bytearray()
    for t in tokens:
        if t[0] == "L":
            out.append(t[1])
        else:
            assert 3 <= t[1] <= 258 and 1 <= t[2] <= min(32768, len(out)), t
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)
