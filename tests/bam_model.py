"""A BAM / BGZF reader and the rules of the device encoder in plain Python (struct + zlib): what tests/test_bam_cpu.py,
tests/test_gpu_bgzf.py and tests/test_gpu_bam.py compare gm_bam.hip against.

parse_bgzf           walks the gzip members by hand (SAMv1 section 4.1): magic, the BC subfield, BSIZE, raw inflate up to the trailer, CRC-32, ISIZE
sam_to_bam_records   SAM rows -> the BAM records (SAMv1 section 4.2) the device writes for them
header_bytes         the uncompressed start of a BAM file
reg2bin              SAMv1 section 5.3
huffman_lengths      an unlimited Huffman code's lengths (for the test that the device's length limit has to act)
"""
import heapq
import re
import struct
import zlib

PAYLOAD = 65280
EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
NIBBLES = "=ACMGRSVTWYHKDBN"


def parse_bgzf(data):
    """[(payload, BTYPE of its first deflate block, member size)] of every member; asserts on anything the format forbids"""
    out = []
    at = 0
    while at < len(data):
        assert len(data) - at >= 28, f"{len(data) - at} stray bytes at {at}"
        magic = data[at:at + 4]
        assert magic == b"\x1f\x8b\x08\x04", f"bad magic {magic!r} at {at}"
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        assert xlen == 6 and data[at + 12:at + 16] == b"BC\x02\x00", f"no BC subfield at {at}"
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert bsize <= 65536 and at + bsize <= len(data), f"BSIZE {bsize} at {at}"
        body = data[at + 18:at + bsize - 8]
        d = zlib.decompressobj(-15)
        payload = d.decompress(body)
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", f"the deflate stream does not end at the trailer (member at {at})"
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        assert isize == len(payload) and isize <= PAYLOAD, f"ISIZE {isize} for {len(payload)} bytes"
        assert crc == zlib.crc32(payload), f"CRC-32 of the member at {at}"
        btype = (body[0] >> 1) & 3
        assert body[0] & 1 or btype == 0
        out.append((payload, btype, bsize))
        at += bsize
    return out


def bgzf_payload(data):
    return b"".join(p for p, _, _ in parse_bgzf(data))


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def header_bytes(text, contigs):
    """text: the SAM header lines (bytes); contigs: [(name, length)]"""
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contigs))
    for name, ln in contigs:
        nm = name.encode() if isinstance(name, str) else name
        out += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", ln)
    return out


def parse_header(payload):
    """(header text, [(name, length)], offset of the first record)"""
    assert payload[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", payload, 4)[0]
    text = payload[8:8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", payload, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", payload, at)[0]
        name = payload[at + 4:at + 4 + ln]
        assert name.endswith(b"\0")
        refs.append((name[:-1].decode(), struct.unpack_from("<i", payload, at + 4 + ln)[0]))
        at += 8 + ln
    return text, refs, at


_CIGAR = re.compile(rb"(\d+)([MIDNSHP=X])")


def sam_row_to_record(row, contigs):
    """one SAM row (bytes, with or without its newline) -> the record; XA / XP are encoded from the printed field's value"""
    f = row.rstrip(b"\n").split(b"\t")
    name, flag, rname, pos, mapq, cigar, seq, qual = f[0], int(f[1]), f[2].decode(), int(f[3]) - 1, int(f[4]), f[5], f[9], f[10]
    names = [c[0] for c in contigs]
    ops = [(int(n), b"MIDNSHP=X".index(o)) for n, o in _CIGAR.findall(cigar)]
    ref_len = sum(n for n, o in ops if o in (0, 2, 3, 7, 8)) or 1
    name = name[:254] + b"\0"
    l_seq = len(seq)
    nib = [NIBBLES.index(chr(c).upper()) if chr(c).upper() in NIBBLES else 15 for c in seq]
    if l_seq & 1:
        nib.append(0)
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))
    q = bytes(max(c - 33, 0) for c in qual[:l_seq])
    assert len(q) == l_seq
    body = struct.pack("<iiBBHHHiiii", names.index(rname), pos, len(name), min(max(mapq, 0), 255), reg2bin(pos, pos + ref_len), len(ops), flag, l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + packed + q
    for tag in f[11:]:
        k, t, v = tag.split(b":", 2)
        body += k + (b"f" + struct.pack("<f", float(v)) if t == b"f" else b"i" + struct.pack("<i", int(v)))
    return struct.pack("<i", len(body)) + body


def sam_to_bam_records(sam_text, contigs):
    """the records of every row of sam_text (header lines skipped), as a list of bytes"""
    return [sam_row_to_record(l, contigs) for l in sam_text.splitlines() if l and not l.startswith(b"@")]


def split_records(raw):
    out, at = [], 0
    while at < len(raw):
        n = struct.unpack_from("<i", raw, at)[0]
        assert n >= 32 and at + 4 + n <= len(raw), f"record of {n} bytes at {at} of {len(raw)}"
        out.append(raw[at:at + 4 + n])
        at += 4 + n
    return out


def float_tag_offsets(rec):
    """offsets in a record of the 4 value bytes of XA and XP (the first two tags)"""
    l_name, n_ops, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    at = 36 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq
    assert rec[at:at + 3] == b"XAf" and rec[at + 7:at + 10] == b"XPf" and rec[at + 14:at + 17] == b"X0i" and at + 21 == len(rec)
    return at + 3, at + 10


def records_equal(got, want, rel=5.1e-6):
    """byte for byte, except the 4 bytes of XA and XP: those by value against the model's (which come from the printed "%g" field).
    Returns None, or a description of the first difference"""
    if len(got) != len(want):
        return f"{len(got)} records, the model has {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        if len(a) != len(b):
            return f"record {i}: {len(a)} bytes, the model has {len(b)}"
        xa, xp = float_tag_offsets(b)
        mask = bytearray(a)
        for o in (xa, xp):
            v, t = struct.unpack_from("<f", a, o)[0], struct.unpack_from("<f", b, o)[0]
            if not abs(v - t) <= rel * abs(t):
                return f"record {i}: float tag at {o} is {v!r}, the row prints {t!r}"
            mask[o:o + 4] = b[o:o + 4]
        if bytes(mask) != b:
            at = next(k for k in range(len(b)) if mask[k] != b[k])
            return f"record {i} differs at byte {at}: {bytes(mask[max(0, at - 8):at + 8])!r} vs {b[max(0, at - 8):at + 8]!r}"
    return None


def huffman_lengths(counts):
    """code lengths of an unlimited Huffman code over the symbols with a count above 0: {symbol: length}"""
    heap = [(c, s, (s,)) for s, c in enumerate(counts) if c]
    heapq.heapify(heap)
    depth = {s: 0 for _, s, _ in heap}
    tick = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return depth


def zlib_huffman_only(data):
    """total bytes of zlib's Z_HUFFMAN_ONLY raw deflate of data's payloads of 65280 bytes"""
    total = 0
    for at in range(0, len(data), PAYLOAD):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        total += len(c.compress(data[at:at + PAYLOAD]) + c.flush())
    return total
