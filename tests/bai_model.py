"""The .bai of a coordinate-sorted BAM in plain Python: the rules gm_bai.hip follows where SAMv1 section 5.2 leaves a choice, applied
literally to the bytes of a BAM file, and the specification's reader.  tests/test_bai_cpu.py checks it against an index written out by
hand; tests/test_gpu_bai.py compares the device's bytes with build_bai.

scan                 the records of a BAM file with the virtual offsets of their first byte and of the byte behind them
build_bai            the index file
parse_bai            its structure
reg2bins, query      SAMv1 section 5.3: the bins a region may lie in; the chunks a reader has to visit for it
records_in_chunks    the records a reader reaches by seeking to each chunk's start and reading up to its end
overlapping          brute force: the records that overlap a region

The rules:
  * a record starts at the virtual offset (coffset << 16 | uoffset) of its block_size field and ends at that of the byte behind it; when
    that byte opens the next block the end is (that block's coffset, 0), and behind the last record it is (the coffset of whatever
    follows the last block with data, 0);
  * refID, pos, flag and the CIGAR come from the record: beg = pos, end = pos + the CIGAR's reference length (M D N = X), pos + 1 when
    that is 0; bin = reg2bin(beg, end); an end above 2^29 is refused;
  * in file order a maximal run of consecutive records of one (refID, bin) is a chunk; two chunks of a bin are merged when the later
    starts in the compressed block in which the earlier ends, or before; bins ascend; bins without records are not written;
  * the pseudo-bin 37450 comes last for every reference with records: (first start, last end), (records with flag 0x4 clear, set);
  * n_intv = ((max end - 1) >> 14) + 1; entry w = the smallest start of the records that overlap window w; a window without a record
    takes the entry before it; leading empty windows hold 0;
  * n_no_coor = the records with refID < 0."""
import bisect
import functools
import struct

import numpy as np

import bam_model as bm

MAX_END = 1 << 29
PSEUDO_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)                       # M D N = X


@functools.lru_cache(maxsize=16)
def scan(bam):
    """dict: recs (the records' bytes), vbeg / vend (their virtual offsets), ref, pos, end, flag, n_ref"""
    blocks, at, u = [], 0, 0                     # (coffset, first uncompressed byte, bytes) of the members with data
    after = 0                                    # the coffset behind the last of them
    payload = []
    for pl, _, bsize in bm.parse_bgzf(bam):
        if pl:
            blocks.append((at, u, len(pl)))
            payload.append(pl)
            u += len(pl)
            after = at + bsize
        at += bsize
    payload = b"".join(payload)
    ends = [b[1] + b[2] for b in blocks]

    def locate(p):                               # the byte p of the payload: the first block that holds it
        k = bisect.bisect_right(ends, p)
        return after << 16 if k == len(blocks) else blocks[k][0] << 16 | (p - blocks[k][1])

    _, refs, p = bm.parse_header(payload)
    out = dict(recs=[], vbeg=[], vend=[], ref=[], pos=[], end=[], flag=[], n_ref=len(refs))
    for rec in bm.split_records(payload[p:]):
        ref, pos, l_name, _, _, n_ops, flag = struct.unpack_from("<iiBBHHH", rec, 4)
        ops = struct.unpack_from(f"<{n_ops}I", rec, 36 + l_name)
        ref_len = sum(w >> 4 for w in ops if w & 15 in REF_OPS)
        out["recs"].append(rec); out["vbeg"].append(locate(p)); out["vend"].append(locate(p + len(rec)))
        out["ref"].append(ref); out["pos"].append(pos); out["end"].append(pos + (ref_len or 1)); out["flag"].append(flag)
        p += len(rec)
    for k in ("vbeg", "vend", "ref", "pos", "end", "flag"):
        out[k] = np.array(out[k], np.int64)
    return out


def build_bai(bam, n_ref=None):
    s = scan(bam)
    n_ref = s["n_ref"] if n_ref is None else n_ref
    n = len(s["recs"])
    bins = [dict() for _ in range(n_ref)]        # bin -> [[beg, end]] in file order
    lin = [dict() for _ in range(n_ref)]
    first, last, mapped, unmapped, max_end = [None] * n_ref, [None] * n_ref, [0] * n_ref, [0] * n_ref, [0] * n_ref
    n_no_coor, run, prev = 0, None, None
    for i in range(n):
        ref, pos, end, vbeg, vend = (int(s[k][i]) for k in ("ref", "pos", "end", "vbeg", "vend"))
        key = (ref & 0xFFFFFFFF, pos)
        if prev is not None and (key[0] < prev[0] or (key[0] == prev[0] and ref >= 0 and key[1] < prev[1])):
            raise ValueError(f"record {i} is not in coordinate order")
        prev = key
        if ref < 0:
            n_no_coor += 1; run = None
            continue
        if ref >= n_ref:
            raise ValueError(f"record {i} names reference {ref} of {n_ref}")
        if pos < 0 or end > MAX_END:
            raise ValueError(f"record {i} at {pos} ends at {end}: beyond 2^29")
        b = bm.reg2bin(pos, end)
        if run == (ref, b):
            bins[ref][b][-1][1] = vend
        else:
            bins[ref].setdefault(b, []).append([vbeg, vend]); run = (ref, b)
        if first[ref] is None:
            first[ref] = vbeg
        last[ref] = vend
        if s["flag"][i] & 4:
            unmapped[ref] += 1
        else:
            mapped[ref] += 1
        max_end[ref] = max(max_end[ref], end)
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            lin[ref][w] = min(lin[ref].get(w, vbeg), vbeg)
    out = [b"BAI\x01", struct.pack("<i", n_ref)]
    for r in range(n_ref):
        if first[r] is None:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(bins[r]) + 1))
        for b in sorted(bins[r]):
            chunks = []
            for c in bins[r][b]:
                if chunks and chunks[-1][1] >> 16 >= c[0] >> 16:
                    chunks[-1][1] = c[1]
                else:
                    chunks.append(list(c))
            out.append(struct.pack("<Ii", b, len(chunks)) + b"".join(struct.pack("<QQ", *c) for c in chunks))
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, first[r], last[r], mapped[r], unmapped[r]))
        n_intv = ((max_end[r] - 1) >> 14) + 1
        entries, cur = [], 0
        for w in range(n_intv):
            cur = lin[r].get(w, cur)
            entries.append(cur)
        out.append(struct.pack("<i", n_intv) + struct.pack(f"<{n_intv}Q", *entries))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def parse_bai(data):
    """dict: refs = [dict(bins = {bin: [(beg, end)]} in file order, pseudo = None | (beg, end, mapped, unmapped), lin = [entries])], n_no_coor"""
    assert data[:4] == b"BAI\x01"
    n_ref = struct.unpack_from("<i", data, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, at)[0]; at += 4
        bins, pseudo, order = {}, None, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at); at += 8
            chunks = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]; at += 16 * n_chunk
            assert b not in bins and n_chunk > 0
            order.append(b)
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and pseudo is None
                pseudo = chunks[0] + chunks[1]
            else:
                bins[b] = chunks
        n_intv = struct.unpack_from("<i", data, at)[0]; at += 4
        lin = list(struct.unpack_from(f"<{n_intv}Q", data, at)); at += 8 * n_intv
        refs.append(dict(bins=bins, pseudo=pseudo, lin=lin, order=order))
    n_no_coor = struct.unpack_from("<Q", data, at)[0]; at += 8
    assert at == len(data), f"{len(data) - at} stray bytes"
    return dict(refs=refs, n_no_coor=n_no_coor)


def reg2bins(beg, end):
    """SAMv1 section 5.3"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def query(bai, ref, beg, end):
    """the chunks a reader visits for [beg, end) of reference ref: those of the region's bins that end behind the linear index's entry for beg >> 14"""
    r = bai["refs"][ref]
    lin = r["lin"]
    low = 0 if not lin else lin[min(beg >> 14, len(lin) - 1)]
    return sorted(c for b in reg2bins(beg, end) for c in r["bins"].get(b, ()) if c[1] > low)


def records_in_chunks(bam, chunks):
    """the ordinals of the records a reader meets: it seeks to a chunk's start, which has to be a record's, and reads records while its position is in front of the chunk's end"""
    s = scan(bam)
    starts = s["vbeg"]
    hit = set()
    for beg, end in chunks:
        a = int(np.searchsorted(starts, beg))
        assert a < len(starts) and starts[a] == beg, f"chunk start {beg >> 16}:{beg & 0xFFFF} is no record's"
        hit.update(range(a, int(np.searchsorted(starts, end))))
    return hit


def overlapping(bam, ref, beg, end):
    s = scan(bam)
    return set(np.nonzero((s["ref"] == ref) & (s["pos"] < end) & (s["end"] > beg))[0].tolist())


def check_queries(bam, bai_bytes, regions):
    """every record that overlaps a region is among those its chunks reach; returns the number of (region, record) pairs seen"""
    bai = parse_bai(bai_bytes)
    seen = 0
    for ref, beg, end in regions:
        want = overlapping(bam, ref, beg, end)
        got = records_in_chunks(bam, query(bai, ref, beg, end))
        assert want <= got, f"reference {ref} [{beg}, {end}): records {sorted(want - got)[:5]} overlap it and are not reached"
        seen += len(want)
    return seen


def regions_of(bam, seed=5, n_random=200):
    """every window-aligned region of every reference with records, and n_random seeded random ones per reference"""
    s = scan(bam)
    rng = np.random.default_rng(seed)
    out = []
    for ref in range(s["n_ref"]):
        ends = s["end"][s["ref"] == ref]
        if not len(ends):
            out.append((ref, 0, 1 << 14))
            continue
        top = int(ends.max())
        out += [(ref, w << 14, (w + 1) << 14) for w in range(((top - 1) >> 14) + 2)]
        for _ in range(n_random):
            a = int(rng.integers(0, top + 100))
            out.append((ref, a, a + int(rng.choice([1, 50, 20000, 1 << 18, 1 << 27]))))
    return out
