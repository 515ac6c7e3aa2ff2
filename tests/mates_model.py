"""What gm_batch_set_mates / --mates has to write, as a plain Python model (the rule: include/gnumap_hip.h).  The reference program has no
paired mode, so the yardsticks are the project's own mates-off output (pinned byte for byte to the reference elsewhere) and this file:
the rows with the setting on are the mates-off rows with QNAME, FLAG, RNEXT, PNEXT and TLEN replaced by the model's.

Records are anything indexable by "read", "contig", "chr_pos", "strand", "post_prob" (Batch.output's array, or dicts); cigars one bytes per
record; reads 2i and 2i + 1 are the mates of pair i.

span             M + D runs of a CIGAR; 1 where that is 0 ("*")
resolve          records -> (primary of every read: a record index or None, proper of every pair)
row_fields       -> (flag, rnext, pnext, tlen) of every row; rows: None = one per record, or a list of ("r", record) / ("u", read)
stats            -> dict(pairs, both_mapped, proper, one_mapped, none_mapped)
qname / qnames   the QNAME rule
text_row         a mates-off SAM row (of a record, or unmapped_model's flag-4 row) -> the row with mates on
bam_record       the same for a BAM record
"""
import re
import struct

import numpy as np

_TOKEN = re.compile(rb"(\d+)([A-Z=])")
STATS = ("pairs", "both_mapped", "proper", "one_mapped", "none_mapped")


def span(cigar):
    s = sum(int(n) for n, op in _TOKEN.findall(bytes(cigar)) if op in (b"M", b"D"))
    return s if s else 1


def _ranges(recs, n):
    """[first, end) of every read's records: the records lie in read order"""
    reads = [int(r["read"]) for r in recs]
    assert all(a <= b for a, b in zip(reads, reads[1:])) and all(0 <= x < n for x in reads)
    first, end = [0] * n, [0] * n
    for k, rd in enumerate(reads):
        if k == 0 or reads[k - 1] != rd:
            first[rd] = k
        end[rd] = k + 1
    return [range(first[i], end[i]) if end[i] else range(0) for i in range(n)]


def concordant(a, sa, b, sb, lo, hi):
    """a, b: records of the two mates, sa, sb their spans"""
    if int(a["contig"]) != int(b["contig"]) or bool(a["strand"]) == bool(b["strand"]):
        return False
    (f, _), (r, sr) = ((a, sa), (b, sb)) if not a["strand"] else ((b, sb), (a, sa))
    pf, pr = int(f["chr_pos"]), int(r["chr_pos"])
    if pf > pr:
        return False
    return lo <= (pr + sr - 1) - pf + 1 <= hi


def above(x, y):
    """x ranks above y: the larger number, and any number above a NaN; two NaNs rank alike (the header's NaN rule)"""
    return bool(x > y) or bool(x == x and y != y)


def resolve(recs, cigars, n, lo, hi):
    with np.errstate(all="ignore"):                     # (a product of the test cases may underflow, or be inf * 0)
        return _resolve(recs, cigars, n, lo, hi)


def _resolve(recs, cigars, n, lo, hi):
    assert n % 2 == 0 and lo <= hi
    rng = _ranges(recs, n)
    sp = [span(c) for c in cigars]
    post = [np.float32(r["post_prob"]) for r in recs]
    prim, proper = [None] * n, [False] * (n // 2)
    for i in range(n // 2):
        A, B = rng[2 * i], rng[2 * i + 1]
        best, pick = None, None
        for a in A:                                     # ascending (first, second): a strict "above" keeps the first of equals
            for b in B:
                if concordant(recs[a], sp[a], recs[b], sp[b], lo, hi):
                    prod = post[a] * post[b]            # one fp32 multiply
                    if pick is None or above(prod, best):
                        best, pick = prod, (a, b)
        if pick:
            prim[2 * i], prim[2 * i + 1], proper[i] = pick[0], pick[1], True
            continue
        for rd, R in ((2 * i, A), (2 * i + 1, B)):
            for k in R:
                if prim[rd] is None or above(post[k], post[prim[rd]]):
                    prim[rd] = k
    return prim, proper


def row_fields(recs, cigars, n, lo, hi, rows=None, resolved=None):
    """resolved: resolve()'s answer for the same arguments, where the caller has it already"""
    prim, proper = resolved if resolved is not None else resolve(recs, cigars, n, lo, hi)
    sp = [span(c) for c in cigars]
    if rows is None:
        rows = [("r", k) for k in range(len(recs))]
    out = []
    for kind, k in rows:
        rd = int(recs[k]["read"]) if kind == "r" else int(k)
        pm = prim[rd ^ 1]
        flag = 0x1 | (0x80 if rd & 1 else 0x40)
        rnext, pnext, tlen = -1, 0, 0
        if pm is None:
            flag |= 0x8
        else:
            m = recs[pm]
            flag |= 0x20 if m["strand"] else 0
            rnext, pnext = int(m["contig"]), int(m["chr_pos"]) & 0xFFFFFFFF      # gm_mate_row.pnext has 32 bits (no index has a longer POS)
        if kind == "u":
            flag |= 0x4
        else:
            r = recs[k]
            flag |= 0x10 if r["strand"] else 0
            is_prim = prim[rd] == k
            if not is_prim:
                flag |= 0x100
            elif proper[rd >> 1]:
                flag |= 0x2
            if is_prim and pm is not None and int(recs[pm]["contig"]) == int(r["contig"]):
                p0, p1 = int(r["chr_pos"]), int(recs[pm]["chr_pos"])
                v = max(p0 + sp[k] - 1, p1 + sp[pm] - 1) - min(p0, p1) + 1
                if v <= 2 ** 31 - 1:
                    plus = p0 < p1 if p0 != p1 else not (rd & 1)
                    tlen = v if plus else -v
        out.append((flag, rnext, pnext, tlen))
    return out


def stats(recs, cigars, n, lo, hi, resolved=None):
    rng = _ranges(recs, n)
    _, proper = resolved if resolved is not None else resolve(recs, cigars, n, lo, hi)
    have = [len(r) > 0 for r in rng]
    pairs = n // 2
    both = sum(have[2 * i] and have[2 * i + 1] for i in range(pairs))
    none = sum(not have[2 * i] and not have[2 * i + 1] for i in range(pairs))
    return dict(pairs=pairs, both_mapped=both, proper=sum(proper), one_mapped=pairs - both - none, none_mapped=none)


def _cut(name):
    m = re.search(rb"[ \t]", name)
    return name[:m.start()] if m else name


def qnames(a, b):
    """the names of the first and the second mate as the rule leaves them (before the cut to 1023 / 254 bytes)"""
    a, b = _cut(bytes(a)), _cut(bytes(b))
    if a.endswith(b"/1") and b.endswith(b"/2"):
        a, b = a[:-2], b[:-2]
    return a, b


def block_qnames(names):
    out = []
    for i in range(0, len(names), 2):
        out.extend(qnames(names[i], names[i + 1]))
    return out


def first_mismatch(names, cut=1023):
    """index of the first pair whose printed names differ, or None"""
    q = block_qnames(names)
    for i in range(0, len(q), 2):
        if q[i][:cut] != q[i + 1][:cut]:
            return i // 2
    return None


def text_row(row, f, name, contig_names):
    """row: the mates-off row; f: its (flag, rnext, pnext, tlen); name: the read's name after qnames"""
    c = row.split(b"\t")
    flag, rnext, pnext, tlen = f
    c[0] = name[:1023]
    c[1] = b"%d" % flag
    own = c[2]
    rn = b"*" if rnext < 0 else contig_names[rnext].encode() if isinstance(contig_names[rnext], str) else contig_names[rnext]
    c[6] = b"=" if rnext >= 0 and own != b"*" and rn == own else rn
    c[7] = b"%d" % pnext
    c[8] = b"%d" % tlen
    return b"\t".join(c)


def bam_record(rec, f, name):
    """rec: the mates-off BAM record (block_size first); f, name as in text_row"""
    flag, rnext, pnext, tlen = f
    size, ref_id, pos, l_name, mapq, bin_, n_op, _flag, l_seq, _nr, _np, _tl = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    rest = rec[36 + l_name:]
    nm = name[:254] + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(nm), mapq, bin_, n_op, flag, l_seq, rnext, pnext - 1, tlen) + nm + rest
    return struct.pack("<i", len(body)) + body


def bam_fields(rec):
    """(flag, next_refID, next_pos, tlen, name) of a record"""
    l_name = rec[12]
    flag, = struct.unpack_from("<H", rec, 18)
    nr, npos, tl = struct.unpack_from("<iii", rec, 24)
    return flag, nr, npos, tl, rec[36:36 + l_name - 1]
