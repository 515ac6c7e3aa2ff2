"""A restatement of the rule by which the driver cuts a byte range of FASTQ text into reads (FastqScanner::parse_range of
gnumap_main.cpp, chunk mode), and of what the host then packs for gm_reads / gm_read_text (pack_block).  gm_batch_upload_text has
to reproduce it on the device.  This is a model, not the authority: the driver comparisons of test_gpu_read_text.py pin it to
parse_range through the reference program's outputs.

    lines    a line starts at 0 and at every i + 1 with text[i] == '\\n' and i + 1 < len(text); it runs to the next '\\n' or to the
             end.  No other byte is special.
    records  in order; empty lines are skipped before a name line only; the next three lines are sequence, plus and quality
    good     four lines, name starts with '@', plus is non-empty and starts with '+', len(sequence) <= len(quality)
    the first record that is not good (MALFORMED), or is good with more than 2048 bases (TOO_LONG), ends the block
"""
import numpy as np

OK, MALFORMED, TOO_LONG = 0, 1, 2
MAX_NAME = 1023          # MAX_NAME_SZ - 1
MAX_READ = 2048

REC_DTYPE = np.dtype([("name_off", "<u4"), ("seq_off", "<u4"), ("qual_off", "<u4"), ("name_len", "<u4"), ("seq_len", "<u4"), ("qual_len", "<u4")])


def lines_of(text):
    """[(offset, length)] of every line of `text`"""
    out, at, n = [], 0, len(text)
    while at < n:
        e = text.find(b"\n", at)
        if e < 0:
            out.append((at, n - at)); break
        out.append((at, e - at)); at = e + 1
    return out


def parse(text):
    """dict(n, max_len, stride, status, bad_at, recs[n] REC_DTYPE): the block the text gives"""
    text = bytes(text)
    ls = lines_of(text)
    recs, k, status, bad_at = [], 0, OK, 0
    while True:
        while k < len(ls) and ls[k][1] == 0:
            k += 1
        if k >= len(ls):
            break
        four = ls[k:k + 4]
        name = four[0]
        good = len(four) == 4 and text[name[0]:name[0] + 1] == b"@" and four[2][1] > 0 and text[four[2][0]:four[2][0] + 1] == b"+" and four[1][1] <= four[3][1]
        if not good:
            status, bad_at = MALFORMED, name[0]; break
        if four[1][1] > MAX_READ:
            status, bad_at = TOO_LONG, name[0]; break
        recs.append((name[0] + 1, four[1][0], four[3][0], name[1] - 1, four[1][1], four[3][1]))
        k += 4
    r = np.array(recs, REC_DTYPE) if recs else np.zeros(0, REC_DTYPE)
    max_len = int(r["seq_len"].max()) if len(r) else 0
    return dict(n=len(r), max_len=max_len, stride=max(8, (max_len + 7) & ~7), status=status, bad_at=bad_at, recs=r)


def rows(text, recs, stride):
    """(bases[n, stride], quals[n, stride], len[n]) as pack_block lays them out: zero padded, the first len quality bytes"""
    n = len(recs)
    B = np.zeros((n, stride), np.uint8); Q = np.zeros((n, stride), np.uint8); Ln = np.zeros(n, np.uint16)
    t = np.frombuffer(bytes(text), np.uint8)
    for i, r in enumerate(recs):
        L = int(r["seq_len"])
        B[i, :L] = t[int(r["seq_off"]):int(r["seq_off"]) + L]
        Q[i, :L] = t[int(r["qual_off"]):int(r["qual_off"]) + L]
        Ln[i] = L
    return B, Q, Ln


def names(text, recs):
    """what a SAM row prints of every name: the bytes behind '@', cut to 1023"""
    text = bytes(text)
    return [text[int(r["name_off"]):int(r["name_off"]) + min(int(r["name_len"]), MAX_NAME)] for r in recs]


def qual_tails(text, recs):
    """the quality bytes beyond the sequence's length"""
    text = bytes(text)
    return [text[int(r["qual_off"]) + int(r["seq_len"]):int(r["qual_off"]) + int(r["qual_len"])] for r in recs]


def illumina_until(Q, kept):
    """the smallest read with a quality byte below 64 as a signed char within its kept length; n when there is none"""
    for i in range(len(kept)):
        if (Q[i, :int(kept[i])].view(np.int8) < 64).any():
            return i
    return len(kept)


def model(text):
    """everything at once: parse() plus rows, names and tails"""
    m = parse(text)
    m["bases"], m["quals"], m["len"] = rows(text, m["recs"], m["stride"])
    m["names"] = names(text, m["recs"]); m["tails"] = qual_tails(text, m["recs"])
    return m


def fastq(records, end=b"\n", last_newline=True):
    """text of (name, seq, qual) or (name, seq, plus, qual) records; name without '@'"""
    out = []
    for r in records:
        name, seq, plus, qual = (r[0], r[1], b"+", r[2]) if len(r) == 3 else r
        out += [b"@" + name, seq, plus, qual]
    t = end.join(out) + (end if out else b"")
    return t if last_newline or not out else t[:-len(end)]
