"""What gm_batch_set_row_tags / --sam_md and gm_batch_set_cigar_order / --sam_cigar have to write, as a plain Python model.

The reference program prints no NM or MD tag, so it cannot be the yardstick.  The yardstick is the project's flag-off rows (pinned
byte for byte to the reference elsewhere) plus this model, and the model is checked by an independent inverse: rebuild_reference.

The rule, for one row AS PRINTED (what `samtools calmd` derives from POS, the CIGAR field, SEQ and the reference).  T is the contig's
text, upper case: the pac letter, or inside a hole of <fa>.gnumap.amb that hole's character.  code() is the BAM nibble of a character.

    x = POS-1; z = 0; u = 0; nm = 0; md = ""
    for every token (n, op) of the CIGAR field as printed, read as k_bam_sizes reads it (n = 0 contributes nothing):
      M: n times: if z >= len(SEQ) or x >= len(contig): the walk ends
                  if code(SEQ[z]) == code(T[x]) and that code != 15: u += 1
                  else: md += str(u) + T[x]; u = 0; nm += 1
                  x += 1; z += 1
      I: z += n; nm += n
      D: md += str(u) + "^"; u = 0; nm += n; then n times, while x < len(contig): md += T[x]; x += 1
    md += str(u)                                (once, also when the walk ended early)

tags                 (nm, md, a clamp was reached) of a row's fields
insert_tags          a SAM row -> the row with NM:i and MD:Z behind X0 (a row with CIGAR "*", an empty CIGAR or flag 4 stays as it is)
bam_tag_bytes        the bytes the two tags take in a BAM record
tag_record           a flag-off BAM record -> the record with the tags (and, for a minus row under "forward", its operations turned round)
unreverse            the CIGAR field with its tokens last to first: what GM_CIGAR_FORWARD prints for a minus-strand row
strip_tags           the inverse of insert_tags
rebuild_reference    (seq, cigar, md) -> the reference stretch the row covers, without looking at the reference
read_fasta, read_amb, contig_texts   the contigs' text as the index sees it: the FASTA with the holes' characters, upper case
"""
import re
import struct

NIBBLES = "=ACMGRSVTWYHKDBN"
_TOKEN = re.compile(rb"(\d*)([^\d])")


def code(c):
    """the BAM nibble of a character (an int or a one-byte string): either case, anything else 15"""
    ch = (chr(c) if isinstance(c, int) else c.decode("latin-1") if isinstance(c, bytes) else c).upper()
    k = NIBBLES.find(ch)
    return k if k >= 0 else 15


def tokens(cigar):
    """the field as k_bam_sizes reads it: digits accumulate, an operation takes them, any other byte drops them"""
    out = []
    for n, op in _TOKEN.findall(cigar):
        if op in (b"M", b"I", b"D") and n and int(n):
            out.append((int(n), op))
    return out


def tags(pos, cigar, seq, text):
    """pos: the row's POS (1-based); cigar, seq: its fields (bytes); text: the contig's text (bytes, upper case).
    Returns (nm, md, clamped)"""
    x, z, u, nm, md, clamped, ended = pos - 1, 0, 0, 0, [], False, False
    for n, op in tokens(cigar):
        if op == b"M":
            for _ in range(n):
                if z >= len(seq) or x >= len(text) or x < 0:
                    clamped = ended = True
                    break
                c = code(seq[z])
                if c == code(text[x]) and c != 15:
                    u += 1
                else:
                    md.append(b"%d%c" % (u, text[x])); u = 0; nm += 1
                x += 1; z += 1
            if ended:
                break
        elif op == b"I":
            z += n; nm += n
        else:
            md.append(b"%d^" % u); u = 0; nm += n
            for _ in range(n):
                if 0 <= x < len(text):
                    md.append(bytes([text[x]])); x += 1
                else:
                    clamped = True
    md.append(b"%d" % u)
    return nm, b"".join(md), clamped


def has_tags(fields):
    """a record whose CIGAR field is neither "*" nor empty (a field the row kernels print empty has no alignment to describe)"""
    return fields[5] not in (b"*", b"") and int(fields[1]) & 4 == 0


def insert_tags(row, contig_text):
    """row: a SAM row with its newline; contig_text: {contig name (bytes): text}"""
    f = row.rstrip(b"\n").split(b"\t")
    if not has_tags(f):
        return row
    nm, md, _ = tags(int(f[3]), f[5], f[9], contig_text[f[2]])
    assert f[-1].startswith(b"X0:i:")
    return row[:-1] + b"\tNM:i:%d\tMD:Z:%s\n" % (nm, md)


def strip_tags(row):
    f = row.rstrip(b"\n").split(b"\t")
    return b"\t".join(x for x in f if not x.startswith((b"NM:i:", b"MD:Z:"))) + b"\n"


def bam_tag_bytes(nm, md):
    return b"NMi" + struct.pack("<i", nm) + b"MDZ" + md + b"\0"


def unreverse(cigar):
    """the tokens (digits + operation) last to first: reverse_cigar is its own inverse on a field of whole tokens"""
    toks = re.findall(rb"\d*[^\d]", cigar)
    assert b"".join(toks) == cigar, cigar
    return b"".join(reversed(toks))


def forward_row(row):
    """a flag-off row as GM_CIGAR_FORWARD prints it: column 6 of a minus-strand row turned round, everything else untouched"""
    f = row.split(b"\t")
    if int(f[1]) & 16 and f[5] != b"*":
        f[5] = unreverse(f[5])
    return b"\t".join(f)


def tag_record(rec, row, contig_text, forward):
    """rec: the flag-off BAM record of the flag-off SAM row `row`.  The record with the setting(s) on"""
    f = row.rstrip(b"\n").split(b"\t")
    out = bytearray(rec)
    if forward and int(f[1]) & 16:
        l_name, n_ops = rec[12], struct.unpack_from("<H", rec, 16)[0]
        at = 36 + l_name
        ops = [rec[at + 4 * k:at + 4 * k + 4] for k in range(n_ops)]
        out[at:at + 4 * n_ops] = b"".join(reversed(ops))
        f[5] = unreverse(f[5]) if f[5] != b"*" else f[5]
    if contig_text is not None and has_tags(f):
        nm, md, _ = tags(int(f[3]), f[5], f[9], contig_text[f[2]])
        out += bam_tag_bytes(nm, md)
        struct.pack_into("<i", out, 0, len(out) - 4)
    return bytes(out)


_MD = re.compile(rb"(\d+)|(\^[A-Za-z]+)|([A-Za-z])")


def rebuild_reference(seq, cigar, md):
    """the reference bases under the row's M and D columns, from SEQ, the CIGAR field and the MD string alone.  An independent
    inverse of tags(): SEQ's own letter where MD counts a match, MD's letter at a mismatch, MD's letters behind '^' in a deletion.
    Returns (reference stretch in upper case, mismatches, inserted bases, deleted bases)"""
    # MD as a list of per-reference-column items: None = match, a letter = mismatch, ('^', letter) = deleted
    cols = []
    for num, dele, mis in _MD.findall(md):
        if num:
            cols.extend([None] * int(num))
        elif dele:
            cols.extend(("^", c) for c in dele[1:])
        else:
            cols.append(mis[0])
    ref, z, k, n_mis, n_ins, n_del = bytearray(), 0, 0, 0, 0, 0
    for n, op in tokens(cigar):
        if op == b"M":
            for _ in range(n):
                item = cols[k]; k += 1
                assert not isinstance(item, tuple), "a deleted column under M"
                if item is None:
                    ref.append(seq[z])
                else:
                    ref.append(item); n_mis += 1
                z += 1
        elif op == b"I":
            z += n; n_ins += n
        else:
            for _ in range(n):
                item = cols[k]; k += 1
                assert isinstance(item, tuple), "MD has no deletion where the CIGAR has one"
                ref.append(item[1]); n_del += 1
    assert k == len(cols) and z == len(seq), (k, len(cols), z, len(seq))
    return bytes(ref).upper(), n_mis, n_ins, n_del


def read_fasta(path):
    """[(name, text as in the file, case kept)]"""
    out, name, parts = [], None, []
    for line in open(path, "rb"):
        line = line.rstrip(b"\r\n")
        if line.startswith(b">"):
            if name is not None:
                out.append((name, b"".join(parts)))
            name, parts = line[1:].split()[0], []
        elif name is not None:
            parts.append(line)
    if name is not None:
        out.append((name, b"".join(parts)))
    return out


def read_amb(path):
    """[(offset on the concatenated reference, length, character)]"""
    lines = open(path, "rb").read().split(b"\n")
    n = int(lines[0].split()[2])
    holes = []
    for ln in lines[1:1 + n]:
        off, length, ch = ln.split()
        holes.append((int(off), int(length), ch[:1]))
    return sorted(holes)


def pac_text(pac_path, l_pac):
    raw = open(pac_path, "rb").read()
    return bytes(b"ACGT"[(raw[i >> 2] >> ((~i & 3) << 1)) & 3] for i in range(l_pac))


def contig_texts(fa):
    """{name: T} from the index files alone: the pac letters with the holes of <fa>.gnumap.amb put in, upper case - and checked against
    the FASTA's own text, which has to be the same thing"""
    ann = open(fa + ".gnumap.ann", "rb").read().split(b"\n")
    l_pac, n_seqs = int(ann[0].split()[0]), int(ann[0].split()[1])
    text = bytearray(pac_text(fa + ".gnumap.pac", l_pac))
    for off, length, ch in read_amb(fa + ".gnumap.amb"):
        text[off:off + length] = ch.upper() * length
    out = {}
    for i in range(n_seqs):
        name = ann[1 + 2 * i].split()[1]
        off, length = (int(v) for v in ann[2 + 2 * i].split()[:2])
        out[name] = bytes(text[off:off + length])
    for name, seq in read_fasta(fa):
        assert out[name] == seq.upper(), name
    return out
