"""What gm_batch_set_unmapped_rows / --sam_unmapped has to write, as a plain Python model.  The yardstick is the flag-off output (pinned
byte for byte to the reference program elsewhere) plus the SAMv1 text: the rows of a block with the setting on are the flag-off rows,
untouched, merged by read index with one row for every read that has none.

unmapped_row         the SAM row of a read without a record
merge                flag-off rows + their read indices + the block's reads -> (the rows with the setting on, which of them are new)
unmapped_record      the BAM record of such a row (bam_model.sam_row_to_record cannot take RNAME '*': refID -1, and SEQ '*' is l_seq 0)
to_records           rows -> BAM records, either kind
records_differ       got against want: the new records byte for byte, the others under bam_model.records_equal
sort_rows            sam_sort_model.sort_rows (it puts RNAME '*' last, in input order)
YU                   the tag's codes: gm_hits.status
"""
import struct

import bam_model as bm
import sam_sort_model as ssm

YU = {"ok_nothing_printed": 0, "too_many": 1, "none": 2, "too_short": -2, "too_poor": -3}
HEAD = b"\t4\t*\t0\t0\t*\t*\t0\t0\t"
UNMAPPED_BIN = 4680
assert bm.reg2bin(-1, 0) == UNMAPPED_BIN


def unmapped_row(name, seq, qual, status):
    """name: what follows '@', uncut; seq: the bases as uploaded; qual: the whole quality line (a FASTA read: str2qual's string);
    status: gm_hits.status of the read"""
    if len(seq) == 0:
        seq, qual = b"*", b"*"
    return bytes(name[:1023]) + HEAD + bytes(seq) + b"\t" + bytes(qual) + b"\tYU:i:%d\n" % int(status)


def merge(rows, row_reads, names, seqs, quals, status):
    """rows: the flag-off rows (bytes, one per record, in output order); row_reads: the read of each (recs[].read of Batch.output on the
    same hits: ascending); names / seqs / quals / status: one per read of the block.  Returns (rows, flags): flags[k] is True for a row
    this model made"""
    n = len(names)
    assert len(seqs) == n and len(quals) == n and len(status) == n and len(rows) == len(row_reads)
    assert all(int(a) <= int(b) for a, b in zip(row_reads, row_reads[1:])), "the flag-off rows are in read order"
    out, new, k = [], [], 0
    for i in range(n):
        had = False
        while k < len(rows) and int(row_reads[k]) == i:
            out.append(rows[k]); new.append(False); k += 1; had = True
        if not had:
            out.append(unmapped_row(names[i], seqs[i], quals[i], status[i])); new.append(True)
    assert k == len(rows), "a flag-off row names a read beyond the block"
    return out, new


def is_unmapped_row(row):
    f = row.split(b"\t")
    return f[1] == b"4" and f[2] == b"*"


def unmapped_record(row):
    f = row.rstrip(b"\n").split(b"\t")
    assert f[1:9] == [b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0"] and len(f) == 12 and f[11].startswith(b"YU:i:")
    name = f[0][:254] + b"\0"
    seq, qual = (b"", b"") if f[9] == b"*" else (f[9], f[10])
    l_seq = len(seq)
    nib = [bm.NIBBLES.index(chr(c).upper()) if chr(c).upper() in bm.NIBBLES else 15 for c in seq]
    if l_seq & 1:
        nib.append(0)
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))
    q = bytes(max(c - 33, 0) for c in qual[:l_seq]) if len(qual) >= l_seq else b"\xff" * l_seq
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, UNMAPPED_BIN, 0, 4, l_seq, -1, -1, 0) + name + packed + q
    body += b"YUi" + struct.pack("<i", int(f[11][5:]))
    return struct.pack("<i", len(body)) + body


def to_records(rows, contigs):
    return [unmapped_record(r) if is_unmapped_row(r) else bm.sam_row_to_record(r, contigs) for r in rows]


def record_is_unmapped(rec):
    return struct.unpack_from("<i", rec, 4)[0] == -1


def fixed_fields(rec):
    """(refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next refID, next pos, tlen) of a record"""
    return struct.unpack_from("<iiBBHHHiiii", rec, 4)


def records_differ(got, want):
    """None, or the first difference: a record of a read without a row byte for byte, the others under bam_model.records_equal"""
    if len(got) != len(want):
        return f"{len(got)} records, the model has {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        if record_is_unmapped(b):
            if a != b:
                return f"record {i} (no row without the setting): {a!r} vs {b!r}"
        else:
            why = bm.records_equal([a], [b])
            if why:
                return f"record {i}: {why}"
    return None


def sort_rows(rows, contigs):
    """rows (bytes) in coordinate order: stable, the rows without a contig last in input order"""
    return [r.encode("latin-1") for r in ssm.sort_rows([r.decode("latin-1") for r in rows], contigs)]
