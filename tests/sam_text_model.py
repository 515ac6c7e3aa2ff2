"""The SAM row of a record in plain Python: what gm_output_batch_text (k_out_text_sizes / k_out_text_rows) has to print for the records
and CIGARs of gm_output_batch.  Python's "%g" is C's.

revcomp, reverse_cigar   the minus strand's SEQ and CIGAR, as the reference program turns them
sam_rows                 records + CIGARs + the reads' text -> one row (bytes) per record
check_text               a device text and its row offsets against sam_rows, row by row and as a whole
"""
import re

import numpy as np

COMP = {ord(a): ord(b) for a, b in zip("atcgATCG-", "tagcTAGC-")}


def revcomp(s):
    return bytes(COMP.get(c, ord("n")) for c in reversed(s))          # reverse_comp, inc/SequenceOperations.h:56-96


def reverse_cigar(c):
    # inc/SequenceOperations.h:109-123: tokens of "digits" (48..58, so ':' too) + one operation, in reverse order; digits after the last
    # operation are dropped
    return b"".join(reversed(re.findall(rb"[0-9:]*[^0-9:]", c)))


def sam_rows(recs, cigars, names, seqs, quals, contigs, adjust):
    inv = 1.0 / float(np.float32(adjust))
    rows = []
    for r, cg in zip(recs, cigars):
        i = int(r["read"])
        minus = int(r["strand"]) != 0
        xa = "%g" % (float(np.float32(r["a_score"])) * inv)
        xp = "1" if np.float32(r["post_prob"]) == np.float32(1.0) else "%g" % float(np.float32(r["post_prob"]))
        rows.append(b"\t".join([names[i][:1023], b"16" if minus else b"0", contigs[int(r["contig"])].encode(), b"%d" % int(r["chr_pos"]), b"%d" % int(r["mapq"]),
                                reverse_cigar(cg) if minus else cg, b"*", b"0", b"0", revcomp(seqs[i]) if minus else seqs[i],
                                quals[i][::-1] if minus else quals[i], b"XA:f:" + xa.encode(), b"XP:f:" + xp.encode(), b"X0:i:%d" % int(r["sim_matches"])]) + b"\n")
    return rows


def check_text(ix, p, seqs, quals, names, recs, cigars, text, row_off):
    contigs = [c for c, _ in ix.contigs()]
    want = sam_rows(recs, cigars, names, seqs, quals, contigs, p.adjust)
    assert len(row_off) == len(recs) + 1 and int(row_off[0]) == 0 and int(row_off[-1]) == len(text)
    got = [text[int(row_off[k]):int(row_off[k + 1])] for k in range(len(recs))]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
    assert text == b"".join(want)
    assert all(r.endswith(b"\n") and r.count(b"\n") == 1 for r in got)
