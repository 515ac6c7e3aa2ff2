"""Planted reads for tests/test_gpu_md.py: stretches of golden/syn.fa cut with Index.window() and edited, each on both strands, so that
the rows carry the shapes the MD walk can get wrong - mismatches at the first and last column and on both sides of a 64-column trip,
adjacent mismatches, deletions across columns 64 and 128, a deletion beside a mismatch, every length around a trip's end, a run of four
digits, N and lower case in the read, and the 150-N hole of chrA (pac offset 120 000) under both ends of a read.

An edit is written in REFERENCE columns of the stretch: ("s", c) substitutes column c, ("d", c, n) deletes columns c .. c+n-1,
("i", c) inserts one base in front of column c.  The minus-strand twin of a read is its reverse complement."""
import numpy as np

HOLE = (120000, 150)                    # golden/syn.fa.gnumap.amb
_COMP = bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _other(c, k=1):
    return b"ACGT"[(b"ACGT".index(c) + k) % 4]


def edit(ref, edits):
    """ref: the stretch, upper case.  Returns the read (plus strand)"""
    out, at = bytearray(), 0
    for e in sorted(edits, key=lambda e: e[1]):
        out += ref[at:e[1]]; at = e[1]
        if e[0] == "s":
            out.append(_other(ref[at], 1 + at % 3)); at += 1
        elif e[0] == "d":
            at += e[2]
        else:
            out.append(_other(ref[at], 2))     # differs from the base behind it: the insertion has one place
    out += ref[at:]
    return bytes(out)


# (tag, read length, edits)
SHAPES = [
    ("ends", 150, [("s", 0), ("s", 63), ("s", 64), ("s", 149)]),
    ("mid", 150, [("s", 9), ("s", 10), ("s", 65), ("s", 99)]),
    ("last100", 100, [("s", 64), ("s", 99)]),
    ("del64", 150, [("d", 63, 2), ("i", 110)]),
    ("del128", 150, [("d", 127, 2), ("i", 30)]),
    ("delmis", 150, [("d", 40, 2), ("s", 42)]),
    ("misdel", 150, [("s", 39), ("d", 40, 2)]),
    ("len63", 63, [("s", 62)]),
    ("len64", 64, [("s", 63)]),
    ("len65", 65, [("s", 64)]),
    ("len128", 128, [("s", 127)]),
    ("len129", 129, [("s", 128)]),
    ("len150", 150, []),
]


def planted(window):
    """window(begin, L) -> the reference stretch (any case).  [(name, sequence, quality line)], names unique"""
    reads = []

    def both(tag, seq):
        reads.append((b"p_%s_f" % tag.encode(), seq, b"I" * len(seq)))
        rc = revcomp(seq)
        reads.append((b"p_%s_r" % tag.encode(), rc, b"I" * len(rc)))

    for k, (tag, L, edits) in enumerate(SHAPES):
        ref_len = L + sum(e[2] for e in edits if e[0] == "d") - sum(1 for e in edits if e[0] == "i")
        begin = 20000 + 1000 * k
        ref = window(begin, ref_len).upper()
        # a deletion inside a repeat of its own bases has several places and the aligner takes the leftmost: move on until it has one
        while any(e[0] == "d" and (ref[e[1] - 1] == ref[e[1] + e[2] - 1] or ref[e[1]] == ref[e[1] + e[2]]) for e in edits):
            begin += 1
            ref = window(begin, ref_len).upper()
        seq = edit(ref, edits)
        assert len(seq) == L, (tag, len(seq))
        both(tag, seq)
    long_ref = window(60000, 1100).upper()
    both("long1100", long_ref)                                   # a perfect read: one run of four digits, 18 trips
    n_ref = bytearray(window(70000, 100).upper())
    n_ref[20] = n_ref[21] = n_ref[77] = ord("N")
    both("withN", bytes(n_ref))
    both("lower", window(71000, 100).lower())
    both("hole_in", window(HOLE[0] - 50, 100).upper())             # the last 50 columns lie in the hole (the pac's drawn letters: they map)
    both("hole_out", window(HOLE[0] + HOLE[1] - 50, 100).upper())    # the first 50
    both("hole_over", window(HOLE[0] - 20, 150).upper()[:150])       # starts in front of it, ends inside
    assert len(set(r[0] for r in reads)) == len(reads)
    return reads


def rand_reads(seed, n, tag, L=100):
    rng = np.random.default_rng(seed)
    return [(b"%s%d" % (tag, i), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)), b"I" * L) for i in range(n)]
