"""A two-sided repeat for gm_batch_set_mates, generated from a seed: nothing of it is committed.  In the world of tests/mates_fixture.py a
repeat is one mate of its pair and the other mate is unique, so no pair there has more than one record on BOTH sides.  Here both are
inside the repeat.

Genome: one contig `rA` of 75 000 i.i.d. bases with one 400-base element planted 70 times, every 1000 bases from 2000 on: every copy
has unique flanks.  Reads are 100 bases of quality 'I'.  A repeat pair has its plus mate at offset x of the element and its minus mate
ending at x + 300, both inside the element: each mate has 70 records of one posterior, and of the 70 x 70 combinations the 70 inside one
copy are concordant (insert 300) under the limits 120 .. 500 - a neighbouring copy is 1000 bases further.  All have one product, so the
rule's primaries are the first record of the first mate and the record of the second mate in the same copy.

PAIRS: three repeat pairs (x = 0; x = 50 with the minus mate first; x = 100) and one unique pair from the flank behind the last copy."""
import os
from collections import namedtuple

import numpy as np

SEED = 43
L = 100
MIN_INSERT, MAX_INSERT = 120, 500
LEN_A = 75_000
ELEM_LEN, ELEM_N, ELEM_AT, ELEM_STEP = 400, 70, 2000, 1000
CONTIGS = [("rA", LEN_A)]
REPEAT_X = ((0, False), (50, True), (100, False))       # (offset of the plus mate in the element, the minus mate is the first mate)
UNIQUE_AT = 73_000

Pair = namedtuple("Pair", "kind name seq1 seq2")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def revcomp(s):
    return bytes(s[::-1]).translate(bytes.maketrans(b"ACGT", b"TGCA"))


def genome():
    rng = np.random.default_rng(SEED)
    a = ACGT[rng.integers(0, 4, LEN_A)].copy()
    elem = ACGT[rng.integers(0, 4, ELEM_LEN)]
    for i in range(ELEM_N):
        a[ELEM_AT + i * ELEM_STEP:ELEM_AT + i * ELEM_STEP + ELEM_LEN] = elem
    return a.tobytes()


def make_pairs():
    g = genome()
    out = []
    for x, minus_first in REPEAT_X:
        s = ELEM_AT + x
        f, r = g[s:s + L], revcomp(g[s + 300 - L:s + 300])
        out.append(Pair("repeat2", b"repeat2:%d" % x, r if minus_first else f, f if minus_first else r))
    out.append(Pair("unique", b"unique", g[UNIQUE_AT:UNIQUE_AT + L], revcomp(g[UNIQUE_AT + 300 - L:UNIQUE_AT + 300])))
    return out


class World:
    """fa, pairs, reads [(name, seq, qual)] in block order"""

    def __init__(self, workdir, build_index):
        self.fa = os.path.join(str(workdir), "repeat2.fa")
        g = genome()
        with open(self.fa, "wb") as f:
            f.write(b">rA\n")
            for i in range(0, len(g), 100):
                f.write(g[i:i + 100] + b"\n")
        build_index(self.fa)
        self.pairs = make_pairs()
        self.reads = []
        for p in self.pairs:
            self.reads += [(p.name, p.seq1, b"I" * L), (p.name, p.seq2, b"I" * L)]


def self_check(world, recs, cigars):
    """the world is what it was built for: asserted from the mates-off records (the oracle's, or the device's), never from the mates-on
    output.  Returns the number of rows"""
    import mates_model as mm
    n = len(world.reads)
    rng = mm._ranges(recs, n)
    sp = [mm.span(c) for c in cigars]
    prim, proper = mm.resolve(recs, cigars, n, MIN_INSERT, MAX_INSERT)
    for i, p in enumerate(world.pairs):
        A, B = rng[2 * i], rng[2 * i + 1]
        if p.kind == "unique":
            assert len(A) == len(B) == 1 and proper[i]
            continue
        assert len(A) == len(B) == ELEM_N, (p.name, len(A), len(B))                                # 70 x 70
        ok = [(a, b) for a in A for b in B if mm.concordant(recs[a], sp[a], recs[b], sp[b], MIN_INSERT, MAX_INSERT)]
        assert len(ok) == ELEM_N and len({a for a, _ in ok}) == len({b for _, b in ok}) == ELEM_N
        prods = {float(np.float32(recs[a]["post_prob"]) * np.float32(recs[b]["post_prob"])) for a, b in ok}
        assert len(prods) == 1 and len({float(recs[k]["post_prob"]) for k in list(A) + list(B)}) == 1     # one product
        assert proper[i] and prim[2 * i] == A[0] and prim[2 * i + 1] == B[0], (p.name, prim[2 * i] - A[0], prim[2 * i + 1] - B[0])
        assert len({int(recs[a]["strand"]) for a in A}) == 1 and int(recs[A[0]]["strand"]) != int(recs[B[0]]["strand"])
    assert len(recs) == 3 * 2 * ELEM_N + 2
    return len(recs)
