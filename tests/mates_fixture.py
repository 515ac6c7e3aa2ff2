"""One small paired-end world for gm_batch_set_mates / --mates, generated from a seed: nothing of it is committed.  tests/test_gpu_mates.py
builds it once per module (FASTA, g.index_build, g.Index), tests/test_mates_cpu.py builds it on the host and takes the records from the
oracle.

Genome: `mA` of 40 000 bases - i.i.d. bases, with one 120-base element planted 70 times, every 400 bases from 2000 on, so that every
copy has unique flanks - and `mB` of 30 000 i.i.d. bases.  Reads are 100 bases of quality 'I' (one of 125: the pair that starts at one
POS and is still concordant).  The run's limits are MIN_INSERT = 120 and MAX_INSERT = 500.

PAIRS is the list of pairs in file order (a seeded shuffle); a Pair's `kind` names what it is there for:

    ordinary      88 forward/reverse pairs from seeded places outside the element's stretch, inserts spread over 150 .. 450, the minus
                  mate first in every other one
    repeat_a      the element as first mate (70 places, one winning sequence), the second mate on the minus strand in the unique flank
                  behind copy 67: the only concordant place has record index 67
    repeat_b      the same with the roles swapped: the element is the second mate, the one that is staged through LDS
    ins_max / ins_over / ins_min / ins_under     inserts of exactly 500, 501, 120, 119
    both_plus / outward / two_contigs            not concordant
    un_first / un_second / un_both               a mate of random bases (no record): two of each of the one-sided kinds, one of both
    del_minus     the minus-strand mate has a two-base deletion
    ins_plus      the plus-strand mate has a two-base insertion
    same_pos / same_pos_rev / same_pos_short     both mates start at one POS: 100 + 125 bases (concordant, insert 125), the same with
                  the minus mate first, and 100 + 100 (insert 100 < MIN_INSERT: not concordant, and still a TLEN)
    first_base / last_base_a / last_base_b       pairs at mB's first base, mA's last (the next contig follows at once) and mB's last
    names: the three styles - `x/1` + `x/2`, `x 1:N:0` + `x 2:N:0`, plain equal names - cycle over all pairs
"""
import os
from collections import namedtuple

import numpy as np

SEED = 41
L = 100
MIN_INSERT, MAX_INSERT = 120, 500
LEN_A, LEN_B = 40_000, 30_000
ELEM_LEN, ELEM_N, ELEM_AT, ELEM_STEP = 120, 70, 2000, 400
ELEM_COPY = 67                                          # the copy the repeat pairs belong to: beyond the first trip of 64 lanes
N_ORDINARY = 88
CONTIGS = [("mA", LEN_A), ("mB", LEN_B)]

Pair = namedtuple("Pair", "kind name1 seq1 name2 seq2 want")    # want: None, or dict(contig, pos1, pos2, strand1, strand2) of the two primaries (1-based)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def revcomp(s):
    return bytes(s[::-1]).translate(bytes.maketrans(b"ACGT", b"TGCA"))


def genome():
    """(mA, mB) as bytes"""
    rng = np.random.default_rng(SEED)
    a = ACGT[rng.integers(0, 4, LEN_A)].copy()
    b = ACGT[rng.integers(0, 4, LEN_B)].copy()
    elem = ACGT[rng.integers(0, 4, ELEM_LEN)]
    for i in range(ELEM_N):
        a[ELEM_AT + i * ELEM_STEP:ELEM_AT + i * ELEM_STEP + ELEM_LEN] = elem
    return a.tobytes(), b.tobytes()


def write_fasta(path, seqs):
    with open(path, "wb") as f:
        for (name, _), s in zip(CONTIGS, seqs):
            f.write(b">" + name.encode() + b"\n")
            for i in range(0, len(s), 100):
                f.write(s[i:i + 100] + b"\n")


def _indel_point(ref, lo):
    """the first offset q >= lo at which neither a 2-base deletion of ref[q:q+2] nor a 2-base insertion in front of ref[q] can slide"""
    for q in range(lo, lo + 30):
        if ref[q - 1] != ref[q + 1] and ref[q] != ref[q + 2] and ref[q - 2:q] != ref[q:q + 2] and ref[q:q + 2] != ref[q + 2:q + 4] and ref[q - 1] != ref[q]:
            return q
    raise AssertionError("no unambiguous indel point")


def _del_read(ref):
    """100 bases that skip two of ref (ref: at least 110 bases from the read's start)"""
    q = _indel_point(ref, 50)
    return ref[:q] + ref[q + 2:L + 2]


def _ins_read(ref):
    q = _indel_point(ref, 49)
    ins = bytes(next(c for c in b"ACGT" if c not in (ref[q - 1], ref[q])) for _ in range(2))
    return ref[:q] + ins + ref[q:L - 2]


def make_pairs():
    seqs = genome()
    rng = np.random.default_rng(SEED + 1)
    raw = []                                            # (kind, seq1, seq2, want)

    def fr(kind, c, s, insert, minus_first=False, len_r=L, edit_f=None, edit_r=None):
        """a forward/reverse pair: the plus mate starts at 0-based s of contig c, the minus mate ends `insert` bases on"""
        g = seqs[c]
        f_seq = edit_f(g[s:s + L + 10]) if edit_f else g[s:s + L]
        r0 = s + insert - len_r
        r_seq = revcomp(edit_r(g[r0:r0 + len_r + 10]) if edit_r else g[r0:r0 + len_r])
        want = dict(contig=c, plus_pos=s + 1, minus_pos=r0 + 1, minus_first=minus_first)
        raw.append((kind, r_seq, f_seq, want) if minus_first else (kind, f_seq, r_seq, want))

    def rand_read():
        return ACGT[rng.integers(0, 4, L)].tobytes()

    # ordinary pairs: outside the element's stretch [2000, 30000) of mA
    for k in range(N_ORDINARY):
        insert = 150 + (k * 300) // (N_ORDINARY - 1)
        if k % 4 == 3:
            c, s = 0, int(rng.integers(30_600, LEN_A - 700))
        else:
            c, s = 1, int(rng.integers(600, LEN_B - 700))
        fr("ordinary", c, s, insert, minus_first=bool(k & 1))
    p67 = ELEM_AT + ELEM_COPY * ELEM_STEP
    fr("repeat_a", 0, p67 + 10, 300)
    fr("repeat_b", 0, p67 + 10, 300, minus_first=True)
    fr("ins_max", 1, 5000, MAX_INSERT)
    fr("ins_over", 1, 6000, MAX_INSERT + 1)
    fr("ins_min", 1, 7000, MIN_INSERT)
    fr("ins_under", 1, 8000, MIN_INSERT - 1)
    g = seqs[1]
    raw.append(("both_plus", g[9000:9100], g[9200:9300], None))
    raw.append(("outward", g[10200:10300], revcomp(g[10000:10100]), None))
    raw.append(("two_contigs", seqs[0][31000:31100], revcomp(g[11000:11100]), None))
    for s in (12000, 12500):
        raw.append(("un_first", rand_read(), revcomp(g[s:s + L]), None))
        raw.append(("un_second", g[s + 200:s + 200 + L], rand_read(), None))
    raw.append(("un_both", rand_read(), rand_read(), None))
    fr("del_minus", 1, 14000, 300, edit_r=_del_read)
    # the aligner's window is exactly the read's length: a read with two foreign bases needs 98 of it, and its last base slides onto the
    # window's last wherever the two are equal (..2D1M, span 100).  Where they differ the CIGAR is xM2IyM and spans 98
    s = next(s for s in range(15000, 15100) if g[s + 97] != g[s + 99] and g[s + 96] != g[s + 99])
    fr("ins_plus", 1, s, 300, edit_f=_ins_read)
    fr("same_pos", 1, 16000, 125, len_r=125)
    fr("same_pos_rev", 1, 17000, 125, len_r=125, minus_first=True)
    fr("same_pos_short", 1, 18000, 100)
    fr("first_base", 1, 0, 300)
    fr("last_base_a", 0, LEN_A - 300, 300)
    fr("last_base_b", 1, LEN_B - 300, 300, minus_first=True)
    order = rng.permutation(len(raw))
    pairs = []
    for n, i in enumerate(order):
        kind, s1, s2, want = raw[i]
        base = b"%s:%d" % (kind.encode(), n)
        style = n % 3
        n1, n2 = (base + b"/1", base + b"/2") if style == 0 else (base + b" 1:N:0:ACGT", base + b" 2:N:0:ACGT") if style == 1 else (base, base)
        pairs.append(Pair(kind, n1, s1, n2, s2, want))
    return pairs


def reads_of(pairs):
    """[(name, seq, qual)] in block order: first mate, second mate, first mate, ..."""
    out = []
    for p in pairs:
        out.append((p.name1, p.seq1, b"I" * len(p.seq1)))
        out.append((p.name2, p.seq2, b"I" * len(p.seq2)))
    return out


def fastq(reads):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads)


class World:
    """fa, pairs, reads"""

    def __init__(self, workdir, build_index):
        self.fa = os.path.join(str(workdir), "mates.fa")
        write_fasta(self.fa, genome())
        build_index(self.fa)
        self.pairs = make_pairs()
        self.reads = reads_of(self.pairs)
        self.kinds = [p.kind for p in self.pairs]

    def pair_of(self, kind):
        return [i for i, k in enumerate(self.kinds) if k == kind]


def oracle_records(world, orc, **kw):
    """the records of every read from the oracle, as the model takes them: (recs [dict with read, contig, chr_pos, strand, post_prob], cigars)"""
    oix = orc.index_load(world.fa)
    op = orc.params(**kw)
    recs, cigars = [], []
    for i, (_, seq, qual) in enumerate(world.reads):
        for q in orc.read_output(oix, op, orc.pwm(seq, qual), seq)[1]:
            recs.append(dict(read=i, contig=int(q["contig"]), chr_pos=int(q["chr_pos"]), strand=int(q["strand"]), post_prob=np.float32(q["post_prob"])))
            cigars.append(bytes(q["cigar"]))
    return recs, cigars


def self_check(world, recs, cigars):
    """the world realises its kinds: asserted from records (the oracle's, or the device's with mates off), never from the mates-on output.
    Returns {kind: [(fields of the first mate's primary row, of the second's)]}"""
    import mates_model as mm
    n = len(world.reads)
    prim, proper = mm.resolve(recs, cigars, n, MIN_INSERT, MAX_INSERT)
    fields = mm.row_fields(recs, cigars, n, MIN_INSERT, MAX_INSERT)
    rng = mm._ranges(recs, n)
    lone, _ = mm.resolve(recs, cigars, n, 0, 0)        # (no combination is concordant under [0, 0]: the choice a mapper without mates makes)
    seen = {}
    for i, p in enumerate(world.pairs):
        a, b = prim[2 * i], prim[2 * i + 1]
        seen.setdefault(p.kind, []).append((None if a is None else fields[a], None if b is None else fields[b]))
        w = p.want
        if p.kind.startswith("un_"):
            assert (a is None) == (p.kind in ("un_first", "un_both")) and (b is None) == (p.kind in ("un_second", "un_both")), (p.kind, a, b)
            assert not proper[i]
            continue
        assert a is not None and b is not None, (p.kind, i)
        if w is not None:
            f_rec, r_rec = (recs[b], recs[a]) if w["minus_first"] else (recs[a], recs[b])
            assert (int(f_rec["contig"]), int(f_rec["chr_pos"]), int(f_rec["strand"])) == (w["contig"], w["plus_pos"], 0), (p.kind, f_rec, w)
            assert (int(r_rec["contig"]), int(r_rec["chr_pos"]), int(r_rec["strand"])) == (w["contig"], w["minus_pos"], 1), (p.kind, r_rec, w)
        want_proper = p.kind not in ("ins_over", "ins_under", "both_plus", "outward", "two_contigs", "same_pos_short")
        assert proper[i] == want_proper, (p.kind, i, recs[a], recs[b], cigars[a], cigars[b])
        if p.kind in ("repeat_a", "repeat_b"):
            elem = 2 * i + (p.kind == "repeat_b")
            assert len(rng[elem]) == ELEM_N and len(rng[elem ^ 1]) == 1, (p.kind, len(rng[elem]), len(rng[elem ^ 1]))
            at = prim[elem] - rng[elem][0]
            assert at == ELEM_COPY >= 64 and lone[elem] - rng[elem][0] != at, (p.kind, at, lone[elem])
            assert len(set(float(recs[k]["post_prob"]) for k in rng[elem])) == 1
        if p.kind == "del_minus":
            assert b"D" in cigars[b] and recs[b]["strand"], cigars[b]
        if p.kind == "ins_plus":
            assert b"I" in cigars[a] and not recs[a]["strand"] and mm.span(cigars[a]) != L, cigars[a]
        if p.kind.startswith("same_pos"):
            assert int(recs[a]["chr_pos"]) == int(recs[b]["chr_pos"])
            assert fields[a][3] > 0 > fields[b][3] and fields[a][3] == -fields[b][3]
        if p.kind == "first_base":
            assert int(recs[a]["chr_pos"]) == 1 and int(recs[a]["contig"]) == 1
        if p.kind.startswith("last_base"):
            r_rec = recs[a] if w["minus_first"] else recs[b]
            k = a if w["minus_first"] else b
            assert int(r_rec["chr_pos"]) + mm.span(cigars[k]) - 1 == CONTIGS[int(r_rec["contig"])][1]
        if p.kind == "two_contigs":
            assert int(recs[a]["contig"]) != int(recs[b]["contig"]) and fields[a][3] == 0 and fields[a][1] == int(recs[b]["contig"])
    kinds = {"ordinary": N_ORDINARY, "repeat_a": 1, "repeat_b": 1, "ins_max": 1, "ins_over": 1, "ins_min": 1, "ins_under": 1, "both_plus": 1, "outward": 1,
             "two_contigs": 1, "un_first": 2, "un_second": 2, "un_both": 1, "del_minus": 1, "ins_plus": 1, "same_pos": 1, "same_pos_rev": 1, "same_pos_short": 1,
             "first_base": 1, "last_base_a": 1, "last_base_b": 1}
    assert {k: len(v) for k, v in seen.items()} == kinds
    assert any(mm.span(c) != L for c in cigars)
    return seen
