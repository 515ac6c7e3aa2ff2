"""One "wide" world for the egress kernels, generated from a seed: coordinates of up to nine digits, BAM bins of every level, indels
beside bin boundaries, contigs at absolute offsets above 10^8.  Nothing of it is committed; tests/test_gpu_wide_coords.py builds it once
per module (FASTA, g.index_build, g.Index) and tests/test_wide_cpu.py checks the part that needs no genome.

Genome (tools/scale_check.write_contigs, i.i.d. bases): contig 0 `chrW` of 100 001 000 bases, then 41 short contigs whose lengths cycle
through 131 172, 150, 1000, 16 384, 16 385 and 20 000; contig 9 is called `Z`, contig 10 has a 200-character name, contig 41 (16 385
bases) ends the genome.

Reads are 100 bases with quality 'I', each place on both strands.  PLACES is the table of planted places: (class, label, contig, 0-based
start in the contig, kind, BAM bin).  kind "M" is the reference's bases, "D" skips two reference bases near the read's middle, "I" has
two foreign bases near its middle.  The reference program aligns a read against a window of exactly its own length.  So a "D" read's
CIGAR spans 100 reference bases, not 102, and ends in insertions that add up to 2 (52M2D46M2I); and an "I" read, which needs 98, has two
spare window bases that its tail slides onto wherever the reference repeats a base there (51M2I46M2D1M).  The "I" places are therefore
the ones of I_PLACES: beside four of the six B the read planted at B-98 or B-99 aligns as xM2IyM, for the 128 KiB level and for
2^26 + k*2^14 another multiple of the same level does (5*2^17, 2^26 + 5*2^14).  SPANS is what a CIGAR of each kind spans here, WRONG_SPANS
what a sizing that counts I runs, or takes the read length, would use.  The bins of BOUNDARIES, I_PLACES and DEEP_BINS are literals of
SAMv1 section 5.3 worked out by hand; the others are 4681 + (start >> 14), none of them crosses a 16 KiB boundary but the last read of
contig 41 (bin 585).

    digits    1-based positions 1, 9, 10, 99, ... 99 999 999, 100 000 000 of chrW and its last 100 bases (100 000 901)
    bins      B in {5*2^14, 3*2^17, 3*2^20, 3*2^23, 2^26, 2^26 + 2^14}: starts B-100 and B (16 KiB level), B-1, B-99, B-50 (crossing B)
    indels    "D" at B-100 beside every B (ends at B; with its I runs counted it would cross), "I" at the places of I_PLACES (ends at B or
              B-1; pos + 100 would cross).  No read of this aligner spans more than its length, so none crosses B through a deletion
    short     the first and the last 100 bases of contigs 1, 9, 10 and 41, one read inside the 150-base contig 2
    ties      eight copies of one read per strand; sixteen random reads that map nowhere

Measured on an MI355X: FASTA and index build (suffix-array stage on the device) 0.7 s, index load, the oracle's records of the 170 reads
and the mapping of the three blocks 0.1 s, 0.8 s in all (tests/test_gpu_wide_coords.py::world prints it).  With the host's SA-IS the
build alone takes about 20 s.
"""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED = 23
L = 100
KW = dict(mer=14, jump=7)
CHRW = 100_001_000
SHORT_LENGTHS = (131_172, 150, 1000, 16_384, 16_385, 20_000)
N_SHORT = 41
BLOCK_SIZES = (37, 101)                               # and the rest: three blocks of unequal size

# B, (bin of [B-100, B), bin of [B, B+100)), bin of a read that crosses B
BOUNDARIES = ((5 << 14, (4685, 4686), 585), (3 << 17, (4704, 4705), 73), (3 << 20, (4872, 4873), 9), (3 << 23, (6216, 6217), 1),
              (1 << 26, (8776, 8777), 0), ((1 << 26) + (1 << 14), (8777, 8778), 1097))
DEEP_BINS = {9_999_998: 5291, 9_999_999: 5291, 99_999_998: 10784, 99_999_999: 10784}      # 0-based start -> bin
DIGIT_POS1 = [1, 9] + [v for e in range(1, 8) for v in (10 ** e, 10 ** (e + 1) - 1)] + [100_000_000]

Place = namedtuple("Place", "cls label contig start kind bin")
Read = namedtuple("Read", "name seq qual place strand")        # place: index into PLACES, or None for a read that maps nowhere


def contig_table():
    """[(name, length)] of the 42 contigs"""
    out = [("chrW", CHRW)]
    for i in range(1, N_SHORT + 1):
        name = "Z" if i == 9 else "L" + "x" * 199 if i == 10 else "s%02d" % i
        out.append((name, SHORT_LENGTHS[(i - 1) % len(SHORT_LENGTHS)]))
    return out


# B, how far in front of B the "I" read starts, its bin, the bin of a read that crosses B
I_PLACES = ((5 << 14, 98, 4685, 585), (5 << 17, 98, 4720, 73), (3 << 20, 99, 4872, 9), (3 << 23, 98, 6216, 1), (1 << 26, 98, 8776, 0),
            ((1 << 26) + (5 << 14), 98, 8781, 1097))
BIN_LITERALS = sorted({b for _, pair, cross in BOUNDARIES for b in pair + (cross,)} | set(DEEP_BINS.values()) | {p[2] for p in I_PLACES})
SPANS = {"M": L, "D": L, "I": L - 2}                      # the reference bases a CIGAR of the kind spans
WRONG_SPANS = {"D": L + 2, "I": L}                        # with the I runs counted / from the read length


def _places():
    out = []
    low = lambda s: 4681 + (s >> 14)                   # a read inside one 16 KiB window
    for p1 in DIGIT_POS1:
        s = p1 - 1
        out.append(Place("digits", "p%d" % p1, 0, s, "M", DEEP_BINS.get(s, low(s))))
    out.append(Place("digits", "end_of_chrW", 0, CHRW - L, "M", low(CHRW - L)))
    for B, (below, at), cross in BOUNDARIES:
        out.append(Place("bins", "B%d-100" % B, 0, B - 100, "M", below))
        out.append(Place("bins", "B%d" % B, 0, B, "M", at))
        for d in (1, 99, 50):
            out.append(Place("bins", "B%d-%d" % (B, d), 0, B - d, "M", cross))
    for B, (below, _), cross in BOUNDARIES:
        out.append(Place("indels", "B%d_D" % B, 0, B - 100, "D", below))
    for B, back, below, cross in I_PLACES:
        out.append(Place("indels", "B%d_I" % B, 0, B - back, "I", below))
    lens = [n for _, n in contig_table()]
    for c in (1, 9, 10, N_SHORT):
        out.append(Place("short", "c%d_first" % c, c, 0, "M", 4681))
        s = lens[c] - L
        out.append(Place("short", "c%d_last" % c, c, s, "M", 585 if c == N_SHORT else low(s)))      # [16285, 16385) crosses 16384
    out.append(Place("short", "c2_inside", 2, 25, "M", 4681))
    out.append(Place("ties", "dup", 0, 50_000_000, "M", low(50_000_000)))
    return out


PLACES = _places()
N_DUP = 8
N_NOWHERE = 16


def bases(pac, pos, n):
    """n bases of the 2-bit reference from absolute position pos, as ASCII"""
    idx = pos + np.arange(n, dtype=np.int64)
    return np.frombuffer(b"ACGT", np.uint8)[(pac[idx >> 2] >> ((~idx & 3) << 1).astype(np.uint8)) & 3].tobytes()


def revcomp(s):
    return bytes(s[::-1]).translate(bytes.maketrans(b"ACGT", b"TGCA"))


def _indel_point(ref, lo):
    """the first offset q >= lo at which neither a 2-base deletion of ref[q:q+2] nor a 2-base insertion in front of ref[q] can slide by one
    or two bases without a mismatch"""
    for q in range(lo, lo + 30):
        if ref[q - 1] != ref[q + 1] and ref[q] != ref[q + 2] and ref[q - 2:q] != ref[q:q + 2] and ref[q:q + 2] != ref[q + 2:q + 4] and ref[q - 1] != ref[q]:
            return q
    raise AssertionError("no unambiguous indel point")


def plus_read(pac, offs, pl):
    """the bases of the plus-strand read of a place"""
    at = offs[pl.contig] + pl.start
    if pl.kind == "M":
        return bases(pac, at, L)
    ref = bases(pac, at, L + 8)
    if pl.kind == "D":
        q = _indel_point(ref, 50)
        return ref[:q] + ref[q + 2:L + 2]
    q = _indel_point(ref, 49)
    ins = bytes(next(c for c in b"ACGT" if c not in (ref[q - 1], ref[q])) for _ in range(2))
    return ref[:q] + ins + ref[q:L - 2]


def make_reads(pac, offs):
    """every read of the world in its file order (a seeded shuffle, so that no block is sorted and no class sits in one block)"""
    rng = np.random.default_rng(SEED + 1)
    reads = []
    for k, pl in enumerate(PLACES):
        fwd = plus_read(pac, offs, pl)
        assert len(fwd) == L
        for strand, seq in ((0, fwd), (1, revcomp(fwd))):
            for d in range(N_DUP if pl.cls == "ties" else 1):
                reads.append(Read(b"%s:%s:%s:%d" % (pl.cls.encode(), pl.label.encode(), b"-" if strand else b"+", d), seq, b"I" * L, k, strand))
    for d in range(N_NOWHERE):
        reads.append(Read(b"nowhere:%d" % d, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)), b"I" * L, None, 0))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def block_ranges(n):
    a, b = BLOCK_SIZES
    assert n > a + b
    return [(0, a), (a, a + b), (a + b, n)]


class World:
    """fa, contigs [(name, length)], offs (absolute contig offsets and the genome's length), reads, blocks [(lo, hi)]"""

    def __init__(self, workdir, build_index):
        import scale_check
        self.fa = os.path.join(str(workdir), "wide.fa")
        self.contigs = contig_table()
        self.offs = scale_check.write_contigs(self.fa, self.contigs, SEED)
        build_index(self.fa)
        pac = np.memmap(self.fa + ".gnumap.pac", np.uint8, "r")
        self.reads = make_reads(pac, self.offs)
        del pac
        self.blocks = block_ranges(len(self.reads))

    def fastq(self):
        return b"".join(b"@" + r.name + b"\n" + r.seq + b"\n+\n" + r.qual + b"\n" for r in self.reads)

    def block(self, k):
        lo, hi = self.blocks[k]
        return self.reads[lo:hi]


def oracle_records(world, orc, **kw):
    """OracleLib.read_output of every read: [(status, records)] in read order"""
    oix = orc.index_load(world.fa)
    op = orc.params(**dict(KW, **kw))
    return [orc.read_output(oix, op, orc.pwm(r.seq, r.qual), r.seq)[:2] for r in world.reads]


def self_check(world, orecs):
    """the world realises its classes: asserted from the oracle's records, never from the device's.  Returns {class: records}"""
    import bam_model as bm
    count, bins_seen, digits, ops = {}, set(), set(), {}
    for r, (st, recs) in zip(world.reads, orecs):
        if r.place is None:
            assert recs == [], (r.name, recs)
            count["nowhere"] = count.get("nowhere", 0) + 1
            continue
        pl = PLACES[r.place]
        assert len(recs) == 1, (r.name, st, recs)
        q = recs[0]
        assert (int(q["contig"]), int(q["chr_pos"]), int(q["strand"])) == (pl.contig, pl.start + 1, r.strand), (r.name, q)
        assert int(q["pos"]) == world.offs[pl.contig] + pl.start, (r.name, q)
        ref_len = sum(int(n) for n, o in bm._CIGAR.findall(q["cigar"]) if o in b"MD")
        assert ref_len == SPANS[pl.kind], (r.name, q["cigar"])
        if pl.kind != "M":
            assert pl.kind.encode() in q["cigar"], (r.name, q["cigar"])
            ops.setdefault(pl.kind, set()).add(r.strand)
        if pl.kind == "D":
            assert sum(int(n) for n, o in bm._CIGAR.findall(q["cigar"]) if o == b"I") == 2, (r.name, q["cigar"])
        assert bm.reg2bin(pl.start, pl.start + ref_len) == pl.bin, (r.name, q["cigar"], pl)
        bins_seen.add(pl.bin)
        digits.add(len(str(int(q["chr_pos"]))))
        count[pl.cls] = count.get(pl.cls, 0) + 1
    assert set(BIN_LITERALS) <= bins_seen, sorted(set(BIN_LITERALS) - bins_seen)
    assert ops == {"D": {0, 1}, "I": {0, 1}}, ops
    assert digits == set(range(1, 10)), digits
    assert count["nowhere"] == N_NOWHERE and count["ties"] == 2 * N_DUP
    return count
