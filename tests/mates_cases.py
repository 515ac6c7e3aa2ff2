"""Cases for the mate kernels alone (gm_dev_mate_resolve: k_mate_spans, k_mate_resolve, k_mate_fields on records of the caller's), generated
from seeds: nothing of them is committed.  The world of tests/mates_fixture.py gives every pair 1 x 1, 70 x 1 or 1 x 70 records; these cases
are the sizes, ties, products and limits no mapped block produces.  tests/test_gpu_mate_resolve.py runs them on the device,
tests/test_mate_cases_cpu.py checks them (and the model) without one.

A case is Case(name, recs, cigars, n_reads, lo, hi, rows, planted):
    recs      dicts in the shape tests/mates_model.py takes (read, contig, chr_pos, strand, post_prob), in record order
    cigars    one bytes per record
    rows      None (one row per record) or [("r", record) | ("u", read)]
    planted   what the case exists for, as the model's own answer.  Keys (all optional):
                pick    {pair: (a, b)}        the pair is proper with these primaries, as indices WITHIN the two mates' records
                single  {read: index | None}  the pair is not proper and this is the read's primary, as an index within its records
                proper  {pair: bool}
                span    [span of every record]
                field   {row: (flag, rnext, pnext, tlen)}
                stats   dict of counters
                lack100 the number of rows without 0x100
              self_check(case) asserts them from the model alone, before any device result is looked at.

The groups (the letters of the issue this file answers):
    A  trips and chunks: ca x cb records, every combination non-concordant (another contig, equal strands, insert below the limit or above
       it, mixed over the records) but one, planted at the lanes' and the LDS chunks' edges.  The planted records have the smallest
       posterior of their reads, so a resolver that falls back to the single choice answers differently
    B  ties: all combinations of one product; equal products from different factors (0.5 * 0.5 = 0.25 * 1.0, exact in fp32) placed so that
       the rule's winner is the one the kernel's order of work meets last; the single choice's ties and its last record
    C  one fp32 multiply: factor pairs found with numpy whose fp32 products are equal and whose exact products differ (fp32_ties).  The
       issue also asks for pairs whose ORDER in fp32 is the reverse of their order after a double multiply rounded once.  None exists: the
       double product of two fp32 values is exact (48 bits), so rounding it once IS the fp32 product, and rounding is monotone;
       fp32_reversals searches all the same and the CPU test asserts that it comes back empty.  What a product kept in double changes is
       the tie: the combination the rule prefers has the smaller exact product in half of the planted pairs.  The ties are planted
       between two lanes (two records of either mate) and inside one (fp32_ties_one_factor: one record against two).  Subnormal
       products too: a multiply that flushes them to zero turns two different products into a tie
    D  zeros and NaNs: the header's NaN rule
    E  concordance edges: inclusive limits, lo = 0, hi = 2^32 - 1 with 64-bit positions, equal POS, outward, equal strands, contig pairs
    F  spans of CIGARs
    G  ranges: reads without records, no records at all, the 256-record seam of k_mate_spans, 3000 small pairs (run capped and uncapped)
    H  fields: TLEN at 2^31 - 1 and 2^31, equal POS, another contig, a row source with reads without a record, secondary rows
"""
from collections import namedtuple

import numpy as np

import mates_model as mm

SEED = 97
Case = namedtuple("Case", "name recs cigars n_reads lo hi rows planted")
NAN = float("nan")
LO, HI = 1000, 5000                                     # the limits of the grouped pairs (A, B, C, D)


def rec(read, contig, pos, strand, post):
    return dict(read=int(read), contig=int(contig), chr_pos=int(pos), strand=int(strand), post_prob=np.float32(post))


# ---- grouped pairs: a record of group g is concordant with exactly the other mate's records of group g, one of group None with none ----
def grouped_pair(recs, cigars, pair, a_specs, b_specs):
    """a_specs / b_specs: [(post, group)] of the first / second mate's records.  Group g: contig 10 + g, the first mate on the plus strand
    at 1000 + i, the second on the minus strand at 3000 + j, 100M: inserts of 1500 .. 2700 for up to 600 records, inside [LO, HI].  A
    first mate's record without a group is, by i % 3, on contig 1, on the minus strand, or 100 .. 800 bases in front of the second mate's
    end (below LO); a second mate's on contig 2, on the plus strand, or at 50 000 + j (above HI).  No two defects cancel: contigs 1 and 2
    meet nothing, minus against plus is outward (3000 + j > 1000 + i), and the far record is far from both near ones"""
    for i, (post, g) in enumerate(a_specs):
        if g is not None:
            r = rec(2 * pair, 10 + g, 1000 + i, 0, post)
        else:
            r = (rec(2 * pair, 1, 1000 + i, 0, post), rec(2 * pair, 10, 1000 + i, 1, post), rec(2 * pair, 10, 2900 + i % 50, 0, post))[i % 3]
        recs.append(r); cigars.append(b"100M")
    for j, (post, g) in enumerate(b_specs):
        if g is not None:
            r = rec(2 * pair + 1, 10 + g, 3000 + j, 1, post)
        else:
            r = (rec(2 * pair + 1, 2, 3000 + j, 1, post), rec(2 * pair + 1, 10, 3000 + j, 0, post), rec(2 * pair + 1, 10, 50_000 + j, 1, post))[j % 3]
        recs.append(r); cigars.append(b"100M")


def grouped_case(name, pairs, planted):
    """pairs: [(a_specs, b_specs)]"""
    recs, cigars = [], []
    for i, (a, b) in enumerate(pairs):
        grouped_pair(recs, cigars, i, a, b)
    return Case(name, recs, cigars, 2 * len(pairs), LO, HI, None, planted)


# ---- A ----
SIZES_A = ((1, 1), (63, 1), (64, 64), (65, 1), (1, 257), (256, 256), (257, 255), (130, 600), (600, 130))
PLACES_A, PLACES_B = (0, 63, 64, 127, 128), (0, 255, 256, 511, 512)


def places(n, edges):
    return sorted({p for p in edges + (n - 1,) if p < n})


def cases_a():
    rng = np.random.default_rng(SEED)
    out = []
    for ca, cb in SIZES_A:
        for a in places(ca, PLACES_A):
            for b in places(cb, PLACES_B):
                pa = [(float(x), None) for x in rng.uniform(0.6, 1.0, ca)]
                pb = [(float(x), None) for x in rng.uniform(0.6, 1.0, cb)]
                pa[a], pb[b] = (0.5, 0), (0.5, 0)
                out.append(grouped_case("A_%dx%d_at_%d_%d" % (ca, cb, a, b), [(pa, pb)], dict(pick={0: (a, b)}, concordant={0: 1}, not_single=True)))
    return out


# ---- B ----
def cases_b():
    out = []
    for ca, cb in ((65, 257), (130, 300)):
        out.append(grouped_case("B_all_equal_%dx%d" % (ca, cb), [([(0.5, 0)] * ca, [(0.5, 0)] * cb)],
                                dict(pick={0: (0, 0)}, concordant={0: ca * cb}, lack100=2)))
    # (winner, loser, ca, cb): both products are 0.25; the loser is what a kernel that takes the first it meets, or the last, would answer
    for (wa, wb), (la, lb), ca, cb in (((3, 599), (70, 300), 71, 600), ((3, 2), (3, 599), 71, 600), ((5, 500), (67, 0), 68, 501), ((1, 256), (64, 0), 65, 257)):
        pa, pb = [(0.9, None)] * ca, [(0.9, None)] * cb
        if wa == la:                                    # one record of the first mate: the two second mates' posteriors are equal
            pa[wa] = (0.5, 0); pb[wb] = (0.5, 0); pb[lb] = (0.5, 0)
        else:
            pa[wa], pb[wb] = ((0.5, 0), (0.5, 0)) if wa > 2 else ((0.25, 0), (1.0, 0))
            pa[la], pb[lb] = ((0.25, 1), (1.0, 1)) if wa > 2 else ((0.5, 1), (0.5, 1))
        out.append(grouped_case("B_tie_%d_%d_over_%d_%d" % (wa, wb, la, lb), [(pa, pb)], dict(pick={0: (wa, wb)}, concordant={0: 2}, tie={0: ((wa, wb), (la, lb))})))
    # the single choice (no combination is concordant): the maximum at 70 and at 5; the maximum only at the last record
    pa = [(0.1, None)] * 100; pa[70] = pa[5] = (0.9, None)
    pb = [(0.2, None)] * 130; pb[129] = pb[64] = (0.8, None)
    out.append(grouped_case("B_single_tie_70_and_5", [(pa, pb)], dict(single={0: 5, 1: 64}, proper={0: False})))
    for cnt in (64, 65, 130, 600):
        pa = [(0.1, None)] * cnt; pa[cnt - 1] = (0.9, None)
        pb = [(0.3, None)] * cnt; pb[cnt - 1] = (0.7, None)
        out.append(grouped_case("B_single_last_of_%d" % cnt, [(pa, pb)], dict(single={0: cnt - 1, 1: cnt - 1}, proper={0: False})))
    return out


# ---- C ----
def fp32_products(n=400_000, seed=SEED + 1):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 1.0, n).astype(np.float32); y = rng.uniform(0.5, 1.0, n).astype(np.float32)
    return x, y, x * y, x.astype(np.float64) * y.astype(np.float64)       # the fp32 product; the exact one (48 bits fit a double)


def fp32_ties(want=8):
    """[(x1, y1, x2, y2)]: x1 * y1 == x2 * y2 in fp32, x1 * y1 < x2 * y2 exactly"""
    x, y, p32, p64 = fp32_products()
    order = np.argsort(p32, kind="stable")
    out = []
    for i, j in zip(order, order[1:]):
        if p32[i] == p32[j] and p64[i] != p64[j]:
            lo, hi = (i, j) if p64[i] < p64[j] else (j, i)
            out.append((x[lo], y[lo], x[hi], y[hi]))
            if len(out) == want:
                break
    return out


def fp32_ties_one_factor(want=8, seed=SEED + 3):
    """[(x, y1, y2)]: y2 the fp32 value behind y1, and x * y1 == x * y2 in fp32 (exactly, x * y1 < x * y2): a tie between two records of
    the second mate against ONE record of the first, which one lane of k_mate_resolve decides on its own"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 0.75, 4000).astype(np.float32); y1 = rng.uniform(0.5, 1.0, 4000).astype(np.float32)
    y2 = np.nextafter(y1, np.float32(2))
    hit = np.nonzero((x * y1 == x * y2) & (y2 < 1))[0][:want]
    return [(x[k], y1[k], y2[k]) for k in hit]


def fp32_reversals():
    """[(i, j)] with p32[i] < p32[j] and the double product, rounded once to fp32, of i above that of j.  Always empty (see the module's text)"""
    x, y, p32, p64 = fp32_products()
    once = p64.astype(np.float32)
    order = np.argsort(p32, kind="stable")
    bad = np.nonzero(np.diff(once[order].astype(np.float64)) < 0)[0]
    return [(int(order[k]), int(order[k + 1])) for k in bad] + [int(k) for k in np.nonzero(once != p32)[0]]


def cases_c():
    ties = fp32_ties()
    pairs, pick = [], {}
    for k, (x1, y1, x2, y2) in enumerate(ties):
        # even k: the exactly larger product second, odd k: first.  Either way the tie in fp32 goes to (0, 0)
        (xa, ya), (xb, yb) = ((x1, y1), (x2, y2)) if k % 2 == 0 else ((x2, y2), (x1, y1))
        pairs.append(([(xa, 0), (xb, 1)], [(ya, 0), (yb, 1)])); pick[k] = (0, 0)
    out = [grouped_case("C_equal_in_fp32", pairs, dict(pick=pick, found=len(ties)))]
    one = fp32_ties_one_factor()
    pairs, pick = [], {}
    for k, (x, y1, y2) in enumerate(one):               # even k: the exactly larger product second, odd k: first
        pairs.append(([(x, 0)], [(y1, 0), (y2, 0)] if k % 2 == 0 else [(y2, 0), (y1, 0)])); pick[k] = (0, 0)
    out.append(grouped_case("C_equal_in_fp32_in_one_lane", pairs, dict(pick=pick, found_one=len(one))))
    # subnormal products: 1e-20 * 1e-20 and 2e-20 * 1e-20 are different numbers below 2^-126, and the larger comes second
    t = np.float32(1e-20)
    assert 0 < t * t < np.float32(2) * t * t < np.finfo(np.float32).tiny
    out.append(grouped_case("C_subnormal_products", [([(t, 0), (2 * t, 1)], [(t, 0), (t, 1)]), ([(2 * t, 0), (t, 1)], [(t, 0), (t, 1)])], dict(pick={0: (1, 1), 1: (0, 0)})))
    return out


# ---- D ----
def cases_d():
    out = [grouped_case("D_zero_product_is_proper", [([(0.0, 0), (0.9, None)], [(0.7, 0), (0.9, None)])], dict(pick={0: (0, 0)}, proper={0: True}))]
    pairs = [([(NAN, 0), (0.3, 1)], [(0.5, 0), (1.0, 1)]),          # the NaN product first, another lane has the number
             ([(0.0, 0), (NAN, 1)], [(0.5, 0), (1.0, 1)]),          # the number (a zero) first
             ([(0.5, 0)], [(NAN, 0), (0.2, 0)]),                    # one lane: NaN, then a number
             ([(0.5, 0)], [(0.2, 0), (NAN, 0)]),
             ([(0.5, 0)] * 66, [(NAN, 0)] * 300 + [(0.0, 0)])]      # every lane of two trips keeps NaNs until the last record of chunk 1
    out.append(grouped_case("D_nan_product_against_a_number", pairs, dict(pick={0: (1, 1), 1: (0, 0), 2: (0, 1), 3: (0, 0), 4: (0, 300)}, proper={i: True for i in range(5)})))
    pairs = [([(NAN, 0)], [(0.5, 0)]),
             ([(0.4, None), (NAN, 0), (NAN, 1)], [(0.9, None), (0.5, 1), (0.5, 0)]),               # (1, 2) and (2, 1): the first in (a, b) order
             ([(NAN, 0)] * 70, [(0.5, 0)] * 300),
             ([(0.5, None)] * 3 + [(NAN, 0)] * 67, [(0.5, None)] * 258 + [(NAN, 0)] * 2)]
    out.append(grouped_case("D_all_nan_products_are_proper", pairs, dict(pick={0: (0, 0), 1: (1, 2), 2: (0, 0), 3: (3, 258)}, proper={i: True for i in range(4)})))
    issue = [0.1, NAN] + [0.1] * 63 + [0.9]
    assert len(issue) == 66 and issue[65] == 0.9
    singles = [(issue, 65), ([NAN, 0.9], 1), ([NAN] * 70, 0), ([0.9, NAN], 0), ([NAN] * 64 + [0.2, NAN], 64), ([NAN, -1.0], 1), ([NAN, 0.0, NAN, 0.0], 1),
               ([NAN] * 129 + [0.1], 129)]
    pairs, single = [], {}
    for k in range(0, len(singles), 2):
        (pa, wa), (pb, wb) = singles[k], singles[k + 1]
        pairs.append(([(p, None) for p in pa], [(p, None) for p in pb])); single[k] = wa; single[k + 1] = wb
    out.append(grouped_case("D_nan_singles", pairs, dict(single=single, proper={i: False for i in range(len(pairs))})))
    return out


# ---- E ----
def plain_case(name, pairs, lo, hi, planted, rows=None):
    """pairs: [([(contig, pos, strand, post, cigar)], [...])]"""
    recs, cigars = [], []
    for i, (a, b) in enumerate(pairs):
        for rd, side in ((2 * i, a), (2 * i + 1, b)):
            for c, pos, s, post, cg in side:
                recs.append(rec(rd, c, pos, s, post)); cigars.append(cg)
    return Case(name, recs, cigars, 2 * len(pairs), lo, hi, rows, planted)


def fr(ins, pos=1000, first_minus=False, contig=0):
    """a forward/reverse 1 x 1 pair of two 100M records with the given insert"""
    f, r = [(contig, pos, 0, 0.5, b"100M")], [(contig, pos + ins - 100, 1, 0.5, b"100M")]
    return (r, f) if first_minus else (f, r)


def cases_e():
    out = []
    ins = (119, 120, 500, 501)
    out.append(plain_case("E_limits_are_inclusive", [fr(i, first_minus=m) for i in ins for m in (False, True)], 120, 500,
                          dict(proper={2 * k + m: i in (120, 500) for k, i in enumerate(ins) for m in (0, 1)})))
    # lo = 0: the smallest insert there is is 1 (equal POS, a minus mate that spans one base)
    one = ([(0, 700, 0, 0.5, b"100M")], [(0, 700, 1, 0.5, b"1M")])
    star = ([(0, 700, 0, 0.5, b"100M")], [(0, 700, 1, 0.5, b"*")])
    two = ([(0, 700, 0, 0.5, b"100M")], [(0, 701, 1, 0.5, b"1M")])
    out.append(plain_case("E_lo_0", [one, star, two, fr(100)], 0, 1, dict(proper={0: True, 1: True, 2: False, 3: False})))
    out.append(plain_case("E_lo_0_hi_0", [one, two], 0, 0, dict(proper={0: False, 1: False})))
    # hi = 2^32 - 1 with 64-bit positions: 5 * 10^9 + 99 is an insert above it, and its low 32 bits would be one below it
    top = 0xFFFFFFFF
    far = ([(0, 1, 0, 0.5, b"100M")], [(0, 5_000_000_000, 1, 0.5, b"100M")])
    out.append(plain_case("E_hi_is_2_32_minus_1", [far, (far[1], far[0]), fr(top, pos=1), fr(top + 1, pos=1), fr(top, pos=1, first_minus=True)], 0, top,
                          dict(proper={0: False, 1: False, 2: True, 3: False, 4: True})))
    eq = ([(0, 900, 0, 0.5, b"100M")], [(0, 900, 1, 0.5, b"100M")])
    outward = ([(0, 901, 0, 0.5, b"100M")], [(0, 900, 1, 0.5, b"100M")])
    plus2 = ([(0, 900, 0, 0.5, b"100M")], [(0, 1000, 0, 0.5, b"100M")])
    minus2 = ([(0, 900, 1, 0.5, b"100M")], [(0, 1000, 1, 0.5, b"100M")])
    out.append(plain_case("E_equal_pos_outward_equal_strands", [eq, (eq[1], eq[0]), outward, (outward[1], outward[0]), plus2, minus2], 50, 500,
                          dict(proper={0: True, 1: True, 2: False, 3: False, 4: False, 5: False})))
    pairs, proper = [], {}
    for ca, cb in ((0, 1), (2, 3), (1, 1), (1, 0), (3, 2)):
        for sa in (0, 1):
            for sb in (0, 1):
                proper[len(pairs)] = ca == cb and sa != sb
                pairs.append(([(ca, 900, sa, 0.5, b"100M")], [(cb, 900, sb, 0.5, b"100M")]))
    out.append(plain_case("E_contig_pairs_and_strands", pairs, 50, 500, dict(proper=proper)))
    return out


# ---- F ----
def cases_f():
    long_cigar = b"".join(b"%dM%dI" % (1 + k % 3, 1 + k % 2) for k in range(199)) + b"3D7M"        # 400 tokens
    assert len(mm._TOKEN.findall(long_cigar)) == 400
    table = ((b"*", 1), (b"100M", 100), (b"50M2D48M", 100), (b"10S90M", 90), (b"40M3I57M", 97), (b"1M", 1), (b"65535M", 65535),
             (long_cigar, sum(1 + k % 3 for k in range(199)) + 10), (b"5S20I3S", 1), (b"100I", 1))
    pairs = []
    for k in range(0, len(table), 2):                   # forward/reverse pairs, so that the spans reach the inserts and the TLENs too
        pairs.append(([(0, 1000, 0, 0.5, table[k][0])], [(0, 1200, 1, 0.5, table[k + 1][0])]))
    return [plain_case("F_spans", pairs, 100, 300, dict(span=[s for _, s in table], proper={0: True, 1: True, 2: True, 3: False, 4: True}))]


# ---- G ----
def cases_g():
    out = []
    have = (2, 3, 5, 8, 9)                              # of 12 reads: none at the start (0, 1), in the middle (4, 6, 7), at the end (10, 11)
    recs = [rec(r, 0, 1000 + 200 * (r & 1), r & 1, 0.5) for r in have]
    out.append(Case("G_reads_without_records", recs, [b"100M"] * len(recs), 12, 100, 500, None,
                    dict(stats=dict(pairs=6, both_mapped=2, proper=2, one_mapped=1, none_mapped=3), single={5: 0, 4: None, 0: None, 11: None})))
    every = [("u", r) for r in range(6)]
    out.append(Case("G_no_records", [], [], 6, 100, 500, None, dict(stats=dict(pairs=3, both_mapped=0, proper=0, one_mapped=0, none_mapped=3))))
    out.append(Case("G_no_records_unmapped_rows", [], [], 6, 100, 500, every,
                    dict(stats=dict(pairs=3, both_mapped=0, proper=0, one_mapped=0, none_mapped=3), field={0: (0x4D, -1, 0, 0), 5: (0x8D, -1, 0, 0)})))
    out.append(Case("G_no_reads", [], [], 0, 100, 500, None, dict(stats=dict(pairs=0, both_mapped=0, proper=0, one_mapped=0, none_mapped=0))))
    # the 256-record seam of k_mate_spans: ranges that end at it, begin at it and straddle it (256, and again 512)
    counts = (250, 6, 3, 1, 248, 8, 1, 1)               # reads 0 .. 7: [0, 250) [250, 256) [256, 259) [259, 260) [260, 508) [508, 516) ...
    pairs = []
    for i in range(0, len(counts), 2):
        ca, cb = counts[i], counts[i + 1]
        pa, pb = [(0.9, None)] * ca, [(0.9, None)] * cb
        pa[ca - 1], pb[cb - 1] = (0.5, 0), (0.5, 0)
        pairs.append((pa, pb))
    c = grouped_case("G_ranges_at_the_seam_of_256_records", pairs, dict(pick={i: (counts[2 * i] - 1, counts[2 * i + 1] - 1) for i in range(4)}))
    assert [r["read"] for r in c.recs][255:257] == [1, 2] and c.recs[511]["read"] == c.recs[512]["read"] == 5
    out.append(c)
    rng = np.random.default_rng(SEED + 2)
    recs, cigars = [], []
    for i in range(3000):
        ins = int(rng.integers(80, 560))
        for rd, strand, pos in ((2 * i, 0, 1000 + i), (2 * i + 1, 1, 1000 + i + ins - 100)):
            for _ in range(int(rng.integers(1, 3))):
                recs.append(rec(rd, int(rng.integers(0, 2)), pos + int(rng.integers(0, 3)), strand ^ int(rng.integers(0, 8) == 0), rng.choice([0.25, 0.5, 1.0])))
                cigars.append(b"100M")
    out.append(Case("G_3000_pairs", recs, cigars, 6000, 100, 500, None, dict(many=True)))
    return out


# ---- H ----
def cases_h():
    out = []
    top = 2 ** 31 - 1
    big = lambda v, first_minus: (([(0, 1, 0, 0.5, b"100M")], [(0, v - 99, 1, 0.5, b"100M")])[::-1] if first_minus else ([(0, 1, 0, 0.5, b"100M")], [(0, v - 99, 1, 0.5, b"100M")]))
    out.append(plain_case("H_tlen_at_2_31", [big(top, False), big(top, True), big(top + 1, False), big(top + 1, True)], 0, 0xFFFFFFFF,
                          dict(field={0: (0x63, 0, top - 99, top), 1: (0x93, 0, 1, -top), 2: (0x53, 0, 1, -top), 3: (0xA3, 0, top - 99, top),
                                      4: (0x63, 0, top - 98, 0), 5: (0x93, 0, 1, 0), 6: (0x53, 0, 1, 0), 7: (0xA3, 0, top - 98, 0)})))
    eq = ([(3, 900, 0, 0.5, b"100M")], [(3, 900, 1, 0.5, b"125M")])
    other = ([(3, 900, 0, 0.5, b"100M")], [(7, 5000, 1, 0.5, b"100M")])
    out.append(plain_case("H_equal_pos_and_another_contig", [eq, (eq[1], eq[0]), other], 100, 500,
                          dict(field={0: (0x63, 3, 900, 125), 1: (0x93, 3, 900, -125), 2: (0x53, 3, 900, 125), 3: (0xA3, 3, 900, -125),
                                      4: (0x61, 7, 5000, 0), 5: (0x91, 3, 900, 0)})))
    # secondary rows, and a row source that mixes records with reads that have none: reads 0 (three records) and 1 (two) are a proper pair
    # through their second records; read 2 has none and read 3 one on the minus strand; reads 4 and 5 have none
    recs = [rec(0, 0, 5000, 0, 0.9), rec(0, 0, 1000, 0, 0.5), rec(0, 1, 1000, 0, 0.9), rec(1, 1, 9000, 1, 0.9), rec(1, 0, 1200, 1, 0.5), rec(3, 2, 777, 1, 0.5)]
    rows = [("r", 0), ("r", 1), ("r", 2), ("r", 3), ("r", 4), ("u", 2), ("r", 5), ("u", 4), ("u", 5)]
    out.append(Case("H_row_source_and_secondary_rows", recs, [b"100M"] * 6, 6, 100, 500, rows,
                    dict(pick={0: (1, 1)}, lack100=6,             # (the three secondary rows have it)
                         field={0: (0x161, 0, 1200, 0), 1: (0x63, 0, 1200, 300), 2: (0x161, 0, 1200, 0), 3: (0x191, 0, 1000, 0), 4: (0x93, 0, 1000, -300),
                                5: (0x65, 2, 777, 0), 6: (0x99, -1, 0, 0), 7: (0x4D, -1, 0, 0), 8: (0x8D, -1, 0, 0)})))
    out.append(Case("H_rows_in_another_order", recs, [b"100M"] * 6, 6, 100, 500, rows[::-1], dict(field={8: (0x161, 0, 1200, 0), 0: (0x8D, -1, 0, 0), 3: (0x65, 2, 777, 0)})))
    return out


_CASES = None


def cases():
    """every case, built once"""
    global _CASES
    if _CASES is None:
        _CASES = cases_a() + cases_b() + cases_c() + cases_d() + cases_e() + cases_f() + cases_g() + cases_h()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


_MODEL = {}


def model(case):
    """the model's answer for a case, computed once and never changed: dict(span, prim, proper, fields, stats, ranges)"""
    if case.name not in _MODEL:
        res = mm.resolve(case.recs, case.cigars, case.n_reads, case.lo, case.hi)
        _MODEL[case.name] = dict(span=[mm.span(c) for c in case.cigars], prim=res[0], proper=res[1],
                                 fields=mm.row_fields(case.recs, case.cigars, case.n_reads, case.lo, case.hi, case.rows, resolved=res),
                                 stats=mm.stats(case.recs, case.cigars, case.n_reads, case.lo, case.hi, resolved=res),
                                 ranges=mm._ranges(case.recs, case.n_reads))
    return _MODEL[case.name]


def check_planted(case, prim, proper, span, fields, stats):
    """`planted` against an answer in the model's shapes (the model's own in self_check, the device's in the GPU test)"""
    p, rng = case.planted, mm._ranges(case.recs, case.n_reads)
    for pair, (a, b) in p.get("pick", {}).items():
        assert proper[pair] and (prim[2 * pair] - rng[2 * pair][0], prim[2 * pair + 1] - rng[2 * pair + 1][0]) == (a, b), (case.name, pair, prim[2 * pair], prim[2 * pair + 1])
    for read, at in p.get("single", {}).items():
        assert not proper[read >> 1] and (prim[read] is None if at is None else prim[read] - rng[read][0] == at), (case.name, read, prim[read])
    for pair, want in p.get("proper", {}).items():
        assert bool(proper[pair]) == want, (case.name, pair)
    if "span" in p:
        assert list(span) == p["span"], case.name
    for row, want in p.get("field", {}).items():
        assert tuple(fields[row]) == want, (case.name, row, fields[row], want)
    if "stats" in p:
        assert stats == p["stats"], (case.name, stats)
    if "lack100" in p:
        assert sum(not f[0] & 0x100 for f in fields) == p["lack100"], case.name


def self_check(case):
    """the case holds what it was built for: asserted from the model alone"""
    m = model(case)
    p = case.planted
    check_planted(case, m["prim"], m["proper"], m["span"], m["fields"], m["stats"])
    rng, sp = m["ranges"], m["span"]
    for pair, want in p.get("concordant", {}).items():
        n = sum(mm.concordant(case.recs[a], sp[a], case.recs[b], sp[b], case.lo, case.hi) for a in rng[2 * pair] for b in rng[2 * pair + 1])
        assert n == want, (case.name, pair, n)
    if p.get("not_single"):                             # the planted records are not what the single choice takes
        lone, _ = mm.resolve(case.recs, case.cigars, case.n_reads, 0, 0)
        assert len(case.recs) == 2 or (lone[0], lone[1]) != (m["prim"][0], m["prim"][1]), case.name
        if len(rng[0]) > 1:
            assert lone[0] != m["prim"][0], case.name
        if len(rng[1]) > 1:
            assert lone[1] != m["prim"][1], case.name
    for pair, ((wa, wb), (la, lb)) in p.get("tie", {}).items():
        post = lambda rd, k: case.recs[rng[rd][0] + k]["post_prob"]
        assert post(0, wa) * post(1, wb) == post(0, la) * post(1, lb) == np.float32(0.25), case.name
    if "found" in p:
        assert p["found"] >= 4, "the search found too few fp32 ties"
        for pair in range(p["found"]):
            a0, a1 = (case.recs[k]["post_prob"] for k in rng[2 * pair]); b0, b1 = (case.recs[k]["post_prob"] for k in rng[2 * pair + 1])
            assert a0 * b0 == a1 * b1 and type(a0 * b0) is np.float32
            exact = (float(a0) * float(b0), float(a1) * float(b1))
            assert (exact[0] < exact[1]) == (pair % 2 == 0) and exact[0] != exact[1], (case.name, pair)
    if "found_one" in p:
        assert p["found_one"] >= 4, "the search found too few fp32 ties"
        for pair in range(p["found_one"]):
            x = case.recs[rng[2 * pair][0]]["post_prob"]; y0, y1 = (case.recs[k]["post_prob"] for k in rng[2 * pair + 1])
            assert x * y0 == x * y1 and type(x * y0) is np.float32 and (float(x) * float(y0) < float(x) * float(y1)) == (pair % 2 == 0) and y0 != y1
    if p.get("many"):
        st = m["stats"]
        assert st["pairs"] == 3000 and 500 < st["proper"] < 2900 and len(case.recs) > 8000
        assert any(f[0] & 0x100 for f in m["fields"])


def pack(case):
    """a case as gm_dev_mate_resolve takes it: (records SAM_DTYPE, the CIGAR pool, the row source or None)"""
    from gnumap_amd import api
    recs = np.zeros(len(case.recs), api.SAM_DTYPE)
    pool, at = bytearray(), {}
    for k, (r, cg) in enumerate(zip(case.recs, case.cigars)):
        if cg not in at:
            at[cg] = len(pool); pool += cg + b"\0"
        for f in ("read", "contig", "chr_pos", "strand", "post_prob"):
            recs[k][f] = r[f]
        recs[k]["pos"] = r["chr_pos"]; recs[k]["cigar_off"] = at[cg]
    src = None if case.rows is None else np.array([k if kind == "r" else api.ROW_UNMAPPED | k for kind, k in case.rows], np.uint64)
    return recs, bytes(pool), src
