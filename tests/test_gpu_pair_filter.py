"""k_vote_pair's filter marks and record loads (gnumap_amd/csrc/gm_pair.hip) on reads built for them, in its three instantiations, against the
ORACLE read by read (_compare of test_gpu_parity.py: status, score bits, denominator, position sets with strand) and against
GM_VOTE_PAIR=0 for raw-hit equality (position, strand, NW step, score of every accepted candidate).

A hit marks two bits of its filter word: bit (b & 31) and bit ((b >> 14) & 31) of the word chosen by bits 5 .. 13 of its window start b.  The
reference below is 1.2 Mbp of seeded random sequence with copies of single 10-mers of the reads PLANTED so that a stray hit's window start
  1a / 1b  agrees with the true window start mod 2^14 and differs in bits 14 .. 18 (no longer listed), the stray seed being the strand's
           first (it arrives with the true window's first marks) / its last (it arrives when all of them are set),
  2        agrees with it mod 2^19 and differs above (equal marks: listed, and the sweep has to find its single vote),
  3        is shared by two seeds (a real second candidate) while a third, single-vote stray agrees with both mod 2^14,
  4a / 4b  has (b & 31) == ((b >> 14) & 31), a mark of ONE bit: as the true window / as a stray whose one bit is among the true window's,
  5        lies below 2^14 (the true window: its second mark is bit 0),
every one as a forward and as a reverse-complemented read.  The blocks hold an odd number of reads in more than 16 pairs (a half-empty last
pair, two workgroups), and run with both strands and with either switched off.  Case 8: a read one of whose 10-mers occurs more than 28
times (its record keeps rank and count where the others keep nothing, and the read is flagged) shares a pair with a kept read - first
and second of the pair; lane 0 of a record holds its header word, which must not vote in anybody's quarter.

Nothing here can hide behind k_vote_bucket: kept() restates on the CPU, from the reference text alone, the conditions under which
k_vote_pair keeps a read, every read of the kept blocks is asserted to meet them, and gm_batch_pair_flagged has to say 0 (case 8: exactly
the engineered reads)."""
import numpy as np
import pytest

import gnumap_amd as g
from reflib import revcomp_str
from test_gpu_edge_reads import BUCKET, run
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

MER = 10
N_REF = 1_200_000
EARLY = 4096                       # a record with a position below this is flagged (GMB_EARLY)
# instantiation -> (read length, jump): seeds per strand at i = 0, jump, .. < L - MER: 6 (<= 8), 13 (<= 14), 15
GROUPS = {"4": (50, 7), "7": (100, 7), "8": (100, 6)}
CONFIGS = {
    "base": {},
    "all": dict(align_score=-1e6, align_is_fraction=0),          # every candidate is accepted: the candidate positions themselves are compared
    "no_nw": dict(nw=0),
    "up": dict(neg_strand=0),
    "down": dict(pos_strand=0),
}


def seed_offsets(L, jump):
    return list(range(0, L - MER, jump))


class Ref:
    """the reference under construction: loci of reads and planted 10-mers claim their bases (with a margin of MER + 2 either side, so that
    no planted copy changes a 10-mer of a read or of another copy)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.G = np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, N_REF)].copy()
        self.G[:EARLY + MER + 4] = ord("A")           # every 10-mer that starts below EARLY is poly-A: no read holds it (kept() would say so)
        self.used = np.zeros(N_REF, bool)
        self.used[:EARLY + 200] = True
        self.used[N_REF - 200:] = True

    def free(self, lo, hi):
        return 0 <= lo - MER - 2 and hi + MER + 2 <= N_REF and not self.used[lo - MER - 2:hi + MER + 2].any()

    def claim(self, lo, hi):
        assert self.free(lo, hi), (lo, hi)
        self.used[lo:hi] = True

    def seq(self, lo, hi):
        return self.G[lo:hi].tobytes()

    def plant(self, pos, kmer):
        self.claim(pos, pos + MER)
        self.G[pos:pos + MER] = np.frombuffer(kmer, np.uint8)

    def find(self, L, ok=lambda T: True, lo=EARLY + 300, hi=N_REF - 300):
        """a free stretch of L bases at a random place in [lo, hi) for which ok(T) holds (the window starts of its strays are free, ..)"""
        for _ in range(100000):
            T = int(self.rng.integers(lo, hi - L))
            if self.free(T, T + L) and ok(T):
                return T
        raise AssertionError("no free stretch")

    def pick(self, L, ok=lambda T: True, **kw):
        T = self.find(L, ok, **kw)
        self.claim(T, T + L)
        return T


def mask_of(b):
    return (1 << (b & 31)) | (1 << ((b >> 14) & 31))


def build_group(R, tag):
    """the engineered loci of one instantiation, {name: where its read is cut}; every stray is planted on the way"""
    L, jump = GROUPS[tag]
    offs = seed_offsets(L, jump)
    last = offs[-1]
    loci, info = {}, {}

    def stray(T, i, W):                               # a copy of the read's 10-mer at offset i, so that its window start is W
        R.plant(W + i, R.seq(T + i, T + i + MER))

    def can(W, i):
        return R.free(W + i, W + i + MER)

    two_bits = lambda b: bin(mask_of(b)).count("1") == 2
    # 1a / 1b: same word, same first bit, another second bit (which is not the first bit either: that would be case 4b)
    for name, i, d in (("c1a", 0, 3), ("c1b", last, 5)):
        ok = lambda T, i=i, d=d: two_bits(T) and can(T + d * 2 ** 14, i) and mask_of(T + d * 2 ** 14) & ~mask_of(T) and two_bits(T + d * 2 ** 14)
        T = R.pick(L, ok, hi=N_REF - 6 * 2 ** 14)
        stray(T, i, T + d * 2 ** 14)
        assert (T + d * 2 ** 14) % 2 ** 14 == T % 2 ** 14 and mask_of(T + d * 2 ** 14) != mask_of(T)
        loci[name] = T
    # 2: equal marks
    T = R.pick(L, lambda T: two_bits(T) and can(T + 2 ** 19, offs[1]), hi=N_REF - 2 ** 19 - 300)
    stray(T, offs[1], T + 2 ** 19)
    assert mask_of(T + 2 ** 19) == mask_of(T) and (T + 2 ** 19) % 2 ** 14 == T % 2 ** 14
    loci["c2"] = T
    # 3: seeds 1 and 5 at one window start W2 (a whole free window: both copies lie in it), seed 3 at W2 + 2 x 2^14
    T = R.pick(L)
    W2 = R.find(L, lambda W: can(W + 2 * 2 ** 14, offs[3]) and two_bits(W), hi=N_REF - 3 * 2 ** 14)
    stray(T, offs[1], W2); stray(T, offs[5], W2); stray(T, offs[3], W2 + 2 * 2 ** 14)
    loci["c3"] = T; info["c3_second"] = W2
    # 4a: the true window's mark is one bit; a stray of the same word and first bit with a second bit of its own
    T = R.pick(L, lambda T: not two_bits(T) and can(T + 7 * 2 ** 14, offs[2]), hi=N_REF - 8 * 2 ** 14)
    stray(T, offs[2], T + 7 * 2 ** 14)
    loci["c4a"] = T
    # 4b: a stray of the last seed whose one bit is the true window's first bit
    def w4b(T):
        a, h0 = T & 31, T >> 14
        return [(T & 16383) + (h << 14) for h in (a, a + 32, a + 64) if h != h0 and (T & 16383) + (h << 14) < N_REF - 400]
    T = R.pick(L, lambda T: two_bits(T) and any(can(W, last) for W in w4b(T)))
    W = [W for W in w4b(T) if can(W, last)][0]
    assert not two_bits(W) and mask_of(W) & mask_of(T) == mask_of(W) and W % 2 ** 14 == T % 2 ** 14 and W != T
    stray(T, last, W)
    loci["c4b"] = T
    # 5: the true window below 2^14; a stray of the same word and first bit further up
    T = R.pick(L, lambda T: (T & 31) != 0 and can(T + 4 * 2 ** 14, offs[2]), lo=EARLY + 300, hi=2 ** 14 - 200)
    stray(T, offs[2], T + 4 * 2 ** 14)
    assert mask_of(T) == (1 << (T & 31)) | 1
    loci["c5"] = T
    # 8: one 10-mer (seed 2) in 30 more places: a record beyond its 28 inline positions
    T = R.pick(L)
    K = R.seq(T + offs[2], T + offs[2] + MER)
    for _ in range(30):
        R.plant(R.find(MER), K)
    loci["c8"] = T
    return loci, info


class KmerIndex:
    """every 10-mer of the finished reference by code, as the bucket table holds them"""

    def __init__(self, G):
        two = np.zeros(256, np.uint32)
        for k, ch in enumerate(b"ACGT"):
            two[ch] = k
        v = two[G]
        codes = np.zeros(len(G) - MER + 1, np.uint32)
        for t in range(MER):
            codes = (codes << np.uint32(2)) | v[t:len(G) - MER + 1 + t]
        self.order = np.argsort(codes, kind="stable")
        self.sorted = codes[self.order]
        self.two = two

    def positions(self, kmer):
        c = np.uint32(0)
        for ch in kmer:
            c = (c << np.uint32(2)) | self.two[ch]
        a, b = np.searchsorted(self.sorted, c, "left"), np.searchsorted(self.sorted, c, "right")
        return self.order[a:b]


def kept(kx, seq, jump):
    """None when k_vote_pair keeps the read (the head of gm_pair.hip), else why not.  The listed keys are bounded from above by the hits
    beyond the first of each 2^14 class - what a filter of one bit per class would list, whatever marks are in use."""
    if set(seq) - set(b"ACGT"):
        return "a base that is not ACGT"
    for strand, t in enumerate((seq, revcomp_str(seq).upper())):
        starts = []
        for i in seed_offsets(len(t), jump):
            pos = kx.positions(t[i:i + MER])
            if not 1 <= len(pos) <= 28:
                return f"strand {strand} seed at {i}: {len(pos)} hits"
            if pos.min() < EARLY:
                return f"strand {strand} seed at {i}: an early position"
            starts += [int(p) - i for p in pos]
        if len(starts) > 384:
            return f"strand {strand}: {len(starts)} hits"
        if len(starts) - len({s % 2 ** 14 for s in starts}) > 16:
            return f"strand {strand}: more than 16 listed keys"
    return None


class World:
    def __init__(self):
        R = Ref(20250)
        self.loci = {}; self.info = {}
        for tag in GROUPS:
            self.loci[tag], self.info[tag] = build_group(R, tag)
        fill = {tag: [R.pick(GROUPS[tag][0]) for _ in range(30)] for tag in GROUPS}
        # a read is kept only when the 10-mers of BOTH its strands occur: those of the strand that is not in the reference get one copy each,
        # scattered (a locus read forwards and read reverse-complemented ask for the same ones)
        for tag, (L, jump) in GROUPS.items():
            for T in list(self.loci[tag].values()) + fill[tag]:
                t = revcomp_str(R.seq(T, T + L)).upper()
                for i in seed_offsets(L, jump):
                    R.plant(R.find(MER), t[i:i + MER])
        self.G = R.G
        kx = KmerIndex(R.G)
        self.blocks = {}
        for tag, (L, jump) in GROUPS.items():
            def two(name, T):
                s = R.seq(T, T + L)
                return [(f"{name}_{tag}_f", s, b"I" * L), (f"{name}_{tag}_r", revcomp_str(s).upper(), b"I" * L)]
            eng = [r for name, T in self.loci[tag].items() if name != "c8" for r in two(name, T)]
            flagged = two("c8", self.loci[tag]["c8"])
            fillers = [r for k, T in enumerate(fill[tag]) for r in two(f"fill{k}", T)[k & 1:][:1]]
            fillers = [r for r in fillers if kept(kx, r[1], jump) is None]
            keep = eng + fillers[:33 - len(eng)]
            # the precondition: every read of the kept block meets k_vote_pair's conditions, the two of case 8 fail exactly the inline count
            assert len(keep) == 33
            for name, s, _ in keep:
                assert kept(kx, s, jump) is None, (name, kept(kx, s, jump))
            for name, s, _ in flagged:
                why = kept(kx, s, jump)
                assert why is not None and " seed at " in why and why.endswith(" hits") and int(why.split()[-2]) > 28, (name, why)
            # case 8: the flagged read first in its pair (beside 1a forward), then second (beside 1a reverse)
            mixed = [flagged[0]] + keep[:2] + [flagged[1]] + keep[2:]
            assert len(mixed) % 2 == 1 and mixed[0][0].startswith("c8") and mixed[3][0].startswith("c8") and mixed[1][0].startswith("c1a") and mixed[2][0].startswith("c1a")
            self.blocks[tag, "kept"] = keep
            self.blocks[tag, "mixed"] = mixed


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def pf_fa(world, tmp_path_factory):
    fa = str(tmp_path_factory.mktemp("pair_filter") / "pf.fa")
    with open(fa, "wb") as f:
        f.write(b">pf\n")
        s = world.G.tobytes()
        for k in range(0, len(s), 100):
            f.write(s[k:k + 100] + b"\n")
    g.index_build(fa, g.GM_BUILD_HOST)
    return fa


@pytest.fixture(scope="module")
def pf_ix(pf_fa):
    ix = g.Index(pf_fa, flags=g.GM_INDEX_FULL_SA)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def pf_oix(oracle, pf_fa):
    return oracle.index_load(pf_fa)


_ORACLE = {}


def oracle_for(oracle, oix, world, tag, block, cfg):
    """computed once per block and configuration, never changed; with it the guards: what the planted copies are for shows in the oracle"""
    key = (tag, block, cfg)
    if key not in _ORACLE:
        L, jump = GROUPS[tag]
        rd = world.blocks[tag, block]
        op = oracle.params(mer=MER, jump=jump, **CONFIGS[cfg])
        ores = [oracle.map_read(oix, op, oracle.pwm(s, q), s) for _, s, q in rd]
        if cfg == "all":
            for (name, _, _), o in zip(rd, ores):
                if name.startswith("c3"):                    # the second candidate is real
                    assert o["status"] == 0 and sum(len(h["pos"]) for h in o["hits"]) >= 2, name
                elif name.startswith("c"):
                    assert o["status"] == 0 and len(o["hits"]) >= 1, name
        _ORACLE[key] = ores
    return _ORACLE[key]


def pair_runs(ix, rd, tag, cfg):
    L, jump = GROUPS[tag]
    kw = dict(mer=MER, jump=jump, **CONFIGS[cfg])
    on = run(ix, rd, kw, BUCKET)
    flagged = on["batch"].pair_flagged()
    off = run(ix, rd, kw, dict(BUCKET, GM_VOTE_PAIR="0"))
    assert f"vote=k_vote_pair<{tag}> + k_vote_bucket<" in on["path"], on["path"]
    assert "k_vote_pair" not in off["path"] and "vote=k_vote_bucket<" in off["path"], off["path"]
    assert off["batch"].pair_flagged() == 0
    return on, off, flagged


def check(on, off, ores, rd):
    for a, b in zip(on["raw"], off["raw"]):
        np.testing.assert_array_equal(a, b)
    mapped = sum(o["status"] == 0 for o in ores)          # (16 or 17 of the 33 with one strand off: the forward or the reversed reads)
    assert mapped >= 16 and len(on["raw"][0]) >= mapped
    for o in (on, off):
        _compare(o["res"], ores, rd)
        o["batch"].destroy()


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("tag", list(GROUPS))
def test_kept_reads_with_planted_strays_match_oracle(tag, cfg, world, pf_ix, oracle, pf_oix):
    rd = world.blocks[tag, "kept"]
    ores = oracle_for(oracle, pf_oix, world, tag, "kept", cfg)
    on, off, flagged = pair_runs(pf_ix, rd, tag, cfg)
    assert flagged == 0                                   # k_vote_pair itself voted for every read of the block
    check(on, off, ores, rd)


@pytest.mark.parametrize("cfg", ["base", "all", "no_nw"])
@pytest.mark.parametrize("tag", list(GROUPS))
def test_flagged_read_beside_a_kept_read(tag, cfg, world, pf_ix, oracle, pf_oix):
    rd = world.blocks[tag, "mixed"]
    ores = oracle_for(oracle, pf_oix, world, tag, "mixed", cfg)
    on, off, flagged = pair_runs(pf_ix, rd, tag, cfg)
    assert flagged == 2                                   # the two reads of case 8 and nobody else
    check(on, off, ores, rd)
