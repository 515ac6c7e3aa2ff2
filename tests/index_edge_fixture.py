"""Shared by tests/test_index_tables_cpu.py and tests/test_gpu_index_tables.py: genomes built to reach the rare records of the seed-lookup
tables (rank planes, memoised k-mer table, its compact form, bucket records, full SA), a PLAIN reference of every lookup, and the probe
reads that make one wrong rank or count visible in the results.

The plain reference is NaiveIndex: the suffix array of text + '$' by sorting the suffixes, '$' smallest, rank 0 the empty suffix (BWA's
convention: ranks 1 .. n are the suffixes of the text in order, primary = the rank of the whole text).  It calls neither the library nor
the oracle.  classify() restates the rules of k_build_kmer_compact from its comment (gm_kernels.hip): 8 consecutive T-mer codes share a
record (leftmost character in the highest bits, so a record = the T-mers that agree up to the upper bit of their second-last character);
a record is an ESCAPE when a count is >= 224 or when two occupied codes' intervals are not adjacent (a suffix shorter than T sorts in
between - only the text's last T-1 characters can, and only when the text ends in C or T), an absent code's byte carries its death depth.

Probe reads have exactly two seeds (length mer + jump + 1): with -k 2 --no_nw a window is reported only if BOTH seeds' intervals are
exactly right.  Every fixture comes from fixed seeds at test time; nothing is committed under tests/golden/."""
import functools
import itertools

import numpy as np

BASES = b"ACGT"
COUNTS = (1, 7, 8, 14, 15, 21, 22, 27, 28, 29, 30)                 # copies of the planted 22-mers: bucket records around 7j and 28 / 29
MT = ((14, 14), (14, 12), (14, 6), (10, 10))                       # (seed length, table length) of the guards
CONFIGS = {
    "m14_j7": dict(mer=14, jump=7, nw=0),
    "m14_j7_h28": dict(mer=14, jump=7, nw=0, max_kmer_hits=28),
    "m10_j5": dict(mer=10, jump=5, nw=0),
}
SWEEP_LENGTHS = (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 383, 384, 385, 3071, 3072, 3073)
CLASSES = ("a_big", "a_nb", "b", "c_lo", "c_hi")

_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return s[::-1].translate(_RC)


def rand_seq(rng, n, alphabet=BASES):
    return bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


# ------------------------------------------------------------------------------------------------ the plain reference
class NaiveIndex:
    """suffix array of text + '$' by plain sorting.  A bytes slice that is a proper prefix of another compares smaller, which is what a
    terminal '$' below every base does."""

    def __init__(self, text, contigs=None):
        assert text and set(text) <= set(BASES)
        self.text = text
        self.n = n = len(text)
        self.contigs = contigs or [(0, n)]                         # [(start, end)]
        self.sa = [n] + sorted(range(n), key=lambda i: text[i:])
        self.primary = self.sa.index(0)
        self._tab = {}

    def table(self, m):
        """{m-mer: (k, l)}: first and last rank of the suffixes that begin with it"""
        if m not in self._tab:
            t = {}
            for r in range(1, self.n + 1):
                p = self.sa[r]
                if p + m <= self.n:
                    w = self.text[p:p + m]
                    if w in t:
                        t[w][1] = r
                    else:
                        t[w] = [r, r]
            self._tab[m] = {w: (k, l) for w, (k, l) in t.items()}
        return self._tab[m]

    def interval(self, kmer):
        return self.table(len(kmer)).get(bytes(kmer).upper(), (0, 0))

    def count(self, kmer):
        k, l = self.interval(kmer)
        return 0 if (k, l) == (0, 0) else l - k + 1

    def occurrences(self, kmer):
        k, l = self.interval(kmer)
        return [] if (k, l) == (0, 0) else sorted(self.sa[r] for r in range(k, l + 1))

    def death_depth(self, kmer):
        """None when the k-mer occurs; else the number of characters, from its right end, after which the backward search dies"""
        for d in range(1, len(kmer) + 1):
            if self.interval(kmer[len(kmer) - d:]) == (0, 0):
                return d
        return None

    def window_ok(self, b, L):
        return b + L <= self.n and any(s <= b and b + L <= e for s, e in self.contigs)


def code_of(tmer):
    c = 0
    for ch in tmer:
        c = c * 4 + BASES.index(ch)
    return c


def classify(nx, T):
    """{T-mer: (code, (k, l), class)} of every occurring T-mer; class in CLASSES or "plain":
    a_big / a_nb  its record escapes because a count is >= 224: the code with that count / another occupied code of the record
    b             its record escapes because two occupied codes' intervals are not adjacent
    c_lo / c_hi   no escape, the code at sub-index 1..3 / 4..7 with at least one occupied AND one empty code below it (its start rank is
                  the record's start + the sum of the bytes below that are counts: the decoders have to mask the empty ones)"""
    tab = nx.table(T)
    recs = {}
    for w, iv in tab.items():
        c = code_of(w)
        recs.setdefault(c >> 3, {})[c & 7] = (w, iv)
    out = {}
    for rec, subs in recs.items():
        order = sorted(subs)
        big = any(subs[s][1][1] - subs[s][1][0] + 1 >= 224 for s in order)
        apart = any(subs[b][1][0] != subs[a][1][1] + 1 for a, b in zip(order, order[1:]))
        for s in order:
            w, iv = subs[s]
            if big:
                cl = "a_big" if iv[1] - iv[0] + 1 >= 224 else "a_nb"
            elif apart:
                cl = "b"
            else:
                below = [q in subs for q in range(s)]
                cl = ("c_lo" if s <= 3 else "c_hi") if any(below) and not all(below) else "plain"
            out[w] = (rec * 8 + s, iv, cl)
    return out


def class_summary(nx, T):
    """what the guards count on a genome: records that escape for non-adjacent intervals, codes in big-count records, c_lo and c_hi codes"""
    cl = classify(nx, T)
    return dict(b_records=len({c >> 3 for c, _, k in cl.values() if k == "b"}),
                a_codes=sum(k in ("a_big", "a_nb") for _, _, k in cl.values()),
                c_lo=sum(k == "c_lo" for _, _, k in cl.values()), c_hi=sum(k == "c_hi" for _, _, k in cl.values()))


# ------------------------------------------------------------------------------------------------ the genomes
@functools.lru_cache(maxsize=None)
def genome_a(end_with_w=True):
    """(text, marks): one contig, ACGT only.  marks: run = start of C A^300 G, planted = {copies: [positions of the 22-mer]}, z / w =
    {suffix: position} of the 12-mers Z / W with their two-character tails; the genome's last 13 bases are W + C, so that for T = 10, 12
    and 14 the text's last T - 1 characters sort between sub-indices 2 (.. AG) and 7 (.. CT) of one record"""
    rng = np.random.default_rng(20240614)
    parts, marks = [rand_seq(rng, 4300)], dict(planted={}, z={}, w={})
    at = lambda: sum(len(p) for p in parts)
    marks["run"] = at()
    parts.append(b"C" + b"A" * 300 + b"G")
    for c in COUNTS:
        e = rand_seq(rng, 22)
        marks["planted"][c] = []
        for _ in range(c):
            parts.append(rand_seq(rng, 40))
            marks["planted"][c].append(at())
            parts.append(e)
    Z, W = rand_seq(rng, 12), rand_seq(rng, 12)
    for key, word, tails in (("z", Z, (b"AC", b"AT", b"CA", b"CG")), ("w", W, (b"AG", b"CT"))):
        for tail in tails:
            parts.append(rand_seq(rng, 40))
            marks[key][tail] = at()
            parts.append(word + tail)
    parts.append(rand_seq(rng, 40))
    parts.append(W + b"C" if end_with_w else rand_seq(rng, 13))
    return b"".join(parts), marks


@functools.lru_cache(maxsize=None)
def genome_b():
    """3000 bases over {A, C, G}: no T, so L2[3] == L2[4], one rank plane is all zero, and a T at index j of a k-mer whose tail occurs
    gives death depth mer - j exactly"""
    return rand_seq(np.random.default_rng(20240615), 3000, b"ACG")


def _primary_of(text):
    return 1 + sum(text[i:] < text for i in range(1, len(text)))


@functools.lru_cache(maxsize=None)
def primary_genomes():
    """[(name, text)]: 300-base random genomes, found by trying seeds, whose primary sits at a granule (96) or BWT block (128) edge, is 1
    (the text is the smallest suffix) or seq_len (the largest)"""
    n = 300
    want = {"p96_0": lambda p: p % 96 == 0, "p96_1": lambda p: p % 96 == 1 and p > 1, "p96_95": lambda p: p % 96 == 95,
            "p128_0": lambda p: p % 128 == 0, "p128_127": lambda p: p % 128 == 127, "p_first": lambda p: p == 1, "p_last": lambda p: p == n}
    found = {}
    for seed in range(100000):
        text = rand_seq(np.random.default_rng(seed), n)
        p = _primary_of(text)
        for name, ok in want.items():
            if name not in found and ok(p):
                found[name] = text
        if len(found) == len(want):
            break
    assert len(found) == len(want), sorted(found)
    return [(k, found[k]) for k in want]


THREE_CONTIGS = (("c1", 337), ("c2", 411), ("c3", 263))


@functools.lru_cache(maxsize=None)
def sweep_genomes():
    """[(name, [(contig name, sequence as written to the FASTA)])]"""
    out = []
    for n in SWEEP_LENGTHS:
        out.append((f"len{n}", [("g", rand_seq(np.random.default_rng(5000 + n), n))]))
    out += [(name, [("g", text)]) for name, text in primary_genomes()]
    rng = np.random.default_rng(77)
    ctg = [(name, bytearray(rand_seq(rng, n))) for name, n in THREE_CONTIGS]
    ctg[1][1][200:220] = b"N" * 20                                  # the builder fills it with lrand48 bases: the text comes from the index
    out.append(("three_contigs_n", [(name, bytes(s)) for name, s in ctg]))
    return out


def write_fasta(path, contigs):
    with open(path, "wb") as f:
        for name, seq in contigs:
            f.write(b">" + name.encode() + b"\n")
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + b"\n")


def build(tmp_dir, name, contigs):
    """write <tmp_dir>/<name>.fa and index it with the library's host builder; returns the path"""
    import gnumap_amd as g
    fa = str(tmp_dir / f"{name}.fa")
    write_fasta(fa, contigs)
    g.index_build(fa, g.GM_BUILD_HOST)
    return fa


def build_genomes(tmp_dir, oracle):
    """{name: (fasta, oracle index, NaiveIndex)} of genome A, genome B and the sweep, indexed under tmp_dir"""
    out = {}
    for name, contigs in [("A", [("A", genome_a()[0])]), ("B", [("B", genome_b())])] + sweep_genomes():
        fa = build(tmp_dir, name, contigs)
        oix = oracle.index_load(fa)
        text, ctg = index_text(oracle, oix)
        if not any(b"N" in s for _, s in contigs):
            assert text == b"".join(s for _, s in contigs)
        out[name] = (fa, oix, NaiveIndex(text, ctg))
    return out


def genome_names():
    return ["A", "B"] + [n for n, _ in sweep_genomes()]


def index_text(oracle, oix):
    """(text, [(start, end)]) as the index holds it (N runs filled by the builder), contig by contig through the oracle's window"""
    ix = oix.contents
    ctg = [(int(ix.contigs[i].offset), int(ix.contigs[i].offset) + int(ix.contigs[i].len)) for i in range(ix.n_seqs)]
    text = b"".join(oracle.window(oix, s, e - s).upper() for s, e in ctg)
    assert len(text) == int(ix.l_pac) == int(ix.seq_len) and ctg[0][0] == 0 and ctg[-1][1] == len(text)
    return text, ctg


# ------------------------------------------------------------------------------------------------ the queries of the direct probes
def interval_queries(nx):
    """{m: [k-mers]}: all 4^m for m = 1..6; for m in (8, 10, 12, 14, 16) every m-mer of the text, every one-substitution neighbour of up to
    200 of them, and the suffixes shorter than m padded to m with each base (the k-mers that cross the text's end)"""
    q = {m: [bytes(t) for t in itertools.product(BASES, repeat=m)] for m in range(1, 7)}
    text, n = nx.text, nx.n
    for m in (8, 10, 12, 14, 16):
        own = sorted({text[p:p + m] for p in range(0, n - m + 1)})
        ks = list(own)
        step = max(1, len(own) // 200)
        for w in own[::step][:200]:
            for i in range(m):
                ks += [w[:i] + bytes([b]) + w[i + 1:] for b in BASES if b != w[i]]
        for j in range(1, min(m, n + 1)):
            if m - j <= n:
                ks += [text[n - (m - j):] + bytes([b]) * j for b in BASES]
        q[m] = ks
    return q


def guard_interval_queries(nx, queries):
    """from the reference alone: a queried interval holds rank primary - 1, primary and primary + 1 (where such a rank exists), and the rank
    arguments of the queries (k - 1 and l), in $-removed coordinates, fall on a granule's first and last position"""
    ivs = {nx.interval(k) for ks in queries.values() for k in ks} - {(0, 0)}
    for r in (nx.primary - 1, nx.primary, nx.primary + 1):
        if 1 <= r <= nx.n:
            assert any(k <= r <= l for k, l in ivs), r
    xs = {x - (x >= nx.primary) for k, l in ivs for x in (k - 1, l) if x != nx.n}
    assert any(x % 96 == 0 for x in xs)
    if nx.n >= 97:
        assert any(x % 96 == 95 for x in xs)


# ------------------------------------------------------------------------------------------------ the walk, in Python
def py_map(nx, read, mer, jump, nw=0, max_kmer_hits=0, min_seed_hits=2):
    """align_sequence at --no_nw restated on the plain reference: (set of (window start, strand) with >= -k votes inside one contig,
    seeds used, SA hits located).  Seeds: the first position >= i whose k-mer occurs (and stays within -h), then i += jump; a hit at
    coordinate c of the seed at i votes for max(0, c - i)."""
    assert nw == 0
    L = len(read)
    pos, n_seeds, n_hits = set(), 0, 0
    if L < mer:
        return pos, 0, 0
    for strand, seq in ((0, read), (1, revcomp(read))):
        votes = {}
        last, i = L - mer, 0
        while i < last:
            iv = (0, 0)
            while i < last:
                iv = nx.interval(seq[i:i + mer])
                if iv != (0, 0) and not (max_kmer_hits and iv[1] - iv[0] + 1 > max_kmer_hits):
                    break
                iv = (0, 0)
                i += 1
            if iv == (0, 0):
                break
            n_seeds += 1
            for r in range(iv[0], iv[1] + 1):
                c = nx.sa[r]
                b = 0 if c <= i else c - i
                votes[b] = votes.get(b, 0) + 1
                n_hits += 1
            i += jump
        pos |= {(b, strand) for b, v in votes.items() if v >= min_seed_hits and nx.window_ok(b, L)}
    return pos, n_seeds, n_hits


_EXP = {}


def expected(nx, seq, cfg):
    """py_map of a read in a configuration of CONFIGS, computed once: what both test files compare the oracle and the device with"""
    key = (id(nx), seq, cfg)
    if key not in _EXP:
        _EXP[key] = (nx, py_map(nx, seq, **CONFIGS[cfg]))
    return _EXP[key][1]


# ------------------------------------------------------------------------------------------------ the probe reads
def _cut(nx, out, kind, p, mer, jump, tags):
    """the two-seed reads around the mer-mer at text position p: it is the seed at offset 0 of one and at offset jump of the other, each
    in both orientations.  tags: what the read is a guard for"""
    L = mer + jump + 1
    for off in (0, jump):
        s = p - off
        if s < 0 or not nx.window_ok(s, L):
            continue
        w = nx.text[s:s + L]
        for o, seq in (("f", w), ("r", revcomp(w))):
            out.setdefault(seq, dict(name=f"{kind}_p{p}_o{off}_{o}", seq=seq, at=s, tags=set()))["tags"] |= set(tags)


def seed_class_tags(nx, mer, kmer):
    """the guard tags of a seed k-mer: ("cls", T, class) for every table length of MT at this seed length, ("count", c | ">=224")"""
    tags = set()
    for m, T in MT:
        if m == mer:
            e = classify_cached(nx, T).get(kmer[mer - T:])
            if e and e[2] != "plain":
                tags.add(("cls", T, e[2]))
    c = nx.count(kmer)
    if mer == 14 and (c in COUNTS or c >= 224):
        tags.add(("count", c if c < 224 else ">=224"))
    return tags


_CLS = {}


def classify_cached(nx, T):
    key = (id(nx), T)
    if key not in _CLS:
        _CLS[key] = (nx, classify(nx, T))
    return _CLS[key][1]


def probe_reads(nx, mer, jump, marks=None, per_class=3):
    """[dict(name, seq, at, tags)]: the classed two-seed reads of a genome at one seed length.  For every table length of MT and every
    class, the reads around up to per_class seeds of that class (text order); on genome A (marks) also the reads the fixture was built
    for: the planted 22-mers, the A run and its small neighbour, W + CT, Z + AT / CA / CG, and the seeds at text positions 4095 / 4096."""
    out = {}
    L = mer + jump + 1
    for m, T in MT:
        if m != mer:
            continue
        cl = classify_cached(nx, T)
        taken = {c: 0 for c in CLASSES}
        seen = set()
        for p in range(jump, nx.n - L + 1):
            kmer = nx.text[p:p + mer]
            e = cl.get(kmer[mer - T:])
            if not e or e[2] == "plain" or kmer in seen or taken[e[2]] >= per_class:
                continue
            seen.add(kmer)
            taken[e[2]] += 1
            _cut(nx, out, f"T{T}{e[2]}", p, mer, jump, ())
    if marks:
        if mer == 14:
            for c, ps in marks["planted"].items():                   # the 22-mers themselves (their 14-mers occur c times)
                _cut(nx, out, f"copies{c}", ps[0], mer, jump, ())
                _cut(nx, out, f"copies{c}", ps[-1] + jump + 1, mer, jump, ())
        run = marks["run"]                                           # C A^300 G
        _cut(nx, out, "run", run + 1, mer, jump, ())                 # A^L (offset 0); C A^.. (offset jump)
        _cut(nx, out, "run", run + 301 - mer, mer, jump, ())         # the last A^mer of the run: the read goes on into G ..
        _cut(nx, out, "runG", run + 301 - (mer - 1), mer, jump, ())  # A^(mer-1) G: the small neighbour in the big record
        for key in ("z", "w"):
            for tail, p in marks[key].items():
                _cut(nx, out, f"{key}{tail.decode()}", p + 14 - mer, mer, jump, ())
        for p in range(4081, 4098):
            if nx.window_ok(p, L):
                w = nx.text[p:p + L]
                for o, seq in (("f", w), ("r", revcomp(w))):
                    out.setdefault(seq, dict(name=f"early_p{p}_{o}", seq=seq, at=p, tags=set()))
    rd = list(out.values())
    for r in rd:                                                     # the tags come from what the read's two seeds ARE, however it was cut
        fwd = r["seq"] if r["name"].endswith("f") else revcomp(r["seq"])
        for off in (0, jump):
            r["tags"] |= seed_class_tags(nx, mer, fwd[off:off + mer])
            for p in nx.occurrences(fwd[off:off + mer]):
                if p in (4095, 4096) and marks:
                    r["tags"].add(("seed_at", p))
    return rd


def depth_probes(nx, mer, jump, rng):
    """[dict(name, seq, at, e, want)]: for e = 1 .. mer, X + S in both orientations.  S: a unique segment of mer + jump + 1 bases at least
    mer from the start; X: e bases whose last, c, makes c + S[:mer - e] absent from the text (T on a genome without T) - the k-mer at
    offset 0 then dies after exactly mer - e + 1 characters, the walk resumes at offset e and finds exactly two seeds.  want = the one
    window start pos(S) - e."""
    out = []
    Ls = mer + jump + 1
    alphabet = bytes(sorted(set(nx.text)))
    for e in range(1, mer + 1):
        for _ in range(400):
            p = int(rng.integers(mer, nx.n - Ls))
            S = nx.text[p:p + Ls]
            if nx.count(S[:mer]) != 1 or nx.count(S[jump:jump + mer]) != 1 or not nx.window_ok(p - e, e + Ls):
                continue
            last = [c for c in b"TGCA" if nx.count(bytes([c]) + S[:mer - e]) == 0]
            if not last:
                continue
            X = rand_seq(rng, e - 1, alphabet) + bytes([last[0]])
            kmer0 = (X + S)[:mer]
            assert nx.death_depth(kmer0) == mer - e + 1
            for o in "fr":
                seq = X + S if o == "f" else revcomp(X + S)
                out.append(dict(name=f"depth{mer - e + 1}_e{e}_p{p}_{o}", seq=seq, at=p - e, e=e, depth=mer - e + 1,
                                want={(p - e, 0 if o == "f" else 1)}))
            break
    return out


def rewalk_probes(nx, mer, jump, probes, rng):
    """[dict(name, seq, at, tags)]: X + S for every classed probe read S (forward orientation): the first k-mer dies as in depth_probes, so
    the lookups that take lane j's k-mer at j * jump give up and the read x strand is walked AGAIN - the re-walk's own decoder of the compact
    record (gm_seed_rewalk_ool) then meets the classed seeds at offsets e and e + jump (e = 3, or less where no 3-base X makes the
    first k-mer die).  tags: ("rewalk", T, class)"""
    out = []
    alphabet = bytes(sorted(set(nx.text)))
    for r in probes:
        cls = {t for t in r["tags"] if t[0] == "cls"}
        if not cls or not r["name"].endswith("f"):
            continue
        S = r["seq"]
        for e in (3, 2, 1):
            last = [c for c in b"TGCA" if nx.count(bytes([c]) + S[:mer - e]) == 0]
            if last and r["at"] >= e and nx.window_ok(r["at"] - e, e + len(S)):
                break
        else:
            continue
        X = rand_seq(rng, e - 1, alphabet) + bytes([last[0]])
        assert nx.death_depth((X + S)[:mer]) == mer - e + 1
        for o in "fr":
            out.append(dict(name=f"rewalk_{r['name'][:-2]}_{o}", seq=X + S if o == "f" else revcomp(X + S), at=r["at"] - e,
                            tags={("rewalk",) + t[1:] for t in cls}))
    return out


def ordinary_reads(nx, rng, n=60, L=100):
    """100-base reads with up to two substitutions, either orientation: the whole path with NW on"""
    out = []
    alphabet = bytes(sorted(set(nx.text)))
    for i in range(n):
        while True:
            p = int(rng.integers(0, nx.n - L))
            if nx.window_ok(p, L):
                break
        s = bytearray(nx.text[p:p + L])
        for _ in range(int(rng.integers(0, 3))):
            j = int(rng.integers(0, L))
            s[j] = alphabet[(alphabet.index(s[j]) + 1) % len(alphabet)]
        s = bytes(s)
        out.append(dict(name=f"ord{i}_p{p}", seq=revcomp(s) if rng.random() < 0.5 else s, at=p, tags=set()))
    return out


_BLOCKS = {}


def blocks(which, nx, mer, jump, marks=None):
    """the reads of one genome ("A" / "B") at one seed length, made once: dict(probes, depth, ordinary, rewalk)"""
    key = (which, mer, jump)
    if key not in _BLOCKS:
        rng = np.random.default_rng(900 + mer + (0 if which == "A" else 50))
        probes = probe_reads(nx, mer, jump, marks)
        _BLOCKS[key] = dict(probes=probes, depth=depth_probes(nx, mer, jump, rng), ordinary=ordinary_reads(nx, rng),
                            rewalk=rewalk_probes(nx, mer, jump, probes, rng))
    return _BLOCKS[key]


def as_fastq(rd):
    return [(r["name"], r["seq"], b"I" * len(r["seq"])) for r in rd]
