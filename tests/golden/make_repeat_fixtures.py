#!/usr/bin/env python3
"""Repeat fixtures: a genome made of repeat families, the reads of every family, and what the UNMODIFIED reference program writes for
them.  What syn.fa / edge.fa / celgen do not have: reads whose accepted hits number 2 .. 3001, in one key or in thousands, so that the
unique map of process_hits (inc/align_seq2_raw.cpp:102-165) - processing order, one group per window string in read orientation,
std::map<string> order, set<(pos, strand)> order, the -T and -u exits - is decided by more than two or three hits.

Run in the build container only (needs the reference sources):
    make -C oracle refbin && python tests/golden/make_repeat_fixtures.py

Inputs written (deterministic; our own generator, fixed seeds):

    rep.fa.gz      three contigs; every family is ONE random base segment planted as copies (some reverse-complemented) between unique
                   random spacers of 7 .. 38 bases, all families shuffled together:
                     s2 s3 s63 s64 s65 s66 s129 s300   same-key families: that many identical copies of a 150-base segment.  The first
                                    item of the genome is a reverse-complemented copy of s63 (position 0, before every forward copy
                                    of s63); the last two are a reverse-complemented copy of s64 (after its last forward copy) and a
                                    forward copy of s65 that ends at l_pac
                     t              180 copies of a 150-base segment, each with its own substitution(s) at offsets >= 32: all keys
                                    share their first word.  Single substitutions at the first and last offset of every word, at
                                    L - 1 of every read length, and elsewhere; then pairs
                     d              70 copies, each with its own substitution below offset 32 (every offset below 15 among them: a
                                    substitution in the first or second seed makes the copy reach -k 2 votes one or two seed steps
                                    later than its neighbours)
                     m              40 variants of a 100-base segment in 1 .. 6 copies each, orientations alternating
                     p              a 100-base segment equal to its own reverse complement, 3 copies
                     l              70 copies of a 640-base segment: differences beyond offset 600 only, a few in word 0
                     x              3001 copies of a 100-base segment, each with two substitutions at its own pair of offsets; 3000
                                    forward, one reverse-complemented
    rep.fq.gz      for each s*, t and d family the prefixes of 31, 32, 33, 63, 64, 65, 96, 100, 128 and 150 bases of its segment, as
                   cut (_f) and reverse-complemented (_r); m and p: the segment both ways; l: the 640-base segment both ways.
                   Qualities: Phred 10 .. 40, drawn per base
    rep_limit.fq   the x segment both ways: the two reads with 3001 keys (3000 on the forward strand)

Outputs committed, one set per entry of MODES (reference run with -c 1; the reference builds its own index of rep.fa in a first run that
is thrown away):

    tests/golden/ref_runs_repeat/<mode>.sam.gz           the SAM file, @PG line dropped
    tests/golden/ref_runs_repeat/<mode>.sgr.gz           the coverage track text
    tests/golden/ref_runs_repeat/manifest.json           argv, oracle / product parameters, FASTQ, tracks, SAM lines per mode

Everything committed is DATA (our inputs, the reference's outputs on them); no reference source text.
"""
import gzip, json, os, shutil, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFBIN = os.path.join(ROOT, "oracle", "_ref", "gnumap_ref")
OUT = os.path.join(HERE, "ref_runs_repeat")

SAME = (2, 3, 63, 64, 65, 66, 129, 300)
LENS = (31, 32, 33, 63, 64, 65, 96, 100, 128, 150)
N_TIE, N_DIFF, N_MIXED_KEYS, N_LONG, N_LIMIT = 180, 70, 40, 70, 3001
T_KEYS = N_TIE                                  # keys of the 150-base read of the t family = the -T pair of MODES (asserted by the guards)

# name -> (reference argv between "-a 0.9 -c 1" and the FASTQ, oracle / product parameter overrides, fastq)
MODES = {
    "default":      ([], {}, "rep.fq"),
    "no_nw":        (["--no_nw"], dict(nw=0), "rep.fq"),
    "all":          (["--print_all_sam"], dict(print_all_sam=1), "rep.fq"),
    "no_nw_all":    (["--no_nw", "--print_all_sam"], dict(nw=0, print_all_sam=1), "rep.fq"),
    "u":            (["-u", "1"], dict(unique_only=1), "rep.fq"),
    "u_no_nw":      (["-u", "1", "--no_nw"], dict(unique_only=1, nw=0), "rep.fq"),
    "up":           (["--up_strand"], dict(neg_strand=0), "rep.fq"),
    "T_keys":       (["-T", str(T_KEYS)], dict(max_matches=T_KEYS), "rep.fq"),
    "T_keys_less1": (["-T", str(T_KEYS - 1)], dict(max_matches=T_KEYS - 1), "rep.fq"),
    "bin1":         (["--bin_size=1"], dict(bin_size=1), "rep.fq"),
    # the set-limit reads: 3001 keys, 3000 of them on the forward strand
    "limit_T3000":    (["-T", "3000"], dict(max_matches=3000), "rep_limit.fq"),
    "limit_T3001":    (["-T", "3001"], dict(max_matches=3001), "rep_limit.fq"),
    "limit_no_nw":    (["--no_nw"], dict(nw=0), "rep_limit.fq"),
}

sys.path.insert(0, os.path.dirname(HERE))
from edge_ref_env import REF_MALLOC_ENV       # tests/edge_ref_env.py: why the reference runs with a malloc setting
REF_ENV = dict(os.environ, **REF_MALLOC_ENV)

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rand_bases(rng, n):
    return bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))


def subst(seg, subs):
    """seg with base (old + k) mod 4 at offset o for every (o, k) of subs, k = 1 .. 3"""
    s = bytearray(seg)
    for o, k in subs:
        s[o] = b"ACGT"[(b"ACGT".index(s[o]) + k) % 4]
    return bytes(s)


def families():
    """{family: base segment}, [(family, copy, sequence as it stands in the genome, reverse-complemented)]"""
    rng = np.random.default_rng(20241019)
    seg, items = {}, []
    for n in SAME:
        f = f"s{n}"
        seg[f] = rand_bases(rng, 150)
        rc = [bool(j % 3 == 1) for j in range(n)]                     # every third copy, the second one first
        items += [(f, j, revcomp(seg[f]) if rc[j] else seg[f], rc[j]) for j in range(n)]
    # t: first word equal
    seg["t"] = rand_bases(rng, 150)
    singles = [32, 33, 62, 63, 64, 65, 94, 95, 96, 97, 99, 100, 126, 127, 128, 129, 148, 149]
    subs = [()] + [((o, 1),) for o in singles] + [((o, 2),) for o in (32, 63, 64, 99, 127, 149)]
    seen = set(subs)
    while len(subs) < 70:
        c = ((int(rng.integers(32, 150)), int(rng.integers(1, 4))),)
        if c not in seen:
            seen.add(c); subs.append(c)
    while len(subs) < N_TIE:
        a, b = sorted(int(x) for x in rng.integers(32, 150, 2))
        c = ((a, int(rng.integers(1, 4))), (b, int(rng.integers(1, 4))))
        if a != b and c not in seen:
            seen.add(c); subs.append(c)
    items += [("t", j, revcomp(subst(seg["t"], c)) if j % 4 == 2 else subst(seg["t"], c), j % 4 == 2) for j, c in enumerate(subs)]
    # d: first word differs
    seg["d"] = rand_bases(rng, 150)
    subs = [()] + [((o, 1 + o % 3),) for o in range(32)]
    seen = set(subs)
    while len(subs) < N_DIFF:
        c = ((int(rng.integers(0, 32)), int(rng.integers(1, 4))),)
        if c not in seen:
            seen.add(c); subs.append(c)
    items += [("d", j, revcomp(subst(seg["d"], c)) if j % 5 == 3 else subst(seg["d"], c), j % 5 == 3) for j, c in enumerate(subs)]
    # m: 40 keys with 1 .. 6 places each, orientations alternating (the first copy of every other key reverse-complemented)
    seg["m"] = rand_bases(rng, 100)
    seen, n = {()}, 0
    for k in range(N_MIXED_KEYS):
        c = ()
        while c in seen:
            c = tuple(sorted((int(rng.integers(0, 100)), int(rng.integers(1, 4))) for _ in range(1 + k % 2)))
            if len({o for o, _ in c}) != len(c):
                c = ()
        seen.add(c)
        v = subst(seg["m"], c) if k else seg["m"]
        for j in range(1 + k % 6):
            rc = (j + k // 6) % 2 == 1
            items.append(("m", n, revcomp(v) if rc else v, rc)); n += 1
    # p: its own reverse complement
    half = rand_bases(rng, 50)
    seg["p"] = half + revcomp(half)
    assert revcomp(seg["p"]) == seg["p"]
    items += [("p", j, seg["p"], False) for j in range(3)]
    # l: 640 bases, differences beyond 600 (and a few in word 0)
    seg["l"] = rand_bases(rng, 640)
    subs = [()] + [((o, 1),) for o in (600, 607, 608, 620, 638, 639)] + [((o, 2),) for o in (0, 9, 31)]
    seen = set(subs)
    while len(subs) < N_LONG:
        a, b = sorted(int(x) for x in rng.integers(600, 640, 2))
        c = ((a, int(rng.integers(1, 4))),) if a == b else ((a, int(rng.integers(1, 4))), (b, int(rng.integers(1, 4))))
        if c not in seen:
            seen.add(c); subs.append(c)
    items += [("l", j, revcomp(subst(seg["l"], c)) if j % 6 == 4 else subst(seg["l"], c), j % 6 == 4) for j, c in enumerate(subs)]
    # x: 3001 keys from two substitutions at distinct offset pairs
    seg["x"] = rand_bases(rng, 100)
    pairs = [(a, b) for a in range(100) for b in range(a + 1, 100)]
    pick = rng.permutation(len(pairs))[:N_LIMIT]
    for j, q in enumerate(pick):
        a, b = pairs[int(q)]
        v = subst(seg["x"], ((a, 1 + j % 3), (b, 1 + (j // 3) % 3)))
        rc = j == 1234
        items.append(("x", j, revcomp(v) if rc else v, rc))
    return seg, items


def make_genome():
    """[(contig name, sequence)], {family: segment}, [(family, copy, position, reverse-complemented)]"""
    seg, items = families()
    rng = np.random.default_rng(20241020)
    order = [items[int(i)] for i in rng.permutation(len(items))]

    def take(pred):
        k = next(i for i, it in enumerate(order) if pred(it))
        return order.pop(k)
    first = take(lambda it: it[0] == "s63" and it[3])                   # a reverse-complemented copy at position 0
    last = take(lambda it: it[0] == "s65" and not it[3])                # a forward copy that ends at l_pac
    before_last = take(lambda it: it[0] == "s64" and it[3])             # a reverse-complemented copy after every forward copy of s64
    order = [first] + order + [before_last, last]
    cut = (len(order) * 3 // 10, len(order) * 13 // 20)
    contigs, placed, pos = [], [], 0
    cur = bytearray()
    for k, it in enumerate(order):
        placed.append((it[0], it[1], pos + len(cur), it[3]))
        cur += it[2]
        if k + 1 == len(order):
            break
        n = int(rng.integers(7, 39))
        if k + 1 in cut or k + 2 == len(order):                         # a contig ends behind this spacer / the last copy follows it
            after = len(order[k + 1][2]) if k + 2 == len(order) else 0
            while (pos + len(cur) + n + after) % 16 in (0, 4, 8, 12):
                n += 1
        cur += rand_bases(rng, n)
        if k + 1 in cut:
            contigs.append(bytes(cur)); pos += len(cur); cur = bytearray()
    contigs.append(bytes(cur))
    return list(zip(("repA", "repB", "repC"), contigs)), seg, placed


def write_fasta(path, contigs):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        for name, s in contigs:
            f.write(b">" + name.encode() + b"\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + b"\n")


def make_reads(seg):
    rng = np.random.default_rng(20241021)
    main, limit = [], []

    def add(out, name, s):
        for tag, t in (("f", s), ("r", revcomp(s))):
            out.append((f"{name}_L{len(s)}_{tag}", t, bytes((33 + rng.integers(10, 41, len(t))).astype(np.uint8))))
    for f in [f"s{n}" for n in SAME] + ["t", "d"]:
        for L in LENS:
            add(main, f, seg[f][:L])
    for f in ("m", "p", "l"):
        add(main, f, seg[f])
    add(limit, "x", seg["x"])
    return main, limit


def write_fastq(path, reads):
    with (gzip.GzipFile(path, "wb", mtime=0) if path.endswith(".gz") else open(path, "wb")) as f:
        for name, s, q in reads:
            f.write(b"@" + name.encode() + b"\n" + s + b"\n+\n" + q + b"\n")


def check_layout(contigs, seg, placed):
    """what the layout promises, on the genome itself (the guards of tests/repeat_fixture.py ask the oracle)"""
    genome = b"".join(s for _, s in contigs)
    l_pac = len(genome)
    off = np.cumsum([0] + [len(s) for _, s in contigs])
    assert all(int(o) % 4 and int(o) % 16 for o in off[1:]), off
    at = {}
    for f, j, p, rc in placed:
        at.setdefault(f, []).append((p, rc))
    assert min(at["s63"]) == (0, True)
    assert max(at["s64"])[1] and max(at["s65"]) == (l_pac - 150, False)
    for f in [f"s{n}" for n in SAME]:
        for p, rc in at[f]:
            assert genome[p:p + 150] == (revcomp(seg[f]) if rc else seg[f])
        assert len(at[f]) == int(f[1:]) and genome.count(seg[f]) + genome.count(revcomp(seg[f])) == len(at[f])
    starts = [p for _, _, p, _ in placed]
    assert {p % 4 for p in starts} == {0, 1, 2, 3} and len({p % 32 for p in starts}) == 32
    return l_pac


def main():
    assert os.path.exists(REFBIN), "make -C oracle refbin first"
    os.makedirs(OUT, exist_ok=True)
    contigs, seg, placed = make_genome()
    l_pac = check_layout(contigs, seg, placed)
    write_fasta(os.path.join(HERE, "rep.fa.gz"), contigs)
    reads, limit = make_reads(seg)
    write_fastq(os.path.join(HERE, "rep.fq.gz"), reads)
    write_fastq(os.path.join(HERE, "rep_limit.fq"), limit)
    print(f"rep.fa: {[len(s) for _, s in contigs]} = {l_pac} bases, {len(placed)} copies; rep.fq: {len(reads)} reads; rep_limit.fq: {len(limit)} reads")
    if "--inputs-only" in sys.argv:
        return

    work = tempfile.mkdtemp()
    for f in ("rep.fa", "rep.fq"):
        with gzip.open(os.path.join(HERE, f + ".gz"), "rb") as src, open(os.path.join(work, f), "wb") as dst:
            shutil.copyfileobj(src, dst)
    shutil.copy(os.path.join(HERE, "rep_limit.fq"), work)
    r = subprocess.run([REFBIN, "-g", "rep.fa", "-o", "index_run", "-a", "0.9", "-c", "1", "-T", "1", "rep_limit.fq"], cwd=work, capture_output=True,
                       text=True, env=REF_ENV)                          # thrown away: this run builds the index
    assert r.returncode == 0, r.stderr[-2000:]
    only = {a for a in sys.argv[1:] if not a.startswith("--")}
    manifest = json.load(open(os.path.join(OUT, "manifest.json"))) if only else {}
    for name, (args, kw, fq) in MODES.items():
        if only and name not in only:
            continue
        r = subprocess.run([REFBIN, "-g", "rep.fa", "-o", name, "-a", "0.9", "-c", "1"] + args + [fq], cwd=work, capture_output=True, text=True,
                           env=REF_ENV)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        sam = [l for l in open(os.path.join(work, name + ".sam"), "rb") if not l.startswith(b"@PG")]
        with gzip.GzipFile(os.path.join(OUT, name + ".sam.gz"), "wb", mtime=0) as g:
            g.write(b"".join(sam))
        tracks = []
        for ext in ("sgr", "gmp"):
            p = os.path.join(work, name + "." + ext)
            if os.path.exists(p):
                with gzip.GzipFile(os.path.join(OUT, name + "." + ext + ".gz"), "wb", mtime=0) as g:
                    g.write(open(p, "rb").read())
                tracks.append(ext)
        manifest[name] = dict(argv=args, params=kw, fastq=fq, sam_lines=len(sam), tracks=tracks)
        print(f"{name:16s} {len(sam):6d} SAM lines  {tracks}  " +
              "  ".join(f"{e} {os.path.getsize(os.path.join(OUT, name + '.' + e + '.gz')) >> 10} KiB" for e in ["sam"] + tracks))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:                 # one line per mode
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(manifest[k], sort_keys=True)}" for k in sorted(manifest)) + "\n}\n")
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
