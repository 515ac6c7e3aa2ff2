"""Shared by the repeat tests (tests/test_repeat_cpu.py, tests/test_gpu_repeat_groups.py): the repeat genome of
tests/golden/make_repeat_fixtures.py indexed in a temporary directory, its reads, and the GUARDS - the facts about the oracle's answers
that keep a comparison of the device's unique map with the oracle's from going vacuous (a fixture whose 65-copy family is accepted in 64
places would still compare equal).  Every guard is computed from the oracle's per-read results alone."""
import gzip
import json
import math
import os
import struct

import numpy as np

import shutil

from conftest import GOLDEN, read_fastq
from edge_ref_env import REF_MALLOC_ENV          # noqa: F401  (why the reference runs with a malloc setting)

RUNS = os.path.join(GOLDEN, "ref_runs_repeat")
MANIFEST = json.load(open(os.path.join(RUNS, "manifest.json")))
SAME = (2, 3, 63, 64, 65, 66, 129, 300)
T_KEYS = 180                                     # keys of t_L150_f: the -T pair of the reference runs
assert MANIFEST["T_keys"]["params"]["max_matches"] == T_KEYS and MANIFEST["T_keys_less1"]["params"]["max_matches"] == T_KEYS - 1


def build_index(tmp_path_factory):
    """rep.fa.gz, rep.fq.gz and rep_limit.fq unpacked into a session directory, the genome indexed there with the library's host builder
    (byte-compatible with bwa_index, tests/test_index_build.py): returns the FASTA path; the read files lie beside it (fastq_path)"""
    import gnumap_amd as g
    d = tmp_path_factory.mktemp("rep")
    for f in ("rep.fa", "rep.fq"):
        with gzip.open(os.path.join(GOLDEN, f + ".gz"), "rb") as src, open(str(d / f), "wb") as dst:
            shutil.copyfileobj(src, dst)
    shutil.copy(os.path.join(GOLDEN, "rep_limit.fq"), str(d))
    g.index_build(str(d / "rep.fa"), g.GM_BUILD_HOST)
    return str(d / "rep.fa")


def fastq_path(rep_fa, which):
    return os.path.join(os.path.dirname(rep_fa), which)


def reads(which="rep.fq"):
    if os.path.exists(os.path.join(GOLDEN, which)):
        return read_fastq(os.path.join(GOLDEN, which))
    lines = gzip.open(os.path.join(GOLDEN, which + ".gz"), "rb").read().split(b"\n")
    return [(lines[k][1:].decode(), lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)]


def all_reads():
    """rep.fq with the two set-limit reads of rep_limit.fq in its middle"""
    rd = reads()
    return rd[:len(rd) // 2] + reads("rep_limit.fq") + rd[len(rd) // 2:]


def ref_text(mode, ext):
    return gzip.open(os.path.join(RUNS, f"{mode}.{ext}.gz"), "rb").read()


def oracle_results(oracle, oix, op, rd):
    return [oracle.map_read(oix, op, oracle.pwm(s, q), s) for _, s, q in rd]


def n_places(o):
    return sum(len(h["pos"]) for h in o["hits"])


def check_geometry(oix):
    ix = oix.contents
    off = [int(ix.contigs[i].offset) for i in range(ix.n_seqs)]
    l_pac = int(ix.l_pac)
    assert len(off) == 3 and all(o % 4 and o % 16 for o in off[1:]) and l_pac % 4 and l_pac % 16
    return l_pac


def first_differences(keys):
    """the offsets at which two keys of a read first differ, over all pairs of keys"""
    K = np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), -1)
    d = K[:, None, :] != K[None, :, :]
    first = d.argmax(axis=2)
    return set(int(x) for x in first[np.triu(d.any(axis=2), 1)])


def guard_hit_counts(rd, ores):
    """reads with exactly 2, 63, 64, 65, 66 and 129 accepted hits and with at least 300 (default parameters): every lane stride of
    k_group_multi and both sides of the switch to the big path"""
    by = {}
    for (name, _, _), o in zip(rd, ores):
        if o["status"] == 0:
            by.setdefault(n_places(o), []).append(name)
    for n in (2, 63, 64, 65, 66, 129):
        assert len(by.get(n, [])) >= 2, (n, sorted(by))
    big = [n for n in by if n >= 300]
    assert big, sorted(by)
    return {n: len(by[n]) for n in sorted(by)}


def guard_one_key(rd, ores):
    """the reads of the same-key families have ONE key with as many places as the family has copies"""
    n = 0
    for (name, _, _), o in zip(rd, ores):
        if name[0] == "s":
            assert o["status"] == 0 and len(o["hits"]) == 1 and n_places(o) == int(name[1:].split("_")[0]), name
            assert {st for _, st in o["hits"][0]["pos"]} == {0, 1}, name
            n += 1
    assert n == 160
    return n


def guard_tie_family(rd, ores):
    """t_L150_f: T_KEYS keys, at least 150 with the same first 32 bases; pairs of keys that first differ in word 1, 2, 3 and in the
    partial last word (4), down to offset L - 1 alone.  The shorter reads of the family: a pair that first differs at L - 1 wherever a
    word is partial"""
    by_name = {r[0]: o for r, o in zip(rd, ores)}
    o = by_name["t_L150_f"]
    keys = [h["key"] for h in o["hits"]]
    assert o["status"] == 0 and len(keys) == T_KEYS
    heads = {}
    for k in keys:
        heads[k[:32]] = heads.get(k[:32], 0) + 1
    assert max(heads.values()) >= 150
    first = first_differences(keys)
    words = {f // 32 for f in first}
    assert {1, 2, 3, 4} <= words and 0 not in words and 149 in first, sorted(first)
    last = []
    for L in (33, 65, 100, 150):
        oo = by_name[f"t_L{L}_f"]
        assert L - 1 in first_differences([h["key"] for h in oo["hits"]]), L
        last.append(len(oo["hits"]))
    return dict(keys=len(keys), same_first_word=max(heads.values()), first_difference_words=sorted(words), keys_of_partial_word_reads=last)


def guard_first_word_family(rd, ores):
    """d_L150_f: at least 60 keys that all differ inside their first word"""
    o = {r[0]: o for r, o in zip(rd, ores)}["d_L150_f"]
    keys = [h["key"] for h in o["hits"]]
    assert len(keys) >= 60 and len({k[:32] for k in keys}) == len(keys)
    return len(keys)


def guard_long_keys(rd, ores):
    """the 640-base read: keys that differ only beyond word 18 (offset 608 and later)"""
    out = []
    for tag in "fr":
        o = {r[0]: o for r, o in zip(rd, ores)}[f"l_L640_{tag}"]
        keys = [h["key"] for h in o["hits"]]
        assert o["status"] == 0 and len(keys) >= 60 and len(keys[0]) == 640
        late = [f for f in first_differences(keys) if f >= 608]
        assert late and 639 in late, sorted(first_differences(keys))
        out.append(len(keys))
    return out


def guard_both_strand_groups(rd, ores):
    """at least 10 groups hold places of both strands; in at least 3 the first hit (a plus-strand hit: that pass runs first) is not the
    lowest position of the set, which begins with a minus-strand place"""
    both = later = 0
    for o in ores:
        for h in o["hits"]:
            if len({st for _, st in h["pos"]}) == 2:
                both += 1
                assert h["first_strand"] == 0
                if h["first_pos"] != h["pos"][0][0]:
                    assert h["pos"][0][1] == 1
                    later += 1
    assert both >= 10 and later >= 3, (both, later)
    return both, later


def guard_palindrome(rd, ores):
    n = 0
    for (name, _, _), o in zip(rd, ores):
        if name[0] == "p":
            assert o["status"] == 0 and len(o["hits"]) == 1
            pos = o["hits"][0]["pos"]
            assert len(pos) == 6 and all(pos[2 * k] == (pos[2 * k][0], 0) and pos[2 * k + 1] == (pos[2 * k][0], 1) for k in range(3)), pos
            n += 1
    assert n == 2
    return n


def guard_set_limit(oracle, oix):
    """x_L100_f: 3000 keys on the forward strand, 3001 on both; -T 3000 is met exactly by the first and missed by one by the second"""
    (name, s, q), _ = reads("rep_limit.fq")
    assert name == "x_L100_f"
    P = oracle.pwm(s, q)
    up = oracle.map_read(oix, oracle.params(neg_strand=0, max_matches=3000), P, s)
    assert up["status"] == 0 and len(up["hits"]) == 3000 and n_places(up) == 3000
    both = oracle.map_read(oix, oracle.params(max_matches=3001), P, s)
    assert both["status"] == 0 and len(both["hits"]) == 3001 and n_places(both) == 3001
    assert oracle.map_read(oix, oracle.params(max_matches=3000), P, s)["status"] == 1
    assert oracle.map_read(oix, oracle.params(neg_strand=0, max_matches=2999), P, s)["status"] == 1
    no_nw = oracle.map_read(oix, oracle.params(nw=0), P, s)
    assert no_nw["status"] == 0 and len(no_nw["hits"]) == 3001
    return len(up["hits"]), len(both["hits"])


def guard_T_pair(oracle, oix, rd):
    """-T equal to the number of keys of t_L150_f maps it, one less does not"""
    name, s, q = next(r for r in rd if r[0] == "t_L150_f")
    P = oracle.pwm(s, q)
    assert oracle.map_read(oix, oracle.params(max_matches=T_KEYS), P, s)["status"] == 0           # GMO_OK
    assert oracle.map_read(oix, oracle.params(max_matches=T_KEYS - 1), P, s)["status"] == 1       # GMO_TOO_MANY


def place_scores(oracle, oix, op, read, o):
    """[(pos, strand, align score)] of every accepted hit of a read: a key keeps the score of its FIRST hit only, and a place on the other
    strand was scored with the reverse-complemented read, so every place is scored again (gmo_nw_score on its window)"""
    from reflib import revcomp_pwm
    _, s, q = read
    P = [oracle.pwm(s, q)]
    P.append(revcomp_pwm(P[0]))
    out = []
    for h in o["hits"]:
        for p, st in h["pos"]:
            sc = float(oracle.lib.gmo_nw_score(op, P[st], len(s), oracle.window(oix, p, len(s))))
            if (p, st) == (h["first_pos"], h["first_strand"]):
                assert sc == h["score"], read[0]
            out.append((p, st, sc))
    return out


def guard_order_sensitive(oracle, oix, rd, ores):
    """the reads whose denominator depends on the ORDER of the additions: the same terms exp(score) added in ascending (position, strand)
    order give another double than the oracle's processing order (plus-strand pass first, seed step, position)"""
    op = oracle.params()
    found = []
    for read, o in zip(rd, ores):
        if o["status"] != 0:
            continue
        den = 0.0
        for _, _, sc in sorted(place_scores(oracle, oix, op, read, o)):
            den += math.exp(sc)
        assert abs(den - o["denominator"]) <= 1e-12 * o["denominator"], read[0]           # the same terms ...
        if struct.pack("<d", den) != struct.pack("<d", o["denominator"]):                 # ... in an order that matters
            found.append(read[0])
    assert len(found) >= 20, found
    return found


def guards(oracle, oix, rd, ores):
    """all guards on the default-parameter results `ores` of rep.fq's reads `rd`; returns the counts as measured"""
    return dict(hit_counts=guard_hit_counts(rd, ores), one_key_reads=guard_one_key(rd, ores), tie=guard_tie_family(rd, ores),
                first_word_keys=guard_first_word_family(rd, ores), long_keys=guard_long_keys(rd, ores),
                both_strand_groups=guard_both_strand_groups(rd, ores), palindrome_reads=guard_palindrome(rd, ores),
                order_sensitive_reads=len(guard_order_sensitive(oracle, oix, rd, ores)))
