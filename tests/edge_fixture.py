"""Shared by the edge tests (tests/test_edge_cpu.py, tests/test_gpu_edge_*.py, the edge cases of tests/test_gpu_driver_golden.py): the edge
genome of tests/golden/make_edge_fixtures.py indexed in a temporary directory, its geometry, its reads by name, and the GUARDS - the facts
about the oracle's answers that keep a comparison of the device with the oracle from going vacuous (a fixture that no longer reaches the
clamped window start would still compare equal).  Every guard is computed from the oracle alone."""
import json
import os
import re
import shutil

import numpy as np

from conftest import GOLDEN, read_fastq
from edge_ref_env import REF_MALLOC_ENV          # noqa: F401  (why the reference runs with a malloc setting)
from reflib import revcomp_str

RUNS = os.path.join(GOLDEN, "ref_runs_edge")
MANIFEST = json.load(open(os.path.join(RUNS, "manifest.json")))
MER = 14
_NAME = re.compile(r"^(s|hs|e|he|dv|sh)(\d+)(?:_(\d+))?_L(\d+)_([fr])$")


def build_index(tmp_path_factory, name="edge.fa"):
    """edge.fa (or both.fa) copied into a session directory and indexed there with the library's host builder (byte-compatible with
    bwa_index, tests/test_index_build.py): returns the FASTA path"""
    import gnumap_amd as g
    d = tmp_path_factory.mktemp(name.split(".")[0])
    fa = str(d / name)
    shutil.copy(os.path.join(GOLDEN, name), fa)
    g.index_build(fa, g.GM_BUILD_HOST)
    return fa


def reads(which="edge.fq"):
    return read_fastq(os.path.join(GOLDEN, which))


def parse(name):
    """(kind, contig or offset, k or d or None, length, strand letter) of a read name of make_edge_fixtures.py"""
    m = _NAME.match(name)
    assert m, name
    return m.group(1), int(m.group(2)), None if m.group(3) is None else int(m.group(3)), int(m.group(4)), m.group(5)


def geometry(oix):
    """([(start, end)] of every contig, l_pac) from the oracle's index"""
    ix = oix.contents
    return [(int(ix.contigs[i].offset), int(ix.contigs[i].offset) + int(ix.contigs[i].len)) for i in range(ix.n_seqs)], int(ix.l_pac)


def check_geometry(oix):
    """what the fixture is for: no inner contig offset on a 16-base word, one not on a pac byte, a partial last word and last byte"""
    ctg, l_pac = geometry(oix)
    assert len(ctg) == 3 and 9000 < l_pac < 11000
    assert all(b % 16 for b, _ in ctg[1:]) and any(b % 4 for b, _ in ctg[1:])
    assert l_pac % 16 and l_pac % 4
    return ctg, l_pac


def oracle_results(oracle, oix, op, rd):
    return [oracle.map_read(oix, op, oracle.pwm(s, q), s) for _, s, q in rd]


def kmer_occurrences(oracle, oix, seq):
    """[(strand, offset, [reference coordinates])] of every MER-mer of the read, in either orientation, that occurs in the reference"""
    out = []
    for st, t in ((0, seq), (1, revcomp_str(seq).upper())):
        for i in range(len(t) - MER + 1):
            s, e = oracle.sa_interval(oix, t[i:i + MER])
            if s or e:
                out.append((st, i, sorted(int(oracle.lib.gmo_locate(oix, k, None)) for k in range(s, e + 1))))
    return out


def guard_double_vote(oracle, oix, rd, ores):
    """(a): indices of the reads that reach -k 2 with ONE seed.  ores: the oracle's results at mer=14, jump=7, nw=0.  Exactly one 14-mer of
    such a read occurs in the reference; two of its occurrences lie nearer to the start of the reference than the 14-mer lies to the
    start of the read, so that both vote for the clamped window start 0 (its other occurrences, at the start of the second contig, vote
    for windows that begin in the first contig and fail the contig test); the result is one hit at 0 with score 2."""
    found = []
    for i, (name, s, q) in enumerate(rd):
        occ = kmer_occurrences(oracle, oix, s)
        if len(occ) != 1:
            continue
        st, off, coords = occ[0]
        if sum(c <= off for c in coords) != 2:
            continue
        o = ores[i]
        if o["status"] == 0 and len(o["hits"]) == 1 and o["hits"][0]["score"] == 2.0 and o["hits"][0]["pos"] == [(0, st)]:
            found.append(i)
    assert len(found) >= 8, [rd[i][0] for i in found]
    return found


def guard_position_zero(rd, ores):
    """(b): at default parameters at least 6 reads have an accepted hit at position 0"""
    found = [i for i, o in enumerate(ores) if o["status"] == 0 and any(p == 0 for h in o["hits"] for p, _ in h["pos"])]
    assert len(found) >= 6, [rd[i][0] for i in found]
    return found


def guard_contig_ends(oix, rd, ores):
    """(c): for every contig end (l_pac included) a read is accepted with its window ending exactly there"""
    ctg, l_pac = geometry(oix)
    for _, e in ctg:
        assert any(o["status"] == 0 and any(p + len(rd[i][1]) == e for h in o["hits"] for p, _ in h["pos"]) for i, o in enumerate(ores)), e
    assert ctg[-1][1] == l_pac


def guard_no_hit_across_a_start(oix, rd, ores):
    """(d): a read that hangs off an inner contig start by d >= 1 bases has no hit that begins in the previous contig"""
    ctg, _ = geometry(oix)
    n = 0
    for i, (name, s, q) in enumerate(rd):
        kind, c, d, L, _ = parse(name)
        if kind == "hs" and c >= 1:
            n += 1
            assert not any(ctg[c - 1][0] <= p < ctg[c][0] for h in ores[i]["hits"] for p, _ in h["pos"]), name
    assert n >= 24


def guard_windows_inside_one_contig(oix, rd, ores):
    """no hit's window lies across a contig boundary or the end of the reference, and the reads that hang off a contig are among those asked"""
    ctg, l_pac = geometry(oix)
    n = 0
    for i, (name, s, q) in enumerate(rd):
        for h in ores[i]["hits"]:
            for p, _ in h["pos"]:
                assert any(b <= p and p + len(s) <= e for b, e in ctg), (name, p)
                n += 1
    assert n > 100 and sum(parse(r[0])[0] in ("hs", "he") for r in rd) >= 72


def guard_single_votes(oracle, oix, op, rd):
    """(e): the read with the planted 14-mer at offset 17 votes once for window start 0 and once for 3 (and once for a window in the
    second contig): no position reaches -k 2, the read is unmapped at -m 14 --no_nw.  With the 14-mer at L - mer (offset 86), which the
    seed walk never reaches, nothing is looked up and the read is unmapped."""
    n = 0
    for i, (name, s, q) in enumerate(rd):
        kind, off, _, L, _ = parse(name)
        if kind != "dv" or L != 100 or off not in (17, 86):
            continue
        occ = kmer_occurrences(oracle, oix, s)
        assert len(occ) == 1 and occ[0][1] == off, name
        o = oracle.map_read(oix, op, oracle.pwm(s, q), s)
        assert o["status"] == 2 and not o["hits"], name
        if off == 17:
            begins = [max(0, c - off) for c in occ[0][2]]
            assert sorted(begins)[:2] == [0, 3] and len(set(begins)) == len(begins), (name, begins)
            assert o["ctr"]["locates"] == len(begins)
        else:
            assert o["ctr"]["locates"] == 0, name
        n += 1
    assert n == 4


def ref_text(mode, ext):
    import gzip
    return gzip.open(os.path.join(RUNS, f"{mode}.{ext}.gz"), "rb").read()


# ------------------------------------------------------------------ --snp (mode 5): tests/golden/make_snp_edge_fixtures.py
SNP_RUNS = os.path.join(GOLDEN, "ref_runs_snp_edge")
SNP_BLOCKS = {"edge": ("edge.fa", "edge.fq"), "mixed": ("edge.fa", "edge_mixed.fq"), "both": ("both.fa", "both.fq")}      # block -> genome, reads
GM_MODE_SNP = 5


def snp_ref_text(run, ext):
    import gzip
    return gzip.open(os.path.join(SNP_RUNS, f"{run}.{ext}.gz"), "rb").read()


def snp_info(oracle, oix, rd, **kw):
    """What the oracle does with a block of reads in --snp mode, read by read: dict(
         kept   = [(read, first strand, number of places, the read holds an N, length)] of every kept sequence of a mapped read,
         places = [(read, position, length, float32 weight, float32 posteriors [length][5] as deposited there, on the other strand)],
         recs   = [(read, contig, chr_pos, strand, mapq, cigar)] of the SAM records)
    gmo_read_output lists its deposits hit by hit and place by place, which is the order of gmo_map_read's hits."""
    op = oracle.params(mode=GM_MODE_SNP, **kw)
    kept, places, recs = [], [], []
    for i, (name, s, q) in enumerate(rd):
        P = oracle.pwm(s, q)
        o = oracle.map_read(oix, op, P, s)
        if o["status"] != 0:
            continue
        st, orecs, deps = oracle.read_output(oix, op, P, s)
        recs += [(i, r["contig"], r["chr_pos"], r["strand"], r["mapq"], r["cigar"]) for r in orecs]
        flat = [(h["first_strand"], pos, strand) for h in o["hits"] for pos, strand in h["pos"]]
        assert len(flat) == len(deps), name
        for h in o["hits"]:
            kept.append((i, h["first_strand"], len(h["pos"]), b"N" in s.upper(), len(s)))
        for (fs, pos, strand), (dpos, span, w, hmm) in zip(flat, deps):
            assert dpos == pos and span == len(s) and hmm.shape == (span, 5) and hmm.dtype == np.float32, name
            places.append((i, int(pos), int(span), np.float32(w), hmm, strand != fs))
    return dict(kept=kept, places=places, recs=recs)


def snp_tracks(info, n_bins, bin_size):
    """(coverage [n_bins], the five tracks [5][n_bins]) of the deposits in float64: AddScore adds float32(w), AddSeqScore the float32
    product float32(hmm) * float32(w) (GenomeBwt.cpp:483-551); what is left to the device is the order of its fp32 additions"""
    cov = np.zeros(n_bins, np.float64); nuc = np.zeros((5, n_bins), np.float64)
    for _, pos, span, w, hmm, _ in info["places"]:
        bins = (pos + np.arange(span)) // bin_size
        np.add.at(cov, bins, float(w))
        prod = (hmm * w).astype(np.float64)                     # float32 x float32 -> float32, then widened
        for c in range(5):
            np.add.at(nuc[c], bins, prod[:, c])
    return cov, nuc


def snp_exact_bins(info, n_bins):
    """at bin size 1, the bins that exactly ONE place covers: no addition order to allow for, so the device has to hold float32(w) and
    float32(hmm) * float32(w) there bit for bit.  Returns (bins, coverage bits, track bits [5][len(bins)], under an other-strand place)"""
    cnt = np.zeros(n_bins, np.int32)
    for _, pos, span, *_ in info["places"]:
        cnt[pos:pos + span] += 1
    cov = np.zeros(n_bins, np.float32); nuc = np.zeros((5, n_bins), np.float32); other = np.zeros(n_bins, bool)
    for _, pos, span, w, hmm, oth in info["places"]:
        one = np.flatnonzero(cnt[pos:pos + span] == 1)
        cov[pos + one] = w
        nuc[:, pos + one] = (hmm[one] * w).T
        other[pos + one] = oth
    bins = np.flatnonzero(cnt == 1)
    return bins, cov[bins].view(np.uint32), nuc[:, bins].view(np.uint32), other[bins]


def snp_edge_positions(oix, block):
    """the positions a --snp deposit has to touch: 0, l_pac - 1 and both sides of every inner contig start of the edge genome; in both.fa
    the planted segment stands at the start of the third contig and ends at l_pac (nothing is planted at 0 or before the third contig)"""
    ctg, l_pac = geometry(oix)
    if block == "both":
        return [ctg[2][0], l_pac - 1]
    return [0, l_pac - 1] + [x for b, _ in ctg[1:] for x in (b - 1, b)]


def guard_snp_other_strand(info, at_least=100):
    n = sum(1 for p in info["places"] if p[5])
    assert n >= at_least, n
    return n


def guard_snp_n_sequences(info, at_least=20):
    n = sum(1 for k in info["kept"] if k[3])
    assert n >= at_least, n
    return n


def guard_snp_kept(info, more_than):
    assert len(info["kept"]) > more_than, len(info["kept"])
    return len(info["kept"])


def guard_snp_lengths(info, at_least=5):
    lens = sorted({k[4] for k in info["kept"]})
    assert len(lens) >= at_least, lens
    return lens


def guard_snp_deposits_touch(info, positions):
    """every one of `positions` lies under a deposit of weight > 0.5 in all"""
    for x in positions:
        assert sum(float(w) for _, pos, span, w, _, _ in info["places"] if pos <= x < pos + span) > 0.5, x


SNP_SINGLE = ("b0_cut_L150_f", "b0_cut_L150_r", "b7_cut_L36_f", "b7_n_L36_r", "b126_cut_L24_f", "b126_cut_L24_r")


def snp_single_reads(rd):
    """six reads of both.fq to map one read per batch: 150, 36 and 24 bases, forward and reverse, one with an N.  The four places of one
    read do not overlap, so every bin it covers is an exact bin, half of them under an other-strand place"""
    by_name = {r[0]: r for r in rd}
    return [by_name[n] for n in SNP_SINGLE]


def edge_genome():
    return b"".join(l.strip() for l in open(os.path.join(GOLDEN, "edge.fa"), "rb") if not l.startswith(b">")).upper()


def snp_interior_reads():
    """100-bp reads at disjoint windows inside the first contig of edge.fa (every 110 bases from 200 on), far from the edge reads: each
    has ONE place that nothing else covers, so all its bins are exact bins.  Alternating orientation, qualities Phred 5 .. 40 from a
    seeded generator, every third read with a substitution, every fifth with an N"""
    genome = edge_genome()
    rng = np.random.default_rng(4242)
    out = []
    for k, b in enumerate(range(200, 4701, 110)):
        s = bytearray(genome[b:b + 100])
        if k % 3 == 1:
            s[40] = b"ACGT"[(b"ACGT".index(s[40]) + 1) % 4]
        if k % 5 == 2:
            s[61] = ord("N")
        q = bytes((33 + rng.integers(5, 41, 100)).astype(np.uint8))
        out.append((f"in{b}_f", bytes(s), q) if k % 2 == 0 else (f"in{b}_r", revcomp_str(bytes(s)).upper(), q))
    return out


def snp_block_reads(block):
    """the reads of a block; edge_plus / mixed_plus: the file's reads between the two halves of the interior reads.  edge.fq and
    edge_mixed.fq alone have NO bin that one place covers (every read stands beside its reverse complement on the same window); with the
    interior reads around them the exact bins lie in the first and in the last chunk of kept sequences"""
    if block.endswith("_plus"):
        inner = snp_interior_reads()
        return inner[:len(inner) // 2] + reads(SNP_BLOCKS[block[:-5]][1]) + inner[len(inner) // 2:]
    return reads(SNP_BLOCKS[block][1])


def guard_snp_exact_bins(info, n_bins, at_least):
    bins, _, _, other = snp_exact_bins(info, n_bins)
    assert len(bins) >= at_least, len(bins)
    return len(bins), int(other.sum())
