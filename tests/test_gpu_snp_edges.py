"""--snp on the device at the edges: k_pair_hmm and k_snp_deposit (gnumap_amd/csrc/gm_snp.hip) and the SNP branch of output_batch_impl
(gm_api.cpp) where no other test reaches them.

  - reads shorter than their block's stride inside ONE pair-HMM block (the scratch of a lane is laid out for the stride, its loops run to
    the read's own length), short and long reads side by side in a wavefront, in two lane orders;
  - the --illumina table of a block whose first reads are Phred+64;
  - the deposit of a block against the oracle's deposits (tests/edge_fixture.py snp_info): places on the other strand than the kept
    sequence's first strand (the mirrored row with a/t and c/g swapped), reads with an N (the fifth track), position 0, l_pac - 1 and
    both sides of the inner contig starts, bin sizes 1 and 8, lengths 16 .. 150 in one block;
  - EXACT comparisons where the order of the fp32 atomic adds cannot matter: a bin that one place covers holds float32(w) and
    float32(hmm) * float32(w) bit for bit (a wrong row or a swapped pair of nucleotides on a few places hides inside the allowance of
    a whole-track comparison, not here);
  - several chunks of kept sequences (GM_SNP_CHUNK=64: chunks of 128; the number of chunks is read from the library's trace line);
  - gm_output_batch_text in GM_MODE_SNP: a call refused for capacity deposits nothing, the repeated call deposits once;
  - the driver on both.fq and on edge_mixed.fq in batches of 64 against the reference program's own --snp runs
    (tests/golden/ref_runs_snp_edge/), .gmp text written by the host and by the device.

The oracle side of every comparison is pinned to the reference program by tests/test_snp_edge_cpu.py; the guards of
tests/edge_fixture.py are asserted again here."""
import os
import re
import subprocess

import numpy as np
import pytest

import edge_fixture as ef
import gnumap_amd as g
from conftest import GOLDEN, ROOT
from test_gpu_driver_golden import compare_tracks
from test_gpu_edge_reads import _track_close
from test_gpu_edge_windows import argmax_cons, want

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
SNP = ef.GM_MODE_SNP
HMM_MIXED_LENS = (16, 33, 100, 150)
PER_LENGTH = 120


@pytest.fixture(scope="module")
def fastas(tmp_path_factory):
    return {"edge.fa": ef.build_index(tmp_path_factory), "both.fa": ef.build_index(tmp_path_factory, "both.fa")}


@pytest.fixture(scope="module")
def indexes(fastas):
    d = {k: g.Index(v, flags=g.GM_INDEX_FULL_SA) for k, v in fastas.items()}
    yield d
    for i in d.values():
        i.close()


@pytest.fixture(scope="module")
def oixs(oracle, fastas):
    d = {k: oracle.index_load(v) for k, v in fastas.items()}
    ef.check_geometry(d["edge.fa"])
    return d


@pytest.fixture(scope="module")
def genome(fastas):
    return b"".join(l.strip() for l in open(fastas["edge.fa"], "rb") if not l.startswith(b">")).upper()


_INFO = {}


def info_of(oracle, oixs, block):
    """the oracle's --snp deposits of a block, computed once and never changed, with the guards that belong to the block"""
    if block not in _INFO:
        fa = ef.SNP_BLOCKS[block.replace("_plus", "")][0]
        info = ef.snp_info(oracle, oixs[fa], ef.snp_block_reads(block))
        if block == "both":
            ef.guard_snp_other_strand(info); ef.guard_snp_n_sequences(info)
        if block.startswith("edge"):
            ef.guard_snp_kept(info, 128)
        if block.startswith("mixed"):
            ef.guard_snp_kept(info, 384); ef.guard_snp_lengths(info)
        if block.endswith("_plus"):
            ef.guard_snp_exact_bins(info, ef.geometry(oixs[fa])[1] + 64, 1000)
        ef.guard_snp_deposits_touch(info, ef.snp_edge_positions(oixs[fa], block.replace("_plus", "")))
        _INFO[block] = info
    return _INFO[block]


# ------------------------------------------------------------------ k_pair_hmm alone
_MIXED = {}


def mixed_probes(oracle, oix, genome):
    """the valid edge windows of four lengths, thinned to about PER_LENGTH per length (every (kind of read, strand) of a window stays
    together with equal share: k % 8 is the kind x strand of probes()), as ONE block of stride 152, with the oracle's rows"""
    if _MIXED:
        return _MIXED
    reads, quals, strand, pos, ref, amb = [], [], [], [], [], 0
    for L in HMM_MIXED_LENS:
        pr, o = want(oracle, oix, genome, L, 3, False, False)
        sel = np.flatnonzero(o["valid"])
        step = max(1, len(sel) // PER_LENGTH)
        sel = np.concatenate([sel[sel % 8 == c][::step] for c in range(8)])        # every read kind on both strands, the N reads (6, 7) too
        assert len(sel) >= 64 and {int(k) % 8 for k in sel} == set(range(8))
        for k in sel:
            reads.append(pr["reads"][k]); quals.append(pr["quals"][k]); strand.append(int(pr["strand"][k])); pos.append(int(pr["pos"][k]))
            P = o["P"][k]
            ref.append(oracle.pair_hmm(P, argmax_cons(P), o["w"][k]))
            amb += b"N" in pr["reads"][k]
    assert amb >= 60
    _MIXED.update(reads=reads, quals=quals, strand=np.array(strand, np.uint8), pos=np.array(pos, np.uint64), ref=ref)
    return _MIXED


def _assert_rows(out, order, m):
    for j, k in enumerate(order):
        L = len(m["reads"][k])
        assert np.array_equal(out[j, :L].view(np.uint32), m["ref"][k].view(np.uint32)), (L, int(m["pos"][k]), int(m["strand"][k]), j)
        assert not out[j, L:].any(), (L, j)                              # nothing written past the read's own rows


@pytest.mark.parametrize("order", ["as_listed", "reversed", "interleaved"])
def test_pair_hmm_mixed_lengths_in_one_block(order, indexes, oracle, oixs, genome):
    """16, 33, 100 and 150 bases in one block of stride 152: every lane indexes its scratch with the stride and loops to its own length.
    as_listed: a wavefront holds one length (and the next at the seams); reversed: the other lanes; interleaved: the four lengths lane
    by lane in every wavefront"""
    m = mixed_probes(oracle, oixs["edge.fa"], genome)
    n = len(m["reads"])
    assert 256 < n <= 4 * (PER_LENGTH + 24)
    idx = list(range(n))
    if order == "reversed":
        idx = idx[::-1]
    elif order == "interleaved":
        idx = sorted(idx, key=lambda k: (k % (n // 4), k))
    B, Q, Ln = g.pack_reads([m["reads"][k] for k in idx], [m["quals"][k] for k in idx])
    assert B.shape[1] == 152 and len(set(Ln[:64].tolist())) == (4 if order == "interleaved" else 1)
    out = indexes["edge.fa"].dev_pair_hmm(g.Params(mode=SNP), B, Q, Ln, np.arange(n, dtype=np.uint32), m["strand"][idx], m["pos"][idx])
    _assert_rows(out, idx, m)


def test_pair_hmm_does_not_depend_on_the_chunk_switch(indexes, oracle, oixs, genome):
    m = mixed_probes(oracle, oixs["edge.fa"], genome)
    n = len(m["reads"])
    B, Q, Ln = g.pack_reads(m["reads"], m["quals"])
    g.set_option("GM_SNP_CHUNK", "64")
    try:
        out = indexes["edge.fa"].dev_pair_hmm(g.Params(mode=SNP), B, Q, Ln, np.arange(n, dtype=np.uint32), m["strand"], m["pos"])
    finally:
        g.set_option("GM_SNP_CHUNK", None)
    _assert_rows(out, range(n), m)


def test_pair_hmm_illumina_rows(indexes, oracle, oixs, genome):
    """--illumina: the reads before the first one that shows a quality below '@' take the Phred+64 table (`lut + 256`), that read and
    all later ones Phred+33 - the same block, the same lanes of one wavefront"""
    oix = oixs["edge.fa"]
    pr, o = want(oracle, oix, genome, 100, 3, False, False)
    sel = np.flatnonzero(o["valid"])[:96:2][:40]                         # forward probes of every kind
    sel = np.concatenate([sel, np.flatnonzero(o["valid"])[1:96:2][:24]])  # ... and reverse ones
    n64 = 23                                                             # not a multiple of anything
    reads, quals, rows = [], [], []
    for j, k in enumerate(sel):
        s, q = pr["reads"][k], pr["quals"][k]
        ill = 1 if j < n64 else 0
        if ill:
            q = bytes(c + 31 for c in q)                                 # Phred+33 '#'.. 'I' -> Phred+64 'B' .. 'h'
            assert min(q) >= 64
        elif j == n64:
            assert min(q) < 64                                           # this read switches the table off
        P = oracle.pwm(s, q, illumina=ill)
        if pr["strand"][k]:
            P = np.ascontiguousarray(P[::-1, ::-1])
        rows.append(oracle.pair_hmm(P, argmax_cons(P), o["w"][k]))
        reads.append(s); quals.append(q)
    B, Q, Ln = g.pack_reads(reads, quals)
    ix = indexes["edge.fa"]
    args = (B, Q, Ln, np.arange(len(sel), dtype=np.uint32), pr["strand"][sel], pr["pos"][sel])
    out = ix.dev_pair_hmm(g.Params(mode=SNP, illumina=1), *args)
    for j in range(len(sel)):
        assert np.array_equal(out[j, :100].view(np.uint32), rows[j].view(np.uint32)), (j, j < n64)
    # the table matters: without --illumina the Phred+64 rows come out different
    plain = ix.dev_pair_hmm(g.Params(mode=SNP), *args)
    assert all(not np.array_equal(plain[j, :100], rows[j]) for j in range(n64))
    assert all(np.array_equal(plain[j, :100].view(np.uint32), rows[j].view(np.uint32)) for j in range(n64, len(sel)))


# ------------------------------------------------------------------ the deposit
def run_block(ix, rd, bin_size, switches=None, text=False, text_cap=None, mode=SNP):
    """map + output (or output_text) of one block on freshly reset tracks: dict(recs, cigars | text, cov, nuc, text_calls)"""
    p = g.Params(mode=mode, bin_size=bin_size)
    B, Q, Ln = g.pack_reads([r[1] for r in rd], [r[2] for r in rd])
    sw = dict(switches or {})
    ix.coverage_reset(bin_size); ix.coverage_enable_nuc()
    for k, v in sw.items():
        g.set_option(k, v)
    batch = g.Batch(ix, len(rd), B.shape[1])
    try:
        res = batch.map(p, B, Q, Ln)
        out = {}
        if text:
            out["text"], _ = batch.output_text(p, res, [r[0].encode() for r in rd], text_cap=text_cap)
            out["text_calls"] = batch.text_calls
        else:
            out["recs"], out["cigars"] = batch.output(p, res)
        out["cov"] = ix.coverage_download(); out["nuc"] = ix.coverage_download_nuc().reshape(5, -1)
    finally:
        for k in sw:
            g.set_option(k, None)
        batch.destroy()
        ix.coverage_reset(8)
    return out


def assert_tracks(out, info, bin_size):
    """coverage and the five tracks against the oracle's deposits within the allowance of compare_tracks"""
    want_cov, want_nuc = ef.snp_tracks(info, len(out["cov"]), bin_size)
    _track_close(out["cov"].astype(np.float64), want_cov)
    _track_close(out["nuc"].astype(np.float64).ravel(), want_nuc.ravel())
    return want_cov, want_nuc


def assert_exact(out, info):
    """bin size 1: the bins one place covers, bit for bit.  Returns (number of such bins, how many lie under an other-strand place)"""
    bins, cov, nuc, other = ef.snp_exact_bins(info, len(out["cov"]))
    bad = np.flatnonzero(out["cov"][bins].view(np.uint32) != cov)
    assert len(bad) == 0, [(int(bins[k]), float(out["cov"][bins[k]])) for k in bad[:8]]
    got = out["nuc"][:, bins].view(np.uint32)
    bad = np.argwhere(got != nuc)
    assert len(bad) == 0, [(int(c), int(bins[k]), bool(other[k]), float(out["nuc"][c, bins[k]]), float(nuc[c, k:k + 1].view(np.float32)[0])) for c, k in bad[:8]]
    return len(bins), int(other.sum())


def got_records(out):
    return [(int(r["read"]), int(r["contig"]), int(r["chr_pos"]), int(r["strand"]), int(r["mapq"]), c) for r, c in zip(out["recs"], out["cigars"])]


@pytest.mark.parametrize("bin_size", [1, 8])
@pytest.mark.parametrize("block", ["edge", "mixed", "both", "edge_plus"])
def test_deposit_matches_oracle(block, bin_size, indexes, oracle, oixs):
    """edge_plus: edge.fq between the interior reads of ef.snp_interior_reads() - edge.fq, edge_mixed.fq and both.fq alone have no bin
    that ONE place covers (every read stands beside its reverse complement, or beside the other cuts of the segment)"""
    fa = ef.SNP_BLOCKS[block.replace("_plus", "")][0]
    rd = ef.snp_block_reads(block)
    info = info_of(oracle, oixs, block)
    out = run_block(indexes[fa], rd, bin_size)
    # --snp does not change the mapping or the records
    dflt = run_block(indexes[fa], rd, bin_size, mode=0)
    assert out["recs"].tobytes() == dflt["recs"].tobytes() and list(out["cigars"]) == list(dflt["cigars"])
    assert got_records(out) == info["recs"] and len(info["recs"]) > 80
    want_cov, want_nuc = assert_tracks(out, info, bin_size)
    for pos in ef.snp_edge_positions(oixs[fa], block.replace("_plus", "")):      # the bins this is about are covered
        assert want_cov[pos // bin_size] > 0.5 and out["cov"][pos // bin_size] > 0.5, pos
    l_pac = ef.geometry(oixs[fa])[1]
    assert not out["cov"][(l_pac - 1) // bin_size + 1:].any() and not out["nuc"][:, (l_pac - 1) // bin_size + 1:].any()
    if block == "both":
        n_sum = float(out["nuc"][4].astype(np.float64).sum())
        allowed = float((1e-4 * np.maximum(1.0, want_nuc[4]) + 2e-5)[want_nuc[4] > 0].sum())       # _track_close's allowance, bin by bin
        assert want_nuc[4].sum() > 10.0 and abs(n_sum - want_nuc[4].sum()) <= allowed
    if bin_size == 1:
        n_exact, n_other = assert_exact(out, info)
        assert n_exact >= (1000 if block == "edge_plus" else 0), n_exact


def test_exact_bins_under_other_strand_places(indexes, oracle, oixs):
    """six reads of both.fq, one read per batch on reset tracks: four places each that do not overlap, two of them on the other strand.
    EVERY covered bin is exact: the row of the mirrored position, a <-> t and c <-> g swapped, n kept, times the weight"""
    rd = ef.snp_single_reads(ef.reads("both.fq"))
    oix = oixs["both.fa"]
    n_all = n_other = 0
    n_track = 0.0
    for r in rd:
        info = ef.snp_info(oracle, oix, [r])
        assert len(info["places"]) == 4 and sum(p[5] for p in info["places"]) == 2, r[0]
        out = run_block(indexes["both.fa"], [r], 1)
        a, b = assert_exact(out, info)
        assert a == 4 * len(r[1]) == int((out["cov"] > 0).sum()) and b == 2 * len(r[1]), (r[0], a, b)
        n_all += a; n_other += b
        if b"N" in r[1]:
            # the fifth track: the N's posterior weight (about 1 at its position) times the weights of the four places, which add up to
            # the read's whole posterior; its bins are exact bins, so the device holds the oracle's bits there (checked above)
            n_track = sum(float((hmm[:, 4] * w).sum()) for _, _, _, w, hmm, _ in info["places"])
            assert n_track > 0.9 and float(out["nuc"][4].sum()) > 0.9, (n_track, float(out["nuc"][4].sum()))
    assert n_other >= 300 and n_all - n_other >= 300 and n_track > 0.9


# ------------------------------------------------------------------ several chunks of kept sequences
def chunks_traced(err):
    return [(int(a), int(b), int(c)) for a, b, c in re.findall(r"snp deposit: (\d+) kept sequences, chunks of (\d+): (\d+) chunks?", err)]


@pytest.mark.parametrize("block,at_least", [("edge_plus", 2), ("mixed_plus", 4)])
def test_deposit_in_several_chunks(block, at_least, indexes, oracle, oixs, capfd):
    """GM_SNP_CHUNK=64: the loop over chunks runs more than once - tb_items + m0, matches[m0 + block], the rows of the chunk's own hmm
    buffer.  Same tracks as in one chunk, same exact bins: the interior reads around edge.fq / edge_mixed.fq put exact bins under the
    FIRST and under the LAST chunk (mixed_plus: 100-base reads in rows of stride 152)"""
    fa = ef.SNP_BLOCKS[block.replace("_plus", "")][0]
    rd = ef.snp_block_reads(block)
    info = info_of(oracle, oixs, block)
    capfd.readouterr()
    out = run_block(indexes[fa], rd, 1, dict(GM_SNP_CHUNK="64", GM_TRACE="1"))
    traced = chunks_traced(capfd.readouterr().err)
    assert len(traced) == 1, traced
    n_kept, chunk, n_chunks = traced[0]
    assert n_chunks >= at_least and n_kept > (n_chunks - 1) * chunk, traced
    one = run_block(indexes[fa], rd, 1, dict(GM_TRACE="1"))
    traced_one = chunks_traced(capfd.readouterr().err)
    assert len(traced_one) == 1 and traced_one[0][2] == 1 and traced_one[0][0] == n_kept, traced_one
    assert_tracks(out, info, 1)
    n_exact, _ = assert_exact(out, info)
    assert n_exact >= 1000
    # ... and they do lie in the first and in the last chunk: kept sequences are in read order, the interior reads come first and last
    assert info["kept"][0][0] == 0 and info["kept"][-1][0] == len(rd) - 1 and rd[0][0].startswith("in") and rd[-1][0].startswith("in")
    bins = ef.snp_exact_bins(info, len(out["cov"]))[0]
    assert np.array_equal(out["nuc"][:, bins].view(np.uint32), one["nuc"][:, bins].view(np.uint32))
    _track_close(out["nuc"].astype(np.float64).ravel(), one["nuc"].astype(np.float64).ravel())
    _track_close(out["cov"].astype(np.float64), one["cov"].astype(np.float64))


# ------------------------------------------------------------------ text output in SNP mode
def test_output_text_in_snp_mode_deposits_once(indexes, oracle, oixs):
    """gm_output_batch_text with a text buffer of one byte: the first call returns GM_E_CAPACITY BEFORE the SNP branch deposits, the
    repeated call deposits once"""
    rd = ef.snp_block_reads("mixed_plus")
    info = info_of(oracle, oixs, "mixed_plus")
    ix = indexes["edge.fa"]
    txt = run_block(ix, rd, 1, text=True, text_cap=1)
    assert txt["text_calls"] >= 2
    rec = run_block(ix, rd, 1)
    assert_tracks(txt, info, 1)
    _track_close(txt["cov"].astype(np.float64), rec["cov"].astype(np.float64))
    _track_close(txt["nuc"].astype(np.float64).ravel(), rec["nuc"].astype(np.float64).ravel())
    n_exact, _ = assert_exact(txt, info)
    assert n_exact >= 1000
    dflt = run_block(ix, rd, 1, text=True, mode=0)
    assert txt["text"] == dflt["text"] and txt["text"].count(b"\n") == len(info["recs"]) > 80


# ------------------------------------------------------------------ the driver
@pytest.mark.parametrize("run,extra", [("both", []), ("mixed", ["--batch=64"])], ids=["both", "mixed_batch64"])
def test_cli_snp_on_the_edge_fixtures_equals_reference_program(run, extra, fastas, indexes, tmp_path):
    """gnumap --snp against the reference program's own --snp run: SAM identical, the first eight columns of the .gmp within the allowance
    of compare_tracks; --batch=64 on the mixed lengths gives several batches with different strides; with --track_text=host and with
    --track_text=device.

    Host text against device text: the two files of the two driver runs are NOT the same bytes and cannot be - each run deposits anew,
    and two deposits differ in the order of their fp32 atomic adds (seen on the MI355X: both.gmp first differs at byte 423, a fifth
    decimal '1' / '0'; mixed at byte 24, '5' / '4').  Between the runs the allowance of compare_tracks holds; the same bytes are
    demanded where they can be had, from the two writers on ONE deposit of the same reads in the same batches through the library."""
    import json
    from test_gpu_track_text import _device_file, _host_file
    m = json.load(open(os.path.join(ef.SNP_RUNS, "manifest.json")))[run]
    ref_sam = ef.snp_ref_text(run, "sam").decode()
    ref_gmp = "".join("\t".join(l.split("\t")[:8]) + "\n" for l in ef.snp_ref_text(run, "gmp").decode().splitlines())
    texts = {}
    for where in ("host", "device"):
        out = str(tmp_path / where)
        r = subprocess.run([EXE, "-g", fastas[m["genome"]], "-o", out, "-a", "0.9"] + m["argv"] + extra + ["--track_text=" + where, os.path.join(GOLDEN, m["fastq"])],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        sam = "".join(l for l in open(out + ".sam") if not l.startswith("@PG"))
        assert sam == ref_sam, where
        assert not os.path.exists(out + ".sgr")
        texts[where] = open(out + ".gmp", "rb").read()
        compare_tracks(texts[where].decode(), ref_gmp, 8)
    assert len(texts["host"]) > 10000
    compare_tracks(texts["device"].decode(), texts["host"].decode(), 8)
    # one deposit, two writers: the same bytes
    ix = indexes[m["genome"]]
    rd = ef.reads(m["fastq"])
    p = g.Params(mode=SNP)
    per = 64 if extra else len(rd)
    ix.coverage_reset(1); ix.coverage_enable_nuc()
    try:
        for lo in range(0, len(rd), per):
            part = rd[lo:lo + per]
            B, Q, Ln = g.pack_reads([r[1] for r in part], [r[2] for r in part])
            batch = g.Batch(ix, len(part), B.shape[1])
            try:
                batch.output(p, batch.map(p, B, Q, Ln))
            finally:
                batch.destroy()
        cov = ix.coverage_download(); nuc = ix.coverage_download_nuc()
        host = _host_file(ix, p, cov, nuc, str(tmp_path / "lib_host.gmp"))
        dev = _device_file(ix, p, str(tmp_path / "lib_device.gmp"))
    finally:
        ix.coverage_reset(8)
    assert host == dev and len(host) > 10000
    compare_tracks(host.decode(), ref_gmp, 8)
