"""FASTA read files on the device: the kernels on FASTA-format blocks against the unmodified reference functions
(tests/golden/fasta_vectors.npz), FASTA against FASTQ where the two must agree, the kernel dispatch, and the driver against the outputs of
the UNMODIFIED reference program (tests/golden/ref_runs_fasta/): SAM text byte for byte, record order included; tracks within the
tolerance of tests/test_gpu_driver_golden.py.  Fixtures: tests/golden/make_fasta_fixtures.py."""
import gzip
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
from conftest import GOLDEN, ROOT
from fasta_model import parse_fasta, pwm_rows
from test_gpu_driver_golden import compare_tracks

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "ref_runs_fasta")
MANIFEST = json.load(open(os.path.join(RUNS, "manifest.json")))
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
GM_E_UNSUPPORTED = -6


@pytest.fixture(scope="module")
def ix(syn_fa):
    i = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    yield i
    i.close()


@pytest.fixture(scope="module")
def vec():
    return np.load(os.path.join(GOLDEN, "fasta_vectors.npz"))


def ref_text(mode, ext):
    return gzip.open(os.path.join(RUNS, f"{mode}.{ext}.gz"), "rt").read()


def records(fa):
    return parse_fasta(open(os.path.join(GOLDEN, fa), "rb").read())


def rle(ops: bytes) -> bytes:
    return b"".join(str(len(list(grp))).encode() + bytes([k]) for k, grp in itertools.groupby(ops))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hits(res):
    m = res["matches"]
    pos = [res["positions"][f][int(a):int(b)].tolist() for a, b in zip(m["pos_begin"], m["pos_end"]) for f in ("pos", "strand")]
    return (res["status"].tobytes(), res["denominator"].tobytes(), res["top_score"].tobytes(), res["match_begin"].tobytes(),
            [m[f].tobytes() for f in ("read", "score", "first_pos", "first_strand")], pos)


# ------------------------------------------------------------------ unit probes against the reference's functions
def test_self_score_bits(ix, vec):
    """k_prep_rows: S's row of the RAW character (K and k are different rows) dotted with the letter's row, summed in index order"""
    seqs = [bytes(s) for s in vec["read_seq"]]
    B, Q, Ln = g.pack_reads(seqs)
    assert Q is None
    batch = g.Batch(ix, len(seqs), B.shape[1])
    res = batch.map(g.Params(), B, None, Ln, fasta=True)
    assert "reads=fasta" in batch.path(), batch.path()
    np.testing.assert_array_equal(bits(res["self_score"]), bits(vec["self_score"]))
    # rows longer than 152 bytes take k_prep: the same reads at a stride of 160
    B2, _, Ln2 = g.pack_reads(seqs, None, 160)
    res2 = batch.map(g.Params(), B2, None, Ln2, fasta=True)
    np.testing.assert_array_equal(bits(res2["self_score"]), bits(vec["self_score"]))
    assert _hits(res2) == _hits(res)
    # -b edits lower-case rows of S only (S['c'][t] becomes a match): the term of a position is S's row of the RAW character dotted
    # with its letter's row, summed in fp32 in index order - restated here from the parameters the library itself finalized
    pb = g.Params(mode=1)
    rb = batch.map(pb, B, None, Ln, fasta=True)
    S = np.array([[pb.c.S[c][k] for k in range(4)] for c in range(256)], np.float32)
    assert S[ord("c"), 3] == S[ord("c"), 1] and S[ord("C"), 3] != S[ord("C"), 1]
    n_lower = 0
    for i in range(0, len(seqs), 7):
        want = np.float32(0)
        for ch, row in zip(seqs[i], pwm_rows(seqs[i])):
            t = np.float32(np.float32(row[0] * S[ch, 0]) + np.float32(row[1] * S[ch, 1]))
            t = np.float32(t + np.float32(row[2] * S[ch, 2]))
            t = np.float32(t + np.float32(row[3] * S[ch, 3]))
            want = np.float32(want + t)
        assert bits(rb["self_score"][i:i + 1])[0] == bits(np.array([want]))[0], i
        n_lower += seqs[i] != seqs[i].upper()
    assert n_lower >= 3
    batch.destroy()


@pytest.mark.parametrize("switch", [None, ("GM_NW", "lane"), ("GM_NW_ROWS", "0")], ids=["default", "lane", "lane_streaming"])
def test_nw_score_bits(ix, vec, switch):
    seqs = [bytes(s) for s in vec["read_seq"]]
    B, _, Ln = g.pack_reads(seqs)
    if switch:
        g.set_option(*switch)
    try:
        score, valid = ix.dev_nw_score(g.Params(), B, None, Ln, vec["nw_read"], vec["nw_rc"].astype(np.uint8), vec["nw_begin"], fasta=True)
    finally:
        if switch:
            g.set_option(switch[0], None)
    assert valid.all()
    np.testing.assert_array_equal(bits(score), bits(vec["nw_score"]))


def test_traceback_ops_and_cigars(ix, vec):
    seqs = [bytes(s) for s in vec["read_seq"]]
    B, _, Ln = g.pack_reads(seqs)
    ops = ix.dev_traceback(g.Params(), B, None, Ln, vec["nw_read"], vec["nw_rc"].astype(np.uint8), vec["nw_begin"], fasta=True)
    n_gapped = 0
    for i, o in enumerate(ops):
        assert len(o) == vec["tb_len"][i], i
        assert rle(o) == bytes(vec["tb_cigar"][i]), i
        aligned = bytes.fromhex(vec["tb_aligned_hex"][i].decode())
        assert [c == ord("-") for c in aligned] == [c == ord("D") for c in o], i          # the gaps of the reference's aligned string
        n_gapped += b"I" in o or b"D" in o
    assert n_gapped > 100


def test_probes_on_a_one_length_block_take_k_nw_rows_in_both_cell_forms(ix, vec):
    """the 100-bp reads of the vectors as a block of their own: k_nw_rows with the pair table, with GM_NW_CELLS=b32, and k_nw_lane"""
    seqs = [bytes(s) for s in vec["read_seq"]]
    keep = [i for i, s in enumerate(seqs) if len(s) == 100]
    renum = {r: k for k, r in enumerate(keep)}
    sel = [k for k, r in enumerate(vec["nw_read"]) if int(r) in renum]
    assert len(keep) > 100 and len(sel) > 200
    B, _, Ln = g.pack_reads([seqs[i] for i in keep])
    ridx = np.array([renum[int(vec["nw_read"][k])] for k in sel], np.uint32)
    args = (ridx, vec["nw_rc"][sel].astype(np.uint8), vec["nw_begin"][sel])
    want = bits(vec["nw_score"][sel])
    for name, value in ((None, None), ("GM_NW_CELLS", "b32"), ("GM_NW", "lane")):
        if name:
            g.set_option(name, value)
        try:
            score, valid = ix.dev_nw_score(g.Params(), B, None, Ln, *args, fasta=True)
        finally:
            if name:
                g.set_option(name, None)
        np.testing.assert_array_equal(bits(score), want, err_msg=str((name, value)))


@pytest.mark.parametrize("G", [1, 5])
def test_band_kernels_against_the_reference_program_rows(ix, G):
    """-M other than 3 (k_nw_band / k_traceback_band): the library's records on the FASTA fixture = the reference program's rows"""
    mode = "M%d" % G
    recs = records(MANIFEST[mode]["fasta"])
    B, _, Ln = g.pack_reads([s for _, s in recs])
    p = g.Params(max_gap=G)
    batch = g.Batch(ix, len(recs), B.shape[1])
    ix.coverage_reset(8)
    res = batch.map(p, B, None, Ln, fasta=True)
    text, _ = batch.output_text(p, res, [n for n, _ in recs])
    assert "nw=k_nw_band" in batch.path()
    assert text.decode() == "".join(l for l in ref_text(mode, "sam").splitlines(True) if not l.startswith("@"))
    batch.destroy()


# ------------------------------------------------------------------ FASTA against FASTQ
def test_acgt_only_fasta_block_equals_the_fastq_block(ix):
    """reads that hold only ACGT: seeds, votes, candidate positions, strands and CIGARs do not depend on the format.  The FASTQ block
    carries quality '~' (Q 93): p = 1 - 5e-10 is 1.0f and q = 1.7e-10 vanishes in every fp32 sum next to a score of 0.5 .. 0.75, so its
    rows give the values of the FASTA rows (1, 0, 0, 0) bit for bit.  (With quality 'I', p = 0.9999, an exact tie between two paths of
    the FASTA DP is a near-tie in the FASTQ DP and the two tracebacks may legitimately pick different, equally good CIGARs: measured on
    this fixture, 1I13M1D86M against 1I11M1D88M for one read of 399.)"""
    recs = [(n, s.upper()) for n, s in records("syn_reads.fa") if all(chr(c) in "ACGTacgt" for c in s)]
    assert len(recs) > 300
    seqs = [s for _, s in recs]
    Bq, Q, Ln = g.pack_reads(seqs, [b"~" * len(s) for s in seqs])
    Bf, _, _ = g.pack_reads(seqs)
    fq, fa = g.Batch(ix, len(seqs), Bq.shape[1]), g.Batch(ix, len(seqs), Bq.shape[1])
    key = lambda h: sorted(zip(h["read"].tolist(), h["pos"].tolist(), h["strand"].tolist(), h["score"].tolist()))
    # --no_nw: the accepted hits ARE the candidates, scored by their vote counts - the seed and vote side, exactly
    pv = g.Params(nw=0)
    fq.map(pv, Bq, Q, Ln); fa.map(pv, Bf, None, Ln, fasta=True)
    hq, _, _, _ = fq.raw_hits(); hf, _, _, _ = fa.raw_hits()
    assert key(hq) == key(hf) and len(hq) > 300
    p = g.Params(print_all_sam=1, align_score=0.8)
    rq = fq.map(p, Bq, Q, Ln)
    rf = fa.map(p, Bf, None, Ln, fasta=True)
    assert "reads=fastq" in fq.path() and "reads=fasta" in fa.path()
    assert fq.path().replace("reads=fastq", "") == fa.path().replace("reads=fasta", "")
    cq, cf = fq.counters(), fa.counters()
    for k in ("kmers_searched", "seeds_used", "sa_hits", "candidates"):
        assert cq[k] == cf[k], k
    np.testing.assert_array_equal(rq["match_begin"], rf["match_begin"])
    for f in ("read", "score", "first_pos", "first_strand", "pos_begin", "pos_end"):
        np.testing.assert_array_equal(rq["matches"][f], rf["matches"][f])
    np.testing.assert_array_equal(bits(rq["self_score"]), bits(rf["self_score"]))
    recq, cigq = fq.output(p, rq); recf, cigf = fa.output(p, rf)
    assert cigq == cigf and len(cigq) > 300
    for f in ("read", "pos", "strand", "contig", "chr_pos"):
        np.testing.assert_array_equal(recq[f], recf[f])
    fq.destroy(); fa.destroy()


def test_an_ambiguity_code_seeds_like_n(ix):
    """every letter outside ACGTacgt ends a k-mer like N: a read with K gets the candidates of the same read with N there"""
    recs = [s.upper() for _, s in records("syn_reads_u100.fa") if all(chr(c) in "ACGTacgt" for c in s)][:64]
    rng = np.random.default_rng(3)
    with_k, with_n = [], []
    for i, s in enumerate(recs):
        pos = sorted(rng.choice(100, 1 + i % 3, replace=False))
        a, b = bytearray(s), bytearray(s)
        for q, code in zip(pos, "KkRyBv"):
            a[q] = ord(code); b[q] = ord("N")
        with_k.append(bytes(a)); with_n.append(bytes(b))
    p = g.Params(nw=0)                                                   # --no_nw: the score is the vote count, the hits are the candidates
    out = []
    for seqs in (with_k, with_n):
        B, _, Ln = g.pack_reads(seqs)
        batch = g.Batch(ix, len(seqs), B.shape[1])
        res = batch.map(p, B, None, Ln, fasta=True)
        h, status, _, _ = batch.raw_hits()
        out.append((sorted(zip(h["read"].tolist(), h["pos"].tolist(), h["strand"].tolist(), h["score"].tolist())), status.tobytes(), batch.counters()))
        batch.destroy()
        del res
    assert out[0][0] == out[1][0] and len(out[0][0]) >= 64
    assert out[0][1] == out[1][1]
    for k in ("kmers_searched", "seeds_used", "sa_hits", "candidates"):
        assert out[0][2][k] == out[1][2][k], k


# ------------------------------------------------------------------ dispatch
def _u100():
    recs = records("syn_reads_u100.fa")
    B, _, Ln = g.pack_reads([s for _, s in recs])
    return recs, B, Ln


def test_one_length_block_takes_k_nw_rows(ix):
    recs, B, Ln = _u100()
    p = g.Params()
    batch = g.Batch(ix, len(recs), B.shape[1])
    res = batch.map(p, B, None, Ln, fasta=True)
    assert "nw=k_nw_rows/pairs" in batch.path() and "reads=fasta" in batch.path(), batch.path()
    want = _hits(res), res["self_score"].copy()
    ix.coverage_reset(8)
    text, _ = batch.output_text(p, res, [n for n, _ in recs])
    assert text.decode() == "".join(l for l in ref_text("u100", "sam").splitlines(True) if not l.startswith("@"))
    with pytest.raises(g.GnumapError) as e:                              # no quality line, so no tail of one: refused, not misprinted
        batch.output_text(p, res, [n for n, _ in recs], qual_tails=[b"II"] * len(recs))
    assert e.value.code == -1 and "qual_tail" in str(e.value)
    for name, value, form in (("GM_NW_CELLS", "b32", "nw=k_nw_rows/cells"), ("GM_NW", "lane", "nw=k_nw_lane")):
        g.set_option(name, value)
        try:
            got = batch.map(p, B, None, Ln, fasta=True)
            assert form in batch.path(), batch.path()
        finally:
            g.set_option(name, None)
        assert _hits(got) == want[0], name
        np.testing.assert_array_equal(got["self_score"], want[1])
    batch.destroy()


def test_forced_fastq_only_form_is_refused_by_name(ix, vec):
    """GM_NW=wave forces k_nw, the one DP form that was not taught FASTA blocks: GM_E_UNSUPPORTED naming the switch, from the batch call and
    from the score probe; the traceback probe, which does not run that kernel, is not affected; a FASTQ block still takes the switch"""
    recs, B, Ln = _u100()
    p = g.Params()
    batch = g.Batch(ix, len(recs), B.shape[1])
    g.set_option("GM_NW", "wave")
    try:
        with pytest.raises(g.GnumapError) as e:
            batch.map(p, B, None, Ln, fasta=True)
        assert e.value.code == GM_E_UNSUPPORTED and "GM_NW=wave" in str(e.value), str(e.value)
        with pytest.raises(g.GnumapError) as e:
            ix.dev_nw_score(p, B, None, Ln, [0], [0], [1000], fasta=True)
        assert e.value.code == GM_E_UNSUPPORTED and "GM_NW=wave" in str(e.value), str(e.value)
        assert len(ix.dev_traceback(p, B, None, Ln, [0], [0], [1000], fasta=True)) == 1
        Q = np.full(B.shape, ord("I"), np.uint8)
        B2 = np.where(np.isin(B, list(b"ACGTacgt")) | (B == 0), B, ord("N")).astype(np.uint8)
        res = batch.map(p, B2, Q, Ln)
        assert (res["status"] == 0).sum() > 50
    finally:
        g.set_option("GM_NW", None)
    batch.destroy()


@pytest.mark.parametrize("name,value", [("GM_PREP", "tile"), ("GM_TRACEBACK", "group")])
def test_long_row_kernel_forms_give_the_same_results(ix, vec, name, value):
    """k_prep and k_traceback are what rows beyond 152 / 511 bytes take; the switches force them on the fixture's short reads: hits, self
    scores, records and CIGARs of the mixed-length FASTA block do not change, and k_traceback's operations equal the reference's"""
    recs = records("syn_reads.fa")
    B, _, Ln = g.pack_reads([s for _, s in recs])
    p = g.Params()
    batch = g.Batch(ix, len(recs), B.shape[1])
    want = batch.map(p, B, None, Ln, fasta=True)
    recs_want, cig_want = batch.output(p, want)
    g.set_option(name, value)
    try:
        got = batch.map(p, B, None, Ln, fasta=True)
        r2, c2 = batch.output(p, got)
        if name == "GM_TRACEBACK":
            seqs = [bytes(s) for s in vec["read_seq"]]
            Bv, _, Lv = g.pack_reads(seqs)
            ops = ix.dev_traceback(p, Bv, None, Lv, vec["nw_read"], vec["nw_rc"].astype(np.uint8), vec["nw_begin"], fasta=True)
    finally:
        g.set_option(name, None)
    assert _hits(got) == _hits(want) and len(cig_want) > 500
    np.testing.assert_array_equal(bits(got["self_score"]), bits(want["self_score"]))
    assert r2.tobytes() == recs_want.tobytes() and c2 == cig_want
    if name == "GM_TRACEBACK":
        assert [rle(o) for o in ops] == [bytes(c) for c in vec["tb_cigar"]]
    batch.destroy()


def test_long_fasta_reads_take_k_prep_and_k_traceback(ix, syn_fa):
    """rows beyond 152 and 511 bytes (k_prep, the streaming k_nw_lane, k_traceback): 600-bp reads cut from the first contig with two
    ambiguity codes and an N put in map where they were cut, with a 600M CIGAR"""
    genome = b"".join(l.strip() for l in open(syn_fa, "rb") if not l.startswith(b">"))
    first_len = 0
    for l in open(syn_fa, "rb"):
        if l.startswith(b">"):
            if first_len:
                break
        else:
            first_len += len(l.strip())
    seqs = []
    for k, p0 in enumerate((2000, 9000, 20000)):
        s = bytearray(genome[p0:p0 + 600].upper())
        assert p0 + 600 < first_len and all(chr(c) in "ACGT" for c in s)
        for q, code in zip((50 + 7 * k, 300, 520), "RyN"):
            s[q] = ord(code)
        seqs.append(bytes(s))
    B, _, Ln = g.pack_reads(seqs)
    assert B.shape[1] > 511
    p = g.Params()
    batch = g.Batch(ix, len(seqs), B.shape[1])
    res = batch.map(p, B, None, Ln, fasta=True)
    recs_, cig = batch.output(p, res)
    assert (res["status"] == 0).all()
    assert [int(x) for x in recs_["pos"]] == [2000, 9000, 20000] and cig == [b"600M"] * 3
    batch.destroy()


def test_adaptor_is_refused(ix):
    recs, B, Ln = _u100()
    batch = g.Batch(ix, len(recs), B.shape[1])
    batch.set_adaptor(b"AGATCGGAAGAGC")
    with pytest.raises(g.GnumapError) as e:
        batch.map(g.Params(), B, None, Ln, fasta=True)
    assert e.value.code == GM_E_UNSUPPORTED and "adaptor" in str(e.value)
    batch.destroy()


def test_fastq_after_fasta_on_one_batch_equals_a_fresh_batch(ix, syn_reads):
    """regression: a batch switched to FASTA and back maps FASTQ blocks exactly as a batch that never saw FASTA"""
    seqs = [r[1] for r in syn_reads]; quals = [r[2] for r in syn_reads]
    B, Q, Ln = g.pack_reads(seqs, quals)
    p = g.Params()
    fresh = g.Batch(ix, len(seqs), B.shape[1])
    want = fresh.map(p, B, Q, Ln)
    recs_want, cig_want = fresh.output(p, want)
    recs = records("syn_reads.fa")
    Bf, _, Lf = g.pack_reads([s for _, s in recs], None, B.shape[1])
    batch = g.Batch(ix, len(seqs), B.shape[1])
    first = batch.map(p, B, Q, Ln)
    assert _hits(first) == _hits(want)
    fa = batch.map(p, Bf, None, Lf, fasta=True)
    assert "reads=fasta" in batch.path() and _hits(fa) != _hits(want)
    got = batch.map(p, B, Q, Ln)
    assert batch.path() == fresh.path() and "reads=fastq" in batch.path()
    assert _hits(got) == _hits(want)
    np.testing.assert_array_equal(got["self_score"], want["self_score"])
    r2, c2 = batch.output(p, got)
    assert r2.tobytes() == recs_want.tobytes() and c2 == cig_want
    batch.destroy(); fresh.destroy()


# ------------------------------------------------------------------ the driver against the reference program
def _run_cli(mode, extra, tmp_path):
    m = MANIFEST[mode]
    out = str(tmp_path / "mine")
    argv = [os.path.join(GOLDEN, a) if a == "subst.txt" else a for a in m["argv"]]
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "-a", "0.9"] + argv + extra + [os.path.join(GOLDEN, m["fasta"])],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _assert_same_sam(sam, ref, what):
    if sam != ref:
        a, b = sam.splitlines(), ref.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{what}: {len(a)} vs {len(b)} lines, first difference at line {first}:\n  mine {a[first] if first < len(a) else None}\n  ref  {b[first] if first < len(b) else None}")


@pytest.mark.parametrize("text", ["host", "device"])
@pytest.mark.parametrize("extra", [[], ["--locate=sampled"], ["--batch=64", "--workers=2"], ["--chunk_reads=37", "--workers=3"]],
                         ids=["full_sa", "sampled_sa", "batch64", "chunks37"])
@pytest.mark.parametrize("mode", sorted(MANIFEST))
def test_cli_on_fasta_reads_equals_reference_program(mode, extra, text, tmp_path):
    m = MANIFEST[mode]
    out = _run_cli(mode, extra + ["--sam_text=" + text], tmp_path)
    _assert_same_sam("".join(l for l in open(out + ".sam") if not l.startswith("@PG")), ref_text(mode, "sam"), mode)
    ext = "sgr" if "sgr" in m["tracks"] else "gmp"
    assert not os.path.exists(out + (".gmp" if ext == "sgr" else ".sgr"))
    compare_tracks(open(out + "." + ext).read(), ref_text(mode, ext), 3 if ext == "sgr" else 8)


@pytest.mark.parametrize("mode,extra", [("default", ["--chunk_reads=50"]), ("bs", ["--sam_text=device", "--batch=100"])], ids=["default_chunks", "bs_device_blocks"])
def test_cli_shards_concatenate_to_the_single_file(mode, extra, tmp_path):
    out = _run_cli(mode, ["--sam_shards=3"] + extra, tmp_path)
    shards = [open(f"{out}.{k}.sam").read() for k in range(3)]
    assert sum(1 for s in shards if any(not l.startswith("@") for l in s.splitlines())) >= 2      # the split is not a no-op
    _assert_same_sam("".join(l for s in shards for l in s.splitlines(True) if not l.startswith("@PG")), ref_text(mode, "sam"), mode)


def test_cli_ignores_illumina_and_takes_a_last_line_without_newline(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_bytes(open(os.path.join(GOLDEN, "syn_reads.fa"), "rb").read().rstrip(b"\n"))
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "-a", "0.9", "--illumina", "--gpus=1", str(fa)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    _assert_same_sam("".join(l for l in open(out + ".sam") if not l.startswith("@PG")), ref_text("default", "sam"), "illumina")
