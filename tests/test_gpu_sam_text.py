"""SAM rows written on the device (gm_output_batch_text: k_out_text_sizes / k_out_text_rows, gm_output.hip) and sharded output.

* the driver with --sam_text=device against the outputs of the UNMODIFIED reference program, every mode of tests/golden/ref_runs/ and
  the celgen fixtures: SAM text byte-identical, tracks through test_gpu_driver_golden.compare_tracks;
* --sam_shards=K: the concatenation of the shards is the single-file SAM, for both --sam_text values;
* the ABI call against the formatter of tests/sam_text_model.py (Python's "%g" is C's), with the capacity retry, a 1500-byte name, lower-case
  and N bases on the minus strand, and the coverage track deposited exactly once;
* gm_dev_fmt_g6 against Python's "%g"."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
from conftest import CELGEN, GOLDEN, ROOT, read_fastq
from sam_text_model import check_text, revcomp, reverse_cigar, sam_rows  # noqa: F401 (other test files import them from here)
from test_gpu_driver_golden import compare_tracks

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "ref_runs")
MANIFEST = json.load(open(os.path.join(RUNS, "manifest.json")))
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
BATCHING_MODES = ("default", "no_nw", "bs_all", "T2", "u", "illumina", "k1_all", "m16_h150_all", "malformed", "malformed_tail")
ALL_MODES = sorted(m for m in MANIFEST if m.endswith("_all") or m == "all")


def ref_text(mode, ext):
    return gzip.open(os.path.join(RUNS, f"{mode}.{ext}.gz"), "rt").read()


def ref_rows(mode):
    return [l.split("\t") for l in ref_text(mode, "sam").splitlines() if not l.startswith("@")]


def run_driver(mode, extra, out, env=None):
    m = MANIFEST[mode]
    argv = [os.path.join(GOLDEN, a) if a == "subst.txt" else a for a in m["argv"]]
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "-a", "0.9"] + argv + extra + [os.path.join(GOLDEN, m["fastq"])],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def assert_same_sam(sam, ref, what):
    if sam != ref:
        a, b = sam.splitlines(), ref.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{what}: {len(a)} vs {len(b)} lines, first difference at line {first}:\n  mine {a[first] if first < len(a) else None}\n  ref  {b[first] if first < len(b) else None}")


def check_against_reference(mode, out):
    m = MANIFEST[mode]
    assert_same_sam("".join(l for l in open(out + ".sam") if not l.startswith("@PG")), ref_text(mode, "sam"), mode)
    if "sgr" in m["tracks"]:
        assert not os.path.exists(out + ".gmp")
        compare_tracks(open(out + ".sgr").read(), ref_text(mode, "sgr"), 3)
    else:
        assert not os.path.exists(out + ".sgr")
        compare_tracks(open(out + ".gmp").read(), ref_text(mode, "gmp"), 8)


def test_fixtures_cover_what_the_text_kernels_have_to_get_right():
    """what the reference program's outputs hold, so that byte equality below means something: minus-strand rows everywhere,
    exponent-form XP, a quality line longer than its sequence, --no_nw / -S / --illumina, indel CIGARs.  (--up_strand maps to the plus
    strand only: its fixture has no minus-strand row by construction, every other mode but the empty `fast` has at least 25.)"""
    assert len(MANIFEST) == 39 and len(ALL_MODES) == 11
    exp_xp = {}
    for mode in sorted(MANIFEST):
        rows = ref_rows(mode)
        if mode == "fast":
            assert rows == []
            continue
        assert len(rows) >= 101, mode
        minus = sum(r[1] == "16" for r in rows)
        if mode == "up":
            assert minus == 0 and "--up_strand" in MANIFEST[mode]["argv"]
        else:
            assert minus >= 25, mode
        exp_xp[mode] = sum(bool(re.fullmatch(r"XP:f:[0-9.]+e-[0-9]+", r[12])) for r in rows)
        assert all(r[5] != "*" for r in rows) and max(len(r[0]) for r in rows) <= 22
    assert [m for m in ALL_MODES if exp_xp[m] == 0] == ["illumina_all"]
    assert all(exp_xp[m] == 0 for m in exp_xp if m not in ALL_MODES)
    assert sum(len(r[9]) != len(r[10]) for mode in ("malformed", "malformed_tail") for r in ref_rows(mode)) >= 1
    assert any(re.search("[ID]", r[5]) for r in ref_rows("default"))
    for flag in ("--no_nw", "-S", "--illumina"):
        assert any(flag in MANIFEST[m]["argv"] for m in MANIFEST)


@pytest.mark.parametrize("mode", sorted(MANIFEST))
def test_cli_device_text_equals_reference_program(mode, tmp_path):
    out = str(tmp_path / "mine")
    r = run_driver(mode, ["--sam_text=device"], out)
    assert "gm_output_batch_text" in r.stderr and "SAM format" not in r.stderr      # the stage-seconds line names the path that ran
    check_against_reference(mode, out)


@pytest.mark.parametrize("extra", [["--locate=sampled"], ["--batch=64", "--workers=2"], ["--chunk_reads=37", "--workers=3"]], ids=["sampled_sa", "batch64", "chunks37"])
@pytest.mark.parametrize("mode", BATCHING_MODES)
def test_cli_device_text_with_batching_variants(mode, extra, tmp_path):
    out = str(tmp_path / "mine")
    run_driver(mode, ["--sam_text=device"] + extra, out)
    check_against_reference(mode, out)


@pytest.mark.parametrize("mode", ["default", "bs_all", "illumina"])
def test_cli_device_text_of_a_block_mapped_in_halves(mode, tmp_path):
    """process_block_split: the halves' text, one behind the other"""
    out = str(tmp_path / "mine")
    r = run_driver(mode, ["--sam_text=device"], out, env=dict(os.environ, GM_TEST_MAX_BLOCK="60"))
    assert "mapped in halves" in r.stderr
    check_against_reference(mode, out)


CELGEN_MODES = {"default": ([], "sgr"), "no_nw": (["--no_nw"], None), "bs": (["-b"], "gmp")}


@pytest.mark.parametrize("mode", sorted(CELGEN_MODES))
def test_cli_device_text_on_real_sequence(mode, celgen, tmp_path):
    flags, track = CELGEN_MODES[mode]
    fa, fq = celgen
    out = str(tmp_path / "mine")
    r = subprocess.run([EXE, "-g", fa, "-o", out, "-a", "0.9", "--sam_text=device"] + flags + [fq], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    ref = gzip.open(os.path.join(CELGEN, mode + ".sam.gz"), "rt").read()
    assert_same_sam("".join(l for l in open(out + ".sam") if not l.startswith("@PG")), ref, "celgen " + mode)
    if track:
        compare_tracks(open(out + "." + track).read(), gzip.open(os.path.join(CELGEN, f"{mode}.{track}.gz"), "rt").read(), 3 if track == "sgr" else 8)


# ---- shards ----------------------------------------------------------------------------------------------------------------------
def check_shards(mode, K, blocks, text, tmp_path):
    out = str(tmp_path / "mine")
    run_driver(mode, [f"--sam_shards={K}", f"--sam_text={text}"] + blocks, out)
    assert not os.path.exists(out + ".sam")
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".sam")) == [f"mine.{k}.sam" for k in range(K)]
    shards = [open(f"{out}.{k}.sam").read() for k in range(K)]
    for k in range(1, K):
        assert not any(l.startswith("@") for l in shards[k].splitlines()), k          # header lines in shard 0 only
    assert shards[0].startswith("@SQ")
    assert sum(1 for s in shards if any(not l.startswith("@") for l in s.splitlines())) >= 2      # the split is not a no-op
    cat = "".join(shards)
    assert_same_sam("".join(l + "\n" for l in cat.splitlines() if not l.startswith("@PG")), ref_text(mode, "sam"), f"{mode} K={K}")
    ext = "sgr" if "sgr" in MANIFEST[mode]["tracks"] else "gmp"
    compare_tracks(open(out + "." + ext).read(), ref_text(mode, ext), 3 if ext == "sgr" else 8)


@pytest.mark.parametrize("text", ["host", "device"])
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("mode", ["default", "all", "bs_all", "malformed", "malformed_tail", "illumina"])
def test_cli_shards_concatenate_to_the_single_file(mode, K, text, tmp_path):
    """byte-range chunks of about 37 records: many blocks, also in the 39-record input of malformed_tail (second pass in file order)"""
    check_shards(mode, K, ["--chunk_reads=37", "--workers=3"], text, tmp_path)


@pytest.mark.parametrize("text", ["host", "device"])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_cli_shards_in_file_order_mode(K, text, tmp_path):
    """--batch=64: blocks of exactly 64 reads from one sequential scanner (551 reads: nine blocks)"""
    check_shards("default", K, ["--batch=64"], text, tmp_path)


@pytest.mark.parametrize("text", ["host", "device"])
def test_cli_one_shard_is_the_single_file(text, tmp_path):
    out = str(tmp_path / "mine")
    run_driver("default", ["--sam_shards=1", f"--sam_text={text}", "--chunk_reads=37"], out)
    assert [f for f in os.listdir(tmp_path) if f.endswith(".sam")] == ["mine.sam"]
    check_against_reference("default", out)


# ---- the ABI call against the formatter of tests/sam_text_model.py -----------------------------------------------------------------------------
def test_the_reversal_helpers_of_this_file():
    assert reverse_cigar(b"77M1I22M1D") == b"1D22M1I77M" and reverse_cigar(b"5M3") == b"5M" and reverse_cigar(b"*") == b"*" and reverse_cigar(b"1:M2I") == b"2I1:M"
    assert revcomp(b"ACgtN-x") == b"n-nacGT"


def both_calls(ix, p, seqs, quals, names, qual_tails=None, bin_size=8, first_cap=None):
    """Batch.output on one mapping, Batch.output_text on a second mapping of the same reads; the coverage track after each"""
    B, Q, Ln = g.pack_reads(seqs, [q[:len(s)] for s, q in zip(seqs, quals)])
    batch = g.Batch(ix, len(seqs), B.shape[1])
    ix.coverage_reset(bin_size)
    res = batch.map(p, B, Q, Ln)
    recs, cigars = batch.output(p, res)
    cov_recs = ix.coverage_download()
    ix.coverage_reset(bin_size)
    res2 = batch.map(p, B, Q, Ln)
    text, row_off = batch.output_text(p, res2, names, qual_tails, text_cap=first_cap)
    cov_text = ix.coverage_download()
    calls = batch.text_calls
    batch.destroy()
    return recs, cigars, text, row_off, cov_recs, cov_text, calls


def same_track(a, b):
    # the tolerance of compare_tracks (fp32 atomic order): a track deposited twice, or never, is far outside it
    assert a.shape == b.shape and float(b.sum()) > 100.0
    assert np.all(np.abs(a.astype(np.float64) - b) <= 1e-4 * np.maximum(1.0, np.abs(b)) + 2e-5)


@pytest.mark.parametrize("kw", [{}, {"print_all_sam": 1}, {"mode": 1}], ids=["default", "print_all", "bs"])
def test_abi_text_equals_an_independent_formatter(kw, syn_fa, syn_reads):
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params(**kw)
    names = [r[0].encode() for r in syn_reads]; seqs = [r[1] for r in syn_reads]; quals = [r[2] for r in syn_reads]
    # a text_cap that is too small: GM_E_CAPACITY with the needed size, then a second call with exactly that size
    recs, cigars, text, row_off, cov_recs, cov_text, calls = both_calls(ix, p, seqs, quals, names, first_cap=16)
    assert calls == 2
    assert len(recs) > 500 and int((recs["strand"] != 0).sum()) > 100
    check_text(ix, p, seqs, quals, names, recs, cigars, text, row_off)
    same_track(cov_text, cov_recs)                  # the retried call deposited once: not twice, not never
    ix.close()


def test_abi_text_capacity_reports_the_needed_size(syn_fa, syn_reads):
    import ctypes as C
    from gnumap_amd import api
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    rd = syn_reads[:120]
    names = [r[0].encode() for r in rd]
    B, Q, Ln = g.pack_reads([r[1] for r in rd], [r[2][:len(r[1])] for r in rd])
    batch = g.Batch(ix, len(rd), B.shape[1])
    ix.coverage_reset(8)
    res = batch.map(p, B, Q, Ln)
    rt, keep = api._pack_read_text(names, None, len(rd))
    small = np.zeros(8, np.uint8)
    st = api.gm_sam_text(); st.text = small.ctypes.data; st.text_cap = 8
    rc = g.lib().gm_output_batch_text(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(st), None)
    assert rc == api.GM_E_CAPACITY and st.text_cap == st.text_len > 8 and st.n_recs > 50
    assert float(ix.coverage_download().sum()) == 0.0              # returned before anything was deposited
    need = int(st.text_cap)
    buf = np.zeros(need, np.uint8)
    st2 = api.gm_sam_text(); st2.text = buf.ctypes.data; st2.text_cap = need
    assert g.lib().gm_output_batch_text(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(st2), None) == 0
    assert st2.text_len == need and buf.tobytes().count(b"\n") == st2.n_recs
    # offsets that do not ascend, and a missing gm_read_text
    bad_off = keep[1].copy(); bad_off[3] = bad_off[5] + 1
    rt_bad = api.gm_read_text(); rt_bad.names = rt.names; rt_bad.name_off = bad_off.ctypes.data
    assert g.lib().gm_output_batch_text(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), C.byref(rt_bad), C.byref(res["_struct"]), C.byref(st2), None) == -1
    assert g.lib().gm_output_batch_text(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), None, C.byref(res["_struct"]), C.byref(st2), None) == -1
    batch.destroy(); ix.close()


def test_abi_records_capacity_reports_the_needed_sizes_and_deposits_once(syn_fa, syn_reads):
    """gm_output_batch with room for one record and one CIGAR byte: GM_E_CAPACITY with both sizes, nothing deposited; the call repeated
    with exactly those sizes gives the records, CIGARs and track of a call that had room from the start"""
    import ctypes as C
    from gnumap_amd import api
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    rd = syn_reads[:300]
    B, Q, Ln = g.pack_reads([r[1] for r in rd], [r[2][:len(r[1])] for r in rd])
    batch = g.Batch(ix, len(rd), B.shape[1])
    ix.coverage_reset(8)
    want_recs, want_cigars = batch.output(p, batch.map(p, B, Q, Ln))
    want_cov = ix.coverage_download()
    assert len(want_recs) > 150

    def call(res, rcap, ccap):
        recs = np.zeros(max(rcap, 1), api.SAM_DTYPE); pool = np.zeros(max(ccap, 1), np.uint8)
        so = api.gm_sam_out(); so.recs = recs.ctypes.data; so.recs_cap = rcap; so.cigar_pool = pool.ctypes.data; so.cigar_cap = ccap
        rc = g.lib().gm_output_batch(ix.h, C.byref(p.c), batch.h, C.byref(res["_reads"]), C.byref(res["_struct"]), C.byref(so), None)
        return rc, so, recs, pool

    ix.coverage_reset(8)
    res = batch.map(p, B, Q, Ln)
    rc, so, _, _ = call(res, 1, 1)
    assert rc == api.GM_E_CAPACITY
    assert so.recs_cap == so.n_recs == len(want_recs) and so.cigar_cap == so.cigar_len > len(want_recs)
    assert float(ix.coverage_download().sum()) == 0.0                # returned before anything was deposited
    rc, so2, recs, pool = call(res, int(so.recs_cap), int(so.cigar_cap))
    assert rc == 0 and so2.n_recs == so.n_recs and so2.cigar_len == so.cigar_len
    assert all(np.ascontiguousarray(recs[f]).tobytes() == np.ascontiguousarray(want_recs[f]).tobytes() for f in want_recs.dtype.names)
    raw = pool.tobytes() + b"\0"
    assert [raw[o:raw.index(b"\0", o)] for o in recs["cigar_off"]] == want_cigars
    same_track(ix.coverage_download(), want_cov)                     # deposited once
    batch.destroy(); ix.close()


def test_abi_text_long_name_lower_case_n_bases_and_quality_tails(syn_fa, syn_reads):
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params(print_all_sam=1)
    names = [r[0].encode() for r in syn_reads]; seqs = [r[1] for r in syn_reads]; quals = [r[2] for r in syn_reads]
    minus_reads = [i for i, nm in enumerate(names) if b"_-_" in nm and len(seqs[i]) >= 100]       # the fixture's names say where a read came from
    assert len(minus_reads) > 60
    for k, i in enumerate(minus_reads[:60]):
        s = bytearray(seqs[i])
        if k % 3 == 0:
            s = bytearray(bytes(s).lower())
        elif k % 3 == 1:
            s[len(s) // 2] = ord("N"); s[7] = ord("n")
        else:
            s[:20] = bytes(s[:20]).lower()
        seqs[i] = bytes(s)
    long_reads = minus_reads[:3] + [0, 2]
    for i in long_reads:
        names[i] = (names[i] + b"_") * 80
        assert len(names[i]) >= 1500
    tails = [b""] * len(seqs)
    for i in minus_reads[5:15] + [0, 4]:
        tails[i] = b"#tail%d" % i
    full_quals = [q[:len(s)] + t for s, q, t in zip(seqs, quals, tails)]
    recs, cigars, text, row_off, cov_recs, cov_text, _ = both_calls(ix, p, seqs, quals, names, tails)
    check_text(ix, p, seqs, full_quals, names, recs, cigars, text, row_off)
    same_track(cov_text, cov_recs)
    rows = [l.split(b"\t") for l in text.splitlines()]
    byread = {}
    for r, row in zip(recs, rows):
        byread.setdefault(int(r["read"]), []).append(row)
    assert any(len(row[0]) == 1023 for i in long_reads for row in byread.get(i, []))              # 1500 bytes given, MAX_NAME_SZ - 1 printed
    assert max(len(row[0]) for row in rows) == 1023
    minus_rows = [row for row in rows if row[1] == b"16"]
    assert any(row[9].islower() for row in minus_rows)                                            # a lower-case read, complemented in its case
    assert any(b"n" in row[9] and re.search(b"[ACGT]", row[9]) for row in minus_rows)             # N -> n inside an upper-case read
    assert any(len(row[10]) > len(row[9]) and row[10][:len(tails[i])] == tails[i][::-1] for i in minus_reads[5:15] for row in byread.get(i, []) if row[1] == b"16")
    ix.close()


def test_abi_text_blocks_of_150bp_and_of_mixed_lengths(syn_fa, syn_reads):
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    r150 = [r for r in syn_reads if len(r[1]) == 150]
    assert len(r150) >= 30
    mixed = [r for r in syn_reads if len(r[1]) != 100] + syn_reads[:40]
    assert len({len(r[1]) for r in mixed}) >= 5
    for rd in (r150, mixed):
        names = [r[0].encode() for r in rd]; seqs = [r[1] for r in rd]; quals = [r[2] for r in rd]
        recs, cigars, text, row_off, cov_recs, cov_text, _ = both_calls(ix, p, seqs, quals, names)
        assert len(recs) >= 20
        check_text(ix, p, seqs, quals, names, recs, cigars, text, row_off)
        assert np.all(np.abs(cov_text.astype(np.float64) - cov_recs) <= 1e-4 * np.maximum(1.0, np.abs(cov_recs)) + 2e-5) and float(cov_recs.sum()) > 10
    ix.close()


# ---- gm_dev_fmt_g6 --------------------------------------------------------------------------------------------------------------
def g6_values():
    rng = np.random.default_rng(5)
    n = 60000
    u = rng.random(n); dec = rng.integers(-5, 8, n)
    f = (u * 10.0 ** dec).astype(np.float32).astype(np.float64)
    fam = [f, -f, f * (1.0 / 0.37), u * 10.0 ** dec, f * (1.0 / np.float32(0.25)), f * (1.0 / np.float32(1.0))]
    p10 = np.array([float("1e%d" % e) for e in range(-60, 61)])
    fam += [p10, np.nextafter(p10, 0), np.nextafter(p10, np.inf), -p10, p10 * 9.999995, p10 * 9.9999949, p10 * 1.000005, p10 * 2.000015, p10 * 1.5]
    six = rng.integers(100000, 1000000, 40000).astype(np.float64)
    fam += [(six + 0.5) * 10.0 ** rng.integers(-9, 1, 40000), (six * 10 + 5) * 1e6, (six * 10 + 5) * 1e12, (six + 0.5) * 1e-11,
            np.ldexp(six + 0.5, rng.integers(-150, 150, 40000).astype(np.int32)), np.ldexp(rng.integers(0, 1 << 24, 40000).astype(np.float64), -rng.integers(0, 30, 40000).astype(np.int32))]
    bits = rng.integers(0, 1 << 32, 120000, dtype=np.uint64).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        fl = bits.view(np.float32).astype(np.float64)                  # floats over the whole exponent range, denormals, inf and nan included
    fl = np.where(np.isnan(fl), np.nan, fl)                            # (Python prints every NaN as "nan": keep the positive one)
    den = np.arange(1, 200000, 7, dtype=np.uint32).view(np.float32).astype(np.float64)
    fam += [fl, fl * 4.0, den, -den]
    lo, hi = np.ldexp(1.0, -200), np.ldexp(1.0, 200)
    fam += [np.array([0.0, -0.0, 1.0, 0.5, 999999.5, 999999.4999, 0.0001, 0.00009999995, 1e6, 123456.5, 0.1, 100000, np.inf, -np.inf, np.nan, 1e-5, 2.5e-7, 8.40759e-05,
                      lo, -lo, np.nextafter(lo, 0), np.nextafter(hi, 0), hi, -hi, 5e-324, 1e300, -1e-300])]
    return np.concatenate(fam), lo, hi


def test_dev_fmt_g6_equals_python_percent_g(syn_fa):
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    v, lo, hi = g6_values()
    assert len(v) > 300000
    got = ix.dev_fmt_g6(v)
    bad, outside = [], 0
    for x, t in zip(v.tolist(), got):
        ax = abs(x)
        if x == 0 or ax != ax or ax == float("inf") or lo <= ax < hi:
            if t != ("%g" % x).encode():
                bad.append((x, t, "%g" % x))
        else:
            outside += 1
            if t != b"":
                bad.append((x, t, "length 0"))
    assert not bad, (len(bad), bad[:10])
    assert outside >= 5
    ix.close()
