"""-A / --adaptor on the device: k_adaptor_trim against the numpy model (tests/adaptor_model.py, pinned to the reference program by
tests/test_adaptor_cpu.py), and the driver with -A against the outputs of the UNMODIFIED reference program
(tests/golden/ref_runs_adaptor/): SAM text byte for byte, record order included; tracks within the tolerance of
tests/test_gpu_driver_golden.py."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
from adaptor_model import kept_length, kept_lengths
from conftest import GOLDEN, ROOT, read_fastq
from test_gpu_driver_golden import compare_tracks

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "ref_runs_adaptor")
MANIFEST = json.load(open(os.path.join(RUNS, "manifest.json")))
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
AD34 = MANIFEST["default"]["adaptor"].encode()
AD60 = MANIFEST["a60"]["adaptor"].encode()


@pytest.fixture(scope="module")
def ix(syn_fa):
    i = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    yield i
    i.close()


def ref_text(mode, ext):
    return gzip.open(os.path.join(RUNS, f"{mode}.{ext}.gz"), "rt").read()


def _pack(seqs, stride=None):
    return g.pack_reads(seqs, [b"I" * len(s) for s in seqs], stride)


@pytest.mark.parametrize("fq", ["syn_adapt.fq", "syn_adapt_ill.fq", "syn_adapt_u100.fq"])
@pytest.mark.parametrize("adaptor", [AD34, AD34[:6], AD60, AD34.lower()], ids=["a34", "a6", "a60", "lower"])
def test_probe_equals_model_on_fixture_reads(ix, fq, adaptor):
    seqs = [r[1] for r in read_fastq(os.path.join(GOLDEN, fq))]
    B, _, Ln = _pack(seqs)
    got = ix.adaptor_trim(B, Ln, adaptor)
    np.testing.assert_array_equal(got, kept_lengths(seqs, adaptor))
    np.testing.assert_array_equal(ix.adaptor_trim(B, Ln, b""), Ln)                  # no adaptor: nothing is trimmed
    np.testing.assert_array_equal(ix.adaptor_trim(B, Ln, None), Ln)


def _random_reads(rng, A, count):
    """reads of 4 .. 2048 bases over a two-letter alphabet (so that chance agreement is common), half of them with the adaptor planted at
    a random offset with k of its j compared characters right, k within 1 of 0.85 j - the boundary ratios - or a little further off"""
    adaptor = bytes(rng.choice([65, 67], A).astype(np.uint8))
    seqs = []
    for c in range(count):
        L = int(rng.choice([4, 5, 6, 7, 8, 9, 36, 63, 64, 65, 68, 69, 100, 127, 128, 129, 132, 133, 150, 2047, 2048])) if c % 3 == 0 else int(rng.integers(4, 2049))
        s = rng.choice([71, 84] if c % 2 else [65, 67], L).astype(np.uint8)           # G/T: no chance agreement; A/C: plenty
        if c % 2 and L > 5:
            i = int(rng.integers(0, L - 4))
            j = min(A, L - i)
            k = int(np.clip(int(np.floor(0.85 * j)) + int(rng.integers(-1, 3)), 0, j))
            w = np.frombuffer(adaptor[:j], np.uint8).copy()
            wrong = rng.choice(j, j - k, replace=False)
            w[wrong] = 71
            s[i:i + j] = w
        seqs.append(bytes(s))
    return adaptor, seqs


@pytest.mark.parametrize("A", list(range(1, 65)))
def test_probe_equals_model_on_random_reads(ix, A):
    rng = np.random.default_rng(1000 + A)
    adaptor, seqs = _random_reads(rng, A, 48)                                         # 64 x 48 = 3072 reads in all
    want = kept_lengths(seqs, adaptor)
    longest = max(len(s) for s in seqs)
    for stride in (None, 2048, ((longest + 7) // 8) * 8 + 8 * (A % 5)):
        if stride is not None and (stride < longest or stride > 2048):
            continue
        B, _, Ln = _pack(seqs, stride)
        np.testing.assert_array_equal(ix.adaptor_trim(B, Ln, adaptor), want, err_msg=f"A={A} stride={stride}")


def test_probe_every_boundary_ratio(ix):
    """every k / j with k within 1 of 0.85 j, j = 1 .. 64, at the end of a read (mismatches first, so that offset 50 is the first that can
    qualify) - the exact fp32 boundaries 17/20, 34/40, 51/60 among them"""
    by_j = {}
    for j in range(5, 65):
        for k in sorted({int(np.floor(0.85 * j)) + d for d in (-1, 0, 1, 2)}):
            if 0 <= k <= j:
                by_j.setdefault(j, []).append(b"G" * 50 + b"T" * (j - k) + b"A" * k)
    for j, seqs in by_j.items():
        adaptor = b"A" * j
        B, _, Ln = _pack(seqs)
        np.testing.assert_array_equal(ix.adaptor_trim(B, Ln, adaptor), kept_lengths(seqs, adaptor), err_msg=f"j={j}")
    assert kept_length(b"G" * 50 + b"TTT" + b"A" * 17, b"A" * 20) == 50


def _run_cli(mode, extra, tmp_path):
    m = MANIFEST[mode]
    out = str(tmp_path / "mine")
    r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "-a", "0.9", "-A", m["adaptor"]] + m["argv"] + extra + [os.path.join(GOLDEN, m["fastq"])],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Using Adaptor Sequence: " + m["adaptor"] in r.stderr
    return out


@pytest.mark.parametrize("text", ["host", "device"])
@pytest.mark.parametrize("extra", [[], ["--locate=sampled"], ["--batch=64", "--workers=2"], ["--chunk_reads=37", "--workers=3"]],
                         ids=["full_sa", "sampled_sa", "batch64", "chunks37"])
@pytest.mark.parametrize("mode", sorted(MANIFEST))
def test_cli_with_adaptor_equals_reference_program(mode, extra, text, tmp_path):
    m = MANIFEST[mode]
    out = _run_cli(mode, extra + ["--sam_text=" + text], tmp_path)
    sam = "".join(l for l in open(out + ".sam") if not l.startswith("@PG"))
    ref = ref_text(mode, "sam")
    if sam != ref:
        a, b = sam.splitlines(), ref.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{mode}: {len(a)} vs {len(b)} lines, first difference at line {first}:\n  mine {a[first] if first < len(a) else None}\n  ref  {b[first] if first < len(b) else None}")
    ext = "sgr" if "sgr" in m["tracks"] else "gmp"
    compare_tracks(open(out + "." + ext).read(), ref_text(mode, ext), 3 if ext == "sgr" else 8)


@pytest.mark.parametrize("extra", [["--sam_shards=3", "--chunk_reads=50"], ["--sam_shards=2", "--sam_text=device", "--batch=100"], ["--gpus=1", "--workers=1"]],
                         ids=["shards3", "shards2_device", "one_worker"])
def test_cli_with_adaptor_and_shards(extra, tmp_path):
    out = _run_cli("default", extra, tmp_path)
    k = next((int(x.split("=")[1]) for x in extra if x.startswith("--sam_shards=")), 1)
    files = [out + ".sam"] if k == 1 else [f"{out}.{i}.sam" for i in range(k)]
    sam = "".join(l for f in files for l in open(f) if not l.startswith("@PG"))
    assert sam == ref_text("default", "sam")


def test_cli_long_option_is_the_lower_cased_string(tmp_path):
    """--adaptor=STRING = -A of the lower-cased string (a departure: the reference reads an unterminated buffer there)"""
    out = str(tmp_path / "o")
    fq = tmp_path / "lower.fq"
    recs = read_fastq(os.path.join(GOLDEN, "syn_adapt.fq"))
    fq.write_bytes(b"".join(b"@" + n.encode() + b"\n" + s.lower() + b"\n+\n" + q + b"\n" for n, s, q in recs))
    runs = []
    for flag in (["--adaptor=" + AD34.decode()], ["-A", AD34.decode().lower()]):
        r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out, "-a", "0.9"] + flag + [str(fq)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        runs.append([l for l in open(out + ".sam") if not l.startswith("@PG")])
    assert runs[0] == runs[1] and len(runs[0]) > 500
    assert sum("\t66M\t" in l for l in runs[0]) > 20                                # 34 bases trimmed from 100-bp reads


def _hits(res):
    m = res["matches"]
    pos = [res["positions"][f][int(a):int(b)].tolist() for a, b in zip(m["pos_begin"], m["pos_end"]) for f in ("pos", "strand")]
    return (res["status"].tobytes(), res["denominator"].tobytes(), res["top_score"].tobytes(), res["match_begin"].tobytes(),
            [m[f].tobytes() for f in ("read", "score", "first_pos", "first_strand")], pos)


def test_uniform_block_takes_the_one_length_dp_kernel(ix):
    """a block of 100-bp reads without adaptor: every read keeps 96 bases, len_min == len_max again, and k_nw_rows takes the block"""
    reads = read_fastq(os.path.join(GOLDEN, "syn_adapt_u100.fq"))
    B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
    p = g.Params()
    batch = g.Batch(ix, len(reads), B.shape[1])
    batch.set_adaptor(AD34)
    res = batch.map(p, B, Q, Ln)
    assert "nw=k_nw_rows" in batch.path(), batch.path()
    assert "seeds=k_seed" in batch.path(), batch.path()
    np.testing.assert_array_equal(batch.trimmed_len(), np.full(len(reads), 96, np.uint16))
    # the same block cut to 96 bases by hand and mapped without an adaptor, plus strand only (the reference's minus strand walks the END
    # of the whole line once reads are trimmed): same results
    pu = g.Params(neg_strand=0)
    res_a = batch.map(pu, B, Q, Ln)
    B2, Q2, Ln2 = g.pack_reads([r[1][:96] for r in reads], [r[2][:96] for r in reads], B.shape[1])
    plain = g.Batch(ix, len(reads), B.shape[1])
    res_b = plain.map(pu, B2, Q2, Ln2)
    assert _hits(res_a) == _hits(res_b)
    np.testing.assert_array_equal(res_a["self_score"], res_b["self_score"])
    assert (res_a["status"] == 0).sum() > 50
    del res
    batch.destroy(); plain.destroy()


def test_trimmed_len_after_map_and_cleared_adaptor(ix):
    reads = read_fastq(os.path.join(GOLDEN, "syn_adapt.fq"))
    seqs = [r[1] for r in reads]
    B, Q, Ln = g.pack_reads(seqs, [r[2] for r in reads])
    p = g.Params()
    never = g.Batch(ix, len(reads), B.shape[1])
    want = never.map(p, B, Q, Ln)
    recs_want, cig_want = never.output(p, want)
    np.testing.assert_array_equal(never.trimmed_len(), Ln)
    batch = g.Batch(ix, len(reads), B.shape[1])
    for adaptor in (AD34, AD60, AD34[:6]):
        batch.set_adaptor(adaptor)
        res = batch.map(p, B, Q, Ln)
        np.testing.assert_array_equal(batch.trimmed_len(), kept_lengths(seqs, adaptor), err_msg=str(adaptor))
        J = batch.trimmed_len()
        assert ((res["status"] == g.GM_READ_TOO_SHORT) == (J < 10)).all()
    assert _hits(res) != _hits(want)
    # cleared: the block maps as on a batch that never had an adaptor - hits, records, CIGARs, path
    for clear in (None, b""):
        batch.set_adaptor(AD34); batch.map(p, B, Q, Ln)
        batch.set_adaptor(clear)
        got = batch.map(p, B, Q, Ln)
        assert _hits(got) == _hits(want)
        np.testing.assert_array_equal(got["self_score"], want["self_score"])
        assert batch.path() == never.path()
        recs, cig = batch.output(p, got)
        assert recs.tobytes() == recs_want.tobytes() and cig == cig_want
        np.testing.assert_array_equal(batch.trimmed_len(), Ln)
    batch.destroy(); never.destroy()


def test_text_rows_print_the_whole_lines(ix):
    """gm_output_batch_text with an adaptor set: SEQ and QUAL at gm_reads.len, CIGAR at the kept length - the rows of the reference"""
    reads = read_fastq(os.path.join(GOLDEN, "syn_adapt.fq"))
    B, Q, Ln = g.pack_reads([r[1] for r in reads], [r[2] for r in reads])
    p = g.Params()
    batch = g.Batch(ix, len(reads), B.shape[1])
    batch.set_adaptor(AD34)
    ix.coverage_reset(8)
    res = batch.map(p, B, Q, Ln)
    text, row_off = batch.output_text(p, res, [r[0].encode() for r in reads])
    want = "".join(l for l in ref_text("default", "sam").splitlines(True) if not l.startswith("@"))
    assert text.decode() == want
    batch.destroy()
