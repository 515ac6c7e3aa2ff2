"""-A / --adaptor without a GPU: the numpy model of the trim rule (tests/adaptor_model.py) is pinned to the outputs of the UNMODIFIED
reference program (tests/golden/ref_runs_adaptor/, made by tests/golden/make_adaptor_fixtures.py), and the new entry points exist,
validate their arguments and refuse to compute without a device."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
from gnumap_amd import api
from adaptor_model import cigar_read_length, kept_length, kept_lengths
from conftest import GOLDEN, ROOT, read_fastq

RUNS = os.path.join(GOLDEN, "ref_runs_adaptor")
MANIFEST = json.load(open(os.path.join(RUNS, "manifest.json")))
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
REFBIN = os.path.join(ROOT, "oracle", "_ref", "gnumap_ref")
AD34 = MANIFEST["default"]["adaptor"]
NEW = ["gm_batch_set_adaptor", "gm_batch_trimmed_len", "gm_dev_adaptor_trim"]


def sam_records(mode):
    return [l.rstrip("\n").split("\t") for l in gzip.open(os.path.join(RUNS, f"{mode}.sam.gz"), "rt") if not l.startswith("@")]


@pytest.mark.parametrize("mode", sorted(MANIFEST))
def test_model_equals_the_reference_program_on_every_record(mode):
    """the CIGAR of every record the reference wrote accounts for exactly the bases the model keeps of that read (M + I = J), while SEQ
    and QUAL stay the whole lines.  --no_nw is the reference's own exception: its CIGAR is "<n>M" with n = the length of the whole
    sequence line (consensus.size(), inc/ScoredSeq.h:365), whatever was trimmed"""
    m = MANIFEST[mode]
    reads = {name: (seq, qual) for name, seq, qual in read_fastq(os.path.join(GOLDEN, m["fastq"]))}
    recs = sam_records(mode)
    assert len(recs) == m["sam_lines"] - 3
    trimmed_more_than_4 = 0
    for f in recs:
        seq, qual = reads[f[0]]
        J = kept_length(seq, m["adaptor"].encode())
        assert len(f[9]) == len(seq) and len(f[10]) == len(qual), f[0]
        if "--no_nw" in m["argv"]:
            assert f[5] == f"{len(seq)}M", (f[0], f[5])
        else:
            assert cigar_read_length(f[5]) == J, (f[0], f[5], J)
        trimmed_more_than_4 += len(seq) - J > 4
    if m["fastq"] == "syn_adapt.fq" and "--down_strand" not in m["argv"]:
        assert trimmed_more_than_4 > 300                      # the fixture does exercise the rule, not only the "lose 4 bases" default
    if mode == "down":
        assert recs == []                                      # the reference finds nothing on the minus strand once reads are trimmed


def test_model_quirks():
    ad = AD34.encode()
    assert kept_length(b"ACGT" * 25, ad) == 96                  # no adaptor anywhere: the last four bases go all the same
    assert kept_length(b"ACGTA", ad) == 1 and kept_length(b"ACGT", ad) == 0 and kept_length(b"ACG", ad) == 0 and kept_length(b"", ad) == 0
    assert kept_length(b"ACGT" * 25, b"") == 100                # no adaptor set
    read = b"C" * 60 + ad + b"TTTTTT"
    assert kept_length(read, ad) == 60
    assert kept_length(read.lower(), ad) == len(read) - 4       # case-sensitive
    assert kept_length(read, ad.lower()) == len(read) - 4
    # exact boundaries of the fp32 division: 17/20 and 34/40 qualify, 16/20 and 33/40 do not
    for j, k, ok in ((20, 17, True), (20, 16, False), (40, 34, True), (40, 33, False), (7, 6, True), (6, 5, False)):
        a = b"A" * j
        tail = b"C" * (j - k) + b"A" * k                          # (mismatches first: no earlier offset sees more matches)
        read = b"G" * 50 + tail
        want = 50 if ok else None
        got = kept_length(read, a)
        if ok:
            assert got == want, (j, k, got)
        else:
            assert got != 50, (j, k, got)
    assert np.float32(17) / np.float32(20) >= np.float32(0.85) and np.float32(34) / np.float32(40) >= np.float32(0.85)


def test_fixture_set_covers_what_the_issue_lists():
    reads = read_fastq(os.path.join(GOLDEN, "syn_adapt.fq"))
    assert len(reads) == len(read_fastq(os.path.join(GOLDEN, "syn.fq"))) > 500        # every read of syn.fq, same order
    J = kept_lengths([r[1] for r in reads], AD34.encode())
    L = np.array([len(r[1]) for r in reads])
    cut = L - J
    assert {4, 5, 8, 12, 20, 34, 45, 60} <= set(cut.tolist())
    assert ((J < 10) & (L >= 36)).sum() >= 5                    # kept length below -m
    assert sum(r[1] != r[1].upper() for r in reads) >= 10       # lower-case reads
    assert ((J == 30) & (L >= 100)).sum() >= 5                  # an adaptor occurrence in mid-read
    ill = read_fastq(os.path.join(GOLDEN, "syn_adapt_ill.fq"))
    Ji = kept_lengths([r[1] for r in ill], AD34.encode())
    first_low = [next((t for t, c in enumerate(q) if c < 64), None) for _, _, q in ill]
    assert first_low[60] is not None and first_low[60] >= Ji[60]          # a Phred+33 character, but in the part the trim drops
    assert first_low[75] is not None and first_low[75] < Ji[75]           # the one that triggers the fallback
    assert all(f is None for k, f in enumerate(first_low) if k not in (60, 75))
    u = read_fastq(os.path.join(GOLDEN, "syn_adapt_u100.fq"))
    assert len(u) >= 100 and set(kept_lengths([r[1] for r in u], AD34.encode()).tolist()) == {96}


def test_new_symbols_are_exported_and_declared():
    L = g.load_library()
    hdr = open(os.path.join(ROOT, "include", "gnumap_hip.h")).read()
    for n in NEW + ["gm_batch_adaptor_time"]:
        assert hasattr(L, n), n
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
        assert n in api.EXPORTS
    assert "src/SeqReader.cpp:1146-1150" in hdr and "1356-1372" in hdr and "1294-1305" in hdr


def test_set_adaptor_validates_its_arguments(syn_fa):
    L = g.load_library()
    assert L.gm_batch_set_adaptor(None, b"ACGT") == -1                     # GM_E_ARG
    assert L.gm_batch_set_adaptor(None, None) == -1
    assert L.gm_batch_trimmed_len(None, None) == -1
    ix = g.Index(syn_fa, flags=g.GM_INDEX_HOST_ONLY)
    B, Q, Ln = g.pack_reads([b"ACGT" * 10], [b"I" * 40])
    with pytest.raises(g.GnumapError, match="at most 256") as e:           # the ABI's cap, checked before anything touches a device
        ix.adaptor_trim(B, Ln, b"A" * 257)
    assert e.value.code == -1
    with pytest.raises(g.GnumapError, match="multiple of 8") as e:
        ix.adaptor_trim(np.zeros((1, 12), np.uint8), np.array([4], np.uint16), b"ACGT")
    assert e.value.code == -1
    with pytest.raises(g.GnumapError, match="no usable HIP device") as e:  # no CPU fallback
        ix.adaptor_trim(B, Ln, b"ACGT")
    assert e.value.code == -3                                              # GM_E_NO_DEVICE


def test_driver_takes_the_flag_and_reaches_the_device(tmp_path, syn_fa):
    import torch
    fq = os.path.join(GOLDEN, "syn_adapt_u100.fq")
    for flag in (["-A", AD34], ["--adaptor=" + AD34]):
        r = subprocess.run([EXE, "-g", syn_fa, "-o", str(tmp_path / "o"), "-a", "0.9"] + flag + [fq], capture_output=True, text=True, timeout=600)
        assert "outside the hot path" not in r.stderr and "No matching arg" not in r.stderr
        if torch.cuda.is_available():
            assert r.returncode == 0, r.stderr[-1500:]
        else:
            assert r.returncode != 0 and "no usable HIP device" in r.stderr          # GM_E_NO_DEVICE, not a parse error
    r = subprocess.run([EXE, "-g", syn_fa, "-o", str(tmp_path / "o"), "-A", "A" * 257, fq], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "at most 256" in r.stderr
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--adaptor=STRING" in r.stderr and "pinned" in r.stderr


@pytest.mark.skipif(not os.path.exists(REFBIN), reason="reference program only exists in the build container")
@pytest.mark.parametrize("mode", ["default", "no_nw", "illumina", "a60"])
def test_fixtures_are_what_the_reference_program_writes_now(mode, tmp_path):
    import shutil
    m = MANIFEST[mode]
    for f in os.listdir(GOLDEN):
        if f.startswith("syn.") or f.startswith("syn_adapt"):
            shutil.copy(os.path.join(GOLDEN, f), tmp_path)
    r = subprocess.run([REFBIN, "-g", "syn.fa", "-o", "r", "-a", "0.9", "-c", "1", "-A", m["adaptor"]] + m["argv"] + [m["fastq"]],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    sam = b"".join(l for l in open(tmp_path / "r.sam", "rb") if not l.startswith(b"@PG"))
    assert sam == gzip.open(os.path.join(RUNS, f"{mode}.sam.gz"), "rb").read()
    for ext in m["tracks"]:
        assert open(tmp_path / f"r.{ext}", "rb").read() == gzip.open(os.path.join(RUNS, f"{mode}.{ext}.gz"), "rb").read()
