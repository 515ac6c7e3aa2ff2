"""FASTA read files without a GPU: the numpy model of the reference's FASTA reader (tests/fasta_model.py) pinned to the outputs of the
UNMODIFIED reference program (tests/golden/ref_runs_fasta/, made by tests/golden/make_fasta_fixtures.py), the fixtures' own sanity,
and the driver's refusals, which come before the device is opened."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from fasta_model import AMBIGUITY, IUPAC, base_mask, mask_rc, parse_fasta, pwm_rows, qual_char, sam_seq_qual, synth_qual

RUNS = os.path.join(GOLDEN, "ref_runs_fasta")
MANIFEST = json.load(open(os.path.join(RUNS, "manifest.json")))
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
MODES = ["default", "all_a80", "no_nw", "bs", "b2", "atog", "m14_j7", "M5", "M1", "up", "down", "q60", "raw60", "T2", "u", "h30", "subst", "bin1", "u100"]


def rows(mode):
    return [l.rstrip("\n").split("\t") for l in gzip.open(os.path.join(RUNS, f"{mode}.sam.gz"), "rt") if not l.startswith("@")]


def records(fa):
    return parse_fasta(open(os.path.join(GOLDEN, fa), "rb").read())


def test_manifest_names_every_mode_of_the_issue():
    assert sorted(MANIFEST) == sorted(MODES)
    for mode, m in MANIFEST.items():
        assert m["records"] >= 100, mode                                 # no vacuous mode
        assert m["records"] == len(rows(mode)), mode
        for ext in m["tracks"]:
            assert os.path.getsize(os.path.join(RUNS, f"{mode}.{ext}.gz")) > 1000, (mode, ext)
        assert m["tracks"] == (["gmp"] if mode in ("bs", "b2", "atog") else ["sgr"]), mode
    for f in os.listdir(RUNS):
        assert os.path.getsize(os.path.join(RUNS, f)) < 200_000, f
    assert os.path.getsize(os.path.join(GOLDEN, "fasta_vectors.npz")) < 200_000


def test_read_files_cover_what_the_issue_asks_for():
    recs = records("syn_reads.fa")
    text = open(os.path.join(GOLDEN, "syn_reads.fa"), "rb").read()
    lens = [len(s) for _, s in recs]
    assert min(lens) == 8 and max(lens) == 150 and sum(1 for x in lens if x < 10) >= 1          # reads shorter than -m
    assert sum(1 for _, s in recs if s == s.lower() and s != s.upper()) >= 50                   # lower-case records
    assert sum(1 for n, _ in recs if b" " in n) >= 50                                           # names with spaces
    assert text.count(b"\n") - 2 * len(recs) >= 150                                             # records over two or three sequence lines
    assert sum(1 for _, s in recs if b"nn" in s.lower()) >= 20                                  # n runs
    for c in AMBIGUITY + AMBIGUITY.upper():
        assert sum(1 for _, s in recs if c.encode() in s) >= 3, c
    coded = [s for _, s in recs if any(chr(c).lower() in AMBIGUITY for c in s)]
    assert len(recs) // 5 <= len(coded) <= len(recs) // 3
    assert all(1 <= sum(chr(c).lower() in AMBIGUITY for c in s) <= 4 for s in coded)
    u = records("syn_reads_u100.fa")
    assert len(u) == 200 and all(len(s) == 100 for _, s in u)
    assert sum(1 for _, s in u if any(chr(c).lower() in AMBIGUITY for c in s)) == 100


def test_default_mode_shows_codes_and_n_on_both_strands():
    r = rows("default")
    with_code = [f for f in r if any(c in f[9] for c in AMBIGUITY + AMBIGUITY.upper())]
    with_n = [f for f in r if "n" in f[9].lower()]
    assert len(with_code) >= 40 and len(with_n) >= 20
    assert {f[1] for f in with_code + with_n} == {"0", "16"}
    by_name = dict(records("syn_reads.fa"))
    minus_coded = [f for f in r if f[1] == "16" and any(chr(c).lower() in AMBIGUITY for c in by_name[f[0].encode()])]
    assert len(minus_coded) >= 20                                        # reads with a code that mapped to the minus strand (SEQ shows 'n' there)


def test_rows_of_the_model():
    P = pwm_rows(b"acgtRYKMSWBDHVNn")
    assert P.dtype == np.float32 and P.shape == (16, 4)
    np.testing.assert_array_equal(P[:4], np.eye(4, dtype=np.float32))
    np.testing.assert_array_equal(P[4], np.float32([0.5, 0, 0.5, 0]))                       # r: a or g
    np.testing.assert_array_equal(P[10], np.float32([0, 1, 1, 1]) * np.float32(1.0 / 3.0))  # b: not a
    np.testing.assert_array_equal(P[14], np.float32([0.25] * 4))
    third = np.float32(1.0 / 3.0)
    assert P[10, 1].view(np.uint32) == third.view(np.uint32) == 0x3EAAAAAB
    # the mask form the device uses: row k = mask bit k ? p : q, the minus strand's row = the mask with its bits reversed
    for ch in IUPAC:
        for c in (ch, ch.upper()):
            m = base_mask(ord(c))
            assert [(m >> k) & 1 for k in range(4)] == [int(x > 0) for x in pwm_rows(c.encode())[0]]
            rc_row = pwm_rows(c.encode())[0][::-1]
            assert [(mask_rc(m) >> k) & 1 for k in range(4)] == [int(x > 0) for x in rc_row]
    pairs = {"r": "y", "k": "m", "b": "v", "d": "h", "s": "s", "w": "w", "n": "n", "a": "t", "c": "g"}
    for a, b in pairs.items():
        assert mask_rc(base_mask(ord(a))) == base_mask(ord(b)) and mask_rc(base_mask(ord(b))) == base_mask(ord(a))
    assert base_mask(ord("x")) == 0 and base_mask(ord(" ")) == 0 and base_mask(ord(">")) == 0


def test_qual_characters_of_the_model():
    assert bytes([qual_char(np.float32(1.0)), qual_char(np.float32(0.5)), qual_char(np.float32(1.0 / 3.0)), qual_char(np.float32(0.25))]) == b'I$""'
    assert synth_qual(b"aCgTrYnNbV") == b'IIII$$""""'


@pytest.mark.parametrize("mode", MODES)
def test_model_gives_seq_and_qual_of_every_reference_row(mode):
    """SEQ and QUAL of every row the reference program printed = the model's, the minus-strand rows un-reversed"""
    by_name = dict(records(MANIFEST[mode]["fasta"]))
    n_minus = 0
    for f in rows(mode):
        seq = by_name[f[0].encode()]
        minus = f[1] == "16"
        n_minus += minus
        want_seq, want_qual = sam_seq_qual(seq, minus)
        assert f[9].encode() == want_seq and f[10].encode() == want_qual, f[0]
        if minus:                                                        # un-reversed: the model's plus-strand strings, codes folded to n
            assert f[10][::-1].encode() == synth_qual(seq)
            assert len(f[9]) == len(seq)
    assert (n_minus > 50) == (mode != "up")


def _run(args, tmp_path):
    return subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", str(tmp_path / "o"), "-a", "0.9"] + args, capture_output=True, text=True, timeout=120)


def test_cli_refuses_what_fasta_reads_do_not_take(tmp_path):
    """status 1 and a message, before the device is opened (this machine may have none)"""
    fa = os.path.join(GOLDEN, "syn_reads.fa")
    r = _run(["-A", "AGATCGGAAGAGC", fa], tmp_path)
    assert r.returncode == 1 and "-A/--adaptor with FASTA reads is not supported" in r.stderr, r.stderr[-500:]
    r = _run(["--snp", fa], tmp_path)
    assert r.returncode == 1 and "--snp with FASTA reads is not supported" in r.stderr, r.stderr[-500:]
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b">one\nACGTACGTAC\n>two words\nACGTXACGT\n")
    r = _run([str(bad)], tmp_path)
    assert r.returncode == 1 and "two words" in r.stderr and "'X'" in r.stderr and "not one of the 15 letters" in r.stderr, r.stderr[-500:]
    for ws in (b"\r", b" ", b"\x0b", b"\x0c"):
        bad.write_bytes(b">one\nACGTACGTAC" + ws + b"\n>two\nACGTACGT\n")
        r = _run([str(bad)], tmp_path)
        assert r.returncode == 1 and "white space (CR, space, VT or FF) inside a sequence line is not supported" in r.stderr, (ws, r.stderr[-500:])
    bad.write_bytes(b">one\n>two\nACGT\n")
    r = _run([str(bad)], tmp_path)
    assert r.returncode == 1 and "has no sequence" in r.stderr, r.stderr[-500:]
    prb = tmp_path / "s_1_prb.txt"
    prb.write_bytes(b"40 -40 -40 -40\t-40 40 -40 -40\n")
    r = _run([str(prb)], tmp_path)
    assert r.returncode == 1 and "_prb.txt and _int.txt read formats are not supported" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(str(tmp_path / "o.sam"))                  # nothing was written by any of them
