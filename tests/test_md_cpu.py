"""--sam_md / --sam_cigar without a device: tests/md_model.py against an independent inverse on every row the reference program wrote,
the string forms pinned on rows written out by hand, the minus-strand finding of DESIGN.md section 5 on record, and the driver's
refusals."""
import glob
import gzip
import os
import struct
import subprocess

import pytest

import md_model as mm
from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
FA = os.path.join(GOLDEN, "syn.fa")


@pytest.fixture(scope="module")
def texts():
    return mm.contig_texts(FA)                      # (asserts that pac + holes is the FASTA's own text)


def sam_rows(path):
    return [r for r in gzip.open(path, "rb") if not r.startswith(b"@")]


# ---- 1. the model against its inverse, on every row of the reference's runs ------------------------------------------------------
def test_rebuilding_the_reference_from_seq_cigar_and_md_gives_syn_fa_on_every_reference_row(texts):
    n = 0
    for path in sorted(glob.glob(os.path.join(GOLDEN, "ref_runs", "*.sam.gz"))):
        for row in sam_rows(path):
            f = row.rstrip(b"\n").split(b"\t")
            if f[5] == b"*":
                continue
            nm, md, clamped = mm.tags(int(f[3]), f[5], f[9], texts[f[2]])
            assert not clamped, (path, f[0])
            ref, n_mis, n_ins, n_del = mm.rebuild_reference(f[9], f[5], md)
            x = int(f[3]) - 1
            assert ref == texts[f[2]][x:x + len(ref)], (path, f[0])
            assert nm == n_mis + n_ins + n_del, (path, f[0])
            n += 1
    assert n == 41982


# ---- 2. the string forms ----------------------------------------------------------------------------------------------------------
#                  0         1         2
#                  0123456789012345678901234
T = {b"c": b"ACGTACGTTTGACCAGTNACGTAAGG", b"long": b"ACGT" * 300}


def md(pos, cigar, seq, contig=b"c"):
    return mm.tags(pos, cigar, seq, T[contig])


def test_adjacent_mismatches_and_mismatches_beside_a_deletion():
    assert md(1, b"8M", b"ACGTACGT") == (0, b"8", False)
    assert md(1, b"8M", b"ACTGACGT") == (2, b"2G0T4", False)                     # adjacent: a zero between them
    assert md(1, b"8M", b"CCGTACGA") == (2, b"0A6T0", False)                     # first and last column
    assert md(1, b"4M2D4M", b"ACGTCTTT") == (3, b"4^AC0G3", False)               # a deletion directly followed by a mismatch: ^AC0G
    assert md(1, b"4M2D4M", b"ACGAGTTT") == (3, b"3T0^AC4", False)               # a mismatch directly followed by a deletion: T0^AC
    assert md(1, b"2D4M", b"GTAC") == (2, b"0^AC4", False)                       # a leading D
    assert md(1, b"4M1I4M", b"ACGTNACGT") == (1, b"8", False)                    # an insertion costs NM and leaves no trace in MD
    assert md(5, b"0M4M0D", b"ACGT") == (0, b"4", False)                         # tokens of length 0 contribute nothing


def test_a_run_of_1100():
    nm, s, clamped = md(1, b"1100M", (b"ACGT" * 275), b"long")
    assert (nm, s, clamped) == (0, b"1100", False)
    nm, s, _ = md(1, b"1100M", (b"ACGT" * 275)[:1050] + b"T" + (b"ACGT" * 275)[1051:], b"long")
    assert (nm, s) == (1, b"1050G49")


def test_n_on_either_side_iupac_lower_case_and_a_hole_character():
    assert md(15, b"6M", b"AGTNAC") == (1, b"3N2", False)                        # N against N: a mismatch (code 15)
    assert md(1, b"4M", b"ACNT") == (1, b"2G1", False)                           # N in the read
    assert md(15, b"6M", b"AGTAAC") == (1, b"3N2", False)                        # N in the reference (a hole's character)
    assert md(1, b"4M", b"RCGT") == (1, b"0A3", False)                           # IUPAC R against A: compared by nibble, not by membership
    assert md(1, b"8M", b"acgtacgt") == (0, b"8", False)                         # lower-case SEQ
    assert md(1, b"8M", b"acgtacga") == (1, b"7T0", False)


def test_clamps_end_the_walk_with_one_closing_count():
    assert md(23, b"8M", b"AAGGTTTT") == (0, b"4", True)                         # the contig ends
    assert md(1, b"8M", b"ACGT") == (0, b"4", True)                              # SEQ ends
    assert md(23, b"2M4D", b"AA") == (4, b"2^GG0", True)                         # a deletion over the contig's end prints what there is


def test_insert_tags_strip_tags_and_the_bam_bytes():
    row = b"r\t16\tc\t1\t30\t4M2D4M\t*\t0\t0\tACGAGTTT\tIIIIIIII\tXA:f:3\tXP:f:1\tX0:i:1\n"
    got = mm.insert_tags(row, T)
    assert got == row[:-1] + b"\tNM:i:3\tMD:Z:3T0^AC4\n" and mm.strip_tags(got) == row
    star = row.replace(b"4M2D4M", b"*")
    unm = b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\tYU:i:2\n"
    assert mm.insert_tags(star, T) == star and mm.insert_tags(unm, T) == unm
    empty = row.replace(b"4M2D4M", b"")                          # what a pool entry of digits alone prints on the minus strand: no tags, as "*"
    assert mm.insert_tags(empty, T) == empty and not mm.has_tags(empty.split(b"\t")) and mm.has_tags(row.split(b"\t"))
    assert mm.tag_record(b"\0" * 40, empty, T, False) == b"\0" * 40
    assert mm.bam_tag_bytes(3, b"3T0^AC4") == b"NMi" + struct.pack("<i", 3) + b"MDZ3T0^AC4\0"
    assert mm.unreverse(b"4M2D14M") == b"14M2D4M" and mm.unreverse(mm.unreverse(b"1I99M")) == b"1I99M"
    assert mm.forward_row(row.replace(b"4M2D4M", b"3M2D5M")).split(b"\t")[5] == b"5M2D3M"
    plus = row.replace(b"\t16\t", b"\t0\t").replace(b"4M2D4M", b"3M2D5M")
    assert mm.forward_row(plus) == plus
    assert mm.rebuild_reference(b"ACGAGTTT", b"4M2D4M", b"3T0^AC4") == (b"ACGTACGTTT", 1, 0, 2)


# ---- 3. the minus-strand finding ---------------------------------------------------------------------------------------------------
def test_minus_strand_indel_rows_of_the_default_run_under_both_cigar_orders(texts):
    rows = [r.rstrip(b"\n").split(b"\t") for r in sam_rows(os.path.join(GOLDEN, "ref_runs", "default.sam.gz"))]
    minus = [f for f in rows if int(f[1]) & 16]
    indel = [f for f in minus if b"I" in f[5] or b"D" in f[5]]
    assert (len(rows), len(minus), len(indel)) == (1297, 383, 101)
    printed = [mm.tags(int(f[3]), f[5], f[9], texts[f[2]])[0] for f in indel]
    forward = [mm.tags(int(f[3]), mm.unreverse(f[5]), f[9], texts[f[2]])[0] for f in indel]
    assert sum(v >= 20 for v in printed) == 84                   # under the CIGAR the reference prints: nonsense alignments
    assert sum(v <= 5 for v in forward) == 95 and sum(v >= 20 for v in forward) == 2
    for f in rows:                                                # every other row: the order makes no difference
        if f not in indel and f[5] != b"*":
            assert mm.tags(int(f[3]), f[5], f[9], texts[f[2]]) == mm.tags(int(f[3]), mm.unreverse(f[5]) if int(f[1]) & 16 else f[5], f[9], texts[f[2]])


# ---- 4. the driver's refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, named", [
    (["--sam_md", "--sam_text=host"], ["--sam_md", "--sam_text=host"]),
    (["--sam_text=host", "--sam_md"], ["--sam_md", "--sam_text=host"]),
    (["--sam_cigar=forward", "--sam_text=host"], ["--sam_cigar", "--sam_text=host"]),
    (["--sam_cigar=gnumap", "--sam_text=host"], ["--sam_cigar", "--sam_text=host"]),
    (["--sam_md", "-A", "ACGTACGTAC"], ["--sam_md", "-A"]),
    (["--sam_md", "--adaptor=ACGTACGTAC"], ["--sam_md", "--adaptor"]),
    (["--sam_cigar=backward"], ["--sam_cigar", "backward"]),
    (["--sam_cigar="], ["--sam_cigar"]),
], ids=["md_host", "host_md", "cigar_forward_host", "cigar_gnumap_host", "md_A", "md_adaptor", "cigar_unknown", "cigar_empty"])
def test_refused_with_status_1_before_a_device_is_opened_or_a_file_is_written(tmp_path, args, named):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "-g", FA, "-o", out] + args + [os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1, r.stderr[-1000:]
    for word in named:
        assert word in r.stderr, (word, r.stderr[-1000:])
    assert "No matching arg" not in r.stderr and "no usable HIP device" not in r.stderr
    assert not os.listdir(tmp_path)                               # no <out>.sam, nothing else


def test_usage_names_both_options():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--sam_md" in r.stderr and "NM:i" in r.stderr and "MD:Z" in r.stderr
    assert "--sam_cigar=gnumap|forward" in r.stderr
