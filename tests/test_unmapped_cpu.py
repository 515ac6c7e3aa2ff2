"""--sam_unmapped without a device: the refusal with --sam_text=host, the usage text, and tests/unmapped_model.py on rows written out
by hand."""
import os
import struct
import subprocess

import unmapped_model as um
from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")


def test_refused_with_an_explicit_host_formatter_before_a_device_is_opened(tmp_path):
    out = str(tmp_path / "o")
    for args in (["--sam_unmapped", "--sam_text=host"], ["--sam_text=host", "--sam_unmapped"]):
        r = subprocess.run([EXE, "-g", os.path.join(GOLDEN, "syn.fa"), "-o", out] + args + [os.path.join(GOLDEN, "syn.fq")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1, r.stderr[-1000:]
        assert "--sam_unmapped" in r.stderr and "--sam_text=host" in r.stderr
        assert "No matching arg" not in r.stderr and "no usable HIP device" not in r.stderr
        assert not [f for f in os.listdir(tmp_path)]                 # no file was written


def test_usage_names_the_option():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--sam_unmapped" in r.stderr and "YU:i:" in r.stderr and "flag 4" in r.stderr


def test_model_formats_rows_written_out_by_hand():
    rows = [b"r1\t0\tchrA\t5\t30\t4M\t*\t0\t0\tACGT\tIIII\tXA:f:3\tXP:f:1\tX0:i:1\n", b"r1\t16\tchrB\t9\t0\t4M\t*\t0\t0\tACGT\tIIII\tXA:f:3\tXP:f:0.5\tX0:i:1\n"]
    names = [b"r0", b"r1", b"n" * 1500, b"", b"r4"]
    seqs = [b"ACGTN", b"ACGT", b"acgtRY", b"", b"GG"]
    quals = [b"IIIII#tail", b"IIII", b"!!!!!!", b"#", b"II"]
    status = [2, 0, -3, -2, 1]
    got, new = um.merge(rows, [1, 1], names, seqs, quals, status)
    assert new == [True, False, False, True, True, True]
    assert got == [b"r0\t4\t*\t0\t0\t*\t*\t0\t0\tACGTN\tIIIII#tail\tYU:i:2\n", rows[0], rows[1],
                   b"n" * 1023 + b"\t4\t*\t0\t0\t*\t*\t0\t0\tacgtRY\t!!!!!!\tYU:i:-3\n",
                   b"\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tYU:i:-2\n",
                   b"r4\t4\t*\t0\t0\t*\t*\t0\t0\tGG\tII\tYU:i:1\n"]
    assert [um.is_unmapped_row(r) for r in got] == new
    # the records of the three kinds of new row, byte by byte
    recs = um.to_records(got, [("chrA", 100), ("chrB", 100)])
    r0 = recs[0]
    assert um.fixed_fields(r0) == (-1, -1, 3, 0, 4680, 0, 4, 5, -1, -1, 0) and um.record_is_unmapped(r0)
    assert r0[36:] == b"r0\0" + bytes([0x12, 0x48, 0xF0]) + bytes([40] * 5) + b"YUi" + struct.pack("<i", 2)
    assert struct.unpack_from("<i", r0, 0)[0] == len(r0) - 4
    long_name = recs[3]
    assert um.fixed_fields(long_name)[2] == 255 and long_name[36:36 + 255] == b"n" * 254 + b"\0"
    assert long_name[36 + 255:36 + 255 + 3] == bytes([0x12, 0x48, 0x5A]) and long_name[-7:] == b"YUi" + struct.pack("<i", -3)
    empty = recs[4]
    assert um.fixed_fields(empty) == (-1, -1, 1, 0, 4680, 0, 4, 0, -1, -1, 0) and empty[36:] == b"\0YUi" + struct.pack("<i", -2)
    assert not um.record_is_unmapped(recs[1]) and um.records_differ(recs, list(recs)) is None
    assert um.records_differ(recs[:1] + [recs[0][:-1] + b"\x07"] + recs[2:], recs) is not None
    # coordinate order: the new rows last, in input order
    assert um.sort_rows(got, ["chrB", "chrA"]) == [rows[1], rows[0], got[0], got[3], got[4], got[5]]
