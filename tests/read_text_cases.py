"""The FASTQ texts the --read_text=device tests cut: each is a few records built to put one edge of the rule of fastq_text_model.py
under the kernels of gm_readtext.hip.  Shared by test_read_text_cpu.py (the model against itself) and test_gpu_read_text.py (the
device against the model)."""
import numpy as np

from fastq_text_model import fastq

TILE = 4096                         # gm_dev_fastq_tile_bytes(): test_gpu_read_text.py asserts that it still is


def _seq(n, salt=0):
    return bytes(b"ACGT"[(i * 7 + salt + i // 5) & 3] for i in range(n))


def _qual(n, salt=0):
    return bytes(33 + ((i * 11 + salt) % 60) for i in range(n))


def rec(i, L, ql=None, name=None):
    return (name if name is not None else b"r%d/len%d" % (i, L), _seq(L, i), _qual(L if ql is None else ql, i))


SMALL = fastq([rec(0, 36), rec(1, 5), rec(2, 50, 57), rec(3, 17)])


def good_texts():
    """{id: text}: every record well-formed"""
    t = {}
    t["empty"] = b""
    t["one_record"] = fastq([rec(0, 36)])
    t["no_trailing_newline"] = fastq([rec(0, 36), rec(1, 20)], last_newline=False)
    t["only_blank_lines"] = b"\n" * 9
    t["one_newline"] = b"\n"
    for k in (1, 2, 70):
        t[f"blank_runs_{k}"] = fastq([rec(0, 30)]) + b"\n" * k + fastq([rec(1, 12)]) + b"\n" * k + fastq([rec(2, 8)]) + b"\n" * k
    t["leading_blank_lines"] = b"\n\n\n" + fastq([rec(0, 30), rec(1, 31)])
    # length 0: the empty sequence and quality lines are those lines, not skipped ones; the blank run behind them is skipped
    t["length_zero_reads"] = fastq([rec(0, 0), rec(1, 9), rec(2, 0)]) + b"\n\n\n\n\n" + fastq([rec(3, 0)])
    t["length_zero_last"] = fastq([rec(0, 4)]) + b"@z\n\n+\n\n"                    # the fourth line is there, and empty (bad_texts has the form without it)
    t["quality_longer_than_sequence"] = fastq([rec(0, 30, 41), rec(1, 10, 11), rec(2, 16), rec(3, 0, 5)])
    t["name_is_only_at"] = fastq([(b"", _seq(20), _qual(20)), rec(1, 10)])
    t["name_1500_bytes"] = fastq([rec(0, 20, name=b"n" * 1500), rec(1, 10), rec(2, 12, name=b"m" * 1023), rec(3, 12, name=b"k" * 1024)])
    t["quality_starts_with_at_and_plus"] = fastq([(b"a", _seq(6), b"@IIIII"), (b"b", _seq(6), b"+IIIII"), (b"c", _seq(3), b"+plus", b"@@@")])
    t["crlf"] = fastq([rec(0, 30), rec(1, 12)], end=b"\r\n")
    t["nul_in_name"] = fastq([rec(0, 20, name=b"na\0me"), rec(1, 10, name=b"\0")])
    t["high_bytes"] = fastq([(b"\xff\x80", b"ACGTNacgtn", bytes(range(246, 256))), rec(1, 10)])
    t["stride_follows_the_maximum"] = fastq([rec(i, L) for i, L in enumerate((1, 7, 8, 9, 63, 64, 65, 2047, 2048))])
    for L in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65):
        t[f"all_length_{L}"] = fastq([rec(i, L, L + (i & 1)) for i in range(5)])
    t["many_records"] = fastq([rec(i, 20 + i % 37, 20 + i % 37 + (3 if i % 11 == 0 else 0)) for i in range(700)])          # several tiles of text and of lines
    return t


def prefix_lengths(tile=TILE):
    """k blank lines in front of SMALL, for k around every multiple of 16 (a lane's bytes; every fourth one a multiple of 64) up to 256,
    and around a wavefront's 1024 bytes, twice that, the tile size and twice that: each of the four lines of a record comes to lie on
    either side of a lane, wave and tile edge"""
    ks = set()
    for m in range(0, 257, 16):
        ks.update((m - 1, m, m + 1))
    # the lines of SMALL's first record start 0, 10, 47 and 49 bytes behind the prefix, the second record 86 bytes behind it
    for edge in (1024, 2048, tile, 2 * tile):
        for back in (0, 10, 47, 49, 86):
            ks.update((edge - back - 1, edge - back, edge - back + 1))
    return sorted(k for k in ks if k >= 0)


def bad_texts():
    """{id: text}: the block ends at a record that is not well-formed, or too long"""
    good = [rec(0, 30), rec(1, 12, 14), rec(2, 8)]
    g = fastq(good)
    t = {}
    t["missing_at"] = g + b"r3\nACGT\n+\nIIII\n" + fastq([rec(4, 9)])
    t["empty_plus_line"] = g + b"@r3\nACGT\n\nIIII\n" + fastq([rec(4, 9)])
    t["plus_line_without_plus"] = g + b"@r3\nACGT\n-\nIIII\n" + fastq([rec(4, 9)])
    t["quality_shorter_than_sequence"] = g + b"@r3\nACGT\n+\nIII\n" + fastq([rec(4, 9)])
    t["ends_after_1_line"] = g + b"@r3\n"
    t["ends_after_1_line_no_newline"] = g + b"@r3"
    t["ends_after_2_lines"] = g + b"@r3\nACGT\n"
    t["ends_after_3_lines"] = g + b"@r3\nACGT\n+r3"
    t["zero_length_ends_in_plus_newline"] = g + b"@z\n\n+\n"
    t["ends_in_plus_newline"] = g + b"@r3\nACGT\n+\n"                       # no fourth line: the text's last newline starts no line
    t["bad_first_record"] = b"r0\nACGT\n+\nIIII\n" + g
    t["bad_first_record_behind_blank_lines"] = b"\n\n" + b"r0\nACGT\n+\nIIII\n" + g
    t["bad_in_the_middle"] = fastq(good[:2]) + b"@r\nACGT\n+\nII\n" + fastq(good[2:])
    # two bad records, the first wins: 100 records are 400 lines and 9 KB.  The earlier bad record lies in the first tile of 256 lines
    # (and of 4096 bytes), a full one; the later one in the last tile, which is short and finishes early
    many = fastq([rec(i, 40) for i in range(100)])
    t["two_bad_first_wins"] = many[:many.index(b"@r20/")] + b"@x\nACGT\n+\nIII\n" + many[many.index(b"@r20/"):] + b"@y\nAC\n+\nI\n"
    t["two_bad_kinds_first_wins"] = many[:many.index(b"@r20/")] + b"@x\nACGT\n+\nIII\n" + many[many.index(b"@r20/"):] + fastq([rec(99, 2049)])
    t["too_long_before_malformed"] = g + fastq([rec(3, 2049)]) + b"r4\nACGT\n+\nIIII\n"
    t["too_long_after_malformed"] = g + b"r3\nACGT\n+\nIIII\n" + fastq([rec(4, 2049)])
    t["too_long_alone"] = fastq([rec(0, 2049)])
    t["too_long_and_short_quality"] = g + b"@r3\n" + _seq(2049) + b"\n+\n" + _qual(2048) + b"\n"         # the well-formed test comes first: malformed
    return t


def as_array(text):
    return np.frombuffer(bytes(text), np.uint8)
