"""The table of tests/wide_fixture.py without a genome: its arithmetic, and its bin literals against bam_model and bai_model (SAMv1
section 5.3).  The reads themselves, and the oracle's records of them, are checked where the world is built
(tests/test_gpu_wide_coords.py::world)."""
import bai_model as bai
import bam_model as bm
import wide_fixture as wf


def test_contigs_lie_behind_chrW_at_offsets_above_10_8():
    contigs = wf.contig_table()
    assert contigs[0] == ("chrW", 100_001_000) and len(contigs) == 42
    assert {n for _, n in contigs[1:]} == {150, 1000, 16_384, 16_385, 20_000, 131_172}
    offs = [0]
    for _, n in contigs:
        offs.append(offs[-1] + n)
    assert all(o > 10 ** 8 for o in offs[1:]) and offs[-1] < 2 ** 29          # one contig would still fit a .bai
    assert sorted(len(name) for name, _ in contigs)[0] == 1 and max(len(name) for name, _ in contigs) == 200
    assert contigs[9][0] == "Z" and len(contigs[10][0]) == 200 and contigs[2][1] == 150 and contigs[41][1] == 16_385
    assert len({name for name, _ in contigs}) == 42


def test_every_place_lies_in_its_contig_and_every_class_is_there():
    lens = [n for _, n in wf.contig_table()]
    for pl in wf.PLACES:
        assert 0 <= pl.start and pl.start + max(wf.SPANS[pl.kind], wf.WRONG_SPANS.get(pl.kind, 0)) <= lens[pl.contig], pl
    assert {pl.cls for pl in wf.PLACES} == {"digits", "bins", "indels", "short", "ties"}
    assert len({(pl.cls, pl.label) for pl in wf.PLACES}) == len(wf.PLACES)
    first_last = {(pl.contig, pl.start) for pl in wf.PLACES if pl.cls == "short"}
    for c in (1, 9, 10, 41):
        assert (c, 0) in first_last and (c, lens[c] - 100) in first_last
    assert (2, 25) in first_last
    assert wf.PLACES[[pl.label for pl in wf.PLACES].index("end_of_chrW")].start == 100_000_900


def test_digit_positions_have_one_to_nine_digits_on_both_sides_of_every_change():
    starts = {pl.start + 1 for pl in wf.PLACES if pl.cls == "digits"}
    for e in range(1, 9):
        assert 10 ** e - 1 in starts and 10 ** e in starts
    assert 1 in starts and 100_000_901 in starts
    assert {len(str(s)) for s in starts} == set(range(1, 10))


def test_bin_literals_are_reg2bin_of_the_span_the_cigar_has():
    for pl in wf.PLACES:
        end = pl.start + wf.SPANS[pl.kind]
        assert bm.reg2bin(pl.start, end) == pl.bin, pl
        assert pl.bin in bai.reg2bins(pl.start, end), pl          # the bins a reader looks into for the place hold the record's
    seen = {pl.bin for pl in wf.PLACES}
    assert set(wf.BIN_LITERALS) <= seen
    for lit in (4685, 4686, 4704, 4705, 4872, 4873, 6216, 6217, 8776, 8777, 8778, 585, 73, 9, 1, 0, 1097, 5291, 10784):
        assert lit in seen, lit


def test_boundary_reads_stay_or_cross_as_the_table_says():
    by = {pl.label: pl for pl in wf.PLACES}
    level = {585: 17, 73: 20, 9: 23, 1: 26, 0: 29, 1097: 17}
    for B, (below, at), cross in wf.BOUNDARIES:
        assert (by["B%d-100" % B].bin, by["B%d" % B].bin) == (below, at) and at == below + 1
        for d in (1, 99, 50):
            pl = by["B%d-%d" % (B, d)]
            assert pl.start < B < pl.start + 100 and pl.bin == cross
        sh = level[cross]                                       # the crossing read lies in one window of this level and in two of the next finer
        assert (B - 1) >> sh == B >> sh and (B - 1) >> (sh - 3) != B >> (sh - 3)
    assert bm.reg2bin(9_999_998, 10_000_098) == 5291 and bm.reg2bin(99_999_999, 100_000_099) == 10784


def test_indel_places_tell_the_cigar_span_from_the_wrong_ones():
    """the bin of a "D" or "I" place changes when the end is taken with the I runs counted, or from the read length"""
    n = {"D": 0, "I": 0}
    for pl in wf.PLACES:
        if pl.kind == "M":
            continue
        wrong = bm.reg2bin(pl.start, pl.start + wf.WRONG_SPANS[pl.kind])
        assert wrong != pl.bin, pl
        n[pl.kind] += 1
    assert n == {"D": 6, "I": 6}
    for (B, back, below, cross), (_, _, want_cross) in zip(wf.I_PLACES, wf.BOUNDARIES):
        assert cross == want_cross and bm.reg2bin(B - back, B - back + 100) == cross and B - back + 98 <= B
    for B, (below, _), cross in wf.BOUNDARIES:
        assert bm.reg2bin(B - 100, B + 2) == cross and bm.reg2bin(B - 100, B) == below


def test_reads_blocks_and_helpers():
    assert wf.revcomp(b"AACGT") == b"ACGTT"
    assert wf.block_ranges(170) == [(0, 37), (37, 138), (138, 170)]
    assert 2 * len(wf.PLACES) + 2 * (wf.N_DUP - 1) + wf.N_NOWHERE == 170
    ref = b"ACGTTGCATGCAAGCTTAGCAT"
    q = wf._indel_point(ref, 4)
    assert ref[q - 1] != ref[q + 1] and ref[q] != ref[q + 2]
