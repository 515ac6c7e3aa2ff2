"""Paired-end reads on the device: gm_batch_set_mates through every sink.

The reference program has no paired mode, so the yardsticks are the project's own mates-off output (pinned byte for byte to the reference
elsewhere) and tests/mates_model.py: with the setting on, every row is the mates-off row with QNAME, FLAG, RNEXT, PNEXT and TLEN from
the model, which runs on the records Batch.output gives for the same hits.  Every comparison is of bytes, for equality, and no row is
left out.  The world is tests/mates_fixture.py (110 pairs, built once per module); its self_check asserts from the mates-off records that
every situation it exists for is there - among them the repeat pair whose concordant place is record 67 of 70, which a choice without
the mate (record 0) gets wrong.  Two more worlds have a test each: tests/mates_repeat2_fixture.py (both mates inside a repeat, 70 x 70
records) and tests/wide_fixture.py as one block of 85 pairs (mate columns of nine and ten characters).  The resolver alone, at sizes and
ties no mapped block gives it, is tests/test_gpu_mate_resolve.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
import bai_model as bai
import bam_model as bm
import fasta_model as fm
import mates_fixture as mx
import mates_model as mm
import sam_sort_model as ssm
import unmapped_model as um
from conftest import ROOT
from gnumap_amd import api

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
GM_E_ARG, GM_E_CAPACITY = -1, -5
LO, HI = mx.MIN_INSERT, mx.MAX_INSERT


def split(text, row_off):
    assert int(row_off[0]) == 0 and int(row_off[-1]) == len(text)
    return [text[int(row_off[k]):int(row_off[k + 1])] for k in range(len(row_off) - 1)]


class Run:
    """a block of pairs mapped once on one handle; rows and records with mates off and on"""

    def __init__(self, ix, p, reads, fasta=False):
        self.ix, self.p, self.n = ix, p, len(reads)
        self.names = [r[0] for r in reads]; self.seqs = [r[1] for r in reads]
        self.quals = [fm.synth_qual(r[1]) for r in reads] if fasta else [r[2] for r in reads]
        B, Q, Ln = g.pack_reads(self.seqs, None if fasta else self.quals)
        self.batch = g.Batch(ix, len(reads), B.shape[1])
        self.res = self.batch.map(p, B, Q, Ln, fasta=fasta)
        self.recs, self.cigars = self.batch.output(p, self.res)             # mates off: the records the model runs on
        self.off_text, off = self.batch.output_text(p, self.res, self.names, None)
        self.off_rows = split(self.off_text, off)
        assert len(self.off_rows) == len(self.recs)
        self.cnames = [c for c, _ in ix.contigs()]
        self.qn = mm.block_qnames(self.names) if self.n % 2 == 0 else None

    def on(self, lo=LO, hi=HI):
        self.batch.set_mates(True, lo, hi)

    def off(self):
        self.batch.set_mates(False)

    def row_source(self, unmapped):
        """(mates-off rows, [("r", record) | ("u", read)]) in row order"""
        if not unmapped:
            return list(self.off_rows), [("r", k) for k in range(len(self.recs))]
        merged, new = um.merge(self.off_rows, self.recs["read"], self.names, self.seqs, self.quals, self.res["status"])
        have = set(int(x) for x in self.recs["read"])
        src, k = [], 0
        for i in range(self.n):
            if i in have:
                while k < len(self.recs) and int(self.recs["read"][k]) == i:
                    src.append(("r", k)); k += 1
            else:
                src.append(("u", i))
        assert len(src) == len(merged) and [s[0] == "u" for s in src] == list(new)
        return merged, src

    def fields(self, unmapped=False, lo=LO, hi=HI):
        return mm.row_fields(self.recs, self.cigars, self.n, lo, hi, self.row_source(unmapped)[1])

    def read_of(self, s):
        return int(self.recs["read"][s[1]]) if s[0] == "r" else s[1]

    def want_rows(self, unmapped=False, lo=LO, hi=HI, base=None):
        rows, src = self.row_source(unmapped)
        if base is not None:
            rows = base
        f = mm.row_fields(self.recs, self.cigars, self.n, lo, hi, src)
        return [mm.text_row(r, ff, self.qn[self.read_of(s)], self.cnames) for r, ff, s in zip(rows, f, src)]

    def want_bam(self, off_recs, unmapped=False, lo=LO, hi=HI):
        _, src = self.row_source(unmapped)
        f = mm.row_fields(self.recs, self.cigars, self.n, lo, hi, src)
        assert len(off_recs) == len(src)
        return [mm.bam_record(r, ff, self.qn[self.read_of(s)]) for r, ff, s in zip(off_recs, f, src)]

    def text(self):
        text, off = self.batch.output_text(self.p, self.res, self.names, None)
        return split(text, off), off

    def bam(self, level=1):
        return bm.split_records(bm.bgzf_payload(self.batch.output_bam(self.p, self.res, self.names, None, level=level)))

    def destroy(self):
        self.batch.destroy()


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    w = mx.World(tmp_path_factory.mktemp("mates"), g.index_build)
    ix = g.Index(w.fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    main = Run(ix, p, w.reads)
    seen = mx.self_check(w, main.recs, main.cigars)               # from the mates-off records: every situation of the table is there
    yield dict(w=w, ix=ix, p=p, main=main, seen=seen, contigs=ix.contigs())
    main.destroy()
    ix.close()


# ---- 1. the fields and the counters ----------------------------------------------------------------------------------------------
def test_mate_rows_and_stats_equal_the_models(env):
    r = env["main"]
    r.on()
    try:
        r.batch.output(r.p, r.res)                                # the records sink runs the step too
        got = r.batch.mate_rows()
        want = r.fields()
        assert [tuple(int(v) for v in x) for x in got] == want and len(want) == len(r.recs) > 256
        assert r.batch.mate_stats() == mm.stats(r.recs, r.cigars, r.n, LO, HI)
        rows, _ = r.text()
        assert [tuple(int(v) for v in x) for x in r.batch.mate_rows()] == want and len(rows) == len(want)
        assert r.batch.mate_stats() == mm.stats(r.recs, r.cigars, r.n, LO, HI)
    finally:
        r.off()
    st = mm.stats(r.recs, r.cigars, r.n, LO, HI)
    assert st["pairs"] == 110 and st["proper"] >= 90 and st["one_mapped"] == 4 and st["none_mapped"] == 1
    # symmetry, on the device's own fields: A's PNEXT is B's POS, opposite TLENs, 0x20 of A is 0x10 of B's primary, 0x2 on both or neither
    prim, proper = mm.resolve(r.recs, r.cigars, r.n, LO, HI)
    for i in range(r.n // 2):
        a, b = prim[2 * i], prim[2 * i + 1]
        if a is None or b is None:
            continue
        fa, fb = got[a], got[b]
        assert int(fa["pnext"]) == int(r.recs[b]["chr_pos"]) and int(fb["pnext"]) == int(r.recs[a]["chr_pos"])
        assert int(fa["tlen"]) == -int(fb["tlen"])
        assert bool(fa["flag"] & 0x20) == bool(fb["flag"] & 0x10) and bool(fb["flag"] & 0x20) == bool(fa["flag"] & 0x10)
        assert bool(fa["flag"] & 0x2) == bool(fb["flag"] & 0x2) == proper[i]


def test_text_rows_equal_the_models(env):
    r = env["main"]
    r.on()
    try:
        rows, off = r.text()
    finally:
        r.off()
    want = r.want_rows()
    assert rows == want
    assert [int(x) for x in off] == [0] + list(np.cumsum([len(x) for x in want]))
    for a, b in zip(rows, r.off_rows):                            # every other field is the mates-off row's
        fa, fb = a.split(b"\t"), b.split(b"\t")
        assert fa[2:6] == fb[2:6] and fa[9:] == fb[9:]
    named = [x.split(b"\t")[6] for x in rows]
    assert b"=" in named and b"*" in named and (b"mA" in named or b"mB" in named)
    i = env["w"].pair_of("repeat_a")[0]
    mine = [x for x, k in zip(rows, r.recs["read"]) if int(k) == 2 * i]
    assert len(mine) == mx.ELEM_N and [int(x.split(b"\t")[1]) & 0x100 == 0 for x in mine].index(True) == mx.ELEM_COPY
    assert sum(int(x.split(b"\t")[1]) & 0x2 != 0 for x in mine) == 1


@pytest.mark.parametrize("level", [0, 1])
def test_bam_records_equal_the_models(env, level):
    r = env["main"]
    off = r.bam(level)
    r.on()
    try:
        got = r.bam(level)
    finally:
        r.off()
    assert got == r.want_bam(off)
    f = r.fields()
    for rec, ff, k in zip(got, f, r.recs["read"]):
        flag, nr, npos, tl, name = mm.bam_fields(rec)
        assert (flag, nr, npos, tl) == (ff[0], ff[1], ff[2] - 1, ff[3]) and name == r.qn[int(k)][:254]
        assert struct.unpack_from("<i", rec, 0)[0] == len(rec) - 4


# ---- 2. the sorter and the index -------------------------------------------------------------------------------------------------
def sorted_rows(rows, contigs):
    return [x.encode("latin-1") for x in ssm.sort_rows([x.decode("latin-1") for x in rows], [c for c, _ in contigs])]


def test_sorter_text_rows(env):
    r = env["main"]
    s = api.SamSorter(env["ix"], rows="text")
    r.on()
    try:
        s.add_block(r.batch, r.p, r.res, 0, names=r.names, qual_tails=None)
    finally:
        r.off()
    want = sorted_rows(r.want_rows(), env["contigs"])
    assert s.finish()[0] == len(want)
    assert s.text() == b"".join(want)
    s.destroy()


def test_sorter_bam_rows_with_unmapped_rows_and_the_bai(env):
    r = env["main"]
    ix = env["ix"]
    r.batch.set_unmapped_rows(True)
    try:
        off = r.bam()
        s = api.SamSorter(ix, rows="bam")
        r.on()
        try:
            s.add_block(r.batch, r.p, r.res, 0, names=r.names, qual_tails=None)
        finally:
            r.off()
    finally:
        r.batch.set_unmapped_rows(False)
    recs = r.want_bam(off, unmapped=True)
    rows = r.want_rows(unmapped=True)
    rank = {c: i for i, (c, _) in enumerate(env["contigs"])}
    order = sorted(range(len(rows)), key=lambda k: ssm.row_key(rows[k].decode("latin-1"), rank))
    assert s.finish()[0] == len(recs)
    head = ix.bgzf_compress(ix.bam_header(b"@HD\tVN:1.0\tSO:coordinate\n"), level=1)
    s.index_begin(len(head))
    slabs = []
    while True:
        t = s.read_bgzf(60000, level=1)
        if not t:
            break
        slabs.append(t)
    data = head + b"".join(slabs) + api.bgzf_eof()
    sc = bai.scan(data)
    got = [bytes(x) for x in sc["recs"]]
    assert got == [recs[k] for k in order]
    n_unmapped = sum(struct.unpack_from("<H", x, 18)[0] & 0x4 != 0 for x in got)
    assert n_unmapped == 6 and all(struct.unpack_from("<i", x, 4)[0] == -1 for x in got[-n_unmapped:])
    index = s.bai()
    assert index == bai.build_bai(data)
    assert bai.check_queries(data, index, bai.regions_of(data, n_random=20)) > 100
    s.destroy()


# ---- 3. with the other row settings ----------------------------------------------------------------------------------------------
def test_unmapped_rows_carry_their_mates_fields(env):
    r = env["main"]
    r.batch.set_unmapped_rows(True)
    try:
        off_bam = r.bam()
        r.on()
        try:
            rows, _ = r.text()
            got_fields = [tuple(int(v) for v in x) for x in r.batch.mate_rows()]
            got_bam = r.bam()
        finally:
            r.off()
    finally:
        r.batch.set_unmapped_rows(False)
    merged, src = r.row_source(True)
    want = r.want_rows(unmapped=True)
    assert rows == want and got_fields == r.fields(unmapped=True)
    assert got_bam == r.want_bam(off_bam, unmapped=True)
    new = [x for x, s in zip(rows, src) if s[0] == "u"]
    assert len(new) == 6
    flags = sorted(int(x.split(b"\t")[1]) for x in new)
    assert all(f & 0x4 and f & 0x1 for f in flags) and sum(bool(f & 0x8) for f in flags) == 2       # the pair with no mapped mate
    for x in new:
        c = x.split(b"\t")
        assert c[2] == b"*" and c[3] == b"0" and c[8] == b"0" and c[-1].startswith(b"YU:i:")
        assert (c[6] == b"*") == (c[7] == b"0") and c[6] != b"="


def test_md_tags_and_forward_cigars_follow_unchanged(env):
    r = env["main"]
    r.batch.set_row_tags(True); r.batch.set_cigar_order("forward")
    try:
        base_rows, _ = r.text()
        base_bam = r.bam()
        r.on()
        try:
            rows, _ = r.text()
            got_bam = r.bam()
        finally:
            r.off()
    finally:
        r.batch.set_row_tags(False); r.batch.set_cigar_order("gnumap")
    assert any(b"\tMD:Z:" in x for x in base_rows)
    assert rows == r.want_rows(base=base_rows)
    assert got_bam == r.want_bam(base_bam)


def check_run(r):
    r.on()
    try:
        rows, _ = r.text()
        fields = [tuple(int(v) for v in x) for x in r.batch.mate_rows()]
        stats = r.batch.mate_stats()
    finally:
        r.off()
    off_bam = r.bam()
    r.on()
    try:
        got_bam = r.bam()
    finally:
        r.off()
    assert rows == r.want_rows() and fields == r.fields() and stats == mm.stats(r.recs, r.cigars, r.n, LO, HI)
    assert got_bam == r.want_bam(off_bam)
    return rows


@pytest.mark.parametrize("kw", [dict(print_all_sam=1), dict(nw=0), dict(max_matches=2)], ids=["print_all_sam", "no_nw", "T2"])
def test_other_parameters(env, kw):
    r = Run(env["ix"], g.Params(**kw), env["w"].reads)
    try:
        rows = check_run(r)
        assert len(rows) >= 100
        if "print_all_sam" in kw:
            assert any(int(x.split(b"\t")[1]) & 0x100 for x in rows)
    finally:
        r.destroy()


def test_fasta_block(env):
    r = Run(env["ix"], g.Params(), [(n, s, b"") for n, s, _ in env["w"].reads], fasta=True)
    try:
        assert len(check_run(r)) >= 100
    finally:
        r.destroy()


def test_resident_form_gives_the_same_rows(env):
    r = env["main"]
    batch = g.Batch(env["ix"], 4096, 2048)
    try:
        info = batch.upload_text(env["p"], mx.fastq(env["w"].reads))
        assert info["n"] == r.n
        res = batch.map_text(env["p"])
        off, _ = batch.output_text_resident(env["p"], res)
        assert off == r.off_text
        off_bam = bm.split_records(bm.bgzf_payload(batch.output_bam_resident(env["p"], res)))
        batch.set_mates(True, LO, HI)
        text, row_off = batch.output_text_resident(env["p"], res)
        assert split(text, row_off) == r.want_rows()
        assert bm.split_records(bm.bgzf_payload(batch.output_bam_resident(env["p"], res))) == r.want_bam(off_bam)
    finally:
        batch.destroy()


# ---- 4. several trips per workgroup, and the setting off ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 2])
def test_grid_cap_gives_the_same_bytes(env, cap):
    r = env["main"]
    want = r.want_rows()
    off_bam = r.bam()
    g.set_option("GM_TEST_GRID_CAP", cap)
    r.on()
    try:
        rows, _ = r.text()
        fields = [tuple(int(v) for v in x) for x in r.batch.mate_rows()]
        capped = r.bam()
    finally:
        r.off()
        g.set_option("GM_TEST_GRID_CAP", None)
    assert r.n // 2 > 8 * cap                                     # k_mate_resolve: several pairs per workgroup
    assert rows == want and fields == r.fields() and capped == r.want_bam(off_bam)


def test_on_off_on_leaves_the_mates_off_bytes(env):
    r = env["main"]
    off_bam = r.batch.output_bam(r.p, r.res, r.names, None, level=1)
    r.on()
    try:
        first, _ = r.text()
    finally:
        r.off()
    text, off = r.batch.output_text(r.p, r.res, r.names, None)
    assert text == r.off_text and split(text, off) == r.off_rows
    assert r.batch.output_bam(r.p, r.res, r.names, None, level=1) == off_bam
    assert len(r.batch.mate_rows()) == 0
    r.on()
    try:
        again, _ = r.text()
    finally:
        r.off()
    assert first == again == r.want_rows()


def test_the_mate_kernels_are_timed_only_with_the_setting_on(env):
    r = env["main"]
    r.batch.set_profiling(True)
    try:
        r.batch.kernel_times()
        r.text()
        assert r.batch.kernel_times()["k_mate_*"][1] == 0
        r.on()
        try:
            r.text()
        finally:
            r.off()
        ms, launches = r.batch.kernel_times()["k_mate_*"]
        assert launches >= 1 and ms > 0
    finally:
        r.batch.set_profiling(False)


def test_insert_limits_are_inclusive(env):
    r, w = env["main"], env["w"]
    prim, proper = mm.resolve(r.recs, r.cigars, r.n, LO, HI)
    for kind, want in (("ins_max", True), ("ins_over", False), ("ins_min", True), ("ins_under", False)):
        assert proper[w.pair_of(kind)[0]] == want
    r.on(LO - 1, HI + 1)                                          # one wider on both sides: the two that were out are in
    try:
        rows, _ = r.text()
    finally:
        r.off()
    assert rows == r.want_rows(lo=LO - 1, hi=HI + 1)
    flags = {int(k): int(x.split(b"\t")[1]) for x, k in zip(rows, r.recs["read"])}
    assert all(flags[2 * w.pair_of(k)[0]] & 0x2 for k in ("ins_max", "ins_over", "ins_min", "ins_under"))


# ---- 4b. two more worlds: both mates inside a repeat, and columns of nine and ten characters --------------------------------------
def test_two_sided_repeat_70_x_70(tmp_path):
    """tests/mates_repeat2_fixture.py: both mates have 70 records, 70 of the 4900 combinations are concordant and all have one product,
    so the primaries are the first records of both mates - the tie goes to the smallest index of the first mate, then of the second"""
    import mates_repeat2_fixture as r2
    w = r2.World(tmp_path, g.index_build)
    ix = g.Index(w.fa, device=0, flags=g.GM_INDEX_FULL_SA)
    r = Run(ix, g.Params(), w.reads)
    lo, hi = r2.MIN_INSERT, r2.MAX_INSERT
    try:
        assert r2.self_check(w, r.recs, r.cigars) == len(r.recs) == 422         # from the mates-off records
        off_bam = r.bam()
        r.on(lo, hi)
        try:
            rows, _ = r.text()
            fields = [tuple(int(v) for v in x) for x in r.batch.mate_rows()]
            stats = r.batch.mate_stats()
            got_bam = r.bam()
        finally:
            r.off()
        assert rows == r.want_rows(lo=lo, hi=hi) and fields == r.fields(lo=lo, hi=hi) and got_bam == r.want_bam(off_bam, lo=lo, hi=hi)
        assert stats == mm.stats(r.recs, r.cigars, r.n, lo, hi) == dict(pairs=4, both_mapped=4, proper=4, one_mapped=0, none_mapped=0)
        for i in range(3):
            mine = [(k, f) for k, f in enumerate(fields) if int(r.recs["read"][k]) >> 1 == i]
            assert len(mine) == 140 and [k - mine[0][0] for k, f in mine if not f[0] & 0x100] == [0, 70]       # the first record of either mate
            assert all(f[0] & 0x2 for k, f in mine if not f[0] & 0x100) and all(f[3] == 0 for k, f in mine if f[0] & 0x100)
            assert sorted(f[3] for k, f in mine if not f[0] & 0x100) == [-300, 300]
    finally:
        r.destroy()
        ix.close()


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """the world of tests/wide_fixture.py (a 100 Mbp contig and 41 short ones), its 170 reads as ONE block of 85 pairs with equal names"""
    import wide_fixture as wf
    w = wf.World(tmp_path_factory.mktemp("mates_wide"), g.index_build)
    ix = g.Index(w.fa, device=0, flags=g.GM_INDEX_FULL_SA)
    assert len(w.reads) == 170
    run = Run(ix, g.Params(**wf.KW), [(b"wide:%d" % (i >> 1), r.seq, r.qual) for i, r in enumerate(w.reads)])
    yield run
    run.destroy()
    ix.close()


def test_wide_columns(wide):
    """PNEXT and TLEN of nine and ten characters, RNEXT a contig's name: k_mate_row_len's digit counts and the row kernels' mate columns
    where tests/mates_fixture.py's 40 000-base contigs never take them.  Every pair of records on one contig with different strands and
    POS_f <= POS_r is concordant under [0, 2^32 - 1]"""
    r = wide
    lo, hi = 0, 0xFFFFFFFF
    assert len(r.cnames) == 42 and len(r.recs) == 154
    want = r.want_rows(lo=lo, hi=hi)
    cols = [x.split(b"\t") for x in want]
    assert any(len(c[7]) == 9 for c in cols)                                                      # PNEXT of nine digits
    assert any(len(c[8]) >= 8 and not c[8].startswith(b"-") for c in cols) and any(len(c[8]) >= 9 and c[8].startswith(b"-") for c in cols)
    named = {c[6] for c in cols} - {b"=", b"*"}
    assert named and named <= {n.encode() for n in r.cnames}                                      # RNEXT that is a contig's name
    assert any(c[6] == b"=" for c in cols) and any(int(c[1]) & 0x2 for c in cols)
    off_bam = r.bam()
    r.batch.set_unmapped_rows(True)
    try:
        off_bam_un = r.bam()
    finally:
        r.batch.set_unmapped_rows(False)
    r.on(lo, hi)
    try:
        rows, off = r.text()
        got_bam = r.bam()
        r.batch.set_unmapped_rows(True)
        try:
            rows_un, _ = r.text()
            got_bam_un = r.bam()
        finally:
            r.batch.set_unmapped_rows(False)
    finally:
        r.off()
    assert rows == want and [int(x) for x in off] == [0] + list(np.cumsum([len(x) for x in want]))
    want_un = r.want_rows(unmapped=True, lo=lo, hi=hi)
    assert rows_un == want_un and len(want_un) == 170 and any(int(x.split(b"\t")[1]) & 0x4 and len(x.split(b"\t")[7]) >= 8 for x in want_un)
    assert got_bam == r.want_bam(off_bam, lo=lo, hi=hi)
    assert got_bam_un == r.want_bam(off_bam_un, unmapped=True, lo=lo, hi=hi)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    r, w = env["main"], env["w"]
    L = g.lib()
    assert L.gm_batch_set_mates(None, 1, 0, 500) == GM_E_ARG
    r.on(10, 5)
    try:
        with pytest.raises(g.GnumapError, match="min_insert 10 is above max_insert 5"):
            r.text()
    finally:
        r.off()
    odd = Run(env["ix"], env["p"], w.reads[:31])
    odd.on()
    try:
        with pytest.raises(g.GnumapError, match="odd number of reads"):
            odd.batch.output(odd.p, odd.res)
        with pytest.raises(g.GnumapError, match="odd number of reads"):
            odd.batch.output_text(odd.p, odd.res, odd.names, None)
    finally:
        odd.off(); odd.destroy()
    # a name mismatch: the message names the first such pair by index
    names = list(r.names)
    names[2 * 7 + 1] = b"someone_else"; names[2 * 30] = b"another"
    assert mm.first_mismatch(names) == 7
    r.on()
    try:
        with pytest.raises(g.GnumapError, match=r"names of pair 7 \(reads 14 and 15") as e:
            r.batch.output_text(r.p, r.res, names, None)
        assert e.value.code == GM_E_ARG
        rows, _ = r.text()                                        # the batch is still good
        assert rows == r.want_rows()
        n = api.u64()
        want = len(rows)
        buf = np.zeros(want, api.MATE_ROW_DTYPE)
        assert L.gm_batch_mate_rows(r.batch.h, buf.ctypes.data, want - 1, n) == GM_E_CAPACITY and n.value == want
        assert not buf.view(np.uint8).any()                       # nothing is written
        assert L.gm_batch_mate_rows(r.batch.h, buf.ctypes.data, want, n) == 0 and n.value == want
    finally:
        r.off()


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------------
def drive(fa, out, extra, reads, ok=True):
    r = subprocess.run([EXE, "-g", fa, "-o", out, f"--min_insert={LO}", f"--max_insert={HI}"] + extra + [reads], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r


def rows_of(path):
    return [l for l in open(path, "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]


@pytest.fixture(scope="module")
def files(env, tmp_path_factory):
    d = tmp_path_factory.mktemp("mates_files")
    reads = env["w"].reads
    paths = dict(one=str(d / "r1.fq"), two=str(d / "r2.fq"), both=str(d / "r12.fq"), short=str(d / "r2_short.fq"), dir=d)
    open(paths["one"], "wb").write(mx.fastq(reads[0::2]))
    open(paths["two"], "wb").write(mx.fastq(reads[1::2]))
    open(paths["both"], "wb").write(mx.fastq(reads))
    open(paths["short"], "wb").write(mx.fastq(reads[1::2][:-1]))
    return paths


def test_cli_two_files_and_interleaved_give_the_models_rows(env, files):
    r, fa = env["main"], env["w"].fa
    want = r.want_rows()
    out = str(files["dir"] / "two")
    run = drive(fa, out, ["--mates=" + files["two"], "--batch=64"], files["one"])
    assert rows_of(out + ".sam") == want
    st = mm.stats(r.recs, r.cigars, r.n, LO, HI)
    assert f"--mates: {st['pairs']} pairs: {st['both_mapped']} with both mates mapped ({st['proper']} of them proper" in run.stderr
    assert f"{st['one_mapped']} with one mate mapped, {st['none_mapped']} with none" in run.stderr
    head = [l for l in open(out + ".sam", "rb").read().splitlines() if l.startswith(b"@PG")]
    assert len(head) == 1 and b"--mates=" in head[0] and b"--max_insert=500" in head[0]
    out = str(files["dir"] / "inter")
    drive(fa, out, ["--interleaved"], files["both"])
    assert rows_of(out + ".sam") == want


def test_cli_archive_run_is_the_models_records_sorted(env, files):
    r, fa = env["main"], env["w"].fa
    r.batch.set_unmapped_rows(True); r.batch.set_row_tags(True)
    try:
        off = r.bam()
    finally:
        r.batch.set_unmapped_rows(False); r.batch.set_row_tags(False)
    want = r.want_bam(off, unmapped=True)
    rows = r.want_rows(unmapped=True)
    rank = {c: i for i, (c, _) in enumerate(env["contigs"])}
    order = sorted(range(len(rows)), key=lambda k: ssm.row_key(rows[k].decode("latin-1"), rank))
    out = str(files["dir"] / "arch")
    drive(fa, out, ["--mates=" + files["two"], "--batch=64", "--sam_format=bam", "--sam_sort=coordinate", "--bam_index", "--sam_unmapped", "--sam_md"], files["one"])
    data, index = open(out + ".bam", "rb").read(), open(out + ".bam.bai", "rb").read()
    got = [bytes(x) for x in bai.scan(data)["recs"]]
    assert got == [want[k] for k in order]
    assert any(b"MDZ" in x for x in got) and sum(um.record_is_unmapped(x) for x in got) == 6
    assert index == bai.build_bai(data)


def test_cli_files_out_of_step_and_a_run_without_mates(env, files):
    fa, w = env["w"].fa, env["w"]
    out = str(files["dir"] / "short")
    run = drive(fa, out, ["--mates=" + files["short"]], files["one"], ok=False)
    assert run.returncode == 1 and files["one"] in run.stderr and files["short"] in run.stderr and "different numbers of reads" in run.stderr
    odd = str(files["dir"] / "odd.fq")
    open(odd, "wb").write(mx.fastq(w.reads[:31]))
    run = drive(fa, out, ["--interleaved"], odd, ok=False)
    assert run.returncode == 1 and odd in run.stderr and "odd number of reads" in run.stderr
    bad = str(files["dir"] / "bad.fq")
    open(bad, "wb").write(mx.fastq(w.reads[1::2][:5]) + b"@broken\nACGT\nIIII\n" + mx.fastq(w.reads[1::2][6:]))
    run = drive(fa, out, ["--mates=" + bad], files["one"], ok=False)
    assert run.returncode == 1 and bad in run.stderr and "malformed" in run.stderr
    # the first file alone, without --mates: the bytes of the rows with mates off
    half = Run(env["ix"], env["p"], w.reads[0::2])
    try:
        out = str(files["dir"] / "single")
        r = subprocess.run([EXE, "-g", fa, "-o", out, "--sam_text=device", files["one"]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert rows_of(out + ".sam") == half.off_rows and "--mates" not in r.stderr
    finally:
        half.destroy()
