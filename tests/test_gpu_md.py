"""NM:i / MD:Z on the device and CIGARs in reference order: gm_batch_set_row_tags and gm_batch_set_cigar_order through every
row-producing sink, --sam_md and --sam_cigar.

The reference program prints no such tag, so the yardsticks are the project's own flag-off rows (pinned byte for byte to the reference
elsewhere) and tests/md_model.py: the rows with the tags on are the flag-off rows with the model's two tags behind X0, the rows under
"forward" are the flag-off rows with column 6 of the minus-strand rows turned round.  Every comparison is of bytes, for equality, and
no row is left out.  rebuild_reference (SEQ + CIGAR + MD -> the reference, without looking at it) checks the device's strings a second
way.

Blocks are syn.fq reads plus tests/md_fixture.py's planted reads (64 to 400 reads).  Each test first asserts from the FLAG-OFF rows that
the shapes it exists for are there.  The fixture yields no row with CIGAR "*" (no run of the reference program over syn.fq prints one
either), so that shape is covered by the CPU test of the model alone and by the kernels' shared rule (md_row_has_tags)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
import bai_model as bai
import bam_model as bm
import fasta_model as fm
import md_fixture as mf
import md_model as mm
import sam_sort_model as ssm
import unmapped_model as um
from conftest import GOLDEN, ROOT
from gnumap_amd import api

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
GM_E_ARG, GM_E_IO, GM_E_UNSUPPORTED = -1, -2, -6


def split(text, row_off):
    assert int(row_off[0]) == 0 and int(row_off[-1]) == len(text)
    return [text[int(row_off[k]):int(row_off[k + 1])] for k in range(len(row_off) - 1)]


def fields(row):
    return row.rstrip(b"\n").split(b"\t")


def ref_columns_of_d(cigar):
    """reference columns (relative to POS-1) every D token of a CIGAR field covers"""
    cols, x = [], 0
    for n, op in mm.tokens(cigar):
        if op == b"D":
            cols.extend(range(x, x + n))
        if op != b"I":
            x += n
    return cols


class Run:
    """a block mapped once on one handle; rows and records under any of the four settings"""

    def __init__(self, ix, p, reads, texts, fasta=False):
        self.ix, self.p, self.T = ix, p, texts
        self.names = [r[0] for r in reads]; self.seqs = [r[1] for r in reads]
        quals = [fm.synth_qual(r[1]) for r in reads] if fasta else [r[2] for r in reads]
        B, Q, Ln = g.pack_reads(self.seqs, None if fasta else quals)
        self.batch = g.Batch(ix, len(reads), B.shape[1])
        self.res = self.batch.map(p, B, Q, Ln, fasta=fasta)
        self.off_text, off = self.text(False, "gnumap")
        self.off_rows = split(self.off_text, off)

    def set(self, md, order):
        self.batch.set_row_tags(md); self.batch.set_cigar_order(order)

    def text(self, md, order):
        self.set(md, order)
        try:
            return self.batch.output_text(self.p, self.res, self.names, None)
        finally:
            self.set(False, "gnumap")

    def bam(self, md, order, level=1):
        self.set(md, order)
        try:
            return bm.split_records(bm.bgzf_payload(self.batch.output_bam(self.p, self.res, self.names, None, level=level)))
        finally:
            self.set(False, "gnumap")

    def want_rows(self, md, order):
        rows = [mm.forward_row(r) for r in self.off_rows] if order == "forward" else list(self.off_rows)
        return [mm.insert_tags(r, self.T) for r in rows] if md else rows

    def check_text(self, md, order):
        text, row_off = self.text(md, order)
        want = self.want_rows(md, order)
        assert split(text, row_off) == want
        assert [int(x) for x in row_off] == [0] + list(np.cumsum([len(r) for r in want]))
        return want

    def destroy(self):
        self.batch.destroy()


@pytest.fixture(scope="module")
def texts(syn_fa):
    return mm.contig_texts(syn_fa)


@pytest.fixture(scope="module")
def env(syn_fa, syn_reads, texts):
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    sr = [(nm.encode(), s, q) for nm, s, q in syn_reads]
    planted = mf.planted(lambda b, L: ix.window(b, L))
    reads = sr[:300] + planted
    assert 64 <= len(reads) <= 400
    runs = {"main": Run(ix, p, reads, texts)}
    yield dict(ix=ix, p=p, sr=sr, planted=planted, runs=runs, T=texts, contigs=ix.contigs())
    for r in runs.values():
        r.destroy()
    ix.close()


def shapes(rows, T):
    """what the flag-off rows hold, from the rows alone (the model's MD is of the row as printed)"""
    out = dict(d_over_64=0, d_over_128=0, n_in_md=0, minus_indel=0, run_1000=0, star=0, multi=0, other_strand=0, lower=0, adjacent=0, del_then_mis=0)
    first_flag = {}
    for r in rows:
        f = fields(r)
        if f[5] == b"*":
            out["star"] += 1
            continue
        nm, md, clamped = mm.tags(int(f[3]), f[5], f[9], T[f[2]])
        assert not clamped
        cols = ref_columns_of_d(f[5])
        out["d_over_64"] += 64 in cols
        out["d_over_128"] += 128 in cols
        out["n_in_md"] += b"N" in md
        out["minus_indel"] += bool(int(f[1]) & 16 and (b"I" in f[5] or b"D" in f[5]))
        out["run_1000"] += any(int(x) >= 1000 for x in re.findall(rb"\d+", md))
        out["multi"] += not f[-1].endswith(b"X0:i:1")
        out["lower"] += f[9] != f[9].upper()
        out["adjacent"] += re.search(rb"[A-Z]0[A-Z]", md) is not None
        out["del_then_mis"] += re.search(rb"\^[A-Z]+0[A-Z]", md) is not None
        out["other_strand"] += first_flag.setdefault(f[0], f[1]) != f[1]
    return out


# ---- 1. text ---------------------------------------------------------------------------------------------------------------------
def test_the_flag_off_rows_hold_the_shapes_the_walk_can_get_wrong(env):
    r = env["runs"]["main"]
    s = shapes(r.off_rows, env["T"])
    for k in ("d_over_64", "d_over_128", "n_in_md", "minus_indel", "run_1000", "multi", "other_strand", "lower", "adjacent", "del_then_mis"):
        assert s[k] >= 1, (k, s)
    assert s["star"] == 0                                         # see the module's docstring
    for tag in (b"p_hole_in", b"p_hole_out", b"p_hole_over"):     # both edges of the hole and the read that ends inside it, each on both strands
        for strand, flag in ((b"_f", 0), (b"_r", 16)):
            mine = [fields(x) for x in r.off_rows if fields(x)[0] == tag + strand]
            assert mine and all(int(f[1]) == flag for f in mine), (tag + strand, mine)
            assert all(b"N" in mm.tags(int(f[3]), f[5], f[9], env["T"][f[2]])[1] for f in mine), tag + strand
    lens = set(len(fields(x)[9]) for x in r.off_rows if x.startswith(b"p_"))
    assert {63, 64, 65, 100, 128, 129, 150, 1100} <= lens
    assert len(r.off_rows) > 256                                  # k_out_text_sizes: more than one workgroup


def test_text_rows_with_tags_equal_the_models(env):
    r = env["runs"]["main"]
    want = r.check_text(True, "gnumap")
    assert sum(b"\tMD:Z:" in x for x in want) == len(want)
    for x in want:                                                # the independent inverse, on the device's own strings
        f = fields(x)
        ref, n_mis, n_ins, n_del = mm.rebuild_reference(f[9], f[5], f[-1][5:])
        at = int(f[3]) - 1
        assert ref == env["T"][f[2]][at:at + len(ref)] and int(f[-2][5:]) == n_mis + n_ins + n_del


def test_forward_order_turns_the_minus_rows_round_and_nothing_else(env):
    r = env["runs"]["main"]
    want = r.check_text(False, "forward")
    changed = [k for k, (a, b) in enumerate(zip(r.off_rows, want)) if a != b]
    assert changed and all(int(fields(r.off_rows[k])[1]) & 16 for k in changed)
    want = r.check_text(True, "forward")
    indel = [fields(x) for x in want if int(fields(x)[1]) & 16 and (b"I" in fields(x)[5] or b"D" in fields(x)[5])]
    small = sum(int(f[-2][5:]) <= 5 for f in indel)
    model = sum(mm.tags(int(f[3]), f[5], f[9], env["T"][f[2]])[0] <= 5 for f in indel)
    assert small == model and len(indel) >= 4                     # (the planted minus-strand reads with an indel alone are four)
    # the planted minus-strand reads: under the printed order their edit distance is nonsense, under "forward" it is the plus twin's
    gn = {fields(x)[0]: int(fields(x)[-2][5:]) for x in r.want_rows(True, "gnumap") if x.startswith(b"p_del")}
    fw = {fields(x)[0]: int(fields(x)[-2][5:]) for x in want if x.startswith(b"p_del")}
    for tag in (b"p_del64", b"p_del128", b"p_delmis"):
        assert fw[tag + b"_r"] == fw[tag + b"_f"] == gn[tag + b"_f"] <= 5 < 20 <= gn[tag + b"_r"], (tag, fw, gn)


# ---- 2. BAM ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("md,order", [(True, "gnumap"), (False, "forward"), (True, "forward")])
def test_bam_records_are_the_flag_off_records_with_the_models_tag_bytes(env, level, md, order):
    r = env["runs"]["main"]
    off = r.bam(False, "gnumap", level)
    assert len(off) == len(r.off_rows)
    want = [mm.tag_record(rec, row, env["T"] if md else None, order == "forward") for rec, row in zip(off, r.off_rows)]
    got = r.bam(md, order, level)
    assert got == want
    if md:
        assert all(struct.unpack_from("<i", x, 0)[0] == len(x) - 4 and x.endswith(b"\0") and b"NMi" in x and b"MDZ" in x for x in got)

# ---- 3. the sorter and the index ---------------------------------------------------------------------------------------------------
def sorted_rows(rows, contigs):
    return [x.encode("latin-1") for x in ssm.sort_rows([x.decode("latin-1") for x in rows], [c for c, _ in contigs])]


def test_sorter_keeps_the_tags_on_text_rows(env):
    r = env["runs"]["main"]
    s = api.SamSorter(env["ix"], rows="text")
    r.set(True, "forward")
    try:
        s.add_block(r.batch, r.p, r.res, 0, names=r.names, qual_tails=None)
    finally:
        r.set(False, "gnumap")
    want = sorted_rows(r.want_rows(True, "forward"), env["contigs"])
    assert s.finish()[0] == len(want)
    assert s.text() == b"".join(want)
    s.destroy()


def test_sorter_keeps_the_tags_on_bam_rows_and_the_bai_reads_right(env):
    r = env["runs"]["main"]
    ix = env["ix"]
    s = api.SamSorter(ix, rows="bam")
    r.set(True, "forward")
    try:
        s.add_block(r.batch, r.p, r.res, 0, names=r.names, qual_tails=None)
    finally:
        r.set(False, "gnumap")
    want_rows = r.want_rows(True, "forward")
    order = sorted(range(len(want_rows)), key=lambda k: ssm.row_key(want_rows[k].decode("latin-1"), {c: i for i, (c, _) in enumerate(env["contigs"])}))
    recs = r.bam(True, "forward")
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
    assert [bytes(x) for x in sc["recs"]] == [recs[k] for k in order]
    got = s.bai()
    assert got == bai.build_bai(data)
    assert bai.check_queries(data, got, bai.regions_of(data, n_random=20)) > 100
    s.destroy()


# ---- 4. with the rows of reads that do not map -------------------------------------------------------------------------------------
def test_unmapped_rows_keep_their_bytes_and_mapped_rows_get_their_tags(env, texts):
    reads = env["sr"][300:380] + mf.rand_reads(11, 12, b"none") + env["planted"][:12]
    r = Run(env["ix"], env["p"], reads, texts)
    recs, _ = r.batch.output(r.p, r.res)
    quals = [x[2] for x in reads]
    r.batch.set_unmapped_rows(True)
    try:
        on_text, on_off = r.text(False, "gnumap")
        merged, new = um.merge(r.off_rows, recs["read"], r.names, r.seqs, quals, r.res["status"])
        assert split(on_text, on_off) == merged and sum(new) >= 12
        text, row_off = r.text(True, "forward")
        want = [x if n else mm.insert_tags(mm.forward_row(x), texts) for x, n in zip(merged, new)]
        assert split(text, row_off) == want
        assert all(b"MD:Z" not in x for x, n in zip(want, new) if n) and all(b"MD:Z" in x for x, n in zip(want, new) if not n)
        off_recs = r.bam(False, "gnumap")
        got = r.bam(True, "forward")
        assert got == [rec if n else mm.tag_record(rec, row, texts, True) for rec, row, n in zip(off_recs, merged, new)]
    finally:
        r.batch.set_unmapped_rows(False)
        r.destroy()


# ---- 5. several trips per workgroup ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 2])
def test_grid_cap_gives_the_same_bytes(env, cap):
    r = env["runs"]["main"]
    want = r.want_rows(True, "forward")
    bam = r.bam(True, "forward")
    assert len(want) > 4 * cap * 8                                # k_md_sizes, k_out_text_rows, k_bam_rows: at least 8 trips per workgroup
    g.set_option("GM_TEST_GRID_CAP", cap)
    try:
        text, row_off = r.text(True, "forward")
        capped = r.bam(True, "forward")
    finally:
        g.set_option("GM_TEST_GRID_CAP", None)
    assert split(text, row_off) == want and capped == bam


# ---- 6. the settings off: the bytes of a batch that never heard of them -------------------------------------------------------------
def test_toggling_on_and_off_leaves_the_flag_off_bytes(env, texts):
    reads = env["sr"][380:460] + env["planted"][12:20]
    r = Run(env["ix"], env["p"], reads, texts)               # (its off_text was taken before any setter was called with a value but the default)
    fresh = g.Batch(env["ix"], len(reads), r.batch._keep[0].shape[1])
    res = fresh.map(env["p"], *r.batch._keep)
    never_text, never_off = fresh.output_text(env["p"], res, r.names, None)
    never_bam = fresh.output_bam(env["p"], res, r.names, None, level=1)
    assert never_text == r.off_text
    before_bam = r.batch.output_bam(r.p, r.res, r.names, None, level=1)
    assert before_bam == never_bam
    r.check_text(True, "forward")
    text, row_off = r.text(False, "gnumap")
    assert text == never_text and np.array_equal(row_off, never_off)
    assert r.batch.output_bam(r.p, r.res, r.names, None, level=1) == never_bam
    for rows in ("text", "bam"):
        a, b = api.SamSorter(env["ix"], rows=rows), api.SamSorter(env["ix"], rows=rows)
        a.add_block(r.batch, r.p, r.res, 0, names=r.names, qual_tails=None)
        b.add_block(fresh, env["p"], res, 0, names=r.names, qual_tails=None)
        assert a.finish() == b.finish()
        if rows == "text":
            assert a.text() == b.text()
        else:
            assert a.read_bgzf(1 << 20, level=0) == b.read_bgzf(1 << 20, level=0)
        a.destroy(); b.destroy()
    assert r.batch.kernel_times().get("k_md_sizes") is not None
    fresh.destroy(); r.destroy()


def test_k_md_sizes_is_timed_only_with_the_setting_on(env):
    r = env["runs"]["main"]
    r.batch.set_profiling(True)
    try:
        r.batch.kernel_times()
        r.text(False, "forward")
        assert r.batch.kernel_times()["k_md_sizes"][1] == 0       # no launch with the tags off
        r.text(True, "gnumap")
        ms, launches = r.batch.kernel_times()["k_md_sizes"]
        assert launches == 1 and ms > 0
    finally:
        r.batch.set_profiling(False)


# ---- other block kinds ---------------------------------------------------------------------------------------------------------------
def test_fasta_block_with_iupac_letters(env, texts):
    reads = [(n, s, b"") for n, s, _ in env["sr"][:100] + env["planted"][:26]]
    k = next(i for i, x in enumerate(reads) if len(x[1]) == 100)
    reads[k] = (reads[k][0], reads[k][1][:40] + b"RYKMN" + reads[k][1][45:], b"")
    r = Run(env["ix"], g.Params(), reads, texts, fasta=True)
    assert any(re.search(rb"[RYKM]", fields(x)[9]) for x in r.off_rows)
    r.check_text(True, "gnumap"); r.check_text(True, "forward")
    off = r.bam(False, "gnumap")
    assert r.bam(True, "forward") == [mm.tag_record(rec, row, texts, True) for rec, row in zip(off, r.off_rows)]
    r.destroy()


@pytest.mark.parametrize("kw", [dict(max_matches=2), dict(nw=0), dict(mode=1), dict(print_all_sam=1)], ids=["T2", "no_nw", "b", "print_all_sam"])
def test_other_parameters(env, texts, kw):
    reads = env["sr"][:160] + env["planted"][:30]
    r = Run(env["ix"], g.Params(**kw), reads, texts)
    assert len(r.off_rows) >= 64
    if "max_matches" in kw:
        assert shapes(r.off_rows, texts)["multi"] >= 1            # reads with two places keep both rows under -T 2
    r.check_text(True, "gnumap"); r.check_text(True, "forward")
    off = r.bam(False, "gnumap")
    assert r.bam(True, "gnumap") == [mm.tag_record(rec, row, texts, False) for rec, row in zip(off, r.off_rows)]
    r.destroy()


# ---- 7. the driver -------------------------------------------------------------------------------------------------------------------
def drive(fa, fq, out, extra):
    r = subprocess.run([EXE, "-g", fa, "-o", out] + extra + [fq], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def rows_of(path):
    return [l for l in open(path, "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]


def test_cli_sam_md_is_the_reference_run_plus_the_two_tags(syn_fa, syn_fq, texts, tmp_path):
    import gzip
    out = str(tmp_path / "o")
    drive(syn_fa, syn_fq, out, ["--sam_md"])
    rows = rows_of(out + ".sam")
    golden = [l for l in gzip.open(os.path.join(GOLDEN, "ref_runs", "default.sam.gz"), "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]
    assert [mm.strip_tags(x) for x in rows] == golden
    assert rows == [mm.insert_tags(x, texts) for x in golden]
    drive(syn_fa, syn_fq, out + "_s", ["--sam_md", "--sam_cigar=forward", "--sam_shards=3", "--chunk_reads=97", "--workers=3"])
    shards = [rows_of(f"{out}_s.{k}.sam") for k in range(3)]
    assert sum(bool(s) for s in shards) >= 2
    assert shards[0] + shards[1] + shards[2] == [mm.insert_tags(mm.forward_row(x), texts) for x in golden]


def test_cli_archive_run_writes_a_tagged_sorted_bam_and_its_index(syn_fa, syn_fq, texts, tmp_path):
    import gzip
    out = str(tmp_path / "o")
    drive(syn_fa, syn_fq, out, ["--sam_md", "--sam_cigar=forward", "--sam_unmapped", "--sam_format=bam", "--sam_sort=coordinate", "--bam_index"])
    data, index = open(out + ".bam", "rb").read(), open(out + ".bam.bai", "rb").read()
    sc = bai.scan(data)
    recs = [bytes(x) for x in sc["recs"]]
    mapped = [x for x in recs if not um.record_is_unmapped(x)]
    golden = [l for l in gzip.open(os.path.join(GOLDEN, "ref_runs", "default.sam.gz"), "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]
    assert len(mapped) == len(golden) and len(recs) > len(mapped)
    assert all(b"NMi" in x and b"MDZ" in x for x in mapped) and all(um.record_is_unmapped(x) and x[-7:-4] == b"YUi" for x in recs[len(mapped):])
    want = sorted(mm.bam_tag_bytes(*mm.tags(int(f[3]), f[5], f[9], texts[f[2]])[:2]) for f in (fields(mm.forward_row(x)) for x in golden))
    assert sorted(x[x.rindex(b"NMi"):] for x in mapped) == want
    assert index == bai.build_bai(data)
    assert bai.check_queries(data, index, bai.regions_of(data, n_random=20)) > 100


# ---- 8. refusals at the ABI ----------------------------------------------------------------------------------------------------------
def test_refusals_at_the_abi(env, tmp_path):
    import shutil
    b = g.Batch(env["ix"], 64, 100)
    L = g.lib()
    assert L.gm_batch_set_row_tags(b.h, 2) == GM_E_ARG and L.gm_batch_set_row_tags(b.h, 3) == GM_E_ARG
    assert L.gm_batch_set_cigar_order(b.h, 2) == GM_E_ARG and L.gm_batch_set_cigar_order(b.h, -1) == GM_E_ARG
    assert L.gm_batch_set_row_tags(None, 1) == GM_E_ARG and L.gm_batch_set_cigar_order(None, 1) == GM_E_ARG
    b.set_adaptor(b"ACGTACGTAC")
    assert L.gm_batch_set_row_tags(b.h, 1) == GM_E_UNSUPPORTED
    msg = L.gm_last_error().decode()
    assert "GM_ROW_TAG_MD" in msg and "adaptor" in msg
    b.set_adaptor(None)
    b.set_row_tags(True)
    assert L.gm_batch_set_adaptor(b.h, b"ACGTACGTAC") == GM_E_UNSUPPORTED
    b.set_row_tags(False)
    b.set_adaptor(b"ACGTACGTAC"); b.set_adaptor(None)
    with pytest.raises(ValueError):
        b.set_cigar_order("backward")
    b.destroy()
    # an index without its .amb
    d = tmp_path / "noamb"
    d.mkdir()
    for f in os.listdir(GOLDEN):
        if f.startswith("syn.fa") and not f.endswith(".amb"):
            shutil.copy(os.path.join(GOLDEN, f), d / f)
    ix = g.Index(str(d / "syn.fa"), device=0, flags=g.GM_INDEX_FULL_SA)
    b = g.Batch(ix, 64, 100)
    assert L.gm_batch_set_row_tags(b.h, 1) == GM_E_IO and "syn.fa.gnumap.amb" in L.gm_last_error().decode()
    b.set_cigar_order("forward")                                  # needs no .amb
    b.destroy(); ix.close()
