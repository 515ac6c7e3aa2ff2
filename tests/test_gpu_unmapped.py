"""Rows for the reads that do not map: gm_batch_set_unmapped_rows through every row-producing sink, and --sam_unmapped.

The reference program prints no such row, so it cannot be the yardstick.  The yardstick is the project's own flag-off output (pinned
byte for byte to the reference elsewhere) and tests/unmapped_model.py: the rows with the setting on are the flag-off rows, untouched,
merged by read index (recs[].read of Batch.output on the same hits) with one row the model formats for every read that has none.
Every comparison is of bytes, for equality.

Blocks are built from golden/syn.fa and syn.fq plus planted reads - seeded random 100-mers, a read shorter than the mer, a read of
all-'!' qualities under -q, -T 2 for the reads with more than two places - and hold 64 to 400 reads.  A read of length 0 can be
uploaded (gm_batch_upload takes it; its status is GM_READ_TOO_SHORT), so the case is kept."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
import bai_model as bai
import bam_model as bm
import fasta_model as fm
import repeat_fixture as rf
import unmapped_model as um
from conftest import ROOT
from gnumap_amd import api
from test_gpu_sam_text import same_track

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
KW = dict(max_matches=2, cutoff=15.0)               # -T 2 -q 15
ARGV = ["-a", "0.9", "-T", "2", "-q", "15"]
NONE, TOO_MANY, TOO_SHORT, TOO_POOR = 2, 1, -2, -3


def rand_reads(rng, n, tag, L=100):
    return [(b"%s%d" % (tag, i), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)), b"I" * L) for i in range(n)]


def syn(reads):
    return [(nm.encode(), s, q) for nm, s, q in reads]


class Block:
    """reads as (name, sequence, whole quality line); quality lines may be longer than their sequences"""

    def __init__(self, reads, fasta=False):
        self.names = [r[0] for r in reads]; self.seqs = [r[1] for r in reads]
        self.quals = [fm.synth_qual(r[1]) for r in reads] if fasta else [r[2] for r in reads]
        self.fasta = fasta
        tails = [q[len(s):] for s, q in zip(self.seqs, self.quals)]
        self.tails = tails if any(tails) and not fasta else None
        self.n = len(reads)

    def text(self):
        return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(self.names, self.seqs, self.quals))


def split(text, row_off):
    assert int(row_off[0]) == 0 and int(row_off[-1]) == len(text)
    return [text[int(row_off[k]):int(row_off[k + 1])] for k in range(len(row_off) - 1)]


class Run:
    """a block mapped once; the flag-off rows, the model's rows, and the rows with the setting on"""

    def __init__(self, ix, p, blk, adaptor=None):
        self.ix, self.p, self.blk = ix, p, blk
        B, Q, Ln = g.pack_reads(blk.seqs, None if blk.fasta else [q[:len(s)] for s, q in zip(blk.seqs, blk.quals)])
        self.batch = g.Batch(ix, blk.n, B.shape[1])
        self.batch.set_adaptor(adaptor)
        self.res = self.batch.map(p, B, Q, Ln, fasta=blk.fasta)
        self.status = self.res["status"].copy()
        self.off_text, off_rowoff = self.text(False)
        self.off_rows = split(self.off_text, off_rowoff)
        recs, _ = self.batch.output(p, self.res)
        assert len(recs) == len(self.off_rows)
        self.want, self.new = um.merge(self.off_rows, recs["read"], blk.names, blk.seqs, blk.quals, self.status)
        has_rows = set(int(x) for x in recs["read"])
        self.read_new = [i not in has_rows for i in range(blk.n)]      # per read: True when the model made its row
        self.n_new = sum(self.new)
        self.on_text, self.on_rowoff = self.text(True)

    def text(self, on, **kw):
        self.batch.set_unmapped_rows(on)
        return self.batch.output_text(self.p, self.res, self.blk.names, self.blk.tails, **kw)

    def bam(self, on, level=1):
        self.batch.set_unmapped_rows(on)
        return self.batch.output_bam(self.p, self.res, self.blk.names, self.blk.tails, level=level)

    def check_text(self):
        assert self.on_text == b"".join(self.want)
        assert [int(x) for x in self.on_rowoff] == [0] + list(np.cumsum([len(r) for r in self.want]))
        assert self.batch.unmapped_rows() == self.n_new

    def destroy(self):
        self.batch.destroy()


@pytest.fixture(scope="module")
def env(syn_fa, syn_reads):
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params(**KW)
    rng = np.random.default_rng(4)
    sr = syn(syn_reads)
    planted = rand_reads(rng, 40, b"none")
    mixed = []
    for k in range(260):                                          # a planted read behind every sixth read of syn.fq, one with a quality tail
        mixed.append(sr[k])
        if k % 6 == 2 and k // 6 < len(planted):
            nm, s, q = planted[k // 6]
            mixed.append((nm, s, q + (b"#tail" if k // 6 == 3 else b"")))
    mixed.insert(17, (b"short", b"ACGTA", b"IIIII"))
    good = next(r for r in sr if len(r[1]) == 100)
    mixed.insert(101, (b"poor", good[1], b"!" * 100))
    assert 64 <= len(mixed) <= 400 and len(set(r[0] for r in mixed)) == len(mixed)
    runs = {"mixed": Run(ix, p, Block(mixed))}
    yield dict(ix=ix, p=p, rng=rng, sr=sr, runs=runs, contigs=ix.contigs())
    for r in runs.values():
        r.destroy()
    ix.close()


# ---- 1. text against the model ---------------------------------------------------------------------------------------------------
def test_mixed_block_text_and_the_statuses_it_holds(env):
    r = env["runs"]["mixed"]
    st = [int(s) for s, new in zip(r.status, r.read_new) if new]
    for code in (NONE, TOO_SHORT, TOO_POOR, TOO_MANY):
        assert code in st, (code, sorted(set(st)))               # from hits.status, not assumed
    assert r.n_new >= 40 and len(r.off_rows) > 150
    assert len(r.want) > 256 and len(r.want) % 256 != 0           # the last workgroup of k_out_text_sizes is partial
    r.check_text()
    assert any(b"#tail\tYU:i:2\n" in row for row in r.want)       # the quality tail of a read without a record


def test_block_of_unmapped_reads_only(env):
    r = Run(env["ix"], env["p"], Block(rand_reads(np.random.default_rng(5), 64, b"u")))
    assert r.off_text == b"" and r.n_new == 64 and all(int(s) == NONE for s in r.status)       # the former early return
    r.check_text()
    assert r.on_text.count(b"\n") == 64
    r.destroy()


def test_block_in_which_every_read_maps(env):
    m = env["runs"]["mixed"]
    keep = [i for i, new in enumerate(m.read_new) if not new][:150]
    r = Run(env["ix"], env["p"], Block([(m.blk.names[i], m.blk.seqs[i], m.blk.quals[i]) for i in keep]))
    assert len(keep) >= 64 and r.n_new == 0 and len(r.off_rows) >= len(keep)
    r.check_text()
    assert r.on_text == r.off_text and r.batch.unmapped_rows() == 0
    r.destroy()


def test_first_and_last_reads_unmapped_and_a_run_of_nine(env):
    rng = np.random.default_rng(6)
    reads = rand_reads(rng, 9, b"head") + env["sr"][300:360] + rand_reads(rng, 1, b"last")
    r = Run(env["ix"], env["p"], Block(reads))
    assert all(r.new[:9]) and r.new[-1] and not all(r.new)
    r.check_text()
    r.destroy()


def test_reads_of_the_repeat_fixture_under_a_small_T(tmp_path_factory):
    fa = rf.build_index(tmp_path_factory)
    ix = g.Index(fa, device=0, flags=g.GM_INDEX_FULL_SA)
    rd = [r for r in syn(rf.reads()) if len(r[1]) <= 152][100:]       # the t_ family: more than three keys from 63 bases on
    assert 64 <= len(rd) <= 400
    r = Run(ix, g.Params(max_matches=3), Block(rd))
    assert TOO_MANY in [int(s) for s, new in zip(r.status, r.read_new) if new] and not all(r.read_new)
    r.check_text()
    r.destroy(); ix.close()


# ---- 2. several trips per workgroup ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 2])
def test_grid_cap_gives_the_same_bytes(env, cap):
    r = env["runs"]["mixed"]
    bam = r.bam(True)
    g.set_option("GM_TEST_GRID_CAP", cap)
    try:
        text, row_off = r.text(True)
        bam_capped = r.bam(True)
    finally:
        g.set_option("GM_TEST_GRID_CAP", None)
    assert text == r.on_text == b"".join(r.want) and np.array_equal(row_off, r.on_rowoff)
    assert bam_capped == bam and r.batch.bam_n_recs == len(r.want)


# ---- 3. unusual fields -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields(env):
    rng = np.random.default_rng(7)
    rd = rand_reads(rng, 6, b"f")
    reads = [(b"", rd[0][1], rd[0][2]), (b"a" * 1023, rd[1][1], rd[1][2]), (b"b" * 1024, rd[2][1], rd[2][2]), (b"c" * 1500, rd[3][1], rd[3][2] + b"#longtail"),
             (b"empty", b"", b"")] + env["sr"][400:460] + [(b"d" * 255, rd[4][1], rd[4][2])]
    r = Run(env["ix"], env["p"], Block(reads))
    yield r
    r.destroy()


def test_names_of_0_1023_1024_1500_bytes_a_quality_tail_and_a_read_of_length_0(fields):
    r = fields
    assert all(r.new[:5]) and r.new[-1] and int(r.status[4]) == TOO_SHORT
    r.check_text()
    rows = [x.split(b"\t") for x in split(r.on_text, r.on_rowoff)]
    assert [len(x[0]) for x in rows[:5]] == [0, 1023, 1023, 1023, 5]
    assert rows[3][10].endswith(b"#longtail") and len(rows[3][10]) == 109 and len(rows[3][9]) == 100
    assert rows[4][9:] == [b"*", b"*", b"YU:i:-2\n"]


@pytest.mark.parametrize("level", [0, 1])
def test_bam_records_of_the_unusual_fields(fields, env, level):
    r = fields
    got = bm.split_records(bm.bgzf_payload(r.bam(True, level)))
    want = um.to_records(r.want, env["contigs"])
    assert um.records_differ(got, want) is None, um.records_differ(got, want)
    assert [um.fixed_fields(x)[2] for x in got[:5]] == [1, 255, 255, 255, 6] and um.fixed_fields(got[-1])[2] == 255
    assert um.fixed_fields(got[4]) == (-1, -1, 6, 0, 4680, 0, 4, 0, -1, -1, 0)


# ---- 4. the resident form ---------------------------------------------------------------------------------------------------------
def test_resident_form_gives_the_bytes_of_the_host_rows_form(env):
    r = env["runs"]["mixed"]
    batch = g.Batch(env["ix"], 4096, 2048)
    info = batch.upload_text(env["p"], r.blk.text())
    assert info["n"] == r.blk.n
    res = batch.map_text(env["p"])
    off, _ = batch.output_text_resident(env["p"], res)
    batch.set_unmapped_rows(True)
    on, row_off = batch.output_text_resident(env["p"], res)
    assert off == r.off_text and on == r.on_text and np.array_equal(row_off, r.on_rowoff) and batch.unmapped_rows() == r.n_new
    bam = bm.split_records(bm.bgzf_payload(batch.output_bam_resident(env["p"], res)))
    assert um.records_differ(bam, um.to_records(r.want, env["contigs"])) is None
    batch.destroy()


# ---- 5. other block kinds ----------------------------------------------------------------------------------------------------------
def test_fasta_block(env):
    m = env["runs"]["mixed"].blk
    reads = [(n, s, b"") for n, s in zip(m.names, m.seqs)][:150]
    reads[3] = (reads[3][0], reads[3][1][:40] + b"RYKMN" + reads[3][1][45:], b"")
    r = Run(env["ix"], g.Params(max_matches=2), Block(reads, fasta=True))
    assert 5 <= r.n_new < 150
    r.check_text()
    r.destroy()


def test_block_with_an_adaptor_keeps_seq_and_qual_whole(env):
    m = env["runs"]["mixed"].blk
    reads = [x for x in zip(m.names, m.seqs, m.quals) if len(x[1]) >= 36][:150]
    r = Run(env["ix"], env["p"], Block(reads), adaptor=b"ACGTTGCAAC")
    kept = r.batch.trimmed_len()
    cut = [i for i, new in enumerate(r.read_new) if new and int(kept[i]) < len(reads[i][1])]
    assert len(cut) >= 5                                          # reads without a record that the trim shortened: their rows print the whole line
    r.check_text()
    r.destroy()


def test_print_all_sam(env):
    m = env["runs"]["mixed"].blk
    r = Run(env["ix"], g.Params(print_all_sam=1, **KW), Block(list(zip(m.names, m.seqs, m.quals))))
    assert len(r.off_rows) >= len(env["runs"]["mixed"].off_rows) and r.n_new >= 40
    r.check_text()
    r.destroy()


# ---- 6. capacity -------------------------------------------------------------------------------------------------------------------
def test_capacity_one_byte_short_reports_the_size_with_the_unmapped_rows_and_deposits_once(env):
    ix, p, r = env["ix"], env["p"], env["runs"]["mixed"]
    B, Q, Ln = r.batch._keep
    ix.coverage_reset(8)
    r.batch.set_unmapped_rows(False)
    r.batch.output_text(p, r.batch.map(p, B, Q, Ln), r.blk.names, r.blk.tails)
    cov_off = ix.coverage_download()
    ix.coverage_reset(8)
    res = r.batch.map(p, B, Q, Ln)
    r.batch.set_unmapped_rows(True)
    need = len(b"".join(r.want))
    rt, keep = api._pack_read_text(r.blk.names, r.blk.tails, r.blk.n)
    buf = np.full(need + 16, 0xAA, np.uint8)
    st = api.gm_sam_text(); st.text = buf.ctypes.data; st.text_cap = need - 1
    rc = g.lib().gm_output_batch_text(ix.h, C.byref(p.c), r.batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(st), None)
    assert rc == api.GM_E_CAPACITY and st.text_cap == st.text_len == need and st.n_recs == len(r.want)
    assert float(ix.coverage_download().sum()) == 0.0 and (buf == 0xAA).all()      # nothing deposited, nothing written
    st.text_cap = need
    rc = g.lib().gm_output_batch_text(ix.h, C.byref(p.c), r.batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(st), None)
    assert rc == 0 and bytes(buf[:need]) == b"".join(r.want) and (buf[need:] == 0xAA).all()
    same_track(ix.coverage_download(), cov_off)                   # a read without a record deposits nothing; the others once
    assert r.batch.unmapped_rows() == r.n_new
    del keep
    r.res = res


# ---- 7. BAM ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
def test_bam_records_equal_the_models(env, level):
    r = env["runs"]["mixed"]
    out = r.bam(True, level)
    got = bm.split_records(bm.bgzf_payload(out))
    want = um.to_records(r.want, env["contigs"])
    assert r.batch.bam_n_recs == len(want) and r.batch.unmapped_rows() == r.n_new
    assert um.records_differ(got, want) is None, um.records_differ(got, want)
    for rec, new in zip(got, r.new):
        assert um.record_is_unmapped(rec) == new
        if new:
            f = um.fixed_fields(rec)
            assert f[:2] == (-1, -1) and f[3:7] == (0, 4680, 0, 4) and f[8:] == (-1, -1, 0) and rec[-7:-4] == b"YUi"
    off = bm.split_records(bm.bgzf_payload(r.bam(False, level)))
    assert off == [rec for rec, new in zip(got, r.new) if not new]             # the other records keep their bytes


# ---- 8. / 9. the sorter and the .bai ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def second(env):
    rng = np.random.default_rng(8)
    reads = rand_reads(rng, 3, b"z") + env["sr"][460:540] + rand_reads(rng, 4, b"y")
    r = Run(env["ix"], env["p"], Block(reads))
    yield r
    r.destroy()


def add_both(env, second, rows):
    a, b = env["runs"]["mixed"], second
    s = api.SamSorter(env["ix"], rows=rows)
    for r, seq in ((b, 20), (a, 10)):                             # descending sequence numbers
        r.batch.set_unmapped_rows(True)
        s.add_block(r.batch, r.p, r.res, seq, names=r.blk.names, qual_tails=r.blk.tails)
    names = [c for c, _ in env["contigs"]]
    want = um.sort_rows(a.want + b.want, names)
    assert s.finish()[0] == len(want)
    tail = [x for x, new in zip(a.want + b.want, a.new + b.new) if new]
    assert want[-len(tail):] == tail                              # the rows without a contig last, in input order across the blocks
    return s, want


def test_sorter_with_text_rows(env, second):
    s, want = add_both(env, second, "text")
    assert s.text() == b"".join(want)
    s.destroy()


@pytest.mark.parametrize("level", [0, 1])
def test_sorter_with_bam_rows_and_the_index(env, second, level):
    s, want = add_both(env, second, "bam")
    ix = env["ix"]
    head = ix.bgzf_compress(ix.bam_header(b"@HD\tVN:1.0\tSO:coordinate\n"), level=level)
    s.index_begin(len(head))
    slabs = []
    while True:
        t = s.read_bgzf(60000, level=level)
        if not t:
            break
        slabs.append(t)
    assert len(slabs) >= 2
    data = head + b"".join(slabs) + api.bgzf_eof()
    sc = bai.scan(data)
    want_recs = um.to_records(want, env["contigs"])
    assert um.records_differ([bytes(x) for x in sc["recs"]], want_recs) is None
    got = s.bai()
    assert got == bai.build_bai(data)
    parsed = bai.parse_bai(got)
    n_new = env["runs"]["mixed"].n_new + second.n_new
    assert parsed["n_no_coor"] == n_new == int((sc["ref"] < 0).sum())
    assert bai.check_queries(data, got, bai.regions_of(data, n_random=20)) > 100
    for ref in range(len(env["contigs"])):                        # a region query over a whole contig reaches no record without a position
        hit = bai.records_in_chunks(data, bai.query(parsed, ref, 0, bai.MAX_END))
        assert all(sc["ref"][k] == ref for k in hit)
    s.destroy()


# ---- 10. the setter and the records form -----------------------------------------------------------------------------------------
def test_setter_off_again_and_the_records_form(env):
    r = env["runs"]["mixed"]
    r.batch.set_unmapped_rows(False)
    recs_off, cig_off = r.batch.output(r.p, r.res)
    r.batch.set_unmapped_rows(True)
    recs_on, cig_on = r.batch.output(r.p, r.res)
    assert recs_on.tobytes() == recs_off.tobytes() and cig_on == cig_off      # gm_output_batch does not read the setting
    text, row_off = r.text(True)
    assert text == r.on_text
    text, row_off = r.text(False)
    assert text == r.off_text and len(row_off) == len(r.off_rows) + 1 and r.batch.unmapped_rows() == 0
    assert bm.split_records(bm.bgzf_payload(r.bam(False))) == um_off_records(r)


def um_off_records(r):
    on = bm.split_records(bm.bgzf_payload(r.bam(True)))
    return [rec for rec, new in zip(on, r.new) if not new]


# ---- 11. the driver ----------------------------------------------------------------------------------------------------------------
def drive(fa, fq, out, extra):
    r = subprocess.run([EXE, "-g", fa, "-o", out] + ARGV + extra + [fq], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def rows_of(path):
    return [l for l in open(path, "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]


@pytest.fixture(scope="module")
def fq(env, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("unmapped") / "mixed.fq")
    with open(path, "wb") as f:
        f.write(env["runs"]["mixed"].blk.text())
    return path


@pytest.mark.parametrize("extra", [[], ["--read_text=device"], ["--chunk_reads=37", "--workers=3"]], ids=["default", "read_text_device", "small_blocks"])
def test_cli_sam_unmapped_equals_the_model(env, fq, syn_fa, extra, tmp_path):
    r = env["runs"]["mixed"]
    out = str(tmp_path / "o")
    res = drive(syn_fa, fq, out, ["--sam_unmapped"] + extra)
    assert rows_of(out + ".sam") == r.want
    assert f"--sam_unmapped: {r.n_new} of the {len(r.want)} SAM records" in res.stderr
    if not extra:
        drive(syn_fa, fq, out + "_off", ["--sam_text=device"])
        assert rows_of(out + "_off.sam") == r.off_rows             # without the flag: the rows the model started from


def test_cli_shards_concatenate_to_the_model(env, fq, syn_fa, tmp_path):
    out = str(tmp_path / "o")
    drive(syn_fa, fq, out, ["--sam_unmapped", "--sam_shards=3", "--chunk_reads=37", "--workers=3"])
    shards = [rows_of(f"{out}.{k}.sam") for k in range(3)]
    assert sum(bool(s) for s in shards) >= 2
    assert shards[0] + shards[1] + shards[2] == env["runs"]["mixed"].want


def test_cli_sorted_bam_with_its_index(env, fq, syn_fa, tmp_path):
    r = env["runs"]["mixed"]
    out = str(tmp_path / "o")
    flags = ["--sam_unmapped", "--sam_format=bam", "--sam_sort=coordinate", "--chunk_reads=64", "--workers=3"]
    drive(syn_fa, fq, out, flags)
    before = open(out + ".bam", "rb").read()
    os.remove(out + ".bam")
    drive(syn_fa, fq, out, flags + ["--bam_index"])
    data, index = open(out + ".bam", "rb").read(), open(out + ".bam.bai", "rb").read()
    assert data == before                                         # <out>.bam is written exactly as without --bam_index
    sc = bai.scan(data)
    want = um.to_records(um.sort_rows(r.want, [c for c, _ in env["contigs"]]), env["contigs"])
    assert um.records_differ([bytes(x) for x in sc["recs"]], want) is None
    assert index == bai.build_bai(data)
    parsed = bai.parse_bai(index)
    assert parsed["n_no_coor"] == r.n_new
    assert bai.check_queries(data, index, bai.regions_of(data, n_random=20)) > 100
    for ref in range(len(env["contigs"])):
        assert all(sc["ref"][k] == ref for k in bai.records_in_chunks(data, bai.query(parsed, ref, 0, bai.MAX_END)))
