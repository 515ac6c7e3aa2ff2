"""--sam_sort=coordinate: the rows kept in HBM, sorted there and gathered in key order (gm_samsort.hip), against tests/sam_sort_model.py.

* the driver: one run with the default options, one with --sam_sort=coordinate in many small blocks that three workers finish out of
  order; the sorted file is the model applied to the unsorted one, byte for byte (the @PG line aside: it quotes the command line),
  the tracks are equal within the fp32 atomic order (test_gpu_driver_golden.compare_tracks).  On the edge genome (three contigs, the
  second without a read; reads at position 1 and ending at the last base of a contig; one read four times, far apart in the file;
  38 unmappable reads), with --read_text=device, with --print_all_sam on the repeat genome, and with FASTA reads;
* the ABI through gnumap_amd.api.SamSorter with GM_SORT_PIECE=65536: blocks added in reverse sequence order, a row longer than 4 KB,
  slabs of 4096 bytes and of one row, GM_E_CAPACITY one byte short of a row, the empty sorter, a sequence number used twice, an add
  after finish, and a block in which no read maps.

A read that does not map has no row in this implementation's SAM (nor in the reference program's, whose files the suite pins): the
`key = ~0` of such rows is the library's rule for a record without a contig, which no block of these tests can produce; what is checked
is that blocks and reads without rows leave the order of the others alone."""
import os
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
import edge_fixture as ef
import repeat_fixture as rf
from conftest import GOLDEN, ROOT
from gnumap_amd import api
from reflib import revcomp_str
from sam_sort_model import HD, sam_sort_model, sort_rows
from test_gpu_driver_golden import compare_tracks

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
L = 50
SORTED = ["--sam_sort=coordinate", "--chunk_reads=64", "--workers=3"]


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def contigs_of(fa):
    out = []
    for l in open(fa, "rb"):
        if l.startswith(b">"):
            out.append([l[1:].strip().decode(), b""])
        else:
            out[-1][1] += l.strip().upper()
    return out


def make_reads(ctg, skip=1, n=2000, seed=77):
    """n reads of L bases from every contig but `skip`, alternating strands; every 53rd a random sequence (unmappable); reads at position 1
    and ending at the last base of each contig on both strands; one read four times, far apart.  Names say where a read came from."""
    rng = np.random.default_rng(seed)
    use = [i for i in range(len(ctg)) if i != skip]

    def read_at(c, p, strand, tag):
        s = ctg[c][1][p:p + L]
        q = bytes((33 + rng.integers(20, 41, L)).astype(np.uint8))
        if strand:
            s = revcomp_str(s).upper()
        if isinstance(s, str):
            s = s.encode()
        return (f"{tag}_{ctg[c][0]}_{p + 1}_{'fr'[strand]}", s, q)

    reads = []
    for k in range(n):
        if k % 53 == 7:
            reads.append((f"u{k}", bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)), b"I" * L))
            continue
        c = use[int(rng.integers(0, len(use)))]
        reads.append(read_at(c, int(rng.integers(0, len(ctg[c][1]) - L + 1)), k & 1, f"r{k}"))
    at = iter([40, 41, 900, 901, 1700, 1701, 1990, 1991])
    for c in use:
        for p in (0, len(ctg[c][1]) - L):
            for st in (0, 1):
                k = next(at)
                reads[k] = read_at(c, p, st, f"e{k}")
    d = read_at(use[0], 1234, 0, "dup")
    for j, k in enumerate((10, 650, 1300, 1950)):
        reads[k] = (f"dup{j}_{d[0]}", d[1], d[2])
    return reads


@pytest.fixture(scope="module")
def edge_run(tmp_path_factory):
    """(genome path, FASTQ path, contigs, reads, the unsorted run's output prefix): the default run is shared by the cases below"""
    fa = ef.build_index(tmp_path_factory)
    ctg = contigs_of(fa)
    assert [len(s) for _, s in ctg] == [5003, 3001, 2003]
    rd = make_reads(ctg)
    fq = os.path.join(os.path.dirname(fa), "sort.fq")
    with open(fq, "wb") as f:
        for name, s, q in rd:
            f.write(b"@" + name.encode() + b"\n" + s + b"\n+\n" + q + b"\n")
    out = os.path.join(os.path.dirname(fa), "unsorted")
    drive(fa, fq, out, [])
    return fa, fq, ctg, rd, out


def drive(fa, fq, out, extra, env=None):
    r = subprocess.run([EXE, "-g", fa, "-o", out, "-a", "0.9"] + extra + [fq], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def no_pg(text):
    return b"".join(l for l in text.splitlines(keepends=True) if not l.startswith(b"@PG"))


def assert_sorted_equals_model(sorted_path, unsorted_path, n_seqs):
    mine, plain = open(sorted_path, "rb").read(), open(unsorted_path, "rb").read()
    lines = mine.splitlines(keepends=True)
    assert lines[0] == HD.encode() and all(l.startswith(b"@SQ") for l in lines[1:1 + n_seqs]) and lines[1 + n_seqs].startswith(b"@PG") and b"--sam_sort=coordinate" in lines[1 + n_seqs]
    assert not plain.startswith(b"@HD")                                       # the default run's bytes are the parent's: no @HD line
    want = no_pg(sam_sort_model(plain))
    got = no_pg(mine)
    if got != want:
        a, b = got.splitlines(), want.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"{len(a)} vs {len(b)} lines, first difference at line {first}:\n  mine  {a[first] if first < len(a) else None}\n  model {b[first] if first < len(b) else None}")
    return [l.split(b"\t") for l in got.splitlines() if not l.startswith(b"@")]


def test_fixture_holds_what_the_sort_has_to_get_right(edge_run):
    """read from the UNSORTED run, so that equality with the model below means something"""
    fa, fq, ctg, rd, out = edge_run
    rows = [l.split("\t") for l in open(out + ".sam") if not l.startswith("@")]
    by_contig = {c: [r for r in rows if r[2] == c] for c, _ in ctg}
    assert len(rows) > 1900 and len(by_contig["edgeA"]) > 800 and len(by_contig["edgeC"]) > 800 and by_contig["edgeB"] == []
    for c, s in ctg:
        if c != "edgeB":
            pos = {int(r[3]) for r in by_contig[c]}
            assert 1 in pos and len(s) - L + 1 in pos, c                      # position 1, and a read that ends at the contig's last base
            assert {r[1] for r in by_contig[c] if int(r[3]) in (1, len(s) - L + 1)} == {"0", "16"}
    names = [r[0] for r in rows]
    dups = [i for i, nm in enumerate(names) if nm.startswith("dup")]
    assert len(dups) == 4 and len({tuple(rows[i][2:4]) for i in dups}) == 1 and dups[-1] - dups[0] > 1800     # equal keys, blocks apart
    keys = [(r[2], r[3]) for r in rows]
    assert len(keys) - len(set(keys)) > 100                                   # many more equal keys: the same place from both strands
    mapped = {nm for nm in names}
    unmapped = [k for k, (nm, _, _) in enumerate(rd) if nm not in mapped]
    assert 30 <= len(unmapped) <= 45 and min(unmapped) < 64 and max(unmapped) > 1900 and all(rd[k][0].startswith("u") for k in unmapped)
    assert sorted(rows, key=lambda r: (r[2], int(r[3]))) != rows              # the input order is not the sorted order


@pytest.mark.parametrize("extra", [[], ["--read_text=device"], ["--track_text=device"], ["--batch=64"]], ids=["read_text_host", "read_text_device", "track_text_device", "file_order_blocks"])
def test_cli_sorted_equals_the_model_of_the_unsorted_run(extra, edge_run, tmp_path):
    fa, fq, ctg, rd, plain = edge_run
    out = str(tmp_path / "sorted")
    r = drive(fa, fq, out, SORTED + extra)
    assert "sam sort on the device:" in r.stderr and " sort " in r.stderr and " gather " in r.stderr and " download " in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.endswith(".sam")] == ["sorted.sam"]
    rows = assert_sorted_equals_model(out + ".sam", plain + ".sam", len(ctg))
    assert f"{len(rows)} rows" in r.stderr and f"{len(rows)} SAM records" in r.stderr
    keys = [((0 if x[2] == b"edgeA" else 2), int(x[3])) for x in rows]
    assert keys == sorted(keys) and keys[0] == (0, 1) and keys[-1] == (2, 2003 - L + 1)
    dups = [x[0] for x in rows if x[0].startswith(b"dup")]
    assert [d[:4] for d in dups] == [b"dup0", b"dup1", b"dup2", b"dup3"]        # equal keys across blocks keep input order
    compare_tracks(open(out + ".sgr").read(), open(plain + ".sgr").read(), 3)


def test_cli_sorted_with_a_small_piece_size(edge_run, tmp_path):
    """GM_SORT_PIECE=65536: about 330 KB of rows in pieces of 64 KiB, every fifth block or so cut at a row boundary"""
    fa, fq, ctg, rd, plain = edge_run
    out = str(tmp_path / "sorted")
    r = drive(fa, fq, out, SORTED, env=dict(os.environ, GM_SORT_PIECE="65536"))
    assert "pieces of 65536 bytes" in r.stderr
    n_pieces = int(r.stderr.split(" text bytes in ")[1].split(" pieces")[0])
    assert n_pieces >= 4
    assert_sorted_equals_model(out + ".sam", plain + ".sam", len(ctg))
    compare_tracks(open(out + ".sgr").read(), open(plain + ".sgr").read(), 3)


def test_cli_sorted_blocks_mapped_in_halves(edge_run, tmp_path):
    """process_block_split: the halves of a block go into the sorter under sequence numbers of their own, in read order"""
    fa, fq, ctg, rd, plain = edge_run
    out = str(tmp_path / "sorted")
    r = drive(fa, fq, out, ["--sam_sort=coordinate", "--chunk_reads=500", "--workers=2"], env=dict(os.environ, GM_TEST_MAX_BLOCK="60"))
    assert "in halves" in r.stderr
    assert_sorted_equals_model(out + ".sam", plain + ".sam", len(ctg))


@pytest.mark.parametrize("extra", [[], ["--read_text=device"]], ids=["read_text_host", "read_text_device"])
def test_cli_sorted_blocks_written_in_halves(extra, edge_run, tmp_path):
    """the OUTPUT call finds the block too large (GM_TEST_MAX_OUT_BLOCK stands in for its two limits: 2^31 matches, a 4 GB CIGAR pool),
    after it has taken the block's sequence number: the number is given back, and the first half may carry it again"""
    fa, fq, ctg, rd, plain = edge_run
    out = str(tmp_path / "sorted")
    r = drive(fa, fq, out, ["--sam_sort=coordinate", "--chunk_reads=500", "--workers=2"] + extra, env=dict(os.environ, GM_TEST_MAX_OUT_BLOCK="60"))
    assert "written in halves" in r.stderr and "mapped in halves" not in r.stderr
    assert_sorted_equals_model(out + ".sam", plain + ".sam", len(ctg))
    compare_tracks(open(out + ".sgr").read(), open(plain + ".sgr").read(), 3)


@pytest.fixture(scope="module")
def rep_fa(tmp_path_factory):
    return rf.build_index(tmp_path_factory)


def test_cli_sorted_print_all_sam_on_the_repeat_genome(rep_fa, tmp_path):
    """many rows per read and many equal keys: 19 264 rows of 206 reads, in blocks of about 16 reads"""
    fq = rf.fastq_path(rep_fa, "rep.fq")
    plain, out = str(tmp_path / "plain"), str(tmp_path / "sorted")
    drive(rep_fa, fq, plain, ["--print_all_sam"])
    drive(rep_fa, fq, out, ["--print_all_sam", "--sam_sort=coordinate", "--chunk_reads=16", "--workers=3"])
    rows = assert_sorted_equals_model(out + ".sam", plain + ".sam", 3)
    keys = [(x[2], x[3]) for x in rows]
    assert len(rows) > 19000 and len(keys) - len(set(keys)) > 1000
    compare_tracks(open(out + ".sgr").read(), open(plain + ".sgr").read(), 3)


def test_cli_sorted_fasta_reads(tmp_path):
    fa, reads = os.path.join(GOLDEN, "syn.fa"), os.path.join(GOLDEN, "syn_reads.fa")
    plain, out = str(tmp_path / "plain"), str(tmp_path / "sorted")
    drive(fa, reads, plain, [])
    drive(fa, reads, out, SORTED)
    rows = assert_sorted_equals_model(out + ".sam", plain + ".sam", 3)
    assert len(rows) > 400 and len({x[2] for x in rows}) == 3
    compare_tracks(open(out + ".sgr").read(), open(plain + ".sgr").read(), 3)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
PIECE = 65536


@pytest.fixture(scope="module")
def abi(syn_fa, syn_reads):
    """the index, the parameters and five blocks of 64 reads: blocks 1 and 3 with names of about 900 bytes, block 2 with a 2048-base read (a
    row longer than 4 KB), block 4 of random reads (nothing maps).  The reference rows of every block, from gm_output_batch_text, and
    the coverage track after those calls, are computed once."""
    ix = g.Index(syn_fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    genome = b"".join(l.strip() for l in open(syn_fa, "rb") if not l.startswith(b">")).upper()
    rng = np.random.default_rng(11)
    blocks = []
    for k in range(4):
        rd = syn_reads[64 * k:64 * (k + 1)]
        names = [r[0].encode() for r in rd]; seqs = [r[1] for r in rd]; quals = [r[2][:len(r[1])] for r in rd]
        if k in (1, 3):
            names = [(nm + b"_") * 45 for nm in names]
        if k == 2:
            names[20] = b"long2048"; seqs[20] = genome[1000:3048]; quals[20] = b"I" * 2048
        blocks.append((names, seqs, quals))
    blocks.append(([b"none%d" % i for i in range(64)], [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)) for _ in range(64)], [b"I" * 100] * 64))
    packed = [g.pack_reads(s, q) for _, s, q in blocks]
    batches = [g.Batch(ix, 64, B.shape[1]) for B, _, _ in packed]
    ix.coverage_reset(8)
    rows = []
    for (names, _, _), (B, Q, Ln), batch in zip(blocks, packed, batches):
        text, row_off = batch.output_text(p, batch.map(p, B, Q, Ln), names)
        rows.append([text[int(row_off[i]):int(row_off[i + 1])] for i in range(len(row_off) - 1)])
    cov = ix.coverage_download()
    assert [len(r) > 40 for r in rows] == [True, True, True, True, False] and rows[4] == []
    assert max(len(r) for r in rows[2]) > 4096 and sum(len(x) for r in rows for x in r) > 2 * PIECE
    yield dict(ix=ix, p=p, blocks=blocks, packed=packed, batches=batches, rows=rows, cov=cov, contigs=[c for c, _ in ix.contigs()])
    for b in batches:
        b.destroy()
    ix.close()


def model_text(abi, order):
    """the model on the blocks' rows joined in sequence order"""
    rows = [r.decode("latin-1") for k in order for r in abi["rows"][k]]
    return "".join(sort_rows(rows, abi["contigs"])).encode("latin-1")


def filled(abi, seqs):
    """a sorter with block k added under sequence number seqs[k], in the order of the dict"""
    g.set_option("GM_SORT_PIECE", PIECE)
    try:
        s = api.SamSorter(abi["ix"])
    finally:
        g.set_option("GM_SORT_PIECE", None)
    for k, seq in seqs.items():
        B, Q, Ln = abi["packed"][k]
        batch = abi["batches"][k]
        s.add_block(batch, abi["p"], batch.map(abi["p"], B, Q, Ln), seq, names=abi["blocks"][k][0])
    return s


def test_abi_blocks_added_in_reverse_order_over_several_pieces(abi):
    ix = abi["ix"]
    ix.coverage_reset(8)
    s = filled(abi, {3: 30, 2: 20, 1: 10, 0: 0})
    cov = ix.coverage_download()
    n_rows, n_bytes = s.finish()
    want = model_text(abi, [0, 1, 2, 3])
    assert n_rows == sum(len(abi["rows"][k]) for k in range(4)) and n_bytes == len(want)
    st = s.stats()
    assert st["piece_bytes"] == PIECE and st["pieces"] >= 3 and st["rows"] == n_rows and st["text_bytes"] == n_bytes
    assert s.finish() == (n_rows, n_bytes)                                    # a second finish: the same numbers
    got = s.text()
    assert got == want
    assert want != b"".join(r for k in range(4) for r in abi["rows"][k])      # (the input order is not the sorted order)
    assert s.read(4096) == b""
    # the four sorted calls deposited what the four text calls deposited (same_track of test_gpu_sam_text.py).  The 2048-base read's
    # posterior is inf / inf = NaN in the reference's arithmetic (exp(1535.7) in fp64), so the bins under it hold NaN in both tracks:
    # they have to be the same bins, and every other bin is compared as usual
    ref = abi["cov"]
    nan = np.isnan(ref)
    assert 2048 // 8 <= int(nan.sum()) <= 2048 // 8 + 1 and np.array_equal(np.isnan(cov), nan)
    a, b = cov[~nan].astype(np.float64), ref[~nan]
    assert float(b.sum()) > 100.0 and np.all(np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b)) + 2e-5)
    s.destroy()


def test_abi_sequence_numbers_decide_among_equal_keys(abi):
    """the same block under two sequence numbers: every key twice, the copy with the lower number first - whichever was added first"""
    rows = [r.decode("latin-1") for r in abi["rows"][0]]
    for order in ((7, 3), (3, 7)):
        g.set_option("GM_SORT_PIECE", PIECE)
        s = api.SamSorter(abi["ix"])
        g.set_option("GM_SORT_PIECE", None)
        B, Q, Ln = abi["packed"][0]
        batch = abi["batches"][0]
        for seq in order:
            names = [nm + (b"/lo" if seq == 3 else b"/hi") for nm in abi["blocks"][0][0]]
            s.add_block(batch, abi["p"], batch.map(abi["p"], B, Q, Ln), seq, names=names)
        s.finish()
        tag = lambda r, t: r.replace("\t", t + "\t", 1)
        want = "".join(sort_rows([tag(r, "/lo") for r in rows] + [tag(r, "/hi") for r in rows], abi["contigs"])).encode("latin-1")
        assert s.text() == want
        s.destroy()


def test_abi_read_returns_whole_rows(abi):
    want = model_text(abi, [0, 1, 2, 3])
    rows = want.splitlines(keepends=True)
    long_row = max(rows, key=len)
    assert len(long_row) > 4096 and sum(len(r) > 4096 for r in rows) == 1
    # slabs of at most 4096 bytes; the long row is asked for with its own length
    s = filled(abi, {3: 3, 2: 2, 1: 1, 0: 0})
    s.finish()
    slabs, at = [], 0
    while True:
        try:
            t = s.read(4096)
        except g.GnumapError as e:
            assert e.code == api.GM_E_CAPACITY and want[at:].startswith(long_row) and e.needed == len(long_row)
            with pytest.raises(g.GnumapError) as e2:                          # one byte short: the same answer, nothing consumed
                s.read(len(long_row) - 1)
            assert e2.value.code == api.GM_E_CAPACITY and e2.value.needed == len(long_row)
            t = s.read(len(long_row))
            assert t == long_row
        if not t:
            break
        assert len(t) <= max(4096, len(long_row)) and t.endswith(b"\n") and want[at:at + len(t)] == t
        nxt = want.find(b"\n", at + len(t)) + 1                               # the next row would not have fit
        assert nxt == 0 or nxt - at > 4096 or t == long_row
        slabs.append(t); at += len(t)
    assert b"".join(slabs) == want and len(slabs) > 20
    s.destroy()
    # a cap of exactly one row's length returns that row; the rest in one piece
    s = filled(abi, {0: 0, 1: 1, 2: 2, 3: 3})
    s.finish()
    for r in rows[:40]:
        with pytest.raises(g.GnumapError) as e:
            s.read(len(r) - 1)
        assert e.value.code == api.GM_E_CAPACITY and e.value.needed == len(r)
        assert s.read(len(r)) == r
    assert s.text(cap=1 << 20) == b"".join(rows[40:])
    s.destroy()


def test_abi_empty_sorter_and_a_block_without_rows(abi):
    s = api.SamSorter(abi["ix"])
    assert s.finish() == (0, 0) and s.read(4096) == b"" and s.text() == b""
    s.destroy()
    s = filled(abi, {4: 0})                                                   # no read of the block maps: no rows
    assert s.finish() == (0, 0) and s.read(4096) == b""
    s.destroy()
    s = filled(abi, {3: 4, 4: 3, 0: 1})                                       # ... and between two others it changes nothing
    n_rows, _ = s.finish()
    assert n_rows == len(abi["rows"][0]) + len(abi["rows"][3]) and s.text() == model_text(abi, [0, 3])
    s.destroy()


def test_abi_duplicate_sequence_number_and_add_after_finish(abi):
    ix = abi["ix"]
    s = filled(abi, {0: 7})
    B, Q, Ln = abi["packed"][3]
    batch = abi["batches"][3]
    ix.coverage_reset(8)
    with pytest.raises(g.GnumapError, match="used twice") as e:
        s.add_block(batch, abi["p"], batch.map(abi["p"], B, Q, Ln), 7, names=abi["blocks"][3][0])
    assert e.value.code == -1                                                 # GM_E_ARG
    assert float(ix.coverage_download().sum()) == 0.0                         # refused before anything was deposited
    s.finish()
    with pytest.raises(g.GnumapError, match="after gm_sam_sorter_finish") as e:
        s.add_block(batch, abi["p"], batch.map(abi["p"], B, Q, Ln), 8, names=abi["blocks"][3][0])
    assert e.value.code == -1
    assert float(ix.coverage_download().sum()) == 0.0
    assert s.text() == model_text(abi, [0])                                   # the refused blocks left nothing behind
    s.destroy()


def test_abi_resident_form_on_a_text_block(abi, syn_fq):
    """gm_output_batch_sorted_resident: blocks cut on the device by gm_batch_upload_text, added in reverse order"""
    ix, p = abi["ix"], abi["p"]
    lines = open(syn_fq, "rb").read().splitlines(keepends=True)
    texts = [b"".join(lines[4 * 64 * k:4 * 64 * (k + 1)]) for k in range(3)]
    batch = g.Batch(ix, 64, 2048)
    want_rows = []
    for t in texts:
        info = batch.upload_text(p, t, want_recs=False)
        assert info["n"] == 64 and info["status"] == api.GM_TEXT_OK
        text, row_off = batch.output_text_resident(p, batch.map_text(p))
        want_rows += [text[int(row_off[i]):int(row_off[i + 1])].decode("latin-1") for i in range(len(row_off) - 1)]
    g.set_option("GM_SORT_PIECE", PIECE)
    s = api.SamSorter(ix)
    g.set_option("GM_SORT_PIECE", None)
    for k in (2, 1, 0):
        batch.upload_text(p, texts[k], want_recs=False)
        s.add_block(batch, p, batch.map_text(p), k)
    n_rows, _ = s.finish()
    assert n_rows == len(want_rows) > 150
    assert s.text() == "".join(sort_rows(want_rows, abi["contigs"])).encode("latin-1")
    s.destroy(); batch.destroy()


def test_abi_output_call_that_fails_gives_its_sequence_number_back(abi):
    ix = abi["ix"]
    s = api.SamSorter(ix)
    B, Q, Ln = abi["packed"][0]
    batch = abi["batches"][0]
    ix.coverage_reset(8)
    g.set_option("GM_TEST_MAX_OUT_BLOCK", 10)
    try:
        with pytest.raises(g.GnumapError) as e:
            s.add_block(batch, abi["p"], batch.map(abi["p"], B, Q, Ln), 5, names=abi["blocks"][0][0])
    finally:
        g.set_option("GM_TEST_MAX_OUT_BLOCK", None)
    assert e.value.code == api.GM_E_BATCH_TOO_LARGE and float(ix.coverage_download().sum()) == 0.0
    s.add_block(batch, abi["p"], batch.map(abi["p"], B, Q, Ln), 5, names=abi["blocks"][0][0])      # the same number again
    s.finish()
    assert s.text() == model_text(abi, [0])
    s.destroy()


# ---- rows and keys of the test's own (gm_sam_sorter_add_rows) ----------------------------------------------------------------------
def own_rows(n, seed, lens):
    """n rows '<seed>.<i>:xxxx\n' of the lengths lens[i % len(lens)], with keys on three contigs (few positions: many equal keys) and
    every seventh row without a contig - alternately contig = n_seqs and 0xFFFFFFFF"""
    rng = np.random.default_rng(seed)
    rows, contig, pos = [], [], []
    for i in range(n):
        head = b"%d.%d:" % (seed, i)
        rows.append(head + b"x" * max(0, lens[i % len(lens)] - len(head) - 1) + b"\n")
        if i % 7 == 3:
            contig.append(3 if i % 2 else 0xFFFFFFFF); pos.append(int(rng.integers(0, 1000)))      # (the position of such a row is not part of its key)
        else:
            contig.append(int(rng.integers(0, 3))); pos.append(int(rng.integers(1, 40)))
    return rows, np.array(contig, np.uint32), np.array(pos, np.uint64)


def own_model(blocks):
    """stable sort of the blocks' rows, joined in sequence order, by (contig, position); rows without a contig last, in input order"""
    items = [(((int(c), int(q)) if c < 3 else (3, 0)), r) for _, (rows, contig, pos) in sorted(blocks.items()) for r, c, q in zip(rows, contig, pos)]
    return b"".join(r for _, r in sorted(items, key=lambda it: it[0]))


@pytest.mark.parametrize("lens, n", [((12, 14, 17), 3000), ((12, 300, 13, 16, 2100, 15), 1500), ((70, 64, 61), 2000)], ids=["short_rows", "mixed", "at_the_switch"])
def test_own_rows_short_enough_for_the_global_search_and_rows_without_a_contig(lens, n, abi):
    """rows of 12 .. 17 bytes: about 290 of them in a 4 KiB span, far beyond the 63 whose table k_ss_gather keeps in LDS, so the spans
    search the sorted offsets in global memory; rows of 61 .. 70 bytes: spans of 60 .. 67 rows, on both sides of the switch; mixed: both
    forms side by side in one slab.  Every seventh row has no contig (key ~0): last, in input order across blocks added in reverse."""
    blocks = {seq: own_rows(n, seq, lens) for seq in (1, 2, 3)}
    g.set_option("GM_SORT_PIECE", PIECE)
    s = api.SamSorter(abi["ix"])
    g.set_option("GM_SORT_PIECE", None)
    for seq in (3, 1, 2):
        s.add_rows(seq, *blocks[seq])
    want = own_model(blocks)
    n_rows, n_bytes = s.finish()
    assert (n_rows, n_bytes) == (3 * n, len(want))
    rows_per_span = 4096 * n_rows / n_bytes
    assert (rows_per_span > 200) if lens[0] == 12 and len(lens) == 3 else True
    got = s.text(cap=50000)                                                   # slabs of a dozen spans, the last span of each partly filled
    assert got == want
    tail = want.splitlines()[-(3 * n // 7 - 2):]
    assert [int(r.split(b".")[0]) for r in tail] == sorted(int(r.split(b".")[0]) for r in tail)       # the rows without a contig: by sequence number
    assert s.stats()["pieces"] >= (2 if n_bytes > PIECE else 1)
    with pytest.raises(g.GnumapError, match="used twice"):
        s2 = api.SamSorter(abi["ix"]); s2.add_rows(1, *blocks[1]); s2.add_rows(1, *blocks[1])
    s2.destroy(); s.destroy()
