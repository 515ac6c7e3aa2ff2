"""--bam_index: the .bai built on the device (gm_bai.hip) against tests/bai_model.py applied to the file the test assembles from what the
sorter returned - byte for byte at both levels - and the specification's reader on it: every record that overlaps a region is among
those the region's chunks reach.

* the sorter: records of tests/test_bai_cpu.py's fixture enter through add_rows with matching keys and leave through read_bgzf(cap =
  200000), three blocks a slab; zero rows, one row, the 2^29 limit, keys that disagree with the records, capacity, call order;
* the real path: blocks mapped on the edge genome, add_block, index_begin, reads, bai();
* the driver: --sam_format=bam --sam_sort=coordinate --bam_index on the edge genome.

The fixture's index has seven contigs (the first, the fourth and the last without a record), which golden/syn.fa's three cannot give;
the other sorter cases run on syn.fa's index."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import gnumap_amd as g
import bai_model as bai
import bam_model as bm
from gnumap_amd import api
from test_bai_cpu import BIG_CONTIGS, big_fixture, check_big_fixture, row, small_fixtures
from test_gpu_sam_sort import SORTED, drive, edge_run  # noqa: F401  (edge_run is a fixture)

pytestmark = pytest.mark.gpu
CAP = 200000


def sorter_with(ix, recs, keys, blocks=3):
    """a finished sorter of BAM rows: the records added in `blocks` calls of add_rows under their keys"""
    s = api.SamSorter(ix, rows="bam")
    cut = [len(recs) * k // blocks for k in range(blocks + 1)]
    for k in range(blocks):
        part = recs[cut[k]:cut[k + 1]]
        if part:
            s.add_rows(k, part, [c for c, _ in keys[cut[k]:cut[k + 1]]], [p for _, p in keys[cut[k]:cut[k + 1]]])
    assert s.finish()[0] == len(recs)
    return s


def indexed_file(ix, s, level, cap=CAP):
    """(the file: header blocks + every slab of read_bgzf + end marker, the number of slabs) of a finished sorter, index_begin called here"""
    head = ix.bgzf_compress(ix.bam_header(b"@HD\tVN:1.0\tSO:coordinate\n"), level=level)
    s.index_begin(len(head))
    slabs = []
    while True:
        t = s.read_bgzf(cap, level=level)
        if not t:
            break
        slabs.append(t)
    return head + b"".join(slabs) + api.bgzf_eof(), len(slabs)


@pytest.fixture(scope="module")
def big_ix(tmp_path_factory):
    d = tmp_path_factory.mktemp("bai")
    fa = str(d / "seven.fa")
    rng = np.random.default_rng(3)
    with open(fa, "wb") as f:
        for name, ln in BIG_CONTIGS:
            f.write(b">" + name.encode() + b"\n" + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), ln)) + b"\n")
    g.index_build(fa, g.GM_BUILD_HOST)
    ix = g.Index(fa, device=0)
    assert [c for c, _ in ix.contigs()] == [c for c, _ in BIG_CONTIGS]
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def syn_ix(syn_fa):
    ix = g.Index(syn_fa, device=0)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def big():
    return big_fixture()


# ---- the device's bytes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
def test_device_bytes_equal_the_model(big_ix, big, level):
    recs, keys = big
    s = sorter_with(big_ix, recs, keys)
    data, n_slabs = indexed_file(big_ix, s, level)
    assert n_slabs >= 3
    assert [bytes(r) for r in bai.scan(data)["recs"]] == recs                 # the file holds the fixture, in its order ...
    check_big_fixture(data, recs)                                            # ... cut as the fixture expects: every case is in it
    want = bai.build_bai(data)
    got = s.bai()
    assert got == want
    assert s.bai() == want                                                   # and again
    st = s.stats()
    p = bai.parse_bai(got)
    assert st["bai_bytes"] == len(got) and st["bai_chunks"] == sum(len(c) for r in p["refs"] for c in r["bins"].values()) and st["bai_ms"] > 0
    s.destroy()


def test_query_property_on_the_device_index(big_ix, big):
    recs, keys = big
    s = sorter_with(big_ix, recs, keys)
    data, _ = indexed_file(big_ix, s, 1)
    got = s.bai()
    assert bai.check_queries(data, got, bai.regions_of(data)) > 5000         # every window-aligned region and 200 random ones per reference
    s.destroy()


# ---- other cases ---------------------------------------------------------------------------------------------------------------
def test_zero_rows_give_the_empty_index(syn_ix):
    s = sorter_with(syn_ix, [], [])
    data, n_slabs = indexed_file(syn_ix, s, 1)
    n_ref = len(syn_ix.contigs())
    assert n_slabs == 0 and s.bai() == b"BAI\x01" + struct.pack("<i", n_ref) + b"\0" * (8 * n_ref + 8) == bai.build_bai(data)
    s.destroy()


def test_one_row(syn_ix):
    contigs = [(c, 0) for c, _ in syn_ix.contigs()]
    recs = small_fixtures(contigs)["one_row"]
    s = sorter_with(syn_ix, recs, [(0, 78)], blocks=1)
    data, n_slabs = indexed_file(syn_ix, s, 1)
    got = s.bai()
    assert n_slabs == 1 and got == bai.build_bai(data)
    p = bai.parse_bai(got)
    assert p["refs"][0]["order"] == [4681, 37450] and p["refs"][0]["pseudo"][2:] == (1, 0) and p["n_no_coor"] == 0
    assert p["refs"][0]["bins"][4681][0][1] == (len(data) - 28) << 16         # the last record ends at (the end marker, 0)
    s.destroy()


def test_capacity_one_byte_short(big_ix, big):
    recs, keys = big
    s = sorter_with(big_ix, recs[:400], keys[:400])
    data, _ = indexed_file(big_ix, s, 0)
    want = bai.build_bai(data)
    with pytest.raises(g.GnumapError) as e:
        s.bai(cap=len(want) - 1)
    assert e.value.code == api.GM_E_CAPACITY and e.value.needed == len(want)
    buf = np.full(len(want) + 16, 0xAA, np.uint8); got = C.c_uint64(0)
    assert g.lib().gm_sam_sorter_bai(s.h, buf.ctypes.data, len(want) - 1, C.byref(got), None) == api.GM_E_CAPACITY
    assert got.value == len(want) and (buf == 0xAA).all()                    # nothing is written
    assert g.lib().gm_sam_sorter_bai(s.h, buf.ctypes.data, len(want), C.byref(got), None) == 0
    assert bytes(buf[:len(want)]) == want and (buf[len(want):] == 0xAA).all()      # nothing past cap
    s.destroy()


def test_end_at_2_29_is_accepted_and_one_more_is_refused(syn_ix):
    contigs = [(c, 0) for c, _ in syn_ix.contigs()]
    name = contigs[1][0]
    ok = bm.sam_to_bam_records(row(b"edge", 0, name.encode(), (1 << 29) - 23, b"23M"), contigs)
    s = sorter_with(syn_ix, ok, [(1, (1 << 29) - 22)], blocks=1)
    data, _ = indexed_file(syn_ix, s, 1)
    got = s.bai()
    assert got == bai.build_bai(data) and len(bai.parse_bai(got)["refs"][1]["lin"]) == 32768
    s.destroy()
    over = bm.sam_to_bam_records(row(b"over", 0, name.encode(), (1 << 29) - 22, b"23M"), contigs)
    s = sorter_with(syn_ix, over, [(1, (1 << 29) - 21)], blocks=1)
    indexed_file(syn_ix, s, 1)
    with pytest.raises(g.GnumapError) as e:
        s.bai()
    assert e.value.code == -6                                                # GM_E_UNSUPPORTED
    assert name in str(e.value) and str((1 << 29) - 21) in str(e.value) and str(1 << 29) in str(e.value)      # reference, position, limit
    s.destroy()


def test_keys_that_disagree_with_the_records_are_refused(syn_ix):
    contigs = [(c, 0) for c, _ in syn_ix.contigs()]
    c0 = contigs[0][0].encode()
    recs = bm.sam_to_bam_records(b"\n".join(row(b"r%d" % i, 0, c0, p, b"23M") for i, p in enumerate((10, 30, 20))), contigs)
    s = sorter_with(syn_ix, recs, [(0, 11), (0, 12), (0, 13)], blocks=1)      # the keys say 10, 11, 12
    indexed_file(syn_ix, s, 1)
    with pytest.raises(g.GnumapError) as e:
        s.bai()
    assert e.value.code == -1 and "not in coordinate order" in str(e.value)
    s.destroy()
    s = sorter_with(syn_ix, [b"\x08\0\0\0garbage!"], [(0, 1)], blocks=1)      # no whole record
    indexed_file(syn_ix, s, 1)
    with pytest.raises(g.GnumapError) as e:
        s.bai()
    assert e.value.code == -1 and "not a whole BAM record" in str(e.value)
    s.destroy()


def test_call_order(syn_ix):
    contigs = [(c, 0) for c, _ in syn_ix.contigs()]
    c0 = contigs[0][0].encode()
    recs = bm.sam_to_bam_records(b"\n".join(row(b"r%d" % i, 0, c0, 10 * i, b"23M") for i in range(40)), contigs)
    keys = [(0, 10 * i + 1) for i in range(40)]

    def refused(call, what):
        with pytest.raises(g.GnumapError) as e:
            call()
        assert e.value.code == -1 and what in str(e.value), str(e.value)

    t = api.SamSorter(syn_ix)                                                # text rows
    t.add_rows(0, [b"a\t0\tx\n"], [0], [1]); t.finish()
    refused(lambda: t.index_begin(0), "BAM records")
    t.destroy()
    s = api.SamSorter(syn_ix, rows="bam")
    s.add_rows(0, recs, [c for c, _ in keys], [p for _, p in keys])
    refused(lambda: s.index_begin(0), "gm_sam_sorter_finish first")
    s.finish()
    refused(lambda: s.bai(), "gm_sam_sorter_index_begin")                     # no index_begin
    head = syn_ix.bgzf_compress(syn_ix.bam_header(b""), level=1)
    s.index_begin(len(head))
    refused(lambda: s.index_begin(len(head)), "twice")
    refused(lambda: s.read(4000), "gm_sam_sorter_read_bgzf")                  # the text read
    refused(lambda: s.bai(), "unread")
    with pytest.raises(g.GnumapError) as e:
        s.read_bgzf(60, level=1)                                             # a cap below one record: nothing is noted, nothing consumed
    assert e.value.code == api.GM_E_CAPACITY
    first = s.read_bgzf(2000, level=1)
    assert first
    refused(lambda: s.read_bgzf(2000, level=0), "one level")
    refused(lambda: s.bai(), "unread")
    rest = []
    while True:
        x = s.read_bgzf(2000, level=1)
        if not x:
            break
        rest.append(x)
    assert len(rest) >= 2
    assert s.bai() == bai.build_bai(head + first + b"".join(rest) + api.bgzf_eof())
    s.destroy()
    r = api.SamSorter(syn_ix, rows="bam")                                     # a row read before index_begin
    r.add_rows(0, recs, [c for c, _ in keys], [p for _, p in keys]); r.finish()
    assert r.read_bgzf(2000)
    refused(lambda: r.index_begin(0), "read already")
    r.destroy()


# ---- through the real path -----------------------------------------------------------------------------------------------------
def test_blocks_mapped_on_the_edge_genome(edge_run):
    fa, fq, ctg, rd, plain = edge_run
    ix = g.Index(fa, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    g.set_option("GM_SORT_PIECE", 65536)
    try:
        s = api.SamSorter(ix, rows="bam")
    finally:
        g.set_option("GM_SORT_PIECE", None)
    batches = []
    for k in (3, 2, 1, 0):                                                    # added in reverse
        part = rd[64 * k:64 * (k + 1)]
        B, Q, Ln = g.pack_reads([r[1] for r in part], [r[2] for r in part])
        batch = g.Batch(ix, 64, B.shape[1])
        s.add_block(batch, p, batch.map(p, B, Q, Ln), 10 * k, names=[r[0].encode() for r in part])
        batches.append(batch)
    n_rows, _ = s.finish()
    assert n_rows > 150
    data, n_slabs = indexed_file(ix, s, 1, cap=30000)
    assert n_slabs >= 2
    got = s.bai()
    assert got == bai.build_bai(data)
    assert bai.check_queries(data, got, bai.regions_of(data, n_random=50)) > 100
    s.destroy()
    for b in batches:
        b.destroy()
    ix.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra, env", [([], None), ([], {"GM_SORT_PIECE": "65536"}), (["--bam_level=0"], None)], ids=["default", "small_pieces", "level_0"])
def test_cli_bam_index_on_the_edge_genome(extra, env, edge_run, tmp_path):
    fa, fq, ctg, rd, plain = edge_run
    out = str(tmp_path / "o")
    env = dict(os.environ, **env) if env else None
    drive(fa, fq, out, ["--sam_format=bam"] + SORTED + extra, env=env)        # without the flag, to the same path (the @PG line names it)
    before = open(out + ".bam", "rb").read()
    os.remove(out + ".bam")
    r = drive(fa, fq, out, ["--sam_format=bam", "--bam_index"] + SORTED + extra, env=env)
    assert sorted(f for f in os.listdir(tmp_path) if not f.endswith(".sgr")) == ["o.bam", "o.bam.bai"]
    data, index = open(out + ".bam", "rb").read(), open(out + ".bam.bai", "rb").read()
    assert data == before                                                    # byte for byte the file of the run without the flag
    assert index == bai.build_bai(data)
    assert bai.check_queries(data, index, bai.regions_of(data)) > 1000
    p = bai.parse_bai(index)
    assert [bool(x["order"]) for x in p["refs"]] == [True, False, True] and p["n_no_coor"] == 0
    assert "bam index on the device" in r.stderr and f"{len(index)} bytes" in r.stderr


# ---- a sorter that outlives its index --------------------------------------------------------------------------------------------
def test_a_sorter_destroyed_after_its_index_leaves_no_hip_error(syn_fa):
    """a sorter that a garbage collector frees late (one held by the traceback of a pytest.raises, say) may be destroyed after its index was
    closed and the index's place in the heap taken by something else: gm_sam_sorter_destroy must not read the closed index for its
    device - a failing hipSetDevice there is what the next launch check of the thread reports ("occ plane construction failed" from
    the next index's open)"""
    ix = g.Index(syn_fa, device=0)
    s = api.SamSorter(ix, rows="bam")
    at = ix.h.value
    ix.close()
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p; libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    libc.memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    held = []
    for size in list(range(64, 16384, 16)) * 4:                               # whatever block takes the closed index's place holds 0xFF bytes
        q = libc.malloc(size); libc.memset(q, 0xFF, size); held.append((q, size))
    covered = any(q <= at < q + size for q, size in held)                    # (usually True; the check below holds either way)
    s.destroy()
    for q, _ in held:
        libc.free(q)
    nxt = g.Index(syn_fa, flags=g.GM_INDEX_FULL_SA)
    nxt.close()
