"""The result of --snp as text: the nine-column <out>.gmp formatted on the device (k_track_sizes<true> / k_track_rows<true>,
gnumap_amd/csrc/gm_tracktext.hip; gm_coverage_write_gmp_calls_device, gm_coverage_calls_text), its "%.2e" (gm_put_e2_hd, gm_dev_fmt_e2)
and <out>.vcf (gm_coverage_write_vcf, --vcf).  The contract of the device writer is the bytes of the host writer
gm_coverage_write_gmp_calls, which tests/test_gpu_snp_call.py pins to the reference function and program:

  1. gm_dev_fmt_e2 against Python's "%.2e";
  2. device writer == host writer, byte for byte, three call settings x three slab sizes, on tracks that hold every column shape on both
     sides of every contig boundary, at position 0 and at l_pac - 1, the print threshold from both sides, p = 0 and p = 1 (flat counts
     give p = 1 under --snp_monop; the diploid test turns them into a diploid call of small p), and a non-zero tail past l_pac; the host
     writer against itself in several slabs and appending;
  3. one tile whose text needs two LDS windows;
  4. gm_coverage_calls_text on ranges, and its capacity protocol;
  5. a NaN and a negative count in printed rows: their slabs, and no other, are formatted by the host;
  6. the VCF against a Python formatter over gm_snp_calls' records and against the 'Y' rows of the .gmp; in many launches, appended, and
     with a stretch of more records than its first buffer holds;
  7. the driver with --snp --snp_calls --vcf --track_text=device against the reference program's nine-column file.

Every count of 2, 3 and 4 lies in [0, 1e9) and every p-value in gm_put_e2_hd's domain: there host_slabs must be 0 - a host-formatted
slab would hide the kernel."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gnumap_amd as g
from gnumap_amd import api
from conftest import GOLDEN, ROOT
from test_gpu_driver_golden import compare_tracks
from test_gpu_snp_call import _allowance, _gmp_rows, _synthetic_tracks, _upload
from test_gpu_track_text import _lines_per_bin
import snpcall_model as M

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "gnumap_amd", "bin", "gnumap")
RUNS = os.path.join(GOLDEN, "ref_runs_snp")
GM_E_ARG, GM_E_CAPACITY = -1, -5
DEFAULT_SLICE = 1 << 24
SETTINGS = [(False, 0.001), (True, 0.001), (False, 0.05)]
IDS = ["diploid", "monop", "pval05"]


class World:
    """one index with bin size 1 and the five sums; the base tracks of tests 2 and 4"""

    def __init__(self, syn_fa):
        self.ix = g.Index(syn_fa)
        self.l_pac = int(self.ix.info.l_pac)
        self.contigs = self.ix.contigs()
        self.offs = [o for _, o in self.contigs]
        pac = np.fromfile(syn_fa + ".gnumap.pac", np.uint8)                       # 2 bits per base, four per byte, first base highest
        k = np.arange(self.l_pac, dtype=np.int64)
        self.ref = ((pac[k >> 2] >> ((~k & 3) << 1)) & 3).astype(np.int64)
        self.ix.coverage_reset(1); self.ix.coverage_enable_nuc()
        self.bins = int(self.ix.coverage_bins())
        assert self.bins > self.l_pac                                             # there is a tail that must not print
        self.cov, self.nuc, self.shapes = self._base_tracks()

    def key(self, k):
        ci = int(np.searchsorted(self.offs, k, side="right")) - 1
        return self.contigs[ci][0], int(k - self.offs[ci] + 1)

    def put(self, cov, nuc, k, counts):
        nuc[:, k] = np.asarray(counts, np.float32)
        cov[k] = np.float32(nuc[:, k].astype(np.float64).sum())

    def shape_counts(self, k, shape):
        r = int(self.ref[k]); c = [0.0] * 5
        if shape == "N":                     # everything in the reference base: \tN
            c[r] = 50.0
        elif shape == "M":                   # everything in another base: [YN]:r->x
            c[(r + 1) % 4] = 50.0
        else:                                # half and half: a diploid call r->x/y (one allele under --snp_monop)
            c[r] = 50.0; c[(r + 1) % 4] = 50.0
        return c

    def _base_tracks(self):
        cov, nuc = _synthetic_tracks(self.bins, self.l_pac, self.contigs)         # seeded; the threshold from both sides, totals up to 5000, the tail set to 7 / 1
        shapes = {}
        plan = [(0, "D"), (1, "M"), (2, "N"), (self.l_pac - 1, "M"), (self.l_pac - 2, "D"), (self.l_pac - 3, "N")]
        for off in self.offs[1:]:
            plan += [(off - 3, "N"), (off - 2, "M"), (off - 1, "D"), (off, "D"), (off + 1, "N"), (off + 2, "M")]
        for k, shape in plan:
            self.put(cov, nuc, k, self.shape_counts(k, shape)); shapes[k] = shape
        # p exactly 0: 5000 in one base that is not the reference's; p exactly 1 under --snp_monop: flat counts whose first maximum (a) is not the reference's
        k0 = next(k for k in range(5000, self.l_pac) if cov[k] == 0 and k not in shapes)
        c = [0.0] * 5; c[(int(self.ref[k0]) + 2) % 4] = 5000.0
        self.put(cov, nuc, k0, c)
        k1 = next(k for k in range(6000, self.l_pac) if cov[k] == 0 and self.ref[k] != 0 and k not in shapes)
        self.put(cov, nuc, k1, [10.0] * 5)
        self.k_p0, self.k_p1 = k0, k1
        assert (cov[self.l_pac:] != 0).all() and (nuc[:, self.l_pac:] != 0).all()
        return cov, nuc, shapes

    def upload(self, cov, nuc):
        _upload(self.ix, np.ascontiguousarray(cov), np.ascontiguousarray(nuc))

    def host_file(self, path, pval, monop):
        self.ix.coverage_write_gmp_calls(path, pval, monop)
        return open(path, "rb").read()

    def device_file(self, path, pval, monop, append=False):
        self.ix.coverage_write_gmp_calls_device(path, pval, monop, append)
        return open(path, "rb").read()


@pytest.fixture(scope="module")
def world(syn_fa):
    w = World(syn_fa)
    yield w
    w.ix.close()


def _with_slice(sl, fn):
    g.set_option("GM_TRACK_SLICE", sl)
    try:
        return fn()
    finally:
        g.set_option("GM_TRACK_SLICE", None)


def _ninth(text):
    """{(contig, pos): ninth column} of a nine-column file"""
    d = {}
    for line in text.decode().splitlines():
        f = line.split("\t")
        assert len(f) == 9, line
        d[(f[0], int(f[1]))] = f[8]
    return d


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_dev_fmt_e2_against_python(world):
    rng = np.random.default_rng(7)
    v = [0.0, 1.0, 0.001, 0.05, 1.125, 1.375, 1.625, 1.005, 1.015, 9.995, 9.994999, 9.985, 99.95, 0.9995, 0.99949999999999994, 2.0 ** -53, 1 - 2.0 ** -53, 2.0 ** -200,
         np.nextafter(2.0 ** 200, 0)]
    v += list(np.ldexp(1.0 + rng.random(1500), rng.integers(-200, 200, 1500)))                 # log-uniform over the domain
    v += list(np.arange(1, 501) * 2.0 ** -53) + list(rng.integers(1, 1 << 53, 500) * 2.0 ** -53)      # what 1 - P can be
    v += list(1.0 - rng.integers(1, 1 << 30, 300) * 2.0 ** -53)
    for e in range(-60, 60, 3):                                                                  # decimal ties with both neighbours, carries, powers of ten
        for m in ("1.005", "1.125", "2.675", "9.995", "9.994999", "1", "9.99", "5.555"):
            x = float(f"{m}e{e}")
            v += [x, float(np.nextafter(x, 0)), float(np.nextafter(x, np.inf))]
    v += [2.0 ** -k for k in range(0, 201, 7)]
    outside = [-0.0, -1.0, -1e-5, np.nan, np.inf, -np.inf, 5e-324, 1e-300, 2.0 ** 200, 1e300, float(np.nextafter(2.0 ** -200, 0)), -2.0 ** -100]
    got = world.ix.dev_fmt_e2(np.array(v + outside, np.float64))
    assert len(v) > 3000
    for x, t in zip(v, got[:len(v)]):
        assert t == ("%.2e" % x).encode() and len(t) == 8, (x, t)
    assert got[len(v):] == [b""] * len(outside)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("monop,pval", SETTINGS, ids=IDS)
def test_device_writer_equals_the_host_writer(world, tmp_path, monop, pval):
    world.upload(world.cov, world.nuc)
    want = world.host_file(str(tmp_path / "host.gmp"), pval, monop)
    col = _ninth(want)
    n_rows = want.count(b"\n")
    assert n_rows == len(col) == int((world.cov[:world.l_pac] > np.float32(0.001)).sum()) > 6000      # the threshold from both sides; nothing of the tail
    # the tracks are worth the run: every shape where it was put, p = 0, p = 1
    for k, shape in world.shapes.items():
        c = col[world.key(k)]
        if shape == "N":
            assert c == "N", (k, c)
        elif shape == "M" or monop:
            assert (c == "N" and shape == "D") or re.fullmatch(r"[YN]:[acgt]->[acgtn] p_val=\d\.\d\de[+-]\d\d", c), (k, shape, c)
        else:
            assert re.fullmatch(r"[YN]:[acgt]->[acgtn]/[acgtn] p_val=\d\.\d\de[+-]\d\d", c), (k, c)
    for side in [(0, 1, 2), (world.l_pac - 3, world.l_pac - 2, world.l_pac - 1)] + [t for off in world.offs[1:] for t in ((off - 3, off - 2, off - 1), (off, off + 1, off + 2))]:
        lens = {len(col[world.key(k)]) for k in side}
        assert lens == ({1, 21} if monop else {1, 21, 23}), (side, lens)                          # + the tab: 2, 22, 24 bytes
    assert col[world.key(world.k_p0)].endswith("p_val=0.00e+00") and col[world.key(world.k_p0)][0] == "Y"
    if monop:
        assert col[world.key(world.k_p1)] == "N:%s->a p_val=1.00e+00" % "acgt"[world.ref[world.k_p1]]
    else:
        assert "/" in col[world.key(world.k_p1)]
    nbk = world.l_pac
    for sl in (None, 4096, 1000):                                   # 1000 is not a multiple of the 256-bin tile
        got, st = _with_slice(sl, lambda: (world.device_file(str(tmp_path / f"dev{sl}.gmp"), pval, monop), world.ix.coverage_text_stats()))
        assert got == want, (sl, len(got), len(want))
        per = sl or DEFAULT_SLICE
        assert st["host_slabs"] == 0, st
        assert st["slabs"] == (nbk + per - 1) // per and st["bytes"] == len(want) and st["rows"] == n_rows, st
        assert st["launches"] == 4 * st["slabs"] and st["kernel_ms"] > 0, st
    out = str(tmp_path / "twice.gmp")
    assert _with_slice(4096, lambda: (world.device_file(out, pval, monop), world.device_file(out, pval, monop, append=True))[1]) == 2 * want


@pytest.mark.parametrize("monop,pval", SETTINGS[:2], ids=IDS[:2])
def test_host_writer_in_several_slabs_and_appending(world, tmp_path, monop, pval):
    """gm_coverage_write_gmp_calls itself: the text does not depend on how many slabs of the tracks it brings down (512 positions per host
    thread, 16 threads unless GM_HOST_THREADS says otherwise: more than 30 slabs), and appending writes behind what is there"""
    world.upload(world.cov, world.nuc)
    want = world.host_file(str(tmp_path / "host.gmp"), pval, monop)                # the text test_device_writer_equals_the_host_writer holds the device writer to
    assert want.count(b"\n") > 6000 and world.l_pac > 30 * 512 * 16
    out = str(tmp_path / "slabs.gmp")
    write = lambda append: g.lib().gm_coverage_write_gmp_calls(world.ix.h, pval, int(monop), out.encode(), append)

    def run():
        assert write(0) == 0
        assert open(out, "rb").read() == want
        assert write(1) == 0
        assert open(out, "rb").read() == 2 * want
    _with_slice(512, run)

# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_tile_of_two_lds_windows(world, tmp_path):
    rng = np.random.default_rng(23)
    cov = np.zeros(world.bins, np.float32); nuc = np.zeros((5, world.bins), np.float32)
    t0 = 256 * 40                                                   # a whole tile of the first slab
    assert world.offs[1] > t0 + 256
    for k in range(t0, t0 + 256):
        c = rng.uniform(1.0e8, 1.2e8, 5)
        two = rng.choice(5, 2, replace=False)
        c[two] = rng.uniform(2.5e8, 2.6e8, 2)                       # two alleles of equal weight: a diploid call
        world.put(cov, nuc, k, c)
    assert (nuc[:, t0:t0 + 256] >= 1e8).all() and (cov[t0:t0 + 256] < 1e9).all() and (nuc[:, t0:t0 + 256] < 1e9).all() and (cov[t0:t0 + 256] >= 1e8).all()
    world.upload(cov, nuc)
    want = world.host_file(str(tmp_path / "host.gmp"), 0.001, False)
    lines = want.split(b"\n")[:-1]
    assert len(lines) == 256 and all(b"/" in l.split(b"\t")[8] for l in lines)
    assert len(want) > 24576 + 256                                  # more than one window of the tile's text
    for sl in (None, 4096):
        got, st = _with_slice(sl, lambda: (world.device_file(str(tmp_path / "dev.gmp"), 0.001, False), world.ix.coverage_text_stats()))
        assert got == want and st["host_slabs"] == 0 and st["rows"] == 256, (sl, st)
    assert world.ix.coverage_calls_text(0.001, False, t0, t0 + 256) == want


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_calls_text_ranges(world, tmp_path):
    pval, monop = 0.001, False
    world.upload(world.cov, world.nuc)
    whole = world.host_file(str(tmp_path / "host.gmp"), pval, monop)
    ix, bins, nbk = world.ix, world.bins, world.l_pac
    assert ix.coverage_calls_text(pval, monop) == whole and ix.coverage_calls_text(pval, monop, 0, bins) == whole
    assert ix.coverage_text_stats()["host_slabs"] == 0
    per = _lines_per_bin(whole, world.cov[:nbk] > np.float32(0.001))
    ranges = [(1000, 1000), (0, 0), (bins, bins), (0, 1), (nbk - 1, nbk), (257, 300), (nbk, bins), (nbk - 300, bins)]
    for off in world.offs[1:]:
        ranges += [(off - 1, off), (off, off + 1), (off - 3, off + 3), (off - 257, off + 257)]
    for sl in (None, 4096, 1000):
        def run():
            for lo, hi in ranges:
                assert ix.coverage_calls_text(pval, monop, lo, hi) == b"".join(per[lo:min(hi, nbk)]), (sl, lo, hi)
        _with_slice(sl, run)
    assert ix.coverage_calls_text(pval, monop, 0, 1) == per[0] != b"" and all(per[off - 1] and per[off] for off in world.offs[1:])
    # the capacity protocol: the size first, and nothing behind cap is touched
    L = g.lib()
    off = world.offs[1]
    lo, hi = off - 300, off + 900
    want = b"".join(per[lo:hi])
    assert len(want) > 2000 and want.count(b"\n") > 100
    got = C.c_uint64()
    assert L.gm_coverage_calls_text(ix.h, pval, 0, lo, hi, None, 0, C.byref(got)) == GM_E_CAPACITY and got.value == len(want)
    buf = np.full(len(want) + 64, 0xAA, np.uint8)
    assert L.gm_coverage_calls_text(ix.h, pval, 0, lo, hi, buf.ctypes.data, len(want) - 1, C.byref(got)) == GM_E_CAPACITY and got.value == len(want)
    assert buf[:len(want) - 1].tobytes() == want[:-1] and (buf[len(want) - 1:] == 0xAA).all()
    assert L.gm_coverage_calls_text(ix.h, pval, 0, lo, hi, buf.ctypes.data, len(want), C.byref(got)) == 0 and got.value == len(want)
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()

    def mid_slab():                                                 # the buffer ends in the middle of a later slab
        buf[:] = 0xAA
        cap = len(want) * 2 // 3
        assert L.gm_coverage_calls_text(ix.h, pval, 0, lo, hi, buf.ctypes.data, cap, C.byref(got)) == GM_E_CAPACITY and got.value == len(want)
        assert buf[:cap].tobytes() == want[:cap] and (buf[cap:] == 0xAA).all()
    _with_slice(512, mid_slab)
    assert L.gm_coverage_calls_text(ix.h, pval, 0, 5, 4, None, 0, C.byref(got)) == GM_E_ARG
    assert L.gm_coverage_calls_text(ix.h, pval, 0, 0, bins + 1, None, 0, C.byref(got)) == GM_E_ARG


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_values_only_snprintf_prints_send_their_slab_to_the_host(world, tmp_path):
    per = 4096
    cov, nuc = world.cov.copy(), world.nuc.copy()
    at = lambda slab: slab * per + 1001
    for slab in (3, 7, 9):
        world.put(cov, nuc, at(slab), [20.0, 30.0, 0.0, 0.0, 0.0])
    nuc[2, at(3)] = np.nan                                          # a printed row of slab 3
    nuc[4, at(7)] = -1.0                                            # a printed row of slab 7
    cov[at(9)] = 0.0; nuc[1, at(9)] = -3.0                          # a row that is not printed flags nothing
    world.upload(cov, nuc)
    want = _with_slice(per, lambda: world.host_file(str(tmp_path / "host.gmp"), 0.001, False))
    assert b"\tnan\t" in want and b"\t-1.00000\t" in want
    got, st = _with_slice(per, lambda: (world.device_file(str(tmp_path / "dev.gmp"), 0.001, False), world.ix.coverage_text_stats()))
    assert got == want
    assert st["host_slabs"] == 2 and st["slabs"] == (world.l_pac + per - 1) // per and st["rows"] == want.count(b"\n"), st
    assert st["launches"] == 4 * st["slabs"] - 2                    # no rows pass for a slab the host formats
    lines = _lines_per_bin(want, cov[:world.l_pac] > np.float32(0.001))
    assert _with_slice(per, lambda: world.ix.coverage_calls_text(0.001, False, at(3) - 5, at(7) + 5)) == b"".join(lines[at(3) - 5:at(7) + 5])


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
HEADER = re.compile(rb"##fileformat=VCFv4\.0\n##fileDate=(\d{8})\n##source=([^\n]+)\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def _vcf_rows(calls, contigs):
    out = []
    for i, r in enumerate(calls):
        head = "%s\t%d\tsnp%d\t%s\t" % (contigs[int(r["contig"])][0], int(r["chr_pos"]), i, "acgtn"[r["ref"]])
        if r["diploid"]:
            ratio = np.float32(r["nuc"][r["alt2"]]) / np.float32(r["nuc"][r["alt1"]])
            out.append(head + "%s%s\t.\t.\tDiploid;pval=%.5f;coverage=%.5f;ratio=%.2f\n" % ("acgtn"[r["alt1"]], "acgtn"[r["alt2"]], r["p_val"], float(r["total"]), float(ratio)))
        else:
            out.append(head + "%s\t.\t.\tMonoploid;pval=%.5f;coverage=%.5f\n" % ("acgtn"[r["alt1"]], r["p_val"], float(r["total"])))
    return "".join(out).encode()


@pytest.mark.parametrize("monop,pval", SETTINGS, ids=IDS)
def test_vcf(world, tmp_path, monop, pval):
    world.upload(world.cov, world.nuc)
    ix = world.ix
    out = str(tmp_path / "o.vcf")
    texts = []
    for sl in (None, 1000):                                         # one stretch of positions, and many
        _with_slice(sl, lambda: ix.coverage_write_vcf(out, pval, monop))
        texts.append(open(out, "rb").read())
    assert texts[0] == texts[1]
    text = texts[0]
    m = HEADER.match(text)
    assert m and m.group(2) == g.version().encode() and 20200101 < int(m.group(1)) < 21000101
    calls = ix.snp_calls(pval, monop)
    body = text[m.end():]
    assert body == _vcf_rows(calls, world.contigs) and len(calls) > 1000
    assert monop or (b"\tDiploid;" in body and b"\tMonoploid;" in body)
    # one to one with the 'Y' rows of the .gmp: contig, position, ref, alleles
    gmp = world.host_file(str(tmp_path / "host.gmp"), pval, monop).decode().splitlines()
    y = [l.split("\t") for l in gmp if l.split("\t")[8].startswith("Y")]
    rows = [l.split("\t") for l in body.decode().splitlines()]
    assert len(rows) == len(y)
    for i, (r, f) in enumerate(zip(rows, y)):
        letters, _ = M.parse_call(f[8])
        assert r[0] == f[0] and r[1] == f[1] and r[2] == "snp%d" % i and r[3] == letters[1] and r[4] == letters[2] + (letters[3] or ""), (r, f)
        assert r[7].split(";")[2] == "coverage=" + f[2] and r[7].startswith("Diploid;" if letters[3] else "Monoploid;"), (r, f)
    # append: no header, the IDs start again
    ix.coverage_write_vcf(out, pval, monop, append=True)
    assert open(out, "rb").read() == text + body
    # a cutoff that no p-value is below: the header alone
    ix.coverage_write_vcf(out, 0.0, monop)
    only = open(out, "rb").read()
    assert HEADER.fullmatch(only)


def test_vcf_in_many_launches_and_a_stretch_beyond_the_first_buffer(world, tmp_path):
    """gm_coverage_write_vcf fetches its records one stretch of 16 x GM_TRACK_SLICE positions at a time, into a buffer of at most 65 536
    records at first.  GM_TRACK_SLICE=64: stretches of 1024 positions, 274 of them, each a call of its own with a launch of its own, a new
    file and appending.  The default (2^20): ONE stretch, the whole reference; with 70 000 substituted positions in a row it holds more
    than 70 000 records, which is more than the first buffer: the fetch is repeated with room for them ("once more with room for it")."""
    pval, monop = 0.001, False
    cov, nuc = world.cov.copy(), world.nuc.copy()
    ks = np.arange(100000, 170000)                                  # across the boundaries it meets; every base read as another one, 50 times
    assert world.l_pac > ks[-1] and world.l_pac <= 16 << 20
    nuc[:, ks] = 0; nuc[(world.ref[ks] + 1) % 4, ks] = 50.0; cov[ks] = 50.0
    world.upload(cov, nuc)
    ix = world.ix
    calls = ix.snp_calls(pval, monop)
    dense = int(((calls["pos"] >= ks[0]) & (calls["pos"] <= ks[-1])).sum())
    assert dense == len(ks) == 70000 > 1 << 16 and len(calls) > dense                # every one of them is called, and others besides
    body = _vcf_rows(calls, world.contigs)
    assert b"\tDiploid;" in body and b"\tMonoploid;" in body
    out = str(tmp_path / "o.vcf")

    def many():
        ix.coverage_write_vcf(out, pval, monop)
        text = open(out, "rb").read()
        ix.coverage_write_vcf(out, pval, monop, append=True)
        return text, open(out, "rb").read()
    text, twice = _with_slice(64, many)
    m = HEADER.match(text)
    assert m and text[m.end():] == body
    assert twice == text + body                                     # one header, the records twice
    ix.coverage_write_vcf(out, pval, monop)                         # one stretch of len(calls) > 65 536 records
    one = open(out, "rb").read()
    assert HEADER.match(one) and one[HEADER.match(one).end():] == body

# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_snp_calls_vcf_with_track_text_device(tmp_path, syn_fa):
    name = "snp"
    m = json.load(open(os.path.join(RUNS, "manifest.json")))["runs"][name]
    ref = _gmp_rows(gzip.open(os.path.join(RUNS, name + ".gmp.gz"), "rt").read())
    out = str(tmp_path / "mine")
    r = subprocess.run([EXE, "-g", syn_fa, "-o", out, "-a", "0.9"] + m["argv"] + ["--snp_calls", "--vcf", "--track_text=device", os.path.join(GOLDEN, m["fastq"])],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, GM_TRACK_SLICE="50000"))
    assert r.returncode == 0, r.stderr[-1500:]
    assert "track text on the device:" in r.stderr and "(0 formatted by the host)" in r.stderr, r.stderr[-1500:]
    assert not os.path.exists(out + ".sgr")
    mine = _gmp_rows(open(out + ".gmp").read())
    # the comparison rule and the caps of test_gpu_snp_call.test_cli_snp_calls_against_the_reference_program
    strip = lambda rows: "".join("\t".join(f[:8]) + "\n" for f in rows.values())
    compare_tracks(strip(mine), strip(ref), 8)
    skipped = n_call = 0
    for k in set(mine) & set(ref):
        a, b = mine[k], ref[k]
        ca, cb = M.parse_call(a[8]), M.parse_call(b[8])
        n_call += cb is not None
        cnt = np.array([float(x) for x in b[3:8]], np.float32)
        if (ca is None) != (cb is None) or (ca is not None and ca[0] != cb[0]):
            top = np.sort(cnt)[-2:]
            p_ref = cb[1] if cb is not None else M.is_snp(cnt, m["monop"])[0]
            tie = abs(float(top[1]) - float(top[0])) <= _allowance(top[1]) + _allowance(top[0])
            ratio_rel = 2 * (_allowance(top[1]) / max(float(top[1]), 1e-30) + _allowance(top[0]) / max(float(top[0]), 1e-30))
            assert tie or M.on_decision_point(cnt, p_ref, m["pval"], m["monop"], M.RUN_REL, ratio_rel=ratio_rel), (a, b)
            skipped += 1
            continue
        if cb is not None:
            assert M.p_close(ca[1], cb[1], M.RUN_REL), (a, b)
    assert n_call > 50 and skipped <= M.MAX_SKIPPED_SHARE * n_call, (skipped, n_call)
    # the .vcf names exactly the 'Y' rows of the same run's .gmp
    text = open(out + ".vcf", "rb").read()
    h = HEADER.match(text)
    assert h
    rows = [l.split("\t") for l in text[h.end():].decode().splitlines()]
    y = [f for f in mine.values() if f[8].startswith("Y")]
    assert len(rows) == len(y) > 10
    for i, (rw, f) in enumerate(zip(rows, y)):
        letters, _ = M.parse_call(f[8])
        assert rw[:5] == [f[0], f[1], "snp%d" % i, letters[1], letters[2] + (letters[3] or "")], (rw, f)
        assert rw[5:7] == [".", "."] and rw[7].split(";")[2] == "coverage=" + f[2], (rw, f)
