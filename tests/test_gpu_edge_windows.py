"""Every kernel that reads the packed reference, at every window where the reference begins and ends: the unit probes dev_nw_score,
dev_traceback and dev_pair_hmm on the edge genome (tests/golden/make_edge_fixtures.py: contigs that start at 0, at 11 mod 16 and at
4 mod 16 and end at 7 mod 16), length x position x kernel form.

Windows of a length L, for every contig [c, e): begins c .. c+17 and e-L-17 .. e-L (all 16 phases of a 16-base word on both sides),
and the begins that are NOT windows: e-L+1 .. e-L+3 (across the end; for the last contig: past l_pac) and c-3 .. c-1 (across the
start).  Reads of a window, both strands, one read per probe (so that the one-lane kernels take their sparse forms): the window with
two substitutions, the reference 2 bases further on and 2 bases back (a gap in the very first or last column: the path runs along
the band's edge at the reference's edge), and the window with an N.

Checked for EVERY probe: `valid` is "the oracle's window has L bases"; the fp32 score bits are gmo_nw_score's; the operations and the
aligned length are gmo_traceback's; the pair-HMM floats are gmo_pair_hmm's, bit for bit.

Loads past the end of pac, as read in the sources: k_nw_lane / k_traceback_lane fetch pac32[w] and pac32[w + 1] for the 16-base word w
of a window base (at the last window: 6 bytes past the last pac byte); go_ref_word (unique-map keys) reads 9 bytes from a window
base's byte; k_nw_rows clamps word indices below 0 and reads no word above the window's last; k_nw, the band kernels and the pair HMM
read single bytes inside the window.  Every one of them tests gm_window_ok first, the host copy of pac carries 64 zero bytes past its
end (gm_index.cpp) and the whole vector is what is uploaded: all of these loads stay inside the allocation."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import edge_fixture as ef
import gnumap_amd as g
from fasta_model import pwm_rows
from reflib import revcomp_pwm, revcomp_str

pytestmark = pytest.mark.gpu

GM_E_UNSUPPORTED = -6
NW_LENS = [14, 16, 17, 19, 23, 24, 25, 31, 33, 100, 104, 105, 150, 152]      # the smallest at which a kernel's shape changes
TB_LENS = NW_LENS + [256, 300, 600]                                             # k_traceback_lane<64>, k_traceback
HMM_LENS = [16, 24, 100]

# name -> (switches, parameters, FASTA reads)
NW_FORMS = {
    "default": ({}, {}, False),                                  # one length, 24 .. 152: k_nw_rows/pairs; else k_nw_lane
    "cells_b32": (dict(GM_NW_CELLS="b32"), {}, False),
    "lane": (dict(GM_NW="lane"), {}, False),                     # stride <= 104: k_nw_lane<13>, <= 152: <19>
    "lane_streaming": (dict(GM_NW_ROWS="0"), {}, False),         # k_nw_lane<0> (and k_nw_rows where it applies)
    "lane_streaming_only": (dict(GM_NW="lane", GM_NW_ROWS="0"), {}, False),
    "wave": (dict(GM_NW="wave"), {}, False),                     # k_nw
    "M1": ({}, dict(max_gap=1), False), "M2": ({}, dict(max_gap=2), False), "M4": ({}, dict(max_gap=4), False),      # k_nw_band
    "M5": ({}, dict(max_gap=5), False), "M7": ({}, dict(max_gap=7), False),
    "fasta": ({}, {}, True), "fasta_lane": (dict(GM_NW="lane"), {}, True),
}
TB_FORMS = {
    "default": ({}, {}, False), "direct": (dict(GM_TRACEBACK="direct"), {}, False), "group": (dict(GM_TRACEBACK="group"), {}, False),
    "M1": ({}, dict(max_gap=1), False), "M5": ({}, dict(max_gap=5), False), "M7": ({}, dict(max_gap=7), False),
    "fasta": ({}, {}, True),
}


def rle(ops: bytes) -> bytes:
    return b"".join(str(len(list(grp))).encode() + bytes([k]) for k, grp in itertools.groupby(ops))


def argmax_cons(P):
    out = bytearray()
    for c in P:
        if c[0] == c[1] == c[2] == c[3]:
            out.append(ord("n"))
        elif c[0] >= c[1]:
            out.append(ord("a" if c[0] >= c[3] else "t") if c[0] >= c[2] else ord("g" if c[2] >= c[3] else "t"))
        else:
            out.append(ord("c" if c[1] >= c[3] else "t") if c[1] >= c[2] else ord("g" if c[2] >= c[3] else "t"))
    return bytes(out)


@pytest.fixture(scope="module")
def edge_fa(tmp_path_factory):
    return ef.build_index(tmp_path_factory)


@pytest.fixture(scope="module")
def ix(edge_fa):
    i = g.Index(edge_fa, flags=g.GM_INDEX_FULL_SA)
    yield i
    i.close()


@pytest.fixture(scope="module")
def oix(oracle, edge_fa):
    o = oracle.index_load(edge_fa)
    ef.check_geometry(o)
    return o


@pytest.fixture(scope="module")
def genome(edge_fa):
    return b"".join(l.strip() for l in open(edge_fa, "rb") if not l.startswith(b">")).upper()


def window_begins(oix, L):
    """(begins, how many of them are windows by construction)"""
    ctg, l_pac = ef.geometry(oix)
    good, bad = set(), set()
    for c, e in ctg:
        good |= set(range(c, c + 18)) | set(range(e - L - 17, e - L + 1))
        bad |= set(range(e - L + 1, e - L + 4)) | {b for b in range(c - 3, c) if b >= 0}
    assert all(b >= 0 for b in good)
    return sorted(good | bad), len(good - bad)


_PROBES = {}


def probes(oix, genome, L, fasta):
    """the reads and the probes (read, strand, begin) of a length: deterministic, one read per probe"""
    key = (L, fasta)
    if key in _PROBES:
        return _PROBES[key]
    rng = np.random.default_rng(1000 * L + fasta)
    rb = lambda n: bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))
    begins, n_good = window_begins(oix, L)

    def piece(b):                                   # the reference from b on, random bases where there is none
        lo = rb(-b) if b < 0 else b""
        s = lo + genome[max(b, 0):max(b, 0) + L - len(lo)]
        return s + rb(L - len(s))

    reads, quals, ridx, strand, pos = [], [], [], [], []
    for b in begins:
        w = bytearray(piece(b))
        sub = bytearray(w)
        for q in (L // 3, L - 2):
            sub[q] = b"ACGT"[(b"ACGT".index(sub[q]) + 1 + (b + q) % 3) % 4]
        amb = bytearray(w)
        amb[L // 2] = ord("N")
        if fasta:                                   # IUPAC letters of two and of three bases, upper and lower case
            amb[1] = ord("R"); amb[L - 1] = ord("y"); amb[L // 4] = ord("b"); amb[L - 5] = ord("V")
        for s in (bytes(sub), piece(b + 2), piece(b - 2), bytes(amb)):
            for st in (0, 1):
                reads.append(revcomp_str(s).upper() if st else s)
                quals.append(bytes((33 + rng.integers(2, 41, L)).astype(np.uint8)))
                ridx.append(len(reads) - 1); strand.append(st); pos.append(b)
    out = dict(reads=reads, quals=quals, ridx=np.array(ridx, np.uint32), strand=np.array(strand, np.uint8), pos=np.array(pos, np.uint64),
               n_good=8 * n_good)
    _PROBES[key] = out
    return out


_WANT = {}


def want(oracle, oix, genome, L, G, fasta, traceback):
    """the oracle's answers to the probes of (L, fasta) at band half-width G: valid, score bits, (aligned length, CIGAR)"""
    key = (L, G, fasta)
    pr = probes(oix, genome, L, fasta)
    if key not in _WANT:
        _WANT[key] = dict(op=oracle.params(max_gap=G), P=[], w=[], valid=None, bits=None, tb=None)
        o = _WANT[key]
        for k in range(len(pr["ridx"])):
            s = pr["reads"][k]
            P = pwm_rows(s) if fasta else oracle.pwm(s, pr["quals"][k])
            o["P"].append(np.ascontiguousarray(revcomp_pwm(P) if pr["strand"][k] else P, np.float32))
            o["w"].append(oracle.window(oix, int(pr["pos"][k]), L))
        o["valid"] = np.array([len(w) == L for w in o["w"]])
        o["bits"] = np.array([np.float32(oracle.lib.gmo_nw_score(C.byref(o["op"]), P, L, w)).view(np.uint32) if v else 0
                              for P, w, v in zip(o["P"], o["w"], o["valid"])], np.uint32)
        # the matrix is not vacuous: every begin meant as a window is one, every other is none, and there are both
        assert o["valid"].sum() == pr["n_good"] and (~o["valid"]).sum() >= 8 * 12
    o = _WANT[key]
    if traceback and o["tb"] is None:
        o["tb"] = [oracle.traceback(o["op"], P, b"n" * L, w)[1:] if v else None for P, w, v in zip(o["P"], o["w"], o["valid"])]
        assert sum(t is not None and (b"I" in t[1] or b"D" in t[1]) for t in o["tb"]) > 100
    return pr, o


def nw_kernel(sw, kw, L):
    """the DP kernel a probe block of one length L (one read per probe: fewer than 2.5 candidates per read) has to take, as gmk_nw picks it;
    a pattern where the choice depends on the block's quality characters"""
    stride = (L + 7) // 8 * 8
    if kw.get("max_gap", 3) != 3:
        return "k_nw_band"
    if sw.get("GM_NW") == "wave":
        return "k_nw"
    if sw.get("GM_NW") != "lane" and 24 <= L <= 152:
        return "k_nw_rows/cells" if sw.get("GM_NW_CELLS") == "b32" else "k_nw_rows/(pairs|cells)"
    if sw.get("GM_NW_ROWS") == "0":
        return "k_nw_lane<0>"
    return "k_nw_lane<13>" if stride <= 104 else "k_nw_lane<19>" if stride <= 152 else "k_nw_lane<0>"


def tb_kernel(sw, kw, L, fasta):
    stride = (L + 7) // 8 * 8
    if kw.get("max_gap", 3) != 3:
        return "k_traceback_band"
    if sw.get("GM_TRACEBACK") == "group" or stride > 511:
        return "k_traceback"
    # (the value table and the move rows of up to 511 columns fit the LDS of a launch together: the table form unless it is switched off)
    return f"k_traceback_lane<{128 if stride <= 255 else 64}>/" + ("direct" if sw.get("GM_TRACEBACK") == "direct" or fasta else "table")


def _switches(sw):
    for k, v in sw.items():
        g.set_option(k, v)


def _clear(sw):
    for k in sw:
        g.set_option(k, None)


@pytest.mark.parametrize("L", NW_LENS)
@pytest.mark.parametrize("form", list(NW_FORMS))
def test_nw_score_at_every_edge_window(form, L, ix, oracle, oix, genome, capfd):
    sw, kw, fasta = NW_FORMS[form]
    shows = nw_kernel(sw, kw, L)
    sw = dict(sw, GM_TRACE="1")
    pr, o = want(oracle, oix, genome, L, kw.get("max_gap", 3), fasta, False)
    B, Q, Ln = g.pack_reads(pr["reads"], None if fasta else pr["quals"])
    _switches(sw)
    try:
        score, valid = ix.dev_nw_score(g.Params(**kw), B, Q, Ln, pr["ridx"], pr["strand"], pr["pos"], fasta=fasta)
    finally:
        _clear(sw)
    ran = re.findall(r"dev_nw_score: \d+ probes, nw=(\S+)", capfd.readouterr().err)
    assert len(ran) == 1 and re.fullmatch(shows, ran[0]), (ran, shows)            # the library's own word for the kernel it launched
    bad = np.flatnonzero(valid.astype(bool) != o["valid"])
    assert len(bad) == 0, [(int(pr["pos"][k]), int(pr["strand"][k])) for k in bad[:8]]
    got = np.where(o["valid"], score.view(np.uint32), 0)
    bad = np.flatnonzero(got != o["bits"])
    assert len(bad) == 0, [(int(pr["pos"][k]), int(pr["strand"][k]), int(k) % 8, float(score[k]), float(o["bits"][k:k + 1].view(np.float32)[0])) for k in bad[:8]]


def test_wave_form_refuses_fasta_reads_by_name(ix, oracle, oix, genome):
    """k_nw reads FASTQ rows only: GM_NW=wave with FASTA reads is GM_E_UNSUPPORTED naming the switch, not a skipped case of the matrix"""
    pr = probes(oix, genome, 100, True)
    B, _, Ln = g.pack_reads(pr["reads"])
    g.set_option("GM_NW", "wave")
    try:
        with pytest.raises(g.GnumapError) as e:
            ix.dev_nw_score(g.Params(), B, None, Ln, pr["ridx"], pr["strand"], pr["pos"], fasta=True)
    finally:
        g.set_option("GM_NW", None)
    assert e.value.code == GM_E_UNSUPPORTED and "GM_NW=wave" in str(e.value), str(e.value)


@pytest.mark.parametrize("L", TB_LENS)
@pytest.mark.parametrize("form", list(TB_FORMS))
def test_traceback_at_every_edge_window(form, L, ix, oracle, oix, genome, capfd):
    sw, kw, fasta = TB_FORMS[form]
    shows = tb_kernel(sw, kw, L, fasta)
    sw = dict(sw, GM_TRACE="1")
    pr, o = want(oracle, oix, genome, L, kw.get("max_gap", 3), fasta, True)
    B, Q, Ln = g.pack_reads(pr["reads"], None if fasta else pr["quals"])
    _switches(sw)
    try:
        ops = ix.dev_traceback(g.Params(**kw), B, Q, Ln, pr["ridx"], pr["strand"], pr["pos"], fasta=fasta)
    finally:
        _clear(sw)
    ran = re.findall(r"dev_traceback: \d+ probes, traceback=(\S+)", capfd.readouterr().err)
    assert ran == [shows], (ran, shows)
    for k, t in enumerate(o["tb"]):
        where = (int(pr["pos"][k]), int(pr["strand"][k]), k % 8)
        if t is None:
            assert len(ops[k]) == 0, where           # not a window: no operations
        else:
            assert len(ops[k]) == t[0] and rle(ops[k]) == t[1], (where, rle(ops[k]), t[1])


@pytest.mark.parametrize("L", HMM_LENS)
def test_pair_hmm_at_every_edge_window(L, ix, oracle, oix, genome):
    pr, o = want(oracle, oix, genome, L, 3, False, False)
    sel = np.flatnonzero(o["valid"])                 # (the probe takes windows only: it refuses a begin past l_pac as an argument error)
    B, Q, Ln = g.pack_reads(pr["reads"], pr["quals"])
    out = ix.dev_pair_hmm(g.Params(mode=5), B, Q, Ln, pr["ridx"][sel], pr["strand"][sel], pr["pos"][sel])
    for j, k in enumerate(sel):
        P = o["P"][k]
        ref = oracle.pair_hmm(P, argmax_cons(P), o["w"][k])
        assert np.array_equal(out[j, :L].view(np.uint32), ref.view(np.uint32)), (int(pr["pos"][k]), int(pr["strand"][k]), int(k) % 8)
