"""-A / --adaptor: the length a read keeps, restated in numpy float32 (the reference: SeqReader::FixReads2 with SeqReader::Compare,
src/SeqReader.cpp:1294-1305, 1356-1372).  Pinned to the reference PROGRAM by tests/test_adaptor_cpu.py: for every record of the
fixtures under tests/golden/ref_runs_adaptor/ the CIGAR's M + I count is this function's value for the record's read."""
import re

import numpy as np


def kept_length(seq, adaptor):
    """J = the smallest offset i in [0, L - 4) with (float)same / j >= 0.85f over j = min(|adaptor|, L - i) raw characters from i on,
    else L - 4; 0 for reads of fewer than 4 bases (where the reference's unsigned bound wraps)"""
    s = np.frombuffer(bytes(seq), np.uint8); a = np.frombuffer(bytes(adaptor), np.uint8)
    L, A = len(s), len(a)
    if A == 0:
        return L
    if L <= 4:
        return 0
    n_off = L - 4
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([s, np.zeros(A, np.uint8)]), A)[:n_off]
    left = (L - np.arange(n_off))[:, None]                              # characters of the read from offset i on
    same = ((win == a[None, :]) & (np.arange(A)[None, :] < left)).sum(1)
    j = np.minimum(A, left[:, 0])
    ok = same.astype(np.float32) / j.astype(np.float32) >= np.float32(0.85)   # an IEEE fp32 division, then the compare
    hit = np.flatnonzero(ok)
    return int(hit[0]) if len(hit) else n_off


def kept_lengths(seqs, adaptor):
    return np.array([kept_length(s, adaptor) for s in seqs], np.uint16)


def cigar_read_length(cigar):
    """bases of the read a CIGAR accounts for (M and I operations)"""
    return sum(int(n) for n, op in re.findall(r"(\d+)([MID])", cigar) if op in "MI")
