"""numpy model of the reference's FASTA reader and of what a SAM row prints of a FASTA read (tests only):

    records   SeqReader::get_more_fasta (src/SeqReader.cpp:813-1018): a record runs from one '>' line to the next; the name is the
              WHOLE header line after '>' (spaces included); the sequence lines are joined
    rows      :875-979, cast to float at :996 - a c g t one 1.0; r y k m s w two 0.5; b d h v three (float)(1.0 / 3.0); n four 0.25
    QUAL      str2qual (inc/SequenceOperations.h:193-217): one character per position from the row's largest entry
    SEQ       the file's letters; on the minus strand reverse_comp (inc/SequenceOperations.h:56-96): every letter outside ACGTacgt -> 'n'

Pinned to the reference program's own output by tests/test_fasta_reads_cpu.py (every row of tests/golden/ref_runs_fasta/)."""
import math

import numpy as np

# letter -> bases of its row, in the reference's column order a c g t
IUPAC = {"a": "a", "c": "c", "g": "g", "t": "t", "r": "ag", "y": "ct", "k": "gt", "m": "ac", "s": "cg", "w": "at",
         "b": "cgt", "d": "agt", "h": "act", "v": "acg", "n": "acgt"}
AMBIGUITY = "rykmswbdhv"
_SHARE = {1: 1.0, 2: 0.5, 3: 1.0 / 3.0, 4: 0.25}          # the reference's fp64 constants


def base_mask(ch: int) -> int:
    """4-bit base mask of a sequence character (bit 0 = A .. bit 3 = T); 0 for a byte that is none of the 15 letters"""
    bases = IUPAC.get(chr(ch).lower(), "")
    return sum(1 << "acgt".index(b) for b in bases)


def mask_rc(m: int) -> int:
    """the mask of reverse_comp_cpy's row (inc/SequenceOperations.h:149-161): A<->T, C<->G"""
    return ((m & 1) << 3) | ((m & 2) << 1) | ((m & 4) >> 1) | ((m & 8) >> 3)


def parse_fasta(data: bytes):
    """[(name, sequence)] of a FASTA text"""
    recs = []
    name, parts = None, []
    for line in data.split(b"\n"):
        if line.startswith(b">"):
            if name is not None:
                recs.append((name, b"".join(parts)))
            name, parts = line[1:], []
        elif name is not None:
            parts.append(line)
    if name is not None:
        recs.append((name, b"".join(parts)))
    return recs


def pwm_rows(seq: bytes) -> np.ndarray:
    """float32 (L, 4) rows of a sequence"""
    P = np.zeros((len(seq), 4), np.float32)
    for i, ch in enumerate(seq):
        bases = IUPAC[chr(ch).lower()]
        for b in bases:
            P[i, "acgt".index(b)] = np.float32(_SHARE[len(bases)])
    return P


def qual_char(pmax) -> int:
    """str2qual's character of a row whose largest entry is the float pmax"""
    MAX_PRB = 0.9999
    if float(pmax) > MAX_PRB:
        return int((-10 * math.log(1 - MAX_PRB) / math.log(10.)) + 33)
    return int((-10 * math.log(float(np.float32(1) - np.float32(pmax))) / math.log(10)) + 33)


def synth_qual(seq: bytes) -> bytes:
    P = pwm_rows(seq)
    return bytes(qual_char(P[i].max()) for i in range(len(seq)))


_COMP = {ord(a): ord(b) for a, b in zip("acgtACGT-", "tgcaTGCA-")}


def revcomp_seq(seq: bytes) -> bytes:
    return bytes(_COMP.get(ch, ord("n")) for ch in reversed(seq))


def sam_seq_qual(seq: bytes, minus: bool):
    """(SEQ, QUAL) columns of a SAM row of this read"""
    q = synth_qual(seq)
    return (revcomp_seq(seq), q[::-1]) if minus else (seq, q)
