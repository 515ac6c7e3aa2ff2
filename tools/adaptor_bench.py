#!/usr/bin/env python3
"""Cost of -A / --adaptor's trim kernel: --reads random reads of --len bases (default 10 M x 100 bp), a 34-character adaptor written over
the tail (5 .. 60 bases) of --frac of them (default 30 %), resident in HBM after the upload's copies.

  * k_adaptor_trim: HIP events around the kernel inside gm_batch_upload (gm_batch_adaptor_time, profiling on), --runs uploads after one
    warm-up: ms per block, bytes read (bases of every read + its length) divided by the time;
  * k_prep_rows from the same process, same block, for comparison (gm_batch_kernel_times, GM_K_PREP): once on the batch without an
    adaptor - the yardstick - and once with it (shorter, mixed lengths).

    python3 tools/adaptor_bench.py
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/adaptor_bench.py --runs 2     # the kernels' own times, a run of its own

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ADAPTOR = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"


def make_reads(n, L, frac, seed):
    rng = np.random.default_rng(seed)
    stride = (L + 7) // 8 * 8
    B = np.zeros((n, stride), np.uint8)
    B[:, :L] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, L), dtype=np.uint8)]
    Q = np.zeros((n, stride), np.uint8)
    Q[:, :L] = 33 + 30
    tail = np.where(rng.random(n) < frac, rng.integers(5, min(61, L - 4), n), 0)
    text = np.frombuffer(ADAPTOR, np.uint8)
    for t in np.unique(tail[tail > 0]):
        rows = np.flatnonzero(tail == t)
        k = min(int(t), len(text))
        B[rows, L - int(t):L - int(t) + k] = text[:k]
    return B, Q, np.full(n, L, np.uint16), tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--frac", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--genome", default=os.path.join(ROOT, "tests", "golden", "syn.fa"))
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as in bench.py)
    import gnumap_amd as g
    B, Q, Ln, tail = make_reads(a.reads, a.len, a.frac, 1)
    ix = g.Index(a.genome, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    batch = g.Batch(ix, a.reads, B.shape[1])
    batch.set_profiling(True)

    def prep_ms():
        batch.kernel_times()
        ms = []
        for _ in range(a.runs + 1):
            batch.map_device(p)
            t = batch.kernel_times()["k_prep"]
            ms.append(t[0] / max(1, t[1]))
        return ms[1:]

    batch.upload(p, B, Q, Ln)
    prep_plain = prep_ms()
    batch.set_adaptor(ADAPTOR)
    trim = []
    for _ in range(a.runs + 1):
        batch.upload(p, B, Q, Ln)
        ms, launches = batch.adaptor_time()
        assert launches == 1
        trim.append(ms)
    trim = trim[1:]
    J = batch.trimmed_len()
    prep_trimmed = prep_ms()
    read_bytes = a.reads * (a.len + 2)
    med = float(np.median(trim))
    out = dict(reads=a.reads, read_len=a.len, adaptor_len=len(ADAPTOR), adaptor_fraction=a.frac, runs=a.runs,
               k_adaptor_trim_ms=[round(x, 4) for x in trim], k_adaptor_trim_ms_median=round(med, 4),
               k_adaptor_trim_ms_per_10M_reads=round(med * 1e7 / a.reads, 4), bytes_read=read_bytes, GB_per_s=round(read_bytes / med / 1e6, 1),
               k_prep_rows_ms_no_adaptor=[round(x, 4) for x in prep_plain], k_prep_rows_ms_no_adaptor_median=round(float(np.median(prep_plain)), 4),
               k_prep_rows_ms_trimmed_block_median=round(float(np.median(prep_trimmed)), 4),
               ratio_to_k_prep_rows=round(med / float(np.median(prep_plain)), 2),
               kept_mean=round(float(J.mean()), 2), reads_cut_by_more_than_4=int((a.len - J.astype(np.int64) > 4).sum()), path=batch.path())
    print(json.dumps(out))
    batch.destroy(); ix.close()


if __name__ == "__main__":
    main()
