#!/usr/bin/env python3
"""tools/sam_sort_bench.py — the gather kernel of --sam_sort=coordinate (k_ss_gather, gm_samsort.hip) beside a device-to-device copy of
the same number of bytes, in one process; the numbers quoted in DESIGN.md §4.  Usage:
    python tools/sam_sort_bench.py [--rows 8000000] [--row_bytes 270] [--slab_mb 64] [--genome tests/golden/syn.fa]
Rows of --row_bytes +- 30 bytes with random keys go into a sorter through gm_sam_sorter_add_rows (what they say does not matter to the
kernel), so the sorted order is a random order of the arena, as after a mapping run.  One untimed pass over a first sorter warms the
code objects up; the timed pass reads every slab of a second one.  gather = HIP events around k_ss_spans + k_ss_gather, summed over
the slabs (gm_sam_sorter_stats).  The yardstick is torch's copy of a tensor of the text's size into another one (hipMemcpyDtoD under
it), timed with events: both are larger than the 256 MB Infinity Cache, so it is a copy from and to HBM like the gather."""
import argparse
import os
import sys

import numpy as np
import torch                                    # before libgnumap_hip (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnumap_amd as g                           # noqa: E402
from gnumap_amd import api                       # noqa: E402


def fill(ix, rows, row_bytes, seed):
    s = api.SamSorter(ix)
    rng = np.random.default_rng(seed)
    n_seqs = len(ix.contigs())
    block = 250_000
    for seq, lo in enumerate(range(0, rows, block)):
        n = min(block, rows - lo)
        lens = rng.integers(row_bytes - 30, row_bytes + 31, n).astype(np.uint64)
        off = np.zeros(n + 1, np.uint64); off[1:] = np.cumsum(lens)
        text = np.full(int(off[-1]) + 1, ord("x"), np.uint8)
        text[(off[1:] - 1).astype(np.int64)] = 10
        s.add_rows(seq, (text, off), rng.integers(0, n_seqs, n).astype(np.uint32), rng.integers(1, 100000, n).astype(np.uint64))
    return s


def drain(s, slab):
    buf = np.empty(slab, np.uint8); got = api.u64(); n = 0
    while True:
        api._chk(g.lib().gm_sam_sorter_read(s.h, buf.ctypes.data, slab, api.C.byref(got), None))
        if not got.value:
            return n
        n += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8_000_000)
    ap.add_argument("--row_bytes", type=int, default=270)
    ap.add_argument("--slab_mb", type=int, default=64)
    ap.add_argument("--genome", default=os.path.join(ROOT, "tests", "golden", "syn.fa"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    ix = g.Index(a.genome, device=0, flags=g.GM_INDEX_FULL_SA)
    warm = fill(ix, 200_000, a.row_bytes, 1); warm.finish(); drain(warm, a.slab_mb << 20); warm.destroy()
    s = fill(ix, a.rows, a.row_bytes, 2)
    n_rows, n_bytes = s.finish()
    slabs = drain(s, a.slab_mb << 20)
    st = s.stats()
    assert st["gather_bytes"] == n_bytes
    s.destroy()
    src = torch.randint(0, 255, (n_bytes,), dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    dst.copy_(src); torch.cuda.synchronize()                                    # untimed: first touch
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    copy_ms = sorted(times)[len(times) // 2]
    print(f"sam_sort_bench: {n_rows} rows of {a.row_bytes} +- 30 bytes, {n_bytes} text bytes in {st['pieces']} pieces, {slabs} slabs of {a.slab_mb} MiB; sort {st['sort_s'] * 1e3:.2f} ms")
    print(f"k_ss_spans + k_ss_gather: {st['gather_ms']:.3f} ms = {n_bytes / st['gather_ms'] / 1e6:.1f} GB/s written ({2 * n_bytes / st['gather_ms'] / 1e6:.1f} GB/s moved)")
    print(f"device-to-device copy of {n_bytes} bytes (median of 5: {', '.join('%.3f' % t for t in times)} ms): {copy_ms:.3f} ms = {n_bytes / copy_ms / 1e6:.1f} GB/s written ({2 * n_bytes / copy_ms / 1e6:.1f} GB/s moved)")
    print(f"gather / copy: {copy_ms / st['gather_ms']:.2f} of the copy's rate")
    ix.close()


if __name__ == "__main__":
    main()
