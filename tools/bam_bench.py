#!/usr/bin/env python3
"""tools/bam_bench.py — the BAM kernels of --sam_format=bam (k_bam_sizes / k_bam_rows and k_bgzf_deflate / k_bgzf_compact, gm_bam.hip)
beside a device-to-device copy of the same number of bytes, in one process; the numbers quoted in DESIGN.md.  Usage:
    python tools/bam_bench.py [--copies 400] [--iters 5] [--genome tests/golden/syn.fa] [--reads tests/golden/syn.fq]
The reads of --reads, --copies times over under names of their own, are mapped as ONE block; gm_output_batch_bam then writes that block's
records and compresses them, --iters times per form (level 0, level 1, level 1 with LZ77 matches) after one untimed call, with gm_batch_set_profiling on: HIP events around the record
kernels and around the BGZF kernels (gm_batch_bam_times).  GB/s are bytes of records (the BGZF kernels' payload) per second of kernel
time; every form's BGZF bytes are named by their SHA-256 (the bytes are a function of the input and the level: a digest to hold a
change of the kernels against); the matched form's output is also put beside zlib's Z_HUFFMAN_ONLY and level 1 on the same payloads.  The yardstick is torch's copy of a tensor of the records' size into another one, timed with events."""
import argparse
import gzip
import hashlib
import os
import sys
import zlib

import numpy as np
import torch                                    # before libgnumap_hip (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gnumap_amd as g                           # noqa: E402
from conftest import read_fastq                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=400)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--genome", default=os.path.join(ROOT, "tests", "golden", "syn.fa"))
    ap.add_argument("--reads", default=os.path.join(ROOT, "tests", "golden", "syn.fq"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    ix = g.Index(a.genome, device=0, flags=g.GM_INDEX_FULL_SA)
    p = g.Params()
    rd = read_fastq(a.reads)
    names = [f"{r[0]}/{c}".encode() for c in range(a.copies) for r in rd]
    seqs = [r[1] for r in rd] * a.copies
    quals = [r[2][:len(r[1])] for r in rd] * a.copies
    B, Q, Ln = g.pack_reads(seqs, quals)
    batch = g.Batch(ix, len(seqs), B.shape[1])
    ix.coverage_reset(8)
    res = batch.map(p, B, Q, Ln)
    print(f"bam_bench: {len(seqs)} reads ({a.copies} x {len(rd)}), stride {B.shape[1]}")
    raw = 0
    for level, lz77 in ((0, False), (1, False), (1, True)):
        out = batch.output_bam(p, res, names, level=level, lz77=lz77)           # untimed: code objects, buffers
        raw = batch.bam_raw_len
        batch.set_profiling(True)
        batch.bam_times()
        for _ in range(a.iters):
            out = batch.output_bam(p, res, names, level=level, lz77=lz77, bam_cap=len(out) + 64)
        t = batch.bam_times()
        batch.set_profiling(False)
        assert t["raw_bytes"] == a.iters * raw and t["bgzf_in"] == a.iters * raw and t["bgzf_out"] == a.iters * len(out)
        rows_ms, bgzf_ms = t["rows_ms"] / a.iters, t["bgzf_ms"] / a.iters
        print(f"level {level}{' + lz77' if lz77 else ''}: {batch.bam_n_recs} records, {raw} bytes -> {len(out)} bytes of BGZF ({100.0 * len(out) / raw:.1f} %)")
        print(f"  k_bam_sizes + k_bam_rows: {rows_ms:.3f} ms = {raw / rows_ms / 1e6:.1f} GB/s of records written")
        print(f"  k_bgzf_deflate{'_lz' if lz77 else ''} + scan + k_bgzf_compact: {bgzf_ms:.3f} ms = {raw / bgzf_ms / 1e6:.1f} GB/s of payload")
        print(f"  sha256 of the BGZF bytes: {hashlib.sha256(out).hexdigest()}")
    payload = gzip.decompress(out)                                              # (the matched form's, the last one written)
    assert len(payload) == raw
    huff = z1 = 0
    for at in range(0, raw, 65280):
        for strategy in (zlib.Z_HUFFMAN_ONLY, zlib.Z_DEFAULT_STRATEGY):
            c = zlib.compressobj(1, zlib.DEFLATED, -15, 9, strategy)
            size = len(c.compress(payload[at:at + 65280]) + c.flush()) + 26
            huff, z1 = (huff + size, z1) if strategy == zlib.Z_HUFFMAN_ONLY else (huff, z1 + size)
    print(f"the same payloads through zlib, 26 bytes of BGZF around each: Z_HUFFMAN_ONLY {100.0 * huff / raw:.1f} %, level 1 {100.0 * z1 / raw:.1f} %")
    src = torch.randint(0, 255, (raw,), dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    dst.copy_(src); torch.cuda.synchronize()                                    # untimed: first touch
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    copy_ms = sorted(times)[len(times) // 2]
    print(f"device-to-device copy of {raw} bytes (median of 5: {', '.join('%.3f' % t for t in times)} ms): {copy_ms:.3f} ms = {raw / copy_ms / 1e6:.1f} GB/s written")
    batch.destroy(); ix.close()


if __name__ == "__main__":
    main()
