#!/usr/bin/env python3
"""Cost of --snp's SNP-call column on a dense synthetic track: a random reference of --mbp Mbp is indexed, the six --snp tracks are
filled on the device (about --depth x coverage at every position, 0.5 % errors, 1 % heterozygous and 1 % homozygous substitutions), then

  * three runs each of the eight-column path (gm_coverage_download + gm_coverage_download_nuc + gm_coverage_write_gmp) and of
    gm_coverage_write_gmp_calls on the same tracks: wall seconds, bytes written;
  * the same number of runs of gm_coverage_write_gmp_calls_device (the nine-column file formatted on the device), alternating with the
    host writer: wall seconds, kernel_ms of gm_coverage_text_stats, and whether the two files are the same bytes;
  * gm_snp_calls: wall seconds, records.

    python3 tools/snp_call_bench.py --mbp 25
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/snp_call_bench.py --mbp 25 --calls-only     # k_snp_call's own time, a run of its own

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def same_file(a, b, piece=64 << 20):
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x = fa.read(piece)
            if x != fb.read(piece):
                return False
            if not x:
                return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, default=25)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls-only", action="store_true", help="gm_snp_calls alone (for a kernel trace)")
    a = ap.parse_args()
    import torch
    import gnumap_amd as g
    from gnumap_amd import dist as gd
    from scale_check import write_genome
    L = g.lib()
    work = tempfile.mkdtemp(prefix="snpcall_")
    fa = os.path.join(work, "g.fa")
    write_genome(fa, a.mbp * 1_000_000, 4, 1)
    t0 = time.time(); g.index_build(fa); t_build = time.time() - t0
    ix = g.Index(fa, flags=g.GM_INDEX_FULL_SA)
    ix.coverage_reset(1); ix.coverage_enable_nuc()
    bins = ix.coverage_bins(); l_pac = int(ix.info.l_pac)
    dev = torch.device("cuda", 0)
    cov = gd.DeviceTrack(ix.coverage_device_ptr(), bins).tensor(dev)
    nuc = gd.DeviceTrack(ix.coverage_nuc_device_ptr(), 5 * bins).tensor(dev).view(5, bins)
    gen = torch.Generator(device=dev); gen.manual_seed(5)
    depth = a.depth * (0.6 + 0.8 * torch.rand(bins, device=dev, generator=gen))
    code = np.zeros(256, np.int64); code[list(b"ACGT")] = [0, 1, 2, 3]
    ref = np.zeros(bins, np.int64)
    ref[:l_pac] = code[np.frombuffer(b"".join(l.strip() for l in open(fa, "rb") if not l.startswith(b">")), np.uint8)]
    ref = torch.from_numpy(ref).to(dev)
    other = (ref + 1 + torch.randint(0, 3, (bins,), device=dev, generator=gen)) % 4
    kind = torch.rand(bins, device=dev, generator=gen)
    first = torch.where(kind < 0.01, other, ref)                        # 1 % homozygous substitutions
    second = torch.where(kind < 0.01, ref, other)
    share2 = torch.where((kind >= 0.01) & (kind < 0.02), 0.4 + 0.2 * torch.rand(bins, device=dev, generator=gen), torch.full((bins,), 0.005, device=dev))
    nuc.zero_()
    nuc.scatter_(0, first[None, :], (depth * (1 - share2))[None, :])
    nuc.scatter_add_(0, second[None, :], (depth * share2)[None, :])
    cov.copy_(nuc.sum(0))
    torch.cuda.synchronize()
    res = dict(mbp=a.mbp, positions=l_pac, depth=a.depth, index_build_s=round(t_build, 2))
    t0 = time.time(); calls = ix.snp_calls(); res["snp_calls_s"] = round(time.time() - t0, 4); res["snp_calls_records"] = int(len(calls))
    t0 = time.time(); calls = ix.snp_calls(); res["snp_calls_second_s"] = round(time.time() - t0, 4)
    if not a.calls_only:
        p5 = g.Params(mode=5)
        out = os.path.join(work, "t.gmp")
        eight, nine, nine_dev, nine_dev_kernel_ms = [], [], [], []
        out_dev = os.path.join(work, "t_dev.gmp")
        for _ in range(a.runs):
            t0 = time.time()
            h_cov = ix.coverage_download(); h_nuc = ix.coverage_download_nuc()
            assert L.gm_coverage_write_gmp(ix.h, C.byref(p5.c), h_cov.ctypes.data, h_nuc.ctypes.data, out.encode(), 0) == 0
            eight.append(round(time.time() - t0, 3)); res["eight_column_bytes"] = os.path.getsize(out)
            del h_cov, h_nuc
            t0 = time.time()
            ix.coverage_write_gmp_calls(out)
            nine.append(round(time.time() - t0, 3)); res["nine_column_bytes"] = os.path.getsize(out)
            t0 = time.time()
            ix.coverage_write_gmp_calls_device(out_dev)
            nine_dev.append(round(time.time() - t0, 3)); st = ix.coverage_text_stats()
            nine_dev_kernel_ms.append(round(st["kernel_ms"], 3)); res["nine_column_device_stats"] = {k: st[k] for k in ("rows", "bytes", "slabs", "host_slabs", "launches")}
        res["nine_column_device_same_bytes"] = same_file(out, out_dev)
        os.remove(out); os.remove(out_dev)
        res["nine_column_write_gmp_calls_device_s"] = nine_dev; res["nine_column_device_kernel_ms"] = nine_dev_kernel_ms
        res["eight_column_download_and_write_s"] = eight; res["nine_column_write_gmp_calls_s"] = nine
    ix.close()
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    os.rmdir(work)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
