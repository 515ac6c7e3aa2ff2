"""The "%.2e" writer the device uses for the p-value of --snp's ninth .gmp column (gm_put_e2_hd, gnumap_amd/csrc/gm_fmt_dev.h), compiled
for the host (the __host__ __device__ markers defined away), against the C library's printf on 8 M values (tests/fmt_e2_check.cpp):
log-uniform doubles over the domain 2^-200 <= v < 2^200; k * 2^-53 for k = 1 .. 10^6 and random k < 2^53 (what 1 - P can be); every
decimal tie candidate d.dd5e+-XX with its two neighbours in ulps; the 9.995 / 9.994999 carries; exactly representable ties (1.125,
1.375, 2^-k); powers of ten from 1e-60 to 1e60 with neighbours; 0.0.  Inside the domain the text is always 8 characters; outside it
(negative, -0.0, nan, inf, denormals, the far ends, random bit patterns) the length must be 0 and no byte written."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_put_e2_hd_equals_printf(tmp_path):
    exe = tmp_path / "fmt_e2_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__host__=", "-D__device__=", "-I", os.path.join(ROOT, "gnumap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fmt_e2_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert " 0 mismatches" in r.stdout
    n = int(r.stdout.split()[0])
    outside = int(r.stdout.split("(")[1].split()[0])
    assert n > 5_000_000 and outside > 1_000_000, r.stdout
