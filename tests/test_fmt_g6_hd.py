"""The "%g" writer the device uses for the XA / XP columns (gnumap_amd/csrc/gm_fmt_dev.h), compiled for the host (the __host__
__device__ markers defined away), against the C library's printf on 17 M values: the families of fmt_g6_check.cpp, every power of ten
from 1e-60 to 1e60 with both neighbours, exact sixth-digit ties in exponent form, floats widened to double over the whole float exponent
range (denormals included) and times 1/0.25 and 1/1.0, +-0, +-inf, +-nan; the two edges of the domain 2^-200 <= |v| < 2^200, and values
outside it, which must give length 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_put_g6_hd_equals_printf(tmp_path):
    exe = tmp_path / "fmt_g6_hd_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__host__=", "-D__device__=", "-I", os.path.join(ROOT, "gnumap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fmt_g6_hd_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert " 0 mismatches" in r.stdout
    n = int(r.stdout.split()[0])
    assert n > 5_000_000, r.stdout
