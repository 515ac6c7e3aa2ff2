#!/usr/bin/env python3
"""BUILD CONTAINER ONLY (needs the reference tree).  Fixtures that pin the likelihood-ratio column of --snp's .gmp
(GenomeBwt::PrintSNPCall, src/GenomeBwt.cpp:1011-1090) to the UNMODIFIED reference, with the reference's own GSL.

In a temporary directory this script
  1. unpacks and builds the reference's vendored lib/gsl-1.9.tar.gz (./configure --disable-shared && make -j16, offline; GSL_PREFIX=<dir>
     reuses an installed build of that tarball instead),
  2. compiles the unmodified reference sources against it with the flags of oracle/Makefile (BIN_FLAGS / CFLAGS_REF) - the program, and a
     small harness of our own that includes src/GenomeBwt.cpp and calls GenomeBwt::is_snp as GenomeBwt::Test does (:1297-1340),
  3. writes
       ref_vectors_snpcall.npz   is_snp on a seeded set of count vectors, both ploidy settings; inputs and p-values as raw bits.  The five
                                 floats are elements 1..5 of a six-float buffer whose element 0 is 0.0f: the forced-monoploid case reads
                                 chars[-1] (:857), which so has a defined value
       syn_snp.fq                100-bp reads simulated from syn.fa: five stretches at about 30x, 15x, 10x, 6x and 3x with planted homozygous
                                 and heterozygous substitutions, 0.5 % errors
       ref_runs_snp/<name>.gmp.gz (+ .sam.gz)   the reference program's nine-column .gmp for --snp, --snp --snp_monop and
                                 --snp --snp_pval=0.05 on syn_snp.fq, and for --snp on syn.fq
  4. measures and prints the tolerances tests/snpcall_model.py carries as named constants (restatement against the reference function;
     sensitivity of the p-value to the fp32 allowance of the deposited sums).
Everything committed is DATA; the harness text below is our own and is compiled outside the repository."""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import snpcall_model as M          # noqa: E402

REF = os.environ.get("GNUMAP_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "ref_runs_snp")
REF_C = "bwt bntseq utils bwtindex bwt_gen is QSufSort".split()
BIN_CXX = "Driver GenomeBwt Genome centers Reader NormalScoredSeq BSScoredSeq SNPScoredSeq bin_seq SeqReader".split()
BIN_FLAGS = "-DDEBUG_NW -DDEBUG_TIME -m64 -O3 -w -std=c++0x".split()
CFLAGS_REF = "-m64 -O3 -fPIC -w".split()

HARNESS = r"""
#include "const_define.h"
#include "GenomeBwt.cpp"
// stdin: int32 n, then n x { int32 monop, float[5] }; stdout: n x { double p, int32 pos1, int32 pos2, int32 dip }
int main() {
    GenomeBwt* g = new GenomeBwt();
    int n;
    if (fread(&n, 4, 1, stdin) != 1) return 1;
    for (int k = 0; k < n; ++k) {
        int monop; float buf[6];
        buf[0] = 0.0f;
        if (fread(&monop, 4, 1, stdin) != 1 || fread(buf + 1, 4, 5, stdin) != 5) return 1;
        gSNP_MONOP = monop != 0;
        int i = -9, j = -9; bool b = false;
        double p = g->is_snp(buf + 1, i, j, b);
        int d = b ? 1 : 0;
        fwrite(&p, 8, 1, stdout); fwrite(&i, 4, 1, stdout); fwrite(&j, 4, 1, stdout); fwrite(&d, 4, 1, stdout);
    }
    fflush(stdout);
    _exit(0);
}
"""


def run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert r.returncode == 0, (cmd, r.stdout[-1500:], r.stderr[-3000:])
    return r


def build(work):
    gsl = os.environ.get("GSL_PREFIX")
    if not gsl:
        run(["tar", "-xzf", os.path.join(REF, "lib", "gsl-1.9.tar.gz"), "-C", work])
        gsl = os.path.join(work, "gsl")
        src = os.path.join(work, "gsl-1.9")
        run(["./configure", "--disable-shared", "--prefix=" + gsl], cwd=src)
        run(["make", "-j16"], cwd=src)
        run(["make", "install"], cwd=src)
    inc = ["-I" + os.path.join(REF, "inc"), "-I" + os.path.join(gsl, "include")]
    obj = os.path.join(work, "obj"); os.makedirs(obj)
    procs = []
    for f in REF_C:
        procs.append(subprocess.Popen(["gcc"] + CFLAGS_REF + inc + ["-c", os.path.join(REF, "src", f + ".c"), "-o", os.path.join(obj, f + ".o")]))
    for f in BIN_CXX:
        procs.append(subprocess.Popen(["g++"] + BIN_FLAGS + inc + ["-c", os.path.join(REF, "src", f + ".cpp"), "-o", os.path.join(obj, "bin_" + f + ".o")]))
    open(os.path.join(work, "harness.cpp"), "w").write(HARNESS)
    procs.append(subprocess.Popen(["g++"] + BIN_FLAGS + inc + ["-I" + os.path.join(REF, "src"), "-c", os.path.join(work, "harness.cpp"), "-o", os.path.join(obj, "harness.o")]))
    for p in procs:
        assert p.wait() == 0
    libs = [os.path.join(gsl, "lib", "libgsl.a"), os.path.join(gsl, "lib", "libgslcblas.a"), "-lz", "-lm", "-lpthread"]
    c_objs = [os.path.join(obj, f + ".o") for f in REF_C]
    exe = os.path.join(work, "gnumap_ref_gsl"); har = os.path.join(work, "is_snp_harness")
    run(["g++", "-rdynamic", "-o", exe] + [os.path.join(obj, "bin_" + f + ".o") for f in BIN_CXX] + c_objs + libs)
    run(["g++", "-rdynamic", "-o", har, os.path.join(obj, "harness.o")] + [os.path.join(obj, "bin_" + f + ".o") for f in BIN_CXX if f not in ("Driver", "GenomeBwt")] + c_objs + libs)
    return exe, har


# ---- count vectors ---------------------------------------------------------------------------------------------------------------------
def vectors():
    rng = np.random.default_rng(20)
    V = []
    # the vectors of GenomeBwt::Test (:1297-1340)
    V += [[0, 0.000001, 0.008909, 0, 0], [0, 0.00172, 0, 7.44906, 0], [0.00084, 5.76128, 0.99737, 0.00077, 0], [0, 1.19790, 0.67151, 9.79130, 0],
          [9.32711, 0.57861, 25.21611, 0.00566, 0], [0.00003, 0.00799, 31.70140, 8.83931, 0], [2.21139, 205.58350, 216.35576, 3.84918, 0],
          [0.07155, 194.00175, 201.30124, 11.62545, 0], [0, 0, 0, 0, 0]]
    def mix(total, shares, noise):
        v = np.array(shares, float) * total
        v = v * (1 + noise * rng.standard_normal(5)).clip(0.1)
        return list(v[rng.permutation(5)] if rng.random() < 0.5 else v)
    for total in np.exp(rng.uniform(np.log(0.002), np.log(400), 220)):                       # totals from 0.002 to 400, any composition
        V.append(list(rng.dirichlet(np.full(5, 0.3)) * total))
    for total in np.exp(rng.uniform(np.log(0.5), np.log(400), 120)):                         # clean homozygous
        e = rng.uniform(0, 0.02)
        V.append(mix(total, [1 - e, e / 2, e / 4, e / 4, 0], 0.05))
    for total in np.exp(rng.uniform(np.log(1), np.log(400), 120)):                           # 50 / 50 and 70 / 30
        V.append(mix(total, [0.5, 0.49, 0.005, 0.005, 0], 0.1))
        V.append(mix(total, [0.7, 0.29, 0.005, 0.005, 0], 0.05))
    for total in np.exp(rng.uniform(np.log(1), np.log(300), 60)):                            # ratios just either side of 3.0
        for eps in (-1e-3, -1e-5, 1e-5, 1e-3):
            c2 = total / 4.1
            V.append([0.01 * total, c2 * 3 * (1 + eps), 0, c2, 0.002])
    for total in np.exp(rng.uniform(np.log(0.01), np.log(200), 40)):                         # ties between maxima
        a = np.float32(total / 2.2)
        V.append([a, a, 0.1 * total, 0, 0]); V.append([0, a, 0, a, a]); V.append([a, 0.2 * a, a, 0, 0.2 * a])
    for total in np.exp(rng.uniform(np.log(0.1), np.log(200), 30)):                          # n-dominated
        V.append([0.05 * total, 0.02 * total, 0.01 * total, 0.02 * total, 0.9 * total])
        V.append([0.3 * total, 0.02 * total, 0.01 * total, 0.02 * total, 0.65 * total])
    for x in np.linspace(60, 80, 81):                                                         # x = -2 log(ratio) across the cancellation zone
        t = x / (2 * np.log(5))
        V.append([0, 0, t, 0, 0]); V.append([0.004 * t, 0, 0, t, 0])
        V.append([0.55 * t * 1.4, 0.45 * t * 1.4, 0, 0.01, 0]); V.append([0, 0.01, 0.6 * t * 1.7, 0, 0.4 * t * 1.7])
    V = np.asarray(V, np.float64)
    tot = V.sum(1, keepdims=True)
    V = np.where(tot > 399.0, V * (399.0 / np.maximum(tot, 1e-30)), V)                       # parity is claimed up to a total of 400
    return np.asarray(V, np.float32)


def run_harness(har, V):
    blob = bytearray(np.int32(2 * len(V)).tobytes())
    for monop in (0, 1):
        for v in V:
            blob += np.int32(monop).tobytes() + v.tobytes()
    r = subprocess.run([har], input=bytes(blob), capture_output=True)
    assert r.returncode == 0 and len(r.stdout) == 2 * len(V) * 20, (r.returncode, len(r.stdout), r.stderr[-2000:])
    rec = np.frombuffer(r.stdout, np.dtype([("p", "<u8"), ("pos1", "<i4"), ("pos2", "<i4"), ("dip", "<i4")]))
    return rec[:len(V)], rec[len(V):]


# ---- reads -----------------------------------------------------------------------------------------------------------------------------
STRETCHES = [("chrA", 20000, 600, 30), ("chrA", 90000, 1000, 15), ("chrB", 40000, 1500, 10), ("chrC", 12000, 1500, 6),
             ("chrB", 70000, 1500, 3)]   # contig, start, length, depth


def read_fasta(path):
    seqs, name = {}, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].split()[0]; seqs[name] = []
        else:
            seqs[name].append(line.strip())
    return {k: "".join(v) for k, v in seqs.items()}


def simulate(fa, dst):
    rng = np.random.default_rng(31)
    genome = read_fasta(fa)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    out, planted = [], []
    for si, (contig, start, length, depth) in enumerate(STRETCHES):
        ref = genome[contig][start:start + length].upper()
        hap = [list(ref), list(ref)]
        for k, pos in enumerate(range(30, length - 30, 50)):
            alt = "ACGT"[("ACGT".index(ref[pos]) + 1 + int(rng.integers(3))) % 4]
            hap[0][pos] = alt
            if k % 2 == 0:
                hap[1][pos] = alt                                         # homozygous; odd k: heterozygous
            planted.append((contig, start + pos + 1, ref[pos], alt, k % 2 == 0))
        for r in range(depth * length // 100):
            b = int(rng.integers(0, length - 100 + 1))
            s = hap[int(rng.integers(2))][b:b + 100]
            s = [c if rng.random() >= 0.005 else "ACGT"[int(rng.integers(4))] for c in s]
            if rng.random() < 0.5:
                s = [comp[c] for c in reversed(s)]
            out.append("@s%d_%d\n%s\n+\n%s\n" % (si, r, "".join(s), "I" * 100))
    open(dst, "w").write("".join(out))
    return planted


RUNS = {"snp": (["--snp"], "syn_snp.fq", 0.001, False), "snp_monop": (["--snp", "--snp_monop"], "syn_snp.fq", 0.001, True),
        "snp_pval05": (["--snp", "--snp_pval=0.05"], "syn_snp.fq", 0.05, False), "snp_synfq": (["--snp"], "syn.fq", 0.001, False)}


def gz_write(path, data):
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(data)


def main():
    work = tempfile.mkdtemp()
    exe, har = build(work)
    # ---- vectors ----
    V = vectors()
    dip_rec, mono_rec = run_harness(har, V)
    np.savez_compressed(os.path.join(HERE, "ref_vectors_snpcall.npz"), counts=V.view(np.uint32), p_dip=dip_rec["p"], pos1_dip=dip_rec["pos1"].astype(np.int8),
                        pos2_dip=dip_rec["pos2"].astype(np.int8), dip=dip_rec["dip"].astype(np.uint8), p_monop=mono_rec["p"], pos1_monop=mono_rec["pos1"].astype(np.int8))
    worst_rel = worst_abs = 0.0; letters = skipped = 0
    for rec, monop in ((dip_rec, False), (mono_rec, True)):
        for v, r in zip(V, rec):
            p_ref = float(np.uint64(r["p"]).view(np.float64))
            p, p1, p2, dip = M.is_snp(v, monop)
            # the reference leaves snp_pos2 = -1 in the forced case and does not touch it with --snp_monop
            same = p1 == r["pos1"] and bool(dip) == bool(r["dip"]) and (monop or p2 == r["pos2"])
            if not same:
                assert M.on_decision_point(v, p_ref, 0.001, monop, 1e-9, 1e-15), (v, monop, (p, p1, p2, dip), r)
                skipped += 1
                continue
            letters += 1
            worst_abs = max(worst_abs, abs(p - p_ref))
            if p_ref > 1e-9:
                worst_rel = max(worst_rel, abs(p - p_ref) / p_ref)
    print(f"{len(V)} vectors x 2 ploidy settings; restatement vs reference function: MEASURED_REL = {worst_rel:.2e}  MEASURED_ABS = {worst_abs:.2e}; "
          f"{skipped} rows on a decision point left out of {letters + skipped}")
    assert skipped <= M.MAX_SKIPPED_SHARE * (letters + skipped)
    # ---- runs ----
    os.makedirs(OUT, exist_ok=True)
    planted = simulate(os.path.join(HERE, "syn.fa"), os.path.join(HERE, "syn_snp.fq"))
    for f in os.listdir(HERE):
        if f.startswith("syn"):
            shutil.copy(os.path.join(HERE, f), work)
    manifest = {}
    track_rel = 0.0
    for name, (args, fq, cut, monop) in RUNS.items():
        run([exe, "-g", "syn.fa", "-o", name, "-a", "0.9"] + args + [fq], cwd=work)
        gmp = open(os.path.join(work, name + ".gmp"), "rb").read()
        sam = b"".join(l for l in open(os.path.join(work, name + ".sam"), "rb") if not l.startswith(b"@PG"))
        gz_write(os.path.join(OUT, name + ".gmp.gz"), gmp)
        if name == "snp":
            gz_write(os.path.join(OUT, name + ".sam.gz"), sam)
        elif fq == "syn_snp.fq":
            assert sam == gzip.open(os.path.join(OUT, "snp.sam.gz"), "rb").read()          # these flags change the ninth column only
        else:
            assert sam == gzip.open(os.path.join(HERE, "ref_runs", "default.sam.gz"), "rb").read()     # --snp does not change the mapping
        rows = [l.split("\t") for l in gmp.decode().splitlines()]
        assert all(len(r) == 9 for r in rows)
        calls = [(r, M.parse_call(r[8])) for r in rows if r[8] != "N"]
        n_y = sum(1 for _, c in calls if c[0][0] == "Y"); n_ydip = sum(1 for _, c in calls if c[0][0] == "Y" and c[0][3]); n_n = len(calls) - n_y
        mid = sum(1 for _, c in calls if c[0][0] == "Y" and 1e-10 < c[1] < cut)
        top = max(float(r[2]) for r in rows)
        print(f"{name:12s} {len(rows):6d} rows, {len(calls)} with a call: {n_y} Y ({n_ydip} diploid, {mid} with 1e-10 < p < cutoff), {n_n} N:, largest total {top:.1f}")
        if fq == "syn_snp.fq":
            assert mid >= 20 and n_n >= 20 and top < 400, name
            assert n_y - n_ydip >= 1 and (monop or n_ydip >= 1)
        # sensitivity of the p-value to compare_tracks' allowance on the sums (1e-4 relative + 2e-5), restatement on the printed counts
        for r, c in calls:
            cnt = np.array([float(x) for x in r[3:8]], np.float32)
            p0, a0, b0, d0 = M.is_snp(cnt, monop)
            if not p0 > M.P_FLOOR:
                continue
            for bits in range(32):                                       # every sum at either end of its interval
                sign = np.array([1.0 if bits >> q & 1 else -1.0 for q in range(5)])
                pert = (cnt + sign * (1e-4 * np.maximum(1.0, cnt) + 2e-5)).clip(0).astype(np.float32)
                p1, a1, b1, d1 = M.is_snp(pert, monop)
                if (a1, b1, d1) == (a0, b0, d0):
                    track_rel = max(track_rel, abs(p1 - p0) / p0)
        manifest[name] = dict(argv=args, fastq=fq, pval=cut, monop=monop, rows=len(rows), calls=len(calls), y=n_y, y_diploid=n_ydip)
    print(f"p-value moved by the fp32 allowance of the sums: MEASURED_TRACK_REL = {track_rel:.2e}")
    json.dump(dict(runs=manifest, planted=[list(p) for p in planted]), open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
