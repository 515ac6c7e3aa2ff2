// gm_snpcall.hip — the ninth column of --snp's .gmp: GenomeBwt::PrintSNPCall (src/GenomeBwt.cpp:1011-1090) and the likelihood-ratio
// tests behind it, is_snp (:875-901), LRT (:739-753) and dipLRT (:758-873), over the total track and the five per-nucleotide tracks
// where k_snp_deposit (gm_snp.hip) left them in HBM.  One lane per position (bin size 1): 24 bytes of counts + 2 bits of reference
// in, one code byte + one fp64 p-value out; the rows the reference marks 'Y' are compacted in position order by a second pass.
//
// The reference calls GSL for one function, gsl_cdf_chisq_P(x, df) with df = 1 and 2; both have closed forms,
//     P(x; 1) = erf(sqrt(x / 2)),   P(x; 2) = 1 - exp(-x / 2),   P = 0 for x <= 0 (GSL's answer),
// and the p-value is formed as ONE MINUS P in fp64 like the reference's, not as erfc: near x = 75 the reference's p-values cancel
// to exactly 0 and dipLRT branches on that.
//
// The likelihood ratios are kept as LOGARITHMS: the reference's pow(.2, sum) / (pow(..) * pow(..)) leaves the normal doubles at a
// total of about 440 and is 0 / 0 from 463, log(ratio) = sum log .2 - sum_i c_i log(arg_i) never underflows (0 log 0 = 0, as
// pow(x, 0) = 1), and x = -2 log(ratio) is what both tests need.  Where dipLRT compares ratio2 < ratio1 the logs are compared.
// Everything else follows the reference's types: the counts and the MONO_DIP_RATIO tests are floats, the 0.2 prior is added to each
// float in double and rounded back to float (and taken off again the same way before the last ratio test), `sum` is a double that
// takes the floats in index order and the prior five times.
//
// Where the reference has no defined answer: the forced-monoploid case evaluates chars[-1]; here it is dip = false,
// p = pval1, the intent stated at :760-763.
#include <hip/hip_runtime.h>
#include "gm_internal.h"

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define SC_MIN_PRINT 0.001f         // MIN_PRINT :928
#define SC_WG 256

// max_pos :727-732: std::max_element, the lowest index wins ties
__device__ __forceinline__ int sc_max_pos(const float c[5]) {
    int m = 0;
    for (int i = 1; i < 5; ++i) if (c[m] < c[i]) m = i;
    return m;
}

// c log(arg) with pow(arg, 0) = 1 for every arg (0, NaN and inf included), as the reference's pow() has it
__device__ __forceinline__ double sc_term(double c, double arg) { return c == 0.0 ? 0.0 : c * log(arg); }

// log of `pow(.2,sum) / (pow(c1/sum, c1) * pow(((sum-c1)/sum)/4, sum-c1))` :744-746, :772-774, :800-802
__device__ __forceinline__ double sc_log_ratio1(double c1, double sum) {
    return sum * log(.2) - (sc_term(c1, c1 / sum) + sc_term(sum - c1, ((sum - c1) / sum) / 4));
}

// 1 - gsl_cdf_chisq_P(-2 log(ratio), df)
__device__ __forceinline__ double sc_pval(double log_ratio, int df) {
    const double x = -2 * log_ratio;
    if (!(x > 0.0)) return 1.0;
    const double P = df == 1 ? erf(sqrt(x / 2)) : 1.0 - exp(-x / 2);
    return 1 - P;
}

// is_snp :875-901.  pos2 = -1 when there is no second allele.
__device__ double sc_is_snp(const float in[5], int monop, int& pos1, int& pos2, bool& dip) {
    float c[5] = { in[0], in[1], in[2], in[3], in[4] };
    dip = false; pos2 = -1;
    pos1 = sc_max_pos(c);
    double sum = 0;
    if (monop) {                                                          // LRT: `double sum = chars[0] + .. + chars[4]` is a FLOAT sum
        const float fs = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(c[0], c[1]), c[2]), c[3]), c[4]);
        sum = (double)fs;
        return sc_pval(sc_log_ratio1((double)c[pos1], sum), 1);
    }
    for (int i = 0; i < 5; ++i) sum += (double)c[i];
    double lr1 = sc_log_ratio1((double)c[pos1], sum);
    double pval1 = sc_pval(lr1, 1);
    float second[5] = { c[0], c[1], c[2], c[3], c[4] };
    second[pos1] = 0.0f;
    const int p2 = sc_max_pos(second);
    if (__fdiv_rn(c[pos1], c[p2]) > 3.0f || pos1 == p2) return pval1;    // forced monoploid: pval2 = MAX_PVAL, the defined outcome
    for (int i = 0; i < 5; ++i) { c[i] = (float)((double)c[i] + 0.2); sum += 0.2; }
    const double c1 = (double)c[pos1], c2 = (double)c[p2];
    lr1 = sc_log_ratio1(c1, sum);
    pval1 = sc_pval(lr1, 1);
    // :808-814, the third factor as written there: ((sum - c1 + c2) / sum) / 3 to the power sum - c1 - c2
    const double lr2 = sum * log(.2) - (sc_term(c1, c1 / sum) + sc_term(c2, c2 / sum) + sc_term(sum - c1 - c2, ((sum - c1 + c2) / sum) / 3));
    const double pval2 = sc_pval(lr2, 2);
    for (int i = 0; i < 5; ++i) c[i] = (float)((double)c[i] - 0.2);
    const bool near = __fdiv_rn(c[pos1], c[p2]) < 3.0f;
    pos2 = p2;
    if (pval2 == 0 && pval1 == 0) { dip = lr2 < lr1 && near; return 0.0; }
    if (pval2 < pval1 && near) { dip = true; return pval2; }
    return pval1;
}

// code byte: bit 7 the row is printed, bit 6 'Y', bit 5 diploid, bits 3-4 the second allele counted among the four bases that are
// not the first (dip only), bits 0-2 the first allele
__device__ __forceinline__ uint8_t sc_code(bool y, bool dip, int pos1, int pos2) {
    const int r2 = dip ? pos2 - (pos2 > pos1 ? 1 : 0) : 0;
    return (uint8_t)(0x80 | (y ? 0x40 : 0) | (dip ? 0x20 : 0) | (r2 << 3) | pos1);
}

__device__ __forceinline__ uint32_t sc_ref_base(const uint8_t* pac, uint64_t g) { return (uint32_t)(pac[g >> 2] >> ((~g & 3u) << 1)) & 3u; }

// positions [lo, lo + n): code[k - lo], pval[k - lo]; ycnt[workgroup] = its 'Y' rows
__global__ void __launch_bounds__(SC_WG) k_snp_call(const float* cov, const float* nuc, uint64_t bins, const uint8_t* pac, uint64_t l_pac, uint64_t lo, uint64_t n,
                                                     float snp_pval, int monop, uint8_t* code, double* pval, uint32_t* ycnt) {
    __shared__ uint32_t wg_y;
    if (threadIdx.x == 0) wg_y = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * SC_WG + threadIdx.x, k = lo + i;
    bool y = false;
    if (i < n) {
        uint8_t cd = 0; double p = 1.0;
        if (k < l_pac && k < bins && cov[k] > SC_MIN_PRINT) {
            float c[5];
            for (int q = 0; q < 5; ++q) c[q] = nuc[(uint64_t)q * bins + k];
            int p1, p2; bool dip;
            p = sc_is_snp(c, monop, p1, p2, dip);
            y = (p1 != (int)sc_ref_base(pac, k) || dip) && p < (double)snp_pval;          // :1065-1066
            cd = sc_code(y, dip, p1, p2);
        }
        code[i] = cd; pval[i] = p;
    }
    const unsigned long long m = __ballot(y);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&wg_y, (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) ycnt[blockIdx.x] = wg_y;
}

// exclusive scan of the workgroups' counts by one workgroup; off[nb] = total
__global__ void __launch_bounds__(1024) k_snp_scan(const uint32_t* cnt, uint32_t nb, unsigned long long* off) {
    __shared__ unsigned long long part[1024];
    const uint32_t t = threadIdx.x, per = (nb + 1023u) / 1024u;
    const uint32_t a = t * per < nb ? t * per : nb, b = a + per < nb ? a + per : nb;
    unsigned long long s = 0;
    for (uint32_t j = a; j < b; ++j) s += cnt[j];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = part[t] - s;
    for (uint32_t j = a; j < b; ++j) { off[j] = run; run += cnt[j]; }
    if (t == 1023) off[nb] = part[1023];
}

// the 'Y' rows of [lo, lo + n) in position order: record base + off[workgroup] + rank within it, while it is below cap
__global__ void __launch_bounds__(SC_WG) k_snp_gather(const float* cov, const float* nuc, uint64_t bins, const uint8_t* pac, const uint32_t* contig_off, uint32_t n_seqs,
                                                       uint64_t lo, uint64_t n, const uint8_t* code, const double* pval, const unsigned long long* off,
                                                       unsigned long long base, unsigned long long cap, GmDevSnpRec* out) {
    __shared__ uint32_t wave_y[SC_WG / 64];
    const uint64_t i = (uint64_t)blockIdx.x * SC_WG + threadIdx.x, k = lo + i;
    const uint8_t cd = i < n ? code[i] : 0;
    const bool y = (cd & 0x40) != 0;
    const unsigned long long m = __ballot(y);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_y[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!y) return;
    uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) rank += wave_y[w];
    const unsigned long long at = base + off[blockIdx.x] + rank;
    if (at >= cap) return;
    uint32_t a = 0, b = n_seqs;                                            // contig_off[a] <= k < contig_off[a + 1]
    while (b - a > 1) { const uint32_t mid = (a + b) / 2; if ((uint64_t)contig_off[mid] <= k) a = mid; else b = mid; }
    GmDevSnpRec r;
    r.pos = k; r.contig = a; r.pad0 = 0; r.chr_pos = k - contig_off[a] + 1;
    r.total = cov[k];
    for (int q = 0; q < 5; ++q) r.nuc[q] = nuc[(uint64_t)q * bins + k];
    r.p_val = pval[i];
    const uint32_t p1 = cd & 7u, dip = (cd >> 5) & 1u, r2 = (cd >> 3) & 3u;
    r.ref = (uint8_t)sc_ref_base(pac, k); r.alt1 = (uint8_t)p1; r.alt2 = dip ? (uint8_t)(r2 + (r2 >= p1 ? 1u : 0u)) : (uint8_t)255; r.diploid = (uint8_t)dip;
    r.pad1[0] = r.pad1[1] = r.pad1[2] = r.pad1[3] = 0;
    out[at] = r;
}

// is_snp on caller-supplied counts
__global__ void __launch_bounds__(SC_WG) k_snp_stat(const float* counts, uint32_t n, int monop, double* pval, int8_t* pos1, int8_t* pos2, uint8_t* dip) {
    const uint32_t i = blockIdx.x * SC_WG + threadIdx.x;
    if (i >= n) return;
    float c[5];
    for (int q = 0; q < 5; ++q) c[q] = counts[(size_t)i * 5u + q];
    int p1, p2; bool d;
    pval[i] = sc_is_snp(c, monop, p1, p2, d);
    pos1[i] = (int8_t)p1; pos2[i] = (int8_t)p2; dip[i] = d ? 1 : 0;
}

uint32_t gmk_snp_call_groups(uint64_t n) { return (uint32_t)((n + SC_WG - 1) / SC_WG); }

int gmk_snp_call(const float* cov, const float* nuc, uint64_t bins, const GmDevIndex& ix, uint64_t lo, uint64_t n, float snp_pval, int monop, uint8_t* code, double* pval,
                 uint32_t* ycnt, void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_snp_call, dim3(gmk_snp_call_groups(n)), dim3(SC_WG), 0, S_(stream), cov, nuc, bins, ix.pac, (uint64_t)ix.l_pac, lo, n, snp_pval, monop, code, pval, ycnt);
    return (int)hipGetLastError();
}

int gmk_snp_gather(const float* cov, const float* nuc, uint64_t bins, const GmDevIndex& ix, uint64_t lo, uint64_t n, const uint8_t* code, const double* pval,
                   const uint32_t* ycnt, unsigned long long* off, unsigned long long base, unsigned long long cap, GmDevSnpRec* out, void* stream) {
    if (n == 0) return 0;
    const uint32_t nb = gmk_snp_call_groups(n);
    hipLaunchKernelGGL(k_snp_scan, dim3(1), dim3(1024), 0, S_(stream), ycnt, nb, off);
    hipLaunchKernelGGL(k_snp_gather, dim3(nb), dim3(SC_WG), 0, S_(stream), cov, nuc, bins, ix.pac, ix.contig_off, ix.n_seqs, lo, n, code, pval, off, base, cap, out);
    return (int)hipGetLastError();
}

int gmk_snp_stat(const float* counts, uint32_t n, int monop, double* pval, int8_t* pos1, int8_t* pos2, uint8_t* dip, void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_snp_stat, dim3((n + SC_WG - 1) / SC_WG), dim3(SC_WG), 0, S_(stream), counts, n, monop, pval, pos1, pos2, dip);
    return (int)hipGetLastError();
}
