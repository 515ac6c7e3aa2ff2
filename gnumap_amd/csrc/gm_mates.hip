// gm_mates.hip — gm_batch_set_mates (a defined extension, include/gnumap_hip.h has the rule): reads 2i and 2i + 1 of a block are the
// two mates of pair i.  The map step is not touched; everything here runs in the output step, on the records k_out_write left in HBM:
//
//   k_mate_spans     one lane per record: the span of its CIGAR in the pool (M + D runs; 1 where that is 0), and the record range
//                    [first, end) of every read - the records lie in read order, so a range is where the read index changes
//   k_mate_resolve   one wavefront per pair: the concordant combination with the largest product of posteriors, else each mate's
//                    best record; the five pair counters
//   k_mate_name_len  the QNAME rule, one lane per pair: the bytes of each mate's name that are printed
//   k_mate_name_copy ... the names cut that way into a pool of their own (the row kernels read it in place of the block's), and
//                    the first pair whose printed names differ
//   k_mate_fields    one lane per row: {flag, contig of the mate's primary, its POS, TLEN}, in row order (rows of reads without a
//                    record included, through the row source)
//   k_mate_row_len   SAM text: the bytes the flag and the three mate columns take beyond the row without mates, onto row_len
//
// Everything is a function of the input alone: the reductions compare keys that carry their tie-break, the only atomics are integer
// adds and one integer minimum.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "gm_internal.h"

namespace {

#define MT_NONE 0xFFFFFFFFu
#define MT_CHUNK 256u                              // records of the second mate staged in LDS at a time

__global__ void __launch_bounds__(256) k_mate_spans(GmDevMates m) {
    const unsigned long long k = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (k >= m.n_recs) return;
    const GmDevSamRec r = m.recs[k];
    const char* cg = m.pool + r.cigar_off;
    uint32_t span = 0, v = 0;
    for (uint32_t i = 0; i < 0xFFFFu; ++i) {
        const char c = cg[i];
        if (c == 0) break;
        if (c >= '0' && c <= '9') v = v * 10u + (uint32_t)(c - '0');
        else { if (c == 'M' || c == 'D') span += v; v = 0; }
    }
    m.span[k] = span ? span : 1u;
    const uint32_t rd = r.read;
    if (rd >= m.n_reads) return;
    if (k == 0 || m.recs[k - 1].read != rd) m.first[rd] = k;
    if (k + 1 == m.n_recs || m.recs[k + 1].read != rd) m.end[rd] = k + 1;
}

// x ranks above y: the larger number, and any number above a NaN (include/gnumap_hip.h: a NaN posterior or product ranks below every
// number; two NaNs rank alike, and so do +0 and -0).  Neither above the other = a tie, which the index decides
__device__ __forceinline__ bool mt_above(float x, float y) { return x > y || (x == x && y != y); }

// is (prod, a, b) better than (prod0, a0, b0)?  The product that ranks above; on a tie the smaller index of the first mate's record,
// then of the second's.  An entry without a combination has both indices MT_NONE: it loses to every combination, also to one whose
// product is NaN
__device__ __forceinline__ bool mt_better(float prod, uint32_t a, uint32_t b, float prod0, uint32_t a0, uint32_t b0) {
    if (a == MT_NONE) return false;
    if (a0 == MT_NONE) return true;
    if (mt_above(prod, prod0)) return true;
    if (mt_above(prod0, prod)) return false;
    return a != a0 ? a < a0 : b < b0;
}
// is record idx with posterior p a better single primary than (p0, idx0)?  The posterior that ranks above, the first one on ties
__device__ __forceinline__ bool mt_better1(float p, uint32_t idx, float p0, uint32_t idx0) {
    if (idx == MT_NONE) return false;
    if (idx0 == MT_NONE) return true;
    if (mt_above(p, p0)) return true;
    if (mt_above(p0, p)) return false;
    return idx < idx0;
}

// the record of [first, first + cnt) whose post_prob ranks highest, the first on ties: every lane gets the answer (MT_NONE for cnt == 0)
__device__ __forceinline__ uint32_t mt_best_single(const GmDevSamRec* recs, unsigned long long first, uint32_t cnt, uint32_t lane) {
    float p = 0.0f; uint32_t idx = MT_NONE;
    for (uint32_t i = lane; i < cnt; i += 64u) {
        const float q = recs[first + i].post_prob;
        if (idx == MT_NONE || mt_above(q, p)) { p = q; idx = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float op = __shfl_xor(p, off); const uint32_t oi = (uint32_t)__shfl_xor((int)idx, off);
        if (mt_better1(op, oi, p, idx)) { p = op; idx = oi; }
    }
    return idx;
}

// One wavefront per pair, the workgroups (one wavefront each) stride over the pairs.  The first mate's records go across the 64 lanes
// in trips of 64; the second mate's are staged through LDS MT_CHUNK at a time and every lane walks them in order, so a lane meets its
// combinations in ascending (first, second) order and a strict mt_above keeps the first of equals.  1000 x 1000 records are 16 trips
// of 4 chunks: 16 000 combinations per lane.
__global__ void __launch_bounds__(64) k_mate_resolve(GmDevMates m) {
    __shared__ unsigned long long s_pos[MT_CHUNK], s_end[MT_CHUNK];
    __shared__ uint32_t s_cs[MT_CHUNK];               // contig << 1 | strand
    __shared__ float s_post[MT_CHUNK];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_pairs = m.n_reads >> 1;
    uint32_t c_pairs = 0, c_both = 0, c_proper = 0, c_one = 0, c_none = 0;        // the same in every lane
    for (uint32_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        unsigned long long fa = m.first[2u * pi], ea = m.end[2u * pi], fb = m.first[2u * pi + 1u], eb = m.end[2u * pi + 1u];
        if (ea > m.n_recs) ea = m.n_recs;
        if (eb > m.n_recs) eb = m.n_recs;
        const uint32_t ca = ea > fa ? (uint32_t)std::min<unsigned long long>(ea - fa, 0xFFFFFFFEull) : 0u;
        const uint32_t cb = eb > fb ? (uint32_t)std::min<unsigned long long>(eb - fb, 0xFFFFFFFEull) : 0u;
        float best = 0.0f; uint32_t ba = MT_NONE, bb = MT_NONE;              // (best counts once ba is set)
        if (ca && cb) {
            for (uint32_t a0 = 0; a0 < ca; a0 += 64u) {
                const uint32_t ai = a0 + lane;
                const bool have = ai < ca;
                unsigned long long a_pos = 0, a_end = 0; uint32_t a_cs = 0; float a_post = 0.0f;
                if (have) {
                    const GmDevSamRec r = m.recs[fa + ai];
                    a_pos = r.chr_pos; a_end = r.chr_pos + m.span[fa + ai] - 1ull; a_cs = (r.contig << 1) | (r.strand ? 1u : 0u); a_post = r.post_prob;
                }
                for (uint32_t b0 = 0; b0 < cb; b0 += MT_CHUNK) {
                    const uint32_t cn = cb - b0 < MT_CHUNK ? cb - b0 : MT_CHUNK;
                    __syncthreads();                  // the chunk before has been read
                    for (uint32_t q = lane; q < cn; q += 64u) {
                        const GmDevSamRec r = m.recs[fb + b0 + q];
                        s_pos[q] = r.chr_pos; s_end[q] = r.chr_pos + m.span[fb + b0 + q] - 1ull; s_cs[q] = (r.contig << 1) | (r.strand ? 1u : 0u); s_post[q] = r.post_prob;
                    }
                    __syncthreads();
                    if (have)
                        for (uint32_t q = 0; q < cn; ++q) {
                            if ((a_cs ^ s_cs[q]) != 1u) continue;                 // one contig, different strands
                            const bool a_fwd = !(a_cs & 1u);
                            const unsigned long long pf = a_fwd ? a_pos : s_pos[q], pr = a_fwd ? s_pos[q] : a_pos, er = a_fwd ? s_end[q] : a_end;
                            if (pf > pr) continue;
                            const unsigned long long ins = er - pf + 1ull;
                            if (ins < m.min_insert || ins > m.max_insert) continue;
                            const float prod = a_post * s_post[q];
                            if (ba == MT_NONE || mt_above(prod, best)) { best = prod; ba = ai; bb = b0 + q; }     // (a NaN product is a combination too)
                        }
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float op = __shfl_xor(best, off);
                const uint32_t oa = (uint32_t)__shfl_xor((int)ba, off), ob = (uint32_t)__shfl_xor((int)bb, off);
                if (mt_better(op, oa, ob, best, ba, bb)) { best = op; ba = oa; bb = ob; }
            }
        }
        const bool proper = ba != MT_NONE;
        uint32_t pa = ba, pb = bb;
        if (!proper) { pa = mt_best_single(m.recs, fa, ca, lane); pb = mt_best_single(m.recs, fb, cb, lane); }
        if (lane == 0) {
            m.prim[2u * pi] = pa != MT_NONE ? fa + pa : ~0ull;
            m.prim[2u * pi + 1u] = pb != MT_NONE ? fb + pb : ~0ull;
            m.proper[pi] = proper ? 1 : 0;
        }
        ++c_pairs;
        if (ca && cb) ++c_both; else if (ca || cb) ++c_one; else ++c_none;
        if (proper) ++c_proper;
    }
    // one workgroup is one wavefront: its sums are in lane 0's registers, one integer add per counter and workgroup
    if (lane == 0 && c_pairs) {
        atomicAdd(&m.meta[MT_META_PAIRS], (unsigned long long)c_pairs);
        if (c_both) atomicAdd(&m.meta[MT_META_BOTH], (unsigned long long)c_both);
        if (c_proper) atomicAdd(&m.meta[MT_META_PROPER], (unsigned long long)c_proper);
        if (c_one) atomicAdd(&m.meta[MT_META_ONE], (unsigned long long)c_one);
        if (c_none) atomicAdd(&m.meta[MT_META_NONE], (unsigned long long)c_none);
    }
}

// the QNAME rule: the name up to its first space or tab; then "/1" of the first mate and "/2" of the second are dropped, if both
// are there
__device__ __forceinline__ uint32_t mt_name_cut(const char* s, unsigned long long len) {
    unsigned long long i = 0;
    while (i < len && s[i] != ' ' && s[i] != '\t') ++i;
    return (uint32_t)std::min<unsigned long long>(i, 0xFFFFFFFFull);
}

__global__ void __launch_bounds__(256) k_mate_name_len(const char* __restrict__ names, const uint64_t* __restrict__ name_off, uint32_t n_pairs, uint32_t* __restrict__ out_len) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    if (pi >= n_pairs) return;
    const unsigned long long o0 = name_off[2u * pi], o1 = name_off[2u * pi + 1u], o2 = name_off[2u * pi + 2u];
    const char* a = names + o0; const char* b = names + o1;
    uint32_t la = mt_name_cut(a, o1 - o0), lb = mt_name_cut(b, o2 - o1);
    if (la >= 2u && lb >= 2u && a[la - 2u] == '/' && a[la - 1u] == '1' && b[lb - 2u] == '/' && b[lb - 1u] == '2') { la -= 2u; lb -= 2u; }
    out_len[2u * pi] = la; out_len[2u * pi + 1u] = lb;
}

// one lane per pair: the two names into the new pool (new_off: the scan of the cut lengths; every store below `room`), and the
// comparison of the names as printed - their first `cut` bytes.  meta[MT_META_BAD_PAIR] = the first pair whose names differ
__global__ void __launch_bounds__(256) k_mate_name_copy(const char* __restrict__ names, const uint64_t* __restrict__ name_off, uint32_t n_pairs,
                                                        const uint32_t* __restrict__ len, const uint64_t* __restrict__ new_off, char* __restrict__ out,
                                                        unsigned long long room, uint32_t cut, unsigned long long* __restrict__ meta) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    if (pi >= n_pairs) return;
    const char* a = names + name_off[2u * pi]; const char* b = names + name_off[2u * pi + 1u];
    const uint32_t la = len[2u * pi], lb = len[2u * pi + 1u];
    const unsigned long long na = new_off[2u * pi], nb = new_off[2u * pi + 1u];
    for (uint32_t i = 0; i < la; ++i) if (na + i < room) out[na + i] = a[i];
    for (uint32_t i = 0; i < lb; ++i) if (nb + i < room) out[nb + i] = b[i];
    const uint32_t pa = la < cut ? la : cut, pb = lb < cut ? lb : cut;
    bool same = pa == pb;
    for (uint32_t i = 0; same && i < pa; ++i) same = a[i] == b[i];
    if (!same) atomicMin(&meta[MT_META_BAD_PAIR], (unsigned long long)pi);
}

__global__ void __launch_bounds__(256) k_mate_fields(GmDevMates m, GmDevText t, GmDevMateRow* __restrict__ out) {
    const unsigned long long k = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (k >= t.n_rows) return;
    unsigned long long rec = 0; uint32_t urd = 0;
    const bool is_rec = gm_row_is_record(t, k, rec, urd);
    GmDevMateRow f; f.flag = 0; f.rnext = -1; f.pnext = 0; f.tlen = 0;
    GmDevSamRec r = {};
    if (is_rec) r = m.recs[rec];
    const uint32_t rd = is_rec ? r.read : urd;
    if (rd >= m.n_reads) { out[k] = f; return; }              // (a row that names nothing of the block: the row kernels write nothing for it)
    const uint32_t mate = rd ^ 1u;
    const unsigned long long pm = m.prim[mate];
    f.flag = 0x1u | ((rd & 1u) ? 0x80u : 0x40u);
    GmDevSamRec mr = {};
    const bool has_mate = pm < m.n_recs;
    if (has_mate) {
        mr = m.recs[pm];
        if (mr.strand) f.flag |= 0x20u;
        f.rnext = (int32_t)mr.contig; f.pnext = (uint32_t)mr.chr_pos;
    } else f.flag |= 0x8u;
    if (!is_rec) f.flag |= 0x4u;
    else {
        if (r.strand) f.flag |= 0x10u;
        const bool is_prim = m.prim[rd] == rec;
        if (!is_prim) f.flag |= 0x100u;
        else if (m.proper[rd >> 1]) f.flag |= 0x2u;
        if (is_prim && has_mate && mr.contig == r.contig) {
            const unsigned long long p0 = r.chr_pos, e0 = p0 + m.span[rec] - 1ull, p1 = mr.chr_pos, e1 = p1 + m.span[pm] - 1ull;
            const unsigned long long v = (e0 > e1 ? e0 : e1) - (p0 < p1 ? p0 : p1) + 1ull;
            if (v <= 0x7FFFFFFFull) {
                const bool plus = p0 != p1 ? p0 < p1 : !(rd & 1u);
                f.tlen = plus ? (int32_t)v : -(int32_t)v;
            }
        }
    }
    out[k] = f;
}

__device__ __forceinline__ uint32_t mt_digits(unsigned long long v) { uint32_t d = 1; while (v >= 10ull) { v /= 10ull; ++d; } return d; }

// SAM text: a row without mates prints flag 0 / 16 / 4 and "\t*\t0\t0\t" (7 bytes) behind its CIGAR; with mates the flag has up to four
// digits and the three columns are "\t<RNEXT>\t<PNEXT>\t<TLEN>\t"
__global__ void __launch_bounds__(256) k_mate_row_len(GmDevText t) {
    const unsigned long long k = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (k >= t.n_rows) return;
    unsigned long long rec = 0; uint32_t urd = 0;
    const bool is_rec = gm_row_is_record(t, k, rec, urd);
    if (!is_rec && urd == MT_NONE) return;
    const GmDevMateRow f = t.mate[k];
    uint32_t old_flag = 1u, own = MT_NONE;
    if (is_rec) { const GmDevSamRec r = t.recs[rec]; old_flag = r.strand ? 2u : 1u; own = r.contig; }
    uint32_t rn = 1u;                                          // "*" or "="
    if (f.rnext >= 0 && (uint32_t)f.rnext != own) rn = t.cname_off[f.rnext + 1] - t.cname_off[f.rnext];
    const uint32_t tl = f.tlen < 0 ? 1u + mt_digits((unsigned long long)(-(long long)f.tlen)) : mt_digits((unsigned long long)f.tlen);
    t.row_len[k] += mt_digits(f.flag) - old_flag + (1u + rn + 1u + mt_digits(f.pnext) + 1u + tl + 1u) - 7u;
}

inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

// spans and ranges, then the pairs.  first / end / prim: n_reads entries each, proper: n_reads / 2 bytes, meta: MT_META_N words
int gmk_mate_resolve(const GmDevMates& m, void* stream) {
    hipError_t e = hipMemsetAsync(m.meta, 0, MT_META_N * 8, S_(stream));
    if (e == hipSuccess) e = hipMemsetAsync(m.meta + MT_META_BAD_PAIR, 0xFF, 8, S_(stream));
    if (e != hipSuccess) return (int)e;
    const uint32_t n_pairs = m.n_reads >> 1;
    if (!n_pairs) return 0;
    e = hipMemsetAsync(m.first, 0, (size_t)m.n_reads * 8, S_(stream));
    if (e == hipSuccess) e = hipMemsetAsync(m.end, 0, (size_t)m.n_reads * 8, S_(stream));
    if (e != hipSuccess) return (int)e;
    if (m.n_recs) hipLaunchKernelGGL(k_mate_spans, dim3(cdiv(m.n_recs, 256)), dim3(256), 0, S_(stream), m);
    hipLaunchKernelGGL(k_mate_resolve, dim3(gm_test_grid(std::min<uint32_t>(n_pairs, 16384u))), dim3(64), 0, S_(stream), m);
    return (int)hipGetLastError();
}

// the QNAME rule: len (n_reads words) and new_off (n_reads + 1) are scratch, out has room for `room` bytes (the block's own name bytes
// always hold the cut names); cut = the bytes of a name the sink prints (1023 text, 254 BAM)
int gmk_mate_names(const char* names, const uint64_t* name_off, uint32_t n_reads, uint32_t* len, uint64_t* new_off, unsigned long long* tmp, char* out, uint64_t room,
                   uint32_t cut, unsigned long long* meta, void* stream) {
    const uint32_t n_pairs = n_reads >> 1;
    if (!n_pairs) return 0;
    hipLaunchKernelGGL(k_mate_name_len, dim3(cdiv(n_pairs, 256)), dim3(256), 0, S_(stream), names, name_off, n_pairs, len);
    if (const int rc = gmk_scan_u32(len, n_reads, new_off, tmp, stream)) return rc;
    hipLaunchKernelGGL(k_mate_name_copy, dim3(cdiv(n_pairs, 256)), dim3(256), 0, S_(stream), names, name_off, n_pairs, len, new_off, out, (unsigned long long)room, cut, meta);
    return (int)hipGetLastError();
}

// the fields of t.n_rows rows (t.row_src / t.n_reads / t.n_recs name the rows)
int gmk_mate_fields(const GmDevMates& m, const GmDevText& t, GmDevMateRow* out, void* stream) {
    if (t.n_rows == 0) return 0;
    hipLaunchKernelGGL(k_mate_fields, dim3(cdiv(t.n_rows, 256)), dim3(256), 0, S_(stream), m, t, out);
    return (int)hipGetLastError();
}

int gmk_mate_row_len(const GmDevText& t, void* stream) {
    if (t.n_rows == 0 || !t.mate) return 0;
    hipLaunchKernelGGL(k_mate_row_len, dim3(cdiv(t.n_rows, 256)), dim3(256), 0, S_(stream), t);
    return (int)hipGetLastError();
}
