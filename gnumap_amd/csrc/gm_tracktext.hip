// gm_tracktext.hip — the per-position files as text, formatted where the tracks live: <out>.sgr (GenomeBwt::PrintFinalSGR
// src/GenomeBwt.cpp:1212-1273), the eight-column <out>.gmp (PrintFinalBisulfite :1092-1210, PrintFinalSNP :930-1009 without
// PrintSNPCall's column) and the nine-column one with it.  The contract is the bytes of the host writers of gm_tracks.cpp
// (gm_coverage_write_sgr / _gmp / _gmp_calls):
//
//   bin k, count = k * bin_size, contig = the last one whose offset is <= count (bins run over the CONCATENATED coordinate)
//   .sgr          a row iff (double)bins[k] > 0.001            name \t count-off+1 \t %.5f \n
//   .gmp  --snp   a row iff bins[k] > 0.001f                   name \t pos \t %.5f  5 x (\t %.5f)  \n
//   .gmp  others  a row iff the reference base at count is the mode's and bins[k] > 0.0f
//                                                              name \t pos \t %f    5 x (\t %.5f)  \n
//
// Numbers: put_fixed (gm_tracks.cpp) is the specification.  For 0 <= v < 1e9 the digits are rint((double)v * 10^N); the product of a
// 24-bit float and 10^5 or 10^6 is exact in a double and rint rounds to nearest even on the device as on the host, so the digits are
// the host's bit for bit (the library is built with -ffp-contract=off).  -0.0f takes that path too and prints as 0.  Every other
// value (negative, NaN, inf, >= 1e9) is snprintf's on the host: a launch that meets one in a row it would print only FLAGS its slab
// (meta[TT_META_HOST]) and the library formats that slab with the host emitters.  Nothing here imitates snprintf.
//
// GM_TRACK_CALLS is the nine-column .gmp of --snp --snp_calls (gm_coverage_write_gmp_calls): the GM_TRACK_SNP rows with PrintSNPCall's
// column (src/GenomeBwt.cpp:1011-1090) in front of the newline, built from k_snp_call's code byte and p-value of the slab (t.code / t.pval,
// written by gmk_snp_call before the sizes pass):
//   \tN                          the first allele is the reference base and the call is not diploid            2 bytes
//   \t[YN]:r->x p_val=d.dde[+-]dd                                                                              22 bytes
//   \t[YN]:r->x/y p_val=d.dde[+-]dd   a diploid call                                                           24 bytes
// The length follows from the code byte alone, so the sizes pass never formats a p-value: it only asks whether gm_put_e2_hd (gm_fmt_dev.h,
// exact "%.2e" for +0.0 and 2^-200 <= p < 2^200) can print it, and flags the slab otherwise.  The calls path is a second instantiation of
// the two kernels (k_track_sizes<true> / k_track_rows<true>): the other kinds' kernels carry none of it and keep their registers.
//
// Two passes over a slab of bins, one lane per bin, tiles of TT_WG consecutive bins:
//   k_track_sizes   length of every row, summed per tile; rows counted; out-of-domain values flagged
//   k_track_scan    exclusive scan of the tile sums by one workgroup (kernel boundaries order the passes: nothing waits for another
//                   workgroup)
//   k_track_rows    a tile's text is one contiguous stretch of the output: it is assembled in LDS, a window of TT_WIN bytes at a time,
//                   laid out so that LDS byte i and output byte i share their alignment, and leaves as whole 16-byte stores; single
//                   bytes only in the ragged first and last 16 bytes of the tile.  A window has no row budget: a contig name of any
//                   length is copied from HBM through as many windows as it takes.
#include <hip/hip_runtime.h>
#include "gm_internal.h"
#include "gm_fmt_dev.h"

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define TT_WG 256u
#define TT_WIN 24576u               // bytes of tile text in LDS at a time (a multiple of 16): most tiles need one window

struct TtRow {
    uint32_t len;                   // bytes of the row, 0 = the bin has none
    uint32_t c0, cl;                // its contig's name in cnames
    uint32_t pos;                   // 1-based position in the contig
    float v[6];                     // the total and, in a .gmp, a c g t n
    bool bad;                       // a printed value outside put_fixed's own domain (or a p-value outside gm_put_e2_hd's)
    uint32_t call;                  // GM_TRACK_CALLS: k_snp_call's code byte, the reference base in bits 8-9
};

__device__ __forceinline__ uint32_t tt_digits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u
           : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ bool tt_in_domain(float v) { return v >= 0.0f && v < 1.0e9f; }
// put_fixed's digits: the integer part (< 2^30 for v < 1e9) and the `decimals` digits behind the point
__device__ __forceinline__ void tt_fixed(float v, bool six, uint32_t& ip, uint32_t& fp) {
    const unsigned long long q = (unsigned long long)rint((double)v * (six ? 1000000.0 : 100000.0));
    const unsigned long long hi = six ? q / 1000000ull : q / 100000ull;      // two constant divisors: no 64-bit division loop
    ip = (uint32_t)hi; fp = (uint32_t)(q - hi * (six ? 1000000ull : 100000ull));
}
__device__ __forceinline__ uint32_t tt_fixed_len(float v, bool six) {
    uint32_t ip, fp;
    tt_fixed(v, six, ip, fp);
    return tt_digits(ip) + (six ? 7u : 6u);
}

// the contig that holds `count`: the last one whose offset is <= count
__device__ __forceinline__ uint32_t tt_contig_search(const uint32_t* off, uint32_t n_seqs, uint64_t count) {
    uint32_t a = 0, b = n_seqs;
    while (b - a > 1u) { const uint32_t mid = (a + b) / 2u; if ((uint64_t)off[mid] <= count) a = mid; else b = mid; }
    return a;
}

// bytes of the ninth column of a row with the code byte cd at a position whose reference base is ref
__device__ __forceinline__ uint32_t tt_call_len(uint32_t cd, uint32_t ref) {
    const uint32_t p1 = cd & 7u, dip = (cd >> 5) & 1u;
    return (p1 != ref || dip) ? (dip ? 24u : 22u) : 2u;
}
// gm_put_e2_hd's domain, from the bits alone
__device__ __forceinline__ bool tt_e2_in_domain(double p) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(p);
    const uint32_t be = (uint32_t)(bits >> 52);             // with the sign: a negative value is >= 2048
    return bits == 0ull || (be >= 1023u - 200u && be < 1023u + 200u);
}

// what lane i of the slab prints; `contig` = the contig of the tile's first bin (the lanes walk on from it)
template <bool CALLS> __device__ __forceinline__ TtRow tt_row(const GmDevTrack& t, uint64_t i, uint32_t contig) {
    TtRow r;
    r.len = 0; r.c0 = 0; r.cl = 0; r.pos = 0; r.bad = false; r.call = 0;
    const uint32_t kind = CALLS ? (uint32_t)GM_TRACK_SNP : t.kind;            // the calls file: --snp's rows, one column more
    for (int q = 0; q < 6; ++q) r.v[q] = 0.0f;
    if (i >= t.n) return r;
    const uint64_t k = t.lo + i, count = k * (uint64_t)t.bin_size;
    const float total = t.cov[k];
    bool print;
    if (kind == GM_TRACK_SGR) print = (double)total > 0.001;
    else if (kind == GM_TRACK_SNP) print = total > 0.001f;
    else print = ((uint32_t)(t.pac[count >> 2] >> ((~count & 3u) << 1)) & 3u) == t.want && total > 0.0f;
    if (!print) return r;
    while (contig + 1u < t.n_seqs && count >= (uint64_t)t.contig_off[contig + 1u]) ++contig;
    r.c0 = t.cname_off[contig]; r.cl = t.cname_off[contig + 1u] - r.c0;
    r.pos = (uint32_t)(count - (uint64_t)t.contig_off[contig]) + 1u;
    r.v[0] = total;
    const bool six = kind == GM_TRACK_BASE;                                   // "%f" of the total there
    r.bad = !tt_in_domain(total);
    uint32_t len = r.cl + 1u + tt_digits(r.pos) + 1u + tt_fixed_len(total, six) + 1u;
    if (kind != GM_TRACK_SGR) {
        for (int q = 0; q < 5; ++q) {
            const float x = t.nuc[(uint64_t)q * t.nuc_stride + k];
            r.v[q + 1] = x;
            r.bad |= !tt_in_domain(x);
            len += 1u + tt_fixed_len(x, false);
        }
    }
    if (CALLS) {
        const uint32_t cd = t.code[i], ref = (uint32_t)(t.pac[count >> 2] >> ((~count & 3u) << 1)) & 3u;
        const uint32_t col = tt_call_len(cd, ref);
        if (col > 2u) r.bad |= !tt_e2_in_domain(t.pval[i]);
        r.call = cd | (ref << 8);
        len += col;
    }
    r.len = len;
    return r;
}

// "acgtn"[b] without a table in memory
__device__ __forceinline__ char tt_letter(uint32_t b) { return b == 0u ? 'a' : b == 1u ? 'c' : b == 2u ? 'g' : b == 3u ? 't' : 'n'; }

// sum over the workgroup (every lane gets it) and the exclusive prefix of the lane
__device__ __forceinline__ uint32_t tt_block_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < TT_WG / 64u; ++w) { const uint32_t x = s_wave[w]; if (w < wave) before += x; all += x; }
    total = all;
    return before + inc - v;
}

template <bool CALLS> __global__ void __launch_bounds__(TT_WG) k_track_sizes(GmDevTrack t) {
    __shared__ uint32_t s_wave[TT_WG / 64u];
    __shared__ uint32_t s_contig, s_rows, s_bad;
    if (threadIdx.x == 0) {
        s_contig = tt_contig_search(t.contig_off, t.n_seqs, (t.lo + (uint64_t)blockIdx.x * TT_WG) * (uint64_t)t.bin_size);
        s_rows = 0; s_bad = 0;
    }
    __syncthreads();
    const TtRow r = tt_row<CALLS>(t, (uint64_t)blockIdx.x * TT_WG + threadIdx.x, s_contig);
    const unsigned long long rows = __ballot(r.len != 0u), bad = __ballot(r.bad);
    if ((threadIdx.x & 63u) == 0u) { if (rows) atomicAdd(&s_rows, (uint32_t)__popcll(rows)); if (bad) s_bad = 1u; }
    uint32_t total;
    (void)tt_block_scan(r.len, s_wave, total);                               // its barrier also publishes s_rows / s_bad
    if (threadIdx.x == 0) {
        t.tile_len[blockIdx.x] = total;
        if (s_rows) atomicAdd(&t.meta[TT_META_ROWS], (unsigned long long)s_rows);
        if (s_bad) t.meta[TT_META_HOST] = 1ull;
    }
}

// exclusive scan of the tile sums by one workgroup; off[nt] = meta[TT_META_BYTES] = the slab's text
__global__ void __launch_bounds__(1024) k_track_scan(const uint32_t* len, uint32_t nt, unsigned long long* off, unsigned long long* meta) {
    __shared__ unsigned long long part[1024];
    const uint32_t t = threadIdx.x, per = (nt + 1023u) / 1024u;
    const uint32_t a = t * per < nt ? t * per : nt, b = a + per < nt ? a + per : nt;
    unsigned long long s = 0;
    for (uint32_t j = a; j < b; ++j) s += len[j];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const unsigned long long v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = part[t] - s;
    for (uint32_t j = a; j < b; ++j) { off[j] = run; run += len[j]; }
    if (t == 1023u) { off[nt] = part[1023]; meta[TT_META_BYTES] = part[1023]; }
}

// the part of a row that falls into the window [w0, w0 + wl) of its tile's text goes to s[a + (offset - w0)]
struct TtWin {
    char* s; uint32_t a, w0, wl;
    __device__ __forceinline__ void put(uint32_t at, char c) const { const uint32_t d = at - w0; if (d < wl) s[a + d] = c; }      // at < w0 wraps to a large d
    // `count` decimal digits of v ending before `end`
    __device__ __forceinline__ void digits(uint32_t end, uint32_t v, uint32_t count) const {
        for (uint32_t q = 0; q < count; ++q) { put(end - 1u - q, (char)('0' + v % 10u)); v /= 10u; }
    }
    __device__ __forceinline__ uint32_t fixed(uint32_t at, float v, bool six) const {
        uint32_t ip, fp;
        tt_fixed(v, six, ip, fp);
        const uint32_t di = tt_digits(ip), df = six ? 6u : 5u;
        digits(at + di, ip, di);
        put(at + di, '.');
        digits(at + di + 1u + df, fp, df);
        return at + di + 1u + df;
    }
};

template <bool CALLS> __global__ void __launch_bounds__(TT_WG) k_track_rows(GmDevTrack t) {
    __shared__ __attribute__((aligned(16))) char s_txt[TT_WIN];
    __shared__ uint32_t s_wave[TT_WG / 64u];
    __shared__ uint32_t s_contig;
    if (threadIdx.x == 0) s_contig = tt_contig_search(t.contig_off, t.n_seqs, (t.lo + (uint64_t)blockIdx.x * TT_WG) * (uint64_t)t.bin_size);
    __syncthreads();
    // the ninth column's p-value first, once for all windows, while nothing else is live.  The sizes pass let only values of
    // gm_put_e2_hd's domain through; should it refuse one all the same, the slab is flagged now and the host formats it after all
    char e2[8] = { '?', '?', '?', '?', '?', '?', '?', '?' };
    if (CALLS) {
        const uint64_t i = (uint64_t)blockIdx.x * TT_WG + threadIdx.x;
        if (i < t.n && t.cov[t.lo + i] > 0.001f) {
            const uint64_t count = t.lo + i;
            if (tt_call_len(t.code[i], (uint32_t)(t.pac[count >> 2] >> ((~count & 3u) << 1)) & 3u) > 2u && gm_put_e2_hd(e2, t.pval[i]) == e2) t.meta[TT_META_HOST] = 1ull;
        }
    }
    const TtRow r = tt_row<CALLS>(t, (uint64_t)blockIdx.x * TT_WG + threadIdx.x, s_contig);
    uint32_t tile_len;
    const uint32_t r0 = tt_block_scan(r.len, s_wave, tile_len);              // where the lane's row starts in the tile's text
    // every store stays inside the range the scan gave this tile, whatever the lengths say
    const unsigned long long T0 = t.tile_off[blockIdx.x], room = t.tile_off[blockIdx.x + 1u] - T0;
    if ((unsigned long long)tile_len > room) tile_len = (uint32_t)room;
    const bool six = !CALLS && t.kind == GM_TRACK_BASE;
    const uint32_t call_len = CALLS && r.len ? tt_call_len(r.call & 0xFFu, r.call >> 8) : 0u;
    for (uint32_t w0 = 0; w0 < tile_len;) {
        const unsigned long long g = T0 + w0;                                // the window's first byte in the output
        const uint32_t a = (uint32_t)(g & 15ull);                            // LDS byte i <-> output byte g - a + i: the same alignment on both sides
        const uint32_t wl = tile_len - w0 < TT_WIN - a ? tile_len - w0 : TT_WIN - a;      // a window that is not the tile's last ends on a 16-byte boundary
        if (r.len && r0 < w0 + wl && r0 + r.len > w0) {
            const TtWin w = { s_txt, a, w0, wl };
            uint32_t at = r0;
            if (at >= w0 && at + r.cl <= w0 + wl) { for (uint32_t j = 0; j < r.cl; ++j) s_txt[a + (at - w0) + j] = t.cnames[r.c0 + j]; }
            else { for (uint32_t j = 0; j < r.cl; ++j) w.put(at + j, t.cnames[r.c0 + j]); }
            at += r.cl;
            w.put(at, '\t'); ++at;
            const uint32_t dp = tt_digits(r.pos);
            w.digits(at + dp, r.pos, dp); at += dp;
            w.put(at, '\t'); ++at;
            at = w.fixed(at, r.v[0], six);
            if (CALLS || t.kind != GM_TRACK_SGR) for (int q = 1; q < 6; ++q) { w.put(at, '\t'); at = w.fixed(at + 1u, r.v[q], false); }
            if (CALLS) {                                                     // the host emitter of gm_coverage_write_gmp_calls, byte for byte
                const uint32_t cd = r.call & 0xFFu, ref = r.call >> 8, p1 = cd & 7u, r2 = (cd >> 3) & 3u;
                w.put(at, '\t'); w.put(at + 1u, (cd & 0x40u) ? 'Y' : 'N'); at += 2u;
                if (call_len > 2u) {
                    w.put(at, ':'); w.put(at + 1u, tt_letter(ref)); w.put(at + 2u, '-'); w.put(at + 3u, '>'); w.put(at + 4u, tt_letter(p1)); at += 5u;
                    if (call_len == 24u) { w.put(at, '/'); w.put(at + 1u, tt_letter(r2 + (r2 >= p1 ? 1u : 0u))); at += 2u; }
                    w.put(at, ' '); w.put(at + 1u, 'p'); w.put(at + 2u, '_'); w.put(at + 3u, 'v'); w.put(at + 4u, 'a'); w.put(at + 5u, 'l'); w.put(at + 6u, '='); at += 7u;
#pragma unroll
                    for (uint32_t j = 0; j < 8u; ++j) w.put(at + j, e2[j]);
                    at += 8u;
                }
            }
            w.put(at, '\n');
        }
        __syncthreads();
        char* const base = t.text + (g - a);                                 // 16-byte aligned: t.text is
        const uint32_t end = a + wl, chunks = (end + 15u) / 16u;
        for (uint32_t c = threadIdx.x; c < chunks; c += TT_WG) {
            const uint32_t lo = c * 16u, hi = lo + 16u;
            if (lo >= a && hi <= end) reinterpret_cast<uint4*>(base)[c] = reinterpret_cast<const uint4*>(s_txt)[c];
            else for (uint32_t i = lo > a ? lo : a; i < (hi < end ? hi : end); ++i) base[i] = s_txt[i];       // the ragged ends of the tile
        }
        __syncthreads();
        w0 += wl;
    }
}

uint32_t gmk_track_tiles(uint64_t n) { return (uint32_t)((n + TT_WG - 1) / TT_WG); }

int gmk_track_sizes(const GmDevTrack& t, void* stream) {
    if (t.n == 0) return 0;
    const uint32_t nt = gmk_track_tiles(t.n);
    if (t.kind == GM_TRACK_CALLS) hipLaunchKernelGGL(k_track_sizes<true>, dim3(nt), dim3(TT_WG), 0, S_(stream), t);
    else hipLaunchKernelGGL(k_track_sizes<false>, dim3(nt), dim3(TT_WG), 0, S_(stream), t);
    hipLaunchKernelGGL(k_track_scan, dim3(1), dim3(1024), 0, S_(stream), t.tile_len, nt, t.tile_off, t.meta);
    return (int)hipGetLastError();
}

int gmk_track_rows(const GmDevTrack& t, void* stream) {
    if (t.n == 0) return 0;
    if (t.kind == GM_TRACK_CALLS) hipLaunchKernelGGL(k_track_rows<true>, dim3(gmk_track_tiles(t.n)), dim3(TT_WG), 0, S_(stream), t);
    else hipLaunchKernelGGL(k_track_rows<false>, dim3(gmk_track_tiles(t.n)), dim3(TT_WG), 0, S_(stream), t);
    return (int)hipGetLastError();
}

// gm_put_e2_hd on the device, one lane per value (gm_dev_fmt_e2)
__global__ void __launch_bounds__(256) k_fmt_e2(const double* v, uint32_t n, char* out, uint8_t* len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    char* w = out + (size_t)i * 16;
    len[i] = (uint8_t)(gm_put_e2_hd(w, v[i]) - w);
}

int gmk_fmt_e2(const double* v, uint32_t n, char* out, uint8_t* len, void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_fmt_e2, dim3((n + 255u) / 256u), dim3(256), 0, S_(stream), v, n, out, len);
    return (int)hipGetLastError();
}
