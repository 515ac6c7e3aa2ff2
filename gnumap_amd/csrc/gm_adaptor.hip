// gm_adaptor.hip — k_adaptor_trim: -A / --adaptor, the reference's SeqReader::FixReads2 with SeqReader::Compare
// (src/SeqReader.cpp:1146-1150, 1294-1305, 1356-1372) for a whole block of reads in HBM.
//
// The rule, quirks included: J = the smallest offset i in [0, L - 4) at which the adaptor and the read agree in at least 85 % of the
// j = min(|adaptor|, L - i) characters compared from i on - `(float)num_same / j >= 0.85f`, an IEEE fp32 division and compare on the
// raw characters, case-sensitive -, or L - 4 when no offset qualifies (FixReads2 has no "chop only more than gMIN_CHOPPED_BASES"
// guard: a read without any adaptor loses its last four bases).  L < 4, where the reference's unsigned bound wraps, gives 0.
//
// One wavefront per read, four wavefronts per workgroup, each on its own from the first read on.  The read's bytes go into the wavefront's own stretch of LDS with
// 8-byte loads (rows are 8-byte aligned: stride is a multiple of 8); the adaptor sits in LDS once per workgroup, as 32-bit words.  A
// pass covers 64 offsets, one per lane.  A lane walks its window four characters at a time: one aligned LDS word per step, joined to
// the previous one by v_alignbit (the window starts at any byte), XORed with the adaptor's word (a broadcast), the equal bytes counted
// with a few bit operations and a mask for the characters beyond j.  Then ONE __fdiv_rn and ONE compare per lane, and the first
// qualifying lane comes out of a ballot; the first pass with a qualifier ends the read.  A lane that can no longer reach even 84 %
// stops mattering (integer test, strictly below the threshold whatever the rounding of the division), and a pass ends as soon as no
// lane is left: on reads without adaptor after 8 .. 16 of the 34 characters.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "gm_internal.h"

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define GA_MAX_LEN 2048u
#define GA_ROW (GA_MAX_LEN + 128u)          // a lane's last word lies at most 63 + 3 + 7 bytes behind the read's end

__global__ void __launch_bounds__(256) k_adaptor_trim(const uint8_t* __restrict__ bases, uint32_t stride, const uint16_t* __restrict__ len, uint32_t n,
                                                      const uint8_t* __restrict__ adaptor, uint32_t a_len, uint16_t* __restrict__ out_len) {
    __shared__ __attribute__((aligned(8))) uint8_t s_read[4][GA_ROW];
    __shared__ uint32_t s_ad[GM_ADAPTOR_MAX / 4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (threadIdx.x < GM_ADAPTOR_MAX / 4) {                                      // the adaptor as little-endian words, zero beyond its end (masked below)
        uint32_t w = 0;
        for (uint32_t q = 0; q < 4u; ++q) { const uint32_t t = 4u * threadIdx.x + q; if (t < a_len) w |= (uint32_t)adaptor[t] << (8u * q); }
        s_ad[threadIdx.x] = w;
    }
    __syncthreads();
    uint8_t* const rd = s_read[wv];
    const uint32_t* const rd32 = reinterpret_cast<const uint32_t*>(rd);
    // a wavefront and its row of LDS are on their own from here on: no workgroup barrier couples a read without adaptor (a few steps per
    // pass) to a neighbour that has one (all of them); the wavefront-scope fences order its own LDS stores and loads
    for (uint32_t r = blockIdx.x * 4u + wv; r < n; r += gridDim.x * 4u) {
        const bool live = true;
        uint32_t L = len[r];
        if (L > stride) L = stride;
        if (L > GA_MAX_LEN) L = GA_MAX_LEN;
        if (live) {
            const uint2* src = reinterpret_cast<const uint2*>(bases + (size_t)r * stride);
            uint2* dst = reinterpret_cast<uint2*>(rd);
            for (uint32_t w = lane; 8u * w < L; w += 64u) dst[w] = src[w];       // (8 w + 7 < stride: stride is a multiple of 8)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (live) {
            const uint32_t n_off = L > 4u ? L - 4u : 0u;
            uint32_t J = n_off;
            for (uint32_t base = 0; base < n_off; base += 64u) {
                const uint32_t i = base + lane;
                const bool act = i < n_off;
                const uint32_t j = act ? min(a_len, L - i) : 0u;               // >= 1 for an active lane (L - i >= 5, a_len >= 1)
                const uint32_t nd = (min(a_len, L - base) + 3u) >> 2;            // words of the longest compare of the pass (lane 0)
                const uint32_t sh = (i & 3u) << 3, w0 = i >> 2;
                uint32_t lo = rd32[w0], cnt = 0;
                for (uint32_t t = 0; t < nd; ++t) {
                    const uint32_t done = 4u * t;
                    // still able to reach 84 % of j with every character left matching?  (strictly below 0.85f: such a lane cannot qualify)
                    if ((t & 1u) == 0u && !__any(done < j && (cnt + (j - done)) * 100u >= 84u * j)) break;
                    const uint32_t hi = rd32[w0 + t + 1u];                      // (inside the row: 4 (w0 + t + 1) + 3 <= L + 73)
                    uint32_t x = __funnelshift_r(lo, hi, sh) ^ s_ad[t];         // the read's bytes i + 4 t .. + 3 against the adaptor's
                    lo = hi;
                    x |= x >> 4; x |= x >> 2; x |= x >> 1;                      // bit 0 of a byte: the byte is not zero
                    const int left = (int)j - (int)done;                         // characters of this word that count
                    const uint32_t keep = left >= 4 ? 0x01010101u : left <= 0 ? 0u : (((1u << (8 * left)) - 1u) & 0x01010101u);
                    cnt += (uint32_t)__popc(~x & keep);
                }
                bool ok = false;
                if (act) ok = __fdiv_rn((float)cnt, (float)j) >= 0.85f;          // (float)num_same / j >= gMIN_ADAPTOR_DIFF
                const unsigned long long m = __ballot(ok);
                if (m) { J = base + (uint32_t)__ffsll((long long)m) - 1u; break; }
            }
            if (lane == 0) out_len[r] = (uint16_t)J;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      // the row is free for the next read
    }
}

// --no_nw with -A: the CIGAR of a record is "<n>M" with n = the length of the WHOLE sequence line (consensus.size(), ScoredSeq.h:365),
// which may have more digits than the CIGAR of the kept part that sized the record's slot in the pool: cig_all[m] = at least digits + 'M' + NUL
__global__ void __launch_bounds__(256) k_adaptor_cigar_room(const GmDevMatch* matches, uint32_t n_m, const uint16_t* full_len, uint32_t n, uint32_t* cig_all) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_m) return;
    const uint32_t r = matches[m].read;
    if (r >= n) return;
    const uint32_t L = full_len[r];
    const uint32_t need = (L >= 1000u ? 4u : L >= 100u ? 3u : L >= 10u ? 2u : 1u) + 2u;
    if (cig_all[m] < need) cig_all[m] = need;
}

int gmk_adaptor_cigar_room(const GmDevMatch* matches, uint32_t n_m, const uint16_t* full_len, uint32_t n, uint32_t* cig_all, void* stream) {
    if (n_m == 0) return 0;
    hipLaunchKernelGGL(k_adaptor_cigar_room, dim3((n_m + 255u) / 256u), dim3(256), 0, S_(stream), matches, n_m, full_len, n, cig_all);
    return (int)hipGetLastError();
}

int gmk_adaptor_trim(const uint8_t* bases, uint32_t stride, const uint16_t* len, uint32_t n, const uint8_t* adaptor, uint32_t a_len, uint16_t* out_len, void* stream) {
    if (n == 0) return 0;
    if (a_len == 0 || a_len > GM_ADAPTOR_MAX || stride % 8u != 0 || stride > GA_MAX_LEN) return (int)hipErrorInvalidValue;
    const uint32_t grid = gm_test_grid((uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 256ull * 8 * 4));
    hipLaunchKernelGGL(k_adaptor_trim, dim3(grid), dim3(256), 0, S_(stream), bases, stride, len, n, adaptor, a_len, out_len);
    return (int)hipGetLastError();
}
