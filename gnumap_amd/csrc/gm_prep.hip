// gm_prep.hip — k_prep_rows: k_prep (gm_kernels.hip: read self score, -a threshold, status, 2-bit forms) with the read row in REGISTERS.
//
// k_prep stages a tile of reads into LDS with coalesced loads, computes, and stages the next: its wavefronts spent 72 % of their time
// waiting (profiles/r04_sq_counters_1M.txt: SQ_WAIT_ANY / SQ_WAVE_CYCLES), the vector units 35 % busy - the load phase of a tile is not
// overlapped with anything, and three workgroups per CU (50 KB of LDS each) is all that fits.  Here a lane holds its own row (bases and
// qualities: 2 x NCH 8-byte words) in registers and works from them at compile-time byte positions: no tile, no workgroup barrier between
// load and compute, the loads of one wavefront overlap the arithmetic of the others.
//
// The 64 rows of a wavefront are ONE contiguous stretch in HBM (64 x stride bytes = 52 whole lines at stride 104), and so are its 64 rows
// of 2-bit forms (64 x pack_words x 4 bytes).  Both cross LDS as whole 16-byte pieces, lane after lane: on the way in every load
// instruction of the wavefront covers eight consecutive lines and every line is asked for once (a lane that loads its own row makes
// every instruction touch 64 lines, each of them again by seven more instructions: it is fetched once only if it survives in L1 in
// between); all loads of both arrays are issued first, then the bases cross the wavefront's stage and each lane picks its row up, then
// the qualities cross the same bytes, and at the end of the trip the same bytes collect the 2-bit forms on their way out.  The stage is
// private to its wavefront, so the hand-overs need no workgroup barrier.
//
// Arithmetic and outputs are k_prep's, statement by statement (self score = fp32 sum in index order of the per-base terms - the term of a
// base is looked up in the (class, quality character) table built with the reference's expression, bin_seq.cpp:975-987; status / cutoff /
// min_score as Driver.cpp:432-502).  The host launches it for rows of up to 152 bytes; longer rows keep k_prep.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "gm_internal.h"
#include "gm_device.h"

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

// LDS of one wavefront: its 64 input rows of one array (+ 16 bytes: the stretch lies at its HBM address modulo 16) or, later in the same
// trip, its 64 rows of 2-bit forms, whichever is larger (both multiples of 16)
__host__ __device__ static inline uint32_t gm_prep_wave_bytes(uint32_t pw, uint32_t stride) {
    const uint32_t in = 64u * stride + 16u, out = 64u * pw * 4u;
    return in > out ? in : out;
}

// A wavefront's rows r0 .. r0 + rows - 1 of one input array: one contiguous stretch of rows x stride bytes, 8-byte aligned (stride is a
// multiple of 8; a sub-batch view starts at any row).  It is cut at the 16-byte boundaries of HBM: `head` bytes (0 or 8) before the first
// one, `nfull` whole 16-byte pieces, `tail` bytes (0 or 8) after the last - so no load reaches before the first row or past the last one.
struct GmStretch { const uint8_t* p; uint32_t head, nfull, tail; };

__device__ __forceinline__ GmStretch gm_stretch(const uint8_t* rows0, uint32_t r0, uint32_t rows, uint32_t stride) {
    GmStretch s;
    s.p = rows0 + (size_t)(rows ? r0 : 0u) * stride;
    const uint32_t bytes = rows * stride;
    s.head = bytes ? (uint32_t)(reinterpret_cast<uintptr_t>(s.p) & 8u) : 0u;
    s.nfull = (bytes - s.head) >> 4;
    s.tail = (bytes - s.head) & 8u;
    return s;
}

// lane q takes pieces q, q + 64, ...: a load instruction of the wavefront covers 1 KB of consecutive bytes (eight whole lines).  The head
// and the tail ride in one 8-byte load of lanes 0 and 1.
template <int NP>
__device__ __forceinline__ void gm_stretch_load(const GmStretch& s, uint32_t lane, uint4 (&P)[NP], uint2& E) {
    const uint4* const body = reinterpret_cast<const uint4*>(s.p + s.head);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint32_t q = lane + 64u * (uint32_t)j;
        P[j] = make_uint4(0u, 0u, 0u, 0u);
        if (q < s.nfull) P[j] = body[q];
    }
    E = make_uint2(0u, 0u);
    if (lane == 0 && s.head) E = *reinterpret_cast<const uint2*>(s.p);
    if (lane == 1 && s.tail) E = *reinterpret_cast<const uint2*>(s.p + s.head + 16u * (size_t)s.nfull);
}

// the stretch in LDS: byte x at stage + head + x, so that the whole pieces are 16-byte aligned there as they are in HBM
template <int NP>
__device__ __forceinline__ void gm_stretch_store(const GmStretch& s, uint32_t lane, uint8_t* stage, const uint4 (&P)[NP], const uint2& E) {
    uint4* const body = reinterpret_cast<uint4*>(stage + 2u * s.head);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint32_t q = lane + 64u * (uint32_t)j;
        if (q < s.nfull) body[q] = P[j];
    }
    if (lane == 0 && s.head) *reinterpret_cast<uint2*>(stage + s.head) = E;
    if (lane == 1 && s.tail) *reinterpret_cast<uint2*>(stage + 2u * s.head + 16u * (size_t)s.nfull) = E;
}

// a lane's own row out of the stage: the words that hold bases of the read, zero beyond them (and for a lane without a read: L = 0)
template <int NCH>
__device__ __forceinline__ void gm_row_from_stage(const uint8_t* row, uint32_t L, uint2 (&R)[NCH]) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        R[k] = make_uint2(0u, 0u);
        if ((uint32_t)(8 * k) < L) R[k] = *reinterpret_cast<const uint2*>(row + 8 * k);
    }
}

// the stage belongs to one wavefront: its LDS accesses complete in program order, the compiler has to keep that order across lanes
__device__ __forceinline__ void gm_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (waves per SIMD: <13> fits 128 registers without scratch when asked to - 133 and three waves otherwise; <19> holds 10 + 10 pieces: 177)
template <int NCH>
__global__ void __launch_bounds__(256, NCH <= 13 ? 4 : 2) k_prep_rows(GmDevIndex ix, GmDevParams p, GmDevBatch b) {
    __shared__ float s_term[2][10][128];                   // [phred table][char class][quality character & 127]
    __shared__ uint8_t s_cls[256];
    __shared__ int s_other_uniform;
    // per wave: its 64 rows of one input array on their way in, then [64 lanes][pack_words] of 2-bit forms on their way out
    extern __shared__ __attribute__((aligned(16))) uint8_t s_wave[];
    constexpr int NP = (32 * NCH + 63) / 64;               // 16-byte pieces per lane of a stretch of 64 rows of NCH words
    const float4* const S4 = reinterpret_cast<const float4*>(p.S256);
    if (threadIdx.x == 0) s_other_uniform = 1;
    __syncthreads();
    {
        const int ch = threadIdx.x;
        int cl = 8;
        switch (ch) { case 'A': cl = 0; break; case 'C': cl = 1; break; case 'G': cl = 2; break; case 'T': cl = 3; break;
                      case 'a': cl = 4; break; case 'c': cl = 5; break; case 'g': cl = 6; break; case 't': cl = 7; break; default: cl = 8; }
        s_cls[ch] = (uint8_t)cl;
        if (cl == 8) {
            const float4 r0 = S4[(int)'N'], r = S4[ch];
            if (r.x != r0.x || r.y != r0.y || r.z != r0.z || r.w != r0.w) atomicAnd(&s_other_uniform, 0);
        }
    }
    for (int e = threadIdx.x; e < 2 * 9 * 128; e += 256) {
        const int tab = e / (9 * 128), cl = (e / 128) % 9, qc = e & 127;
        // FASTA block: the term of a position depends on its raw character alone - S's row of that character (case-sensitive: Read::seq
        // is the file's text) dotted with the letter's PWM row.  The kernel looks it up with the character in the quality's place:
        // class 8 holds one term per character, the classes of ACGTacgt their one term at every index
        const int ch = b.fasta ? (cl < 8 ? "ACGTacgt"[cl] : qc) : (cl < 8 ? "ACGTacgt"[cl] : 'N');
        const uint32_t mask = b.fasta ? gm_iupac_mask((uint32_t)ch) : gm_code_mask(gm_nt4((uint32_t)ch));
        const float2 pq = b.fasta ? p.lut[GM_LUT_FASTA + mask] : p.lut[tab * 256 + qc];
        const float4 sv = S4[ch];
        const float sarr[4] = { sv.x, sv.y, sv.z, sv.w };
        s_term[tab][cl][qc] = gm_get_val_mask(mask, pq.x, pq.y, sarr);
    }
    __syncthreads();
    const bool uni = b.fasta || s_other_uniform != 0;        // (FASTA: class 8 has every character's own term)
    const uint32_t pw = b.pack ? b.pack_words : 0u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;      // (wave: in a scalar register, and what follows from it)
    uint8_t* const stage = s_wave + (size_t)wave * gm_prep_wave_bytes(pw, b.stride);
    uint32_t* const myrow = reinterpret_cast<uint32_t*>(stage) + (size_t)lane * pw;
    unsigned long long bad = 0, high = 0;
    uint32_t qlo = 255u, qhi = 0u;                           // the range of the quality characters (below 128 when it matters: GMK_QUAL_MIN)
    for (uint32_t base = blockIdx.x * 256u; base < b.n; base += gridDim.x * 256u) {
        const uint32_t r = base + threadIdx.x;
        const bool rv = r < b.n;
        const uint32_t L = rv ? b.len[r] : 0u;
        // ---- the wavefront's stretch of rows through LDS, then the lane's own row into registers ----
        uint2 RB[NCH], RQ[NCH];
        {
            const uint32_t r0 = base + 64u * wave;
            const uint32_t rows = r0 < b.n ? (b.n - r0 < 64u ? b.n - r0 : 64u) : 0u;
            const GmStretch sb = gm_stretch(b.bases, r0, rows, b.stride);
            const GmStretch sq = gm_stretch(b.fasta ? b.bases : b.quals, r0, b.fasta ? 0u : rows, b.stride);
            uint4 PB[NP], PQ[NP];
            uint2 EB, EQ;
            // every load of both arrays goes out before the first LDS store
            gm_stretch_load<NP>(sb, lane, PB, EB);
            gm_stretch_load<NP>(sq, lane, PQ, EQ);
            gm_stretch_store<NP>(sb, lane, stage, PB, EB);
            gm_wave_lds_sync();
            gm_row_from_stage<NCH>(stage + sb.head + (size_t)lane * b.stride, L, RB);
            gm_wave_lds_sync();                           // (every lane has its letters: the stage takes the qualities)
            if (b.fasta) {                                // no quality rows: the letters (7 bits) stand in their place
#pragma unroll
                for (int k = 0; k < NCH; ++k) RQ[k] = make_uint2(RB[k].x & 0x7F7F7F7Fu, RB[k].y & 0x7F7F7F7Fu);
            } else {
                gm_stretch_store<NP>(sq, lane, stage, PQ, EQ);
                gm_wave_lds_sync();
                gm_row_from_stage<NCH>(stage + sq.head + (size_t)lane * b.stride, L, RQ);
                gm_wave_lds_sync();                       // (the same bytes take the 2-bit forms below)
            }
        }
        if (pw) {                                         // the lane's row of the output stretch starts out zero
#pragma unroll 1
            for (uint32_t w = 0; w < pw; w += 4) *reinterpret_cast<uint4*>(myrow + w) = make_uint4(0u, 0u, 0u, 0u);
        }
        const int tab = (rv && r < b.illumina_until) ? 1 : 0;
        const float2* lut = p.lut + tab * 256;
        const float (*term)[128] = s_term[tab];
        float score = 0.0f;
        uint32_t pk = 0, any_n = 0, carry = 0;
        bool nan_l = false;
        uint32_t qor = 0;                                    // OR of the quality words (bit 7 of a byte: a character above 127)
        const uint32_t rsh = 2u * (16u * b.pack_w2 - L);     // the reverse-strand form is the complemented read shifted up to the top of its words
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            if ((uint32_t)(8 * k) < L) {
                const uint2 bw = RB[k], qw = RQ[k];
                if ((uint32_t)(8 * k + 8) <= L) {
                    // a whole word of 8 bases: no per-base conditions, the 8 class reads go out together, then the 8 term reads
                    uint32_t cl[8];
                    float v[8];
#pragma unroll
                    for (uint32_t t = 0; t < 8; ++t) cl[t] = s_cls[((t < 4 ? bw.x : bw.y) >> ((t & 3) * 8)) & 255u];
#pragma unroll
                    for (uint32_t t = 0; t < 8; ++t) v[t] = term[cl[t]][((t < 4 ? qw.x : qw.y) >> ((t & 3) * 8)) & 127u];     // NaN when the probability is negative, like the direct form
                    qor |= qw.x | qw.y;
#pragma unroll
                    for (uint32_t t = 0; t < 8; t += 2) {
                        const uint32_t q0 = ((t < 4 ? qw.x : qw.y) >> ((t & 3) * 8)) & 127u, q1 = ((t < 4 ? qw.x : qw.y) >> (((t + 1) & 3) * 8)) & 127u;
                        qlo = min(qlo, min(q0, q1)); qhi = max(qhi, max(q0, q1));         // (v_min3 / v_max3)
                    }
#pragma unroll
                    for (uint32_t t = 0; t < 8; ++t) {
                        pk |= (cl[t] & 3u) << ((((uint32_t)(8 * k) & 8u) + t) << 1); any_n |= cl[t];
                        score = __fadd_rn(score, v[t]);
                    }
#pragma unroll
                    for (uint32_t t = 0; t < 8; t += 2) nan_l |= __builtin_isunordered(v[t], v[t + 1]);
                } else {
#pragma unroll 1
                    for (uint32_t t = 0; t < L - (uint32_t)(8 * k); ++t) {              // the last, partial word
                        const uint32_t ch = ((t < 4 ? bw.x : bw.y) >> ((t & 3) * 8)) & 255u;
                        const uint32_t qc = ((t < 4 ? qw.x : qw.y) >> ((t & 3) * 8)) & 255u;
                        const uint32_t c1 = s_cls[ch];
                        const float v1 = term[c1][qc & 127u];
                        pk |= (c1 & 3u) << ((((uint32_t)(8 * k) & 8u) + t) << 1); any_n |= c1;
                        qor |= qc;
                        qlo = min(qlo, qc); qhi = max(qhi, qc);
                        nan_l |= v1 != v1;
                        score = __fadd_rn(score, v1);
                    }
                }
                if (pw && ((k & 1) || (uint32_t)(8 * k + 8) >= L)) {          // a word of 16 bases is complete (or the read ends)
                    const uint32_t w = (uint32_t)k >> 1;
                    uint32_t rvw = __brev(pk);
                    rvw = ((rvw >> 1) & 0x55555555u) | ((rvw & 0x55555555u) << 1);       // 2-bit groups in reverse order
                    myrow[1u + b.pack_w2 - 1u - w] = rvw;
                    const uint32_t g = ~pk, bs = rsh & 31u;
                    uint32_t* const rform = myrow + b.pack_w2 + 2u + (rsh >> 5);
                    rform[w] = (g << bs) | carry;
                    carry = bs ? g >> (32u - bs) : 0u;
                    if ((uint32_t)(8 * k + 8) >= L) rform[w + 1u] = carry;   // the word above the last one takes what was shifted out (its own padding word when bs = 0)
                    pk = 0;
                }
            }
        }
        any_n >>= 3;                                         // (classes are 0..8: bit 3 of their OR = some character outside ACGTacgt)
        if ((qor & 0x80808080u) || (any_n && !uni)) {
            // a quality character above 127, or a row of S the caller edited (-S file), somewhere in the read: the whole sum again with the
            // direct form for those bases (rare; one copy of this code instead of one per unrolled base - the row is still in cache)
            const uint8_t* rb = b.bases + (size_t)r * b.stride;
            const uint8_t* rq = b.quals + (size_t)r * b.stride;
            score = 0.0f; nan_l = false;
#pragma unroll 1
            for (uint32_t i = 0; i < L; ++i) {
                const uint32_t ch = rb[i], qc = rq[i];
                const uint32_t cl = s_cls[ch];
                float v;
                if (qc < 128u && (cl < 8u || uni)) {
                    v = term[cl][qc];
                } else {
                    const float2 pq = lut[qc];
                    const float4 sv = S4[ch];
                    const float s4[4] = { sv.x, sv.y, sv.z, sv.w };
                    v = gm_get_val(gm_nt4(ch), pq.x, pq.y, s4);
                }
                nan_l |= v != v;
                if (qc >= 128u) high = 1;                    // (k_nw_rows' table of row values covers the characters below 128)
                score = __fadd_rn(score, v);
            }
        }
        if (nan_l) bad = 1;                                  // negative probability (SeqReader.cpp:1171-1189)
        if (rv) {
            int8_t st = 0;
            float self = 0.0f;
            double mn;
            if (L < (uint32_t)p.mer) {
                st = -2;                                     // READ_TOO_SHORT
                mn = 0.0;
            } else if (p.nw) {
                float v = 0.0f;                              // get_align_score(read,cons,0,L-1): begin(=0) + mid + end(=0)
                v = __fadd_rn(v, 0.0f); v = __fadd_rn(v, score); v = __fadd_rn(v, 0.0f);
                self = v;
                if ((double)self < (double)p.cutoff) st = -3;    // READ_TOO_POOR
                mn = p.align_is_fraction ? (double)p.align_score * (double)self : (double)p.align_score;
            } else {
                mn = (double)p.kmin;                         // Driver.cpp:502
            }
            b.status[r] = st;
            if (pw) myrow[0] = L | (any_n << 16) | ((st != 0 ? 1u : 0u) << 17);
            b.self_score[r] = self;
            b.min_score[r] = mn;
            b.top_score[r] = 0.0f;
            b.hit_count[r] = 0;
            b.hit_cursor[r] = 0;
        }
        if (pw) {
            // the wavefront's 64 rows are one stretch of pack[]: out in 16-byte pieces, lane after lane
            __syncthreads();
            const uint32_t r0 = base + 64u * wave;
            if (r0 < b.n) {
                const uint32_t rows = b.n - r0 < 64u ? b.n - r0 : 64u;
                const uint32_t pieces = rows * pw / 4u;                         // (pack_words is a multiple of 4)
                const uint4* src = reinterpret_cast<const uint4*>(stage);
                uint4* dst = reinterpret_cast<uint4*>(b.pack + (size_t)r0 * pw);
                for (uint32_t q = lane; q < pieces; q += 64u) dst[q] = src[q];
            }
            __syncthreads();
        }
    }
    gm_count(b, GMK_BAD_QUAL, bad);
    gm_count(b, GMK_HIGH_QUAL, high);
    gm_count_qual_range(b, qlo, qhi);
}

int gmk_prep_rows(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, void* stream) {
    if (b.n == 0) return 0;
    if (b.stride > 152) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(b.bases) | reinterpret_cast<uintptr_t>(b.quals) | b.stride) & 7u) return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)4 * gm_prep_wave_bytes(b.pack ? b.pack_words : 0u, b.stride);
    const uint32_t grid = gm_test_grid((uint32_t)std::min<uint64_t>(((uint64_t)b.n + 255) / 256, 256ull * 5 * 4));
    if (b.stride <= 104) hipLaunchKernelGGL((k_prep_rows<13>), dim3(grid), dim3(256), lds, S_(stream), ix, p, b);
    else hipLaunchKernelGGL((k_prep_rows<19>), dim3(grid), dim3(256), lds, S_(stream), ix, p, b);
    return (int)hipGetLastError();
}
