// gm_bam.hip — BAM from the device: the records of a block in the binary layout of SAMv1 section 4.2, and BGZF (RFC 1952 members of at
// most 64 KiB with the `BC` extra subfield, SAMv1 section 4.1) around any bytes, both written where the rows already are.
//
//   k_bam_sizes   one lane per record, after k_out_text_sizes (which has left the CIGAR lengths in the record's slot and has checked
//                 XA / XP against the domain the text form prints): operations and reference length of the CIGAR field as the SAM row
//                 prints it, reg2bin, the record's size
//   k_bam_rows    one wavefront per record: the fixed 36 bytes and the three tags through LDS, then name, CIGAR, SEQ nibbles and QUAL
//                 byte-wise; every store stays inside the span the scan gave the record
//   bz_*          the steps of a BGZF block, written once for both deflate kernels: bz_load (the payload into LDS), bz_crc_table and
//                 bz_crc_hist (CRC-32 by sub-chunks folded with crc(A|B) = crc(A) * x^(8|B|) ^ crc(B), the bytes into a histogram),
//                 bz_rank and bz_build_code (a length-limited canonical code, built by one lane), bz_put_block_header, bz_lane_start
//                 (a lane's first bit from the prefix sum of the lanes' bit counts), bz_put_eob, bz_write_member
//   k_bgzf_deflate  one workgroup per payload of at most 65280 bytes, held in LDS: a stored block (level 0) or one dynamic-Huffman
//                 block over literals only (level 1) into the payload's worst-case slot
//   k_bgzf_deflate_lz  level 1 | GM_BGZF_LZ77: the same payload, slot and size, one dynamic-Huffman block over literals and LZ77 matches -
//                 a persistent grid with a token area per workgroup; what it finds is described above the kernel and in DESIGN.md
//   k_bgzf_compact  after the scan of the blocks' sizes: the slots side by side, so that one contiguous run crosses the link
//
// With a row source (GmDevText::row_src, gm_batch_set_unmapped_rows) both record kernels go over ROWS: a read without a record gets
// refID -1, pos -1, bin 4680, MAPQ 0, flag 4, no operation, SEQ / QUAL of a plus-strand record and the one tag YU:i:<status>.
// A record is pinned to the SAM row k_out_text_rows prints for it.  One difference is the format's own: l_read_name is one byte, so
// read_name holds the first 254 bytes of the name (the SAM row keeps up to 1023).
// The output bytes are a function of the input bytes and the level alone: the only atomics are integer adds into the histograms, ORs
// into words of the bit stream and, in k_bgzf_deflate_lz, maxima of positions into the hash table - none of their results depends on the
// order in which they land, and a barrier lies between the maxima and the lookups that read them.
#include "gm_lib.h"
#include "gm_fmt_dev.h"
#include "gm_mdtag_dev.h"
#include <algorithm>
#include <memory>

namespace {

constexpr uint32_t BZ_PAYLOAD = GM_BGZF_PAYLOAD;    // bytes of input per BGZF block
constexpr uint32_t BZ_EXTRA = 31;                   // 18 header + 5 stored-block header + 8 trailer: the largest block is BZ_PAYLOAD + BZ_EXTRA
constexpr uint32_t BZ_SLOT = 65312;                 // worst-case slot of a block, a multiple of 16
constexpr uint32_t BZ_OUT_WORDS = (BZ_PAYLOAD + 16) / 4;
constexpr uint32_t BZ_LDS = BZ_PAYLOAD + BZ_OUT_WORDS * 4;
constexpr uint32_t BZ_FIX_BITS = 3 + 5 + 5 + 4 + 19 * 3;     // BFINAL, BTYPE, HLIT, HDIST, HCLEN = 19, the code-length code: 19 lengths of 3 bits
constexpr uint32_t BZ_HDR_BITS = BZ_FIX_BITS + 4 * (257 + 1);        // the header over literals alone: 257 + 1 code lengths of 4 bits, not run-length coded
constexpr uint32_t BZ_POLY = 0xEDB88320u;

// a * b mod P over GF(2), operands and result bit-reflected as the CRC register is (x^0 = 0x80000000)
__device__ __forceinline__ uint32_t bz_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ BZ_POLY : b >> 1;
    }
    return p;
}
// x^(8k) mod P
__device__ __forceinline__ uint32_t bz_xpow8(uint32_t k) {
    uint32_t r = 0x80000000u, base = 0x00800000u;
    for (; k; k >>= 1) { if (k & 1u) r = bz_mul(r, base); base = bz_mul(base, base); }
    return r;
}

struct BzBits {                                     // one lane's writer into the block's bit stream (LSB first, RFC 1951 section 3.1.1)
    uint32_t* out; uint32_t w, nb; unsigned long long acc;
    __device__ __forceinline__ void start(uint32_t* o, uint32_t bit) { out = o; w = bit >> 5; nb = bit & 31u; acc = 0; }
    __device__ __forceinline__ void put(uint32_t v, uint32_t n) {
        acc |= (unsigned long long)v << nb; nb += n;
        if (nb >= 32u) { atomicOr(&out[w], (uint32_t)acc); acc >>= 32; nb -= 32u; ++w; }
    }
    __device__ __forceinline__ void code(uint32_t c) { put(c & 0xFFFFu, c >> 16); }     // a symbol's code as bz_build_code leaves it
    __device__ __forceinline__ void flush() { if (nb) atomicOr(&out[w], (uint32_t)acc); }
};

// ------------------------------------------------------------------------------------------------
// The steps of a block, for the 256 lanes of a workgroup.  All of them are inlined into the kernels, so their pointers stay LDS
// pointers.  The ones with a barrier inside are called by all lanes under uniform control flow.
// ------------------------------------------------------------------------------------------------
// lane tid's run [*a, *e) of n items cut into 256 contiguous runs
__device__ __forceinline__ void bz_run(uint32_t n, uint32_t tid, uint32_t* a, uint32_t* e) {
    const uint32_t per = (n + 255u) >> 8;
    *a = tid * per < n ? tid * per : n; *e = *a + per < n ? *a + per : n;
}
// The payload into LDS, 16 bytes a load where the source is aligned.  No barrier: one before s_in is read
__device__ __forceinline__ void bz_load(const uint8_t* __restrict__ src, uint32_t len, uint8_t* s_in, uint32_t tid) {
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        const uint32_t n16 = len >> 4;
        for (uint32_t q = tid; q < n16; q += 256u) reinterpret_cast<uint4*>(s_in)[q] = reinterpret_cast<const uint4*>(src)[q];
        for (uint32_t i = (n16 << 4) + tid; i < len; i += 256u) s_in[i] = src[i];
    } else
        for (uint32_t i = tid; i < len; i += 256u) s_in[i] = src[i];
}
// The CRC-32 table, an entry per lane.  No barrier: one before bz_crc_hist
__device__ __forceinline__ void bz_crc_table(uint32_t* s_tab, uint32_t tid) {
    uint32_t c = tid;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? BZ_POLY ^ (c >> 1) : c >> 1;
    s_tab[tid] = c;
}
// A lane's run of the payload: its CRC-32 and, with count (uniform; level 0 has no use for the atomics), its bytes into hist; the
// runs' CRCs folded into the payload's, which every lane gets back.  Two barriers: behind them hist is complete and s_wave is free again
__device__ __forceinline__ uint32_t bz_crc_hist(const uint8_t* s_in, uint32_t len, const uint32_t* s_tab, bool count, uint32_t* hist, uint32_t* s_wave, uint32_t tid) {
    uint32_t a, e;
    bz_run(len, tid, &a, &e);
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = a; i < e; ++i) {
        const uint32_t by = s_in[i];
        crc = s_tab[(crc ^ by) & 255u] ^ (crc >> 8);
        if (count) atomicAdd(&hist[by], 1u);
    }
    crc ^= 0xFFFFFFFFu;                              // (an empty run: 0)
    uint32_t part = a < e ? bz_mul(bz_xpow8(len - e), crc) : 0u;
    for (int off = 32; off; off >>= 1) part ^= __shfl_xor(part, off);
    if ((tid & 63u) == 0) s_wave[tid >> 6] = part;
    __syncthreads();
    const uint32_t crc_all = s_wave[0] ^ s_wave[1] ^ s_wave[2] ^ s_wave[3];
    __syncthreads();
    return crc_all;
}
// Every symbol in use finds its rank in ascending (count, symbol) order: ord[rank] = symbol.  No barrier: one before ord is read
__device__ __forceinline__ void bz_rank(const uint32_t* hist, uint32_t nsym, uint16_t* ord, uint32_t tid) {
    for (uint32_t s = tid; s < nsym; s += 256u) {
        const uint32_t c = hist[s];
        if (!c) continue;
        uint32_t rank = 0;
        for (uint32_t q = 0; q < nsym; ++q) { const uint32_t cq = hist[q]; rank += (cq && (cq < c || (cq == c && q < s))) ? 1u : 0u; }
        ord[rank] = (uint16_t)s;
    }
}
// One lane: the code of the symbols in use into code[] (length << 16 | code; zero beforehand) - Huffman's algorithm on the sorted
// leaves, flatter counts and again while a leaf lies deeper than deflate's 15 bits, canonical codes (RFC 1951 section 3.2.2) kept
// bit-reversed: Huffman codes enter the stream from their most significant bit.  One symbol in use takes the one-bit code 0.
// wt, par, dep: 2 * nsym entries each.  Returns the bits the symbols take under the code, sum of count * length.  No barrier
__device__ __forceinline__ uint32_t bz_build_code(const uint32_t* hist, uint32_t nsym, const uint16_t* ord, uint32_t* wt, uint16_t* par, uint8_t* dep, uint32_t* code) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < nsym; ++s) m += hist[s] ? 1u : 0u;
    if (m == 0) return 0;
    if (m == 1) { code[ord[0]] = 1u << 16; return hist[ord[0]]; }
    for (uint32_t i = 0; i < m; ++i) wt[i] = hist[ord[i]];
    for (;;) {
        // the leaves [0, m) and the nodes made so far [m, nn) are two ascending queues
        uint32_t li = 0, ni = m, nn = m;
        while (nn < 2u * m - 1u) {
            uint32_t pick[2];
            for (int k = 0; k < 2; ++k) pick[k] = (li < m && (ni >= nn || wt[li] <= wt[ni])) ? li++ : ni++;
            wt[nn] = wt[pick[0]] + wt[pick[1]];
            par[pick[0]] = par[pick[1]] = (uint16_t)nn;
            ++nn;
        }
        dep[2u * m - 2u] = 0;
        uint32_t deepest = 0;
        for (uint32_t i = 2u * m - 2u; i-- > 0;) {
            const uint32_t d = (uint32_t)dep[par[i]] + 1u;
            dep[i] = (uint8_t)(d < 255u ? d : 255u);
            if (i < m && d > deepest) deepest = d;
        }
        if (deepest <= 15u) break;
        for (uint32_t i = 0; i < m; ++i) wt[i] = (wt[i] + 1u) >> 1;      // (the order stays ascending)
    }
    uint32_t cnt[16], next[16];
    for (int k = 0; k < 16; ++k) cnt[k] = 0;
    for (uint32_t i = 0; i < m; ++i) { ++cnt[dep[i]]; code[ord[i]] = (uint32_t)dep[i] << 16; }
    uint32_t c = 0, bits = 0;
    next[0] = 0;
    for (int k = 1; k < 16; ++k) { c = (c + cnt[k - 1]) << 1; next[k] = c; }
    for (uint32_t s = 0; s < nsym; ++s) {
        const uint32_t l = code[s] >> 16;
        if (!l) continue;
        code[s] = (l << 16) | (__brev(next[l]++) >> (32u - l));
        bits += hist[s] * l;
    }
    return bits;
}
// One lane: the header of the dynamic block at bit 0 of s_out - BFINAL, BTYPE, HLIT, HDIST, HCLEN, then every code length in four
// bits (code-length symbols 0 .. 15, whose canonical code is their value; 16 .. 18, the run lengths, are not used; the 19 lengths are
// transmitted in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15): nl of lcode, nd of dcode.  dcode == nullptr, or no
// distance in use: one distance code of length 1, never used.  BZ_FIX_BITS + 4 * (nl + nd) bits.  No barrier
__device__ __forceinline__ void bz_put_block_header(uint32_t* s_out, const uint32_t* lcode, uint32_t nl, const uint32_t* dcode, uint32_t nd) {
    BzBits w; w.start(s_out, 0);
    w.put(1u, 1); w.put(2u, 2); w.put(nl - 257u, 5); w.put(nd - 1u, 5); w.put(15u, 4);
    for (int k = 0; k < 19; ++k) w.put(k < 3 ? 0u : 4u, 3);
    for (uint32_t s = 0; s < nl; ++s) w.put(__brev(lcode[s] >> 16) >> 28, 4);
    if (dcode && dcode[nd - 1u])
        for (uint32_t d = 0; d < nd; ++d) w.put(__brev(dcode[d] >> 16) >> 28, 4);
    else
        w.put(__brev(1u) >> 28, 4);
    w.flush();
}
// The lane's first bit behind the header's end, from the prefix sum of the lanes' bit counts.  One barrier; s_wave is read behind it
__device__ __forceinline__ uint32_t bz_lane_start(uint32_t nbits, uint32_t* s_wave, uint32_t lane, uint32_t wv) {
    uint32_t incl = nbits;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(incl, off); if ((int)lane >= off) incl += t; }
    if (lane == 63u) s_wave[wv] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t q = 0; q < wv; ++q) before += s_wave[q];
    return before + incl - nbits;
}
// One lane: the end-of-block code c, the last bits of a stream of total_bits.  No barrier: one before the stream is read
__device__ __forceinline__ void bz_put_eob(uint32_t* s_out, uint32_t c, uint32_t total_bits) {
    BzBits z; z.start(s_out, total_bits - (c >> 16)); z.code(c); z.flush();
}
// The member into its slot o: the 18 bytes of header, the stream of total_bits in s_out (huff) or the stored block of s_in, CRC-32,
// ISIZE.  Returns BSIZE.  No barrier: the stream is complete before, and s_in and s_out are still being read behind it
__device__ __forceinline__ uint32_t bz_write_member(uint8_t* __restrict__ o, bool huff, uint32_t total_bits, uint32_t len, const uint32_t* s_out, const uint8_t* s_in,
                                                    uint32_t crc_all, uint32_t tid) {
    const uint32_t body = huff ? (total_bits + 7u) >> 3 : len + 5u;
    const uint32_t bsize = 18u + body + 8u;
    if (tid < 18u) {
        const uint32_t bs1 = bsize - 1u;
        const uint8_t hd[18] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bs1 & 255u), (uint8_t)(bs1 >> 8) };
        o[tid] = hd[tid];
    }
    if (huff) {
        const uint8_t* const sb = reinterpret_cast<const uint8_t*>(s_out);
        for (uint32_t i = tid; i < body; i += 256u) o[18u + i] = sb[i];
    } else {
        if (tid < 5u) {
            const uint32_t nl = ~len & 0xFFFFu;
            const uint8_t sh[5] = { 1, (uint8_t)(len & 255u), (uint8_t)(len >> 8), (uint8_t)(nl & 255u), (uint8_t)(nl >> 8) };
            o[18u + tid] = sh[tid];
        }
        for (uint32_t i = tid; i < len; i += 256u) o[23u + i] = s_in[i];
    }
    if (tid < 8u) { const uint32_t v = tid < 4u ? crc_all : len; o[18u + body + tid] = (uint8_t)(v >> (8u * (tid & 3u))); }
    return bsize;
}

__global__ void __launch_bounds__(256) k_bgzf_deflate(const uint8_t* __restrict__ in, unsigned long long n, int level, uint8_t* __restrict__ slots,
                                                      uint32_t* __restrict__ sizes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    uint8_t* const s_in = s_dyn;
    uint32_t* const s_out = reinterpret_cast<uint32_t*>(s_dyn + BZ_PAYLOAD);
    __shared__ uint32_t s_tab[256], s_hist[257], s_code[257], s_wt[514], s_wave[4], s_misc[4];
    __shared__ uint16_t s_par[514], s_ord[257];
    __shared__ uint8_t s_dep[514];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const unsigned long long p0 = (unsigned long long)blockIdx.x * BZ_PAYLOAD;
    if (p0 >= n) return;
    const uint32_t len = (uint32_t)(n - p0 < BZ_PAYLOAD ? n - p0 : BZ_PAYLOAD);
    // ---- the payload into LDS, the CRC table, an empty histogram and bit stream ----
    bz_load(in + p0, len, s_in, tid);
    bz_crc_table(s_tab, tid);
    for (uint32_t i = tid; i < 257u; i += 256u) s_hist[i] = i == 256u ? 1u : 0u;          // the end-of-block symbol occurs once
    if (level == 1) for (uint32_t i = tid; i < BZ_OUT_WORDS; i += 256u) s_out[i] = 0;
    __syncthreads();
    const uint32_t crc_all = bz_crc_hist(s_in, len, s_tab, level == 1, s_hist, s_wave, tid);
    bool huff = false;
    uint32_t total_bits = 0;
    if (level == 1) {
        bz_rank(s_hist, 257u, s_ord, tid);
        for (uint32_t s = tid; s < 257u; s += 256u) s_code[s] = 0;
        __syncthreads();
        if (tid == 0) {                              // the code, the block's bits and its header in one stretch
            const uint32_t bits = BZ_HDR_BITS + bz_build_code(s_hist, 257u, s_ord, s_wt, s_par, s_dep, s_code);
            const bool use = (bits + 7u) / 8u < len + 5u;                                 // not smaller than stored: stored
            s_misc[0] = use ? 1u : 0u; s_misc[1] = bits;
            if (use) bz_put_block_header(s_out, s_code, 257u, nullptr, 1u);
        }
        __syncthreads();
        huff = s_misc[0] != 0; total_bits = s_misc[1];
        if (huff) {
            // ---- every lane's bit count, their prefix sum, and the lane's codes ORed into the stream behind the header ----
            uint32_t a, e, nbits = 0;
            bz_run(len, tid, &a, &e);
            for (uint32_t i = a; i < e; ++i) nbits += s_code[s_in[i]] >> 16;
            BzBits w; w.start(s_out, BZ_HDR_BITS + bz_lane_start(nbits, s_wave, lane, wv));
            for (uint32_t i = a; i < e; ++i) w.code(s_code[s_in[i]]);
            w.flush();
            if (tid == 0) bz_put_eob(s_out, s_code[256], total_bits);
            __syncthreads();
        }
    }
    const uint32_t bsize = bz_write_member(slots + (size_t)blockIdx.x * BZ_SLOT, huff, total_bits, len, s_out, s_in, crc_all, tid);
    if (tid == 0) sizes[blockIdx.x] = bsize;
}

// ------------------------------------------------------------------------------------------------
// level 1 | GM_BGZF_LZ77: one dynamic-Huffman block over literals and LZ77 matches ("BGZF with LZ77 matches")
// ------------------------------------------------------------------------------------------------
constexpr uint32_t LZ_HEAD = 8192;                  // entries of the hash table; it lies where the bit stream is built afterwards
constexpr uint32_t LZ_MIN = 4, LZ_MAX = 258, LZ_WINDOW = 32768;
constexpr uint32_t LZ_NL = 286, LZ_ND = 30;         // literal/length and distance symbols
constexpr uint32_t LZ_MATCH = 0x80000000u;          // a token: a literal's byte, or LZ_MATCH | (length - 3) << 16 | (distance - 1)

// the four bytes at byte q of an array of words (LDS takes no unaligned word); reads the word behind q's as well
__device__ __forceinline__ uint32_t lz_get32(const uint32_t* w, uint32_t q) { return __builtin_amdgcn_alignbyte(w[(q >> 2) + 1u], w[q >> 2], q & 3u); }
// RFC 1951 section 3.2.5: length - 3 -> symbol - 257, distance - 1 -> symbol; *nx extra bits of value *xv
__device__ __forceinline__ uint32_t lz_len_sym(uint32_t y, uint32_t* nx, uint32_t* xv) {
    if (y < 8u || y == 255u) { *nx = 0; *xv = 0; return y < 8u ? y : 28u; }
    const uint32_t n = 31u - (uint32_t)__clz((int)y);
    *nx = n - 2u; *xv = y & ((1u << (n - 2u)) - 1u);
    return 4u * (n - 1u) + ((y >> (n - 2u)) & 3u);
}
__device__ __forceinline__ uint32_t lz_dist_sym(uint32_t x, uint32_t* nx, uint32_t* xv) {
    if (x < 4u) { *nx = 0; *xv = 0; return x; }
    const uint32_t n = 31u - (uint32_t)__clz((int)x);
    *nx = n - 1u; *xv = x & ((1u << (n - 1u)) - 1u);
    return 2u * n + ((x >> (n - 1u)) & 1u);
}
__device__ __forceinline__ uint32_t lz_len_extra(uint32_t i) { return i < 8u || i == 28u ? 0u : (i >> 2) - 1u; }      // of length symbol 257 + i
__device__ __forceinline__ uint32_t lz_dist_extra(uint32_t d) { return d < 4u ? 0u : (d >> 1) - 1u; }


// A persistent grid: workgroup g takes payloads g, g + gridDim.x, ... and keeps their tokens in its own tokens[g * BZ_PAYLOAD ...).
// Per payload:
//   1. the payload into LDS, its CRC-32 and the histogram of its bytes
//   2. the matches, in tiles of 256 positions, one per lane: the lane's candidate is head[hash of its 4 bytes] - the largest position of
//      an EARLIER tile with that hash, put there with atomicMax behind a barrier, so what a lane finds does not depend on timing -,
//      compared forward byte for byte (up to 258, never past the payload's end); a match counts from 4 bytes and within 32768.  The
//      greedy parse of the tile - from where the last token of the tile before ended, next[p] = p + max(length, 1) - is marked by
//      pointer doubling in 8 steps; the marked positions are the tokens: counted into the two histograms, ranked by a prefix sum over
//      the tile and written to the workgroup's token area
//   3. the two codes, and level 1's code over the bytes, built side by side by one lane each of waves 0, 1 and 2; the smallest of the
//      matched form, level 1's form and the stored form is written - so a block is never larger than level 1 writes it
//   4. every lane a contiguous run of tokens (or bytes): its bit count, a prefix sum, its codes and extra bits ORed into the stream
__global__ void __launch_bounds__(256) k_bgzf_deflate_lz(const uint8_t* __restrict__ in, unsigned long long n, uint32_t n_blocks, uint8_t* __restrict__ slots,
                                                         uint32_t* __restrict__ sizes, uint32_t* tokens) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    uint8_t* const s_in = s_dyn;
    const uint32_t* const s_in32 = reinterpret_cast<const uint32_t*>(s_dyn);
    uint32_t* const s_out = reinterpret_cast<uint32_t*>(s_dyn + BZ_PAYLOAD);
    uint32_t* const s_head = s_out;                  // position + 1 (0: none) by hash, while the matches are looked for
    constexpr uint32_t NS = LZ_NL + LZ_ND + 257u;     // the symbols of the three codes: literal/length, distance, and level 1's over the bytes
    __shared__ uint32_t s_tab[256], s_lhist[LZ_NL], s_dhist[LZ_ND], s_bhist[257], s_lcode[LZ_NL], s_dcode[LZ_ND], s_bcode[257], s_wt[2 * NS], s_wave[4], s_misc[4];
    __shared__ uint16_t s_par[2 * NS], s_ord[NS], s_jump[256];
    __shared__ uint8_t s_dep[2 * NS], s_mark[256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t* const tk = tokens + (size_t)blockIdx.x * BZ_PAYLOAD;
    bz_crc_table(s_tab, tid);
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long p0 = (unsigned long long)blk * BZ_PAYLOAD;
        const uint32_t len = (uint32_t)(n - p0 < BZ_PAYLOAD ? n - p0 : BZ_PAYLOAD);
        // ---- 1. the payload into LDS; empty histograms and hash table ----
        bz_load(in + p0, len, s_in, tid);
        for (uint32_t i = tid; i < LZ_NL; i += 256u) { s_lhist[i] = i == 256u ? 1u : 0u; s_lcode[i] = 0; }
        if (tid < LZ_ND) { s_dhist[tid] = 0; s_dcode[tid] = 0; }
        for (uint32_t i = tid; i < 257u; i += 256u) { s_bhist[i] = i == 256u ? 1u : 0u; s_bcode[i] = 0; }
        for (uint32_t i = tid; i < LZ_HEAD; i += 256u) s_head[i] = 0;
        if (tid == 0) s_misc[0] = 0;
        __syncthreads();
        const uint32_t crc_all = bz_crc_hist(s_in, len, s_tab, true, s_bhist, s_wave, tid);
        // ---- 2. the matches and the tokens, tile by tile ----
        uint32_t n_tok = 0;
        for (uint32_t tb = 0; tb < len; tb += 256u) {
            const uint32_t start = s_misc[0];         // where the next token begins (written behind the last barrier of the tile before)
            const uint32_t p = tb + tid;
            const bool hashed = p + LZ_MIN <= len;
            uint32_t h = 0, mlen = 1, dist = 0;
            if (hashed) {
                h = (lz_get32(s_in32, p) * 0x9E3779B1u) >> 19;
                const uint32_t c1 = s_head[h];
                if (p >= start && c1 && p - (c1 - 1u) <= LZ_WINDOW) {
                    const uint32_t c = c1 - 1u, mx = len - p < LZ_MAX ? len - p : LZ_MAX;
                    uint32_t l = 0;
                    while (l < mx) {                  // 16 bytes a trip: the eight reads are issued together (what lies behind mx is cut off below)
                        uint32_t x[4];
                        for (uint32_t k = 0; k < 4u; ++k) x[k] = lz_get32(s_in32, c + l + 4u * k) ^ lz_get32(s_in32, p + l + 4u * k);
                        if (x[0] | x[1] | x[2] | x[3]) {
                            const uint32_t k = x[0] ? 0u : x[1] ? 1u : x[2] ? 2u : 3u, xk = x[0] ? x[0] : x[1] ? x[1] : x[2] ? x[2] : x[3];
                            l += 4u * k + ((uint32_t)__builtin_ctz(xk) >> 3);
                            break;
                        }
                        l += 16u;
                    }
                    if (l > mx) l = mx;
                    if (l >= LZ_MIN) { mlen = l; dist = p - c; }
                }
            }
            const bool parse = start < tb + 256u;     // (uniform) a match of the tile before may cover this one
            if (parse) {
                s_jump[tid] = (uint16_t)(tid + mlen < 256u ? tid + mlen : 256u);
                s_mark[tid] = p == start ? 1 : 0;
            }
            __syncthreads();                          // every lane has looked its candidate up: this tile's positions into the table
            if (hashed) atomicMax(&s_head[h], p + 1u);
            bool tok = false;
            if (parse) {
                for (int k = 0; k < 8; ++k) {
                    const uint32_t j = s_jump[tid], m = s_mark[tid], jj = j < 256u ? s_jump[j] : 256u;
                    __syncthreads();
                    if (m && j < 256u) s_mark[j] = 1;
                    s_jump[tid] = (uint16_t)jj;
                    __syncthreads();
                }
                tok = s_mark[tid] && p < len;
            }
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(tok);
            if (lane == 0) s_wave[wv] = (uint32_t)__popcll(bal);
            if (tok && (tid + mlen >= 256u || p + mlen >= len)) s_misc[0] = p + mlen;       // the one token that leaves the tile
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t q = 0; q < 4u; ++q) { const uint32_t c = s_wave[q]; before += q < wv ? c : 0u; all += c; }
            if (tok) {
                const uint32_t at = n_tok + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                uint32_t t = s_in[p];
                if (dist) {
                    uint32_t nx, xv;
                    t = LZ_MATCH | ((mlen - 3u) << 16) | (dist - 1u);
                    atomicAdd(&s_lhist[257u + lz_len_sym(mlen - 3u, &nx, &xv)], 1u);
                    atomicAdd(&s_dhist[lz_dist_sym(dist - 1u, &nx, &xv)], 1u);
                } else
                    atomicAdd(&s_lhist[t], 1u);
                if (at < BZ_PAYLOAD) tk[at] = t;
            }
            n_tok += all;
            __syncthreads();                          // s_wave and s_misc[0] are read; the next tile writes them again
        }
        // ---- 3. the codes: literal/length and distance over the tokens, and the literal code of level 1 over the bytes ----
        for (uint32_t i = tid; i < BZ_OUT_WORDS; i += 256u) s_out[i] = 0;
        bz_rank(s_lhist, LZ_NL, s_ord, tid);
        bz_rank(s_dhist, LZ_ND, s_ord + LZ_NL, tid);
        bz_rank(s_bhist, 257u, s_ord + LZ_NL + LZ_ND, tid);
        __syncthreads();
        if (tid == 0) bz_build_code(s_lhist, LZ_NL, s_ord, s_wt, s_par, s_dep, s_lcode);
        if (tid == 64u) bz_build_code(s_dhist, LZ_ND, s_ord + LZ_NL, s_wt + 2 * LZ_NL, s_par + 2 * LZ_NL, s_dep + 2 * LZ_NL, s_dcode);
        if (tid == 128u) bz_build_code(s_bhist, 257u, s_ord + LZ_NL + LZ_ND, s_wt + 2 * (LZ_NL + LZ_ND), s_par + 2 * (LZ_NL + LZ_ND), s_dep + 2 * (LZ_NL + LZ_ND), s_bcode);
        __syncthreads();
        if (tid == 0) {
            uint32_t nl = 257, nd = 1;
            unsigned long long bits = 0, plain = BZ_HDR_BITS;
            for (uint32_t s = 0; s < LZ_NL; ++s) {
                const uint32_t c = s_lhist[s];
                if (!c) continue;
                if (s >= nl) nl = s + 1u;
                bits += (unsigned long long)c * ((s_lcode[s] >> 16) + (s > 256u ? lz_len_extra(s - 257u) : 0u));
            }
            for (uint32_t d = 0; d < LZ_ND; ++d) {
                const uint32_t c = s_dhist[d];
                if (!c) continue;
                if (d >= nd) nd = d + 1u;
                bits += (unsigned long long)c * ((s_dcode[d] >> 16) + lz_dist_extra(d));
            }
            for (uint32_t s = 0; s < 257u; ++s) plain += (unsigned long long)s_bhist[s] * (s_bcode[s] >> 16);
            uint32_t hdr = BZ_FIX_BITS + 4u * (nl + nd);
            bits += hdr;
            // the smallest of three: the matched form, level 1's block over the bytes (short far matches can cost more than their
            // literals), the stored block.  Ties go to the simpler form
            const bool matched = bits < plain;
            if (!matched) { bits = plain; hdr = BZ_HDR_BITS; nl = 257; nd = 1; }
            const bool use = (bits + 7u) / 8u < (unsigned long long)len + 5u;
            s_misc[1] = use ? (matched ? 1u : 2u) : 0u; s_misc[2] = (uint32_t)bits; s_misc[3] = hdr;
            if (use) bz_put_block_header(s_out, matched ? s_lcode : s_bcode, nl, matched ? s_dcode : nullptr, nd);
        }
        __syncthreads();
        const bool huff = s_misc[1] != 0, matched = s_misc[1] == 1u;
        const uint32_t total_bits = s_misc[2];
        if (huff) {
            // ---- 4. every lane's tokens (or, in level 1's form, bytes) into the stream behind the header ----
            const uint32_t* const lc = matched ? s_lcode : s_bcode;
            uint32_t a, e, nbits = 0;
            bz_run(matched ? n_tok : len, tid, &a, &e);
            for (uint32_t i = a; i < e; ++i) {
                const uint32_t t = matched ? tk[i] : s_in[i];
                if (t & LZ_MATCH) {
                    uint32_t nx, xv, nb = 0;
                    nb += lc[257u + lz_len_sym((t >> 16) & 255u, &nx, &xv)] >> 16; nb += nx;
                    nb += s_dcode[lz_dist_sym(t & 0x7FFFu, &nx, &xv)] >> 16; nb += nx;
                    nbits += nb;
                } else
                    nbits += lc[t] >> 16;
            }
            BzBits w; w.start(s_out, s_misc[3] + bz_lane_start(nbits, s_wave, lane, wv));
            for (uint32_t i = a; i < e; ++i) {
                const uint32_t t = matched ? tk[i] : s_in[i];
                if (t & LZ_MATCH) {
                    uint32_t nx, xv;
                    w.code(lc[257u + lz_len_sym((t >> 16) & 255u, &nx, &xv)]); w.put(xv, nx);
                    w.code(s_dcode[lz_dist_sym(t & 0x7FFFu, &nx, &xv)]); w.put(xv, nx);
                } else
                    w.code(lc[t]);
            }
            w.flush();
            if (tid == 0) bz_put_eob(s_out, lc[256], total_bits);
            __syncthreads();
        }
        const uint32_t bsize = bz_write_member(slots + (size_t)blk * BZ_SLOT, huff, total_bits, len, s_out, s_in, crc_all, tid);
        if (tid == 0) sizes[blk] = bsize;
        __syncthreads();                              // the payload and the stream are read: the next payload may overwrite them
    }
}

__global__ void __launch_bounds__(256) k_bgzf_compact(const uint8_t* __restrict__ slots, const unsigned long long* __restrict__ off, uint8_t* __restrict__ out) {
    const unsigned long long a = off[blockIdx.x];
    const uint32_t size = (uint32_t)(off[blockIdx.x + 1] - a);
    const uint8_t* const s = slots + (size_t)blockIdx.x * BZ_SLOT;
    uint8_t* const d = out + a;
    if (size > BZ_SLOT) return;
    // the destination's first 16-byte boundary onward in whole 16-byte stores, the two ends byte-wise
    const uint32_t to16 = (uint32_t)((16u - (reinterpret_cast<uintptr_t>(d) & 15u)) & 15u), head = to16 < size ? to16 : size;
    const uint32_t n16 = (size - head) >> 4;
    for (uint32_t i = threadIdx.x; i < head; i += 256u) d[i] = s[i];
    for (uint32_t q = threadIdx.x; q < n16; q += 256u) { uint4 v; __builtin_memcpy(&v, s + head + (q << 4), 16); *reinterpret_cast<uint4*>(d + head + (q << 4)) = v; }
    for (uint32_t i = head + (n16 << 4) + threadIdx.x; i < size; i += 256u) d[i] = s[i];
}

// ------------------------------------------------------------------------------------------------
// BAM records
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool bm_op(char c) { return c == 'M' || c == 'I' || c == 'D'; } // all k_out_write ever puts into the pool
__device__ __forceinline__ uint32_t bm_nibble(char c) { return gm_bam_nibble(c); }      // "=ACMGRSVTWYHKDBN": gm_fmt_dev.h, shared with the NM / MD walk
#define BM_UNMAPPED_BIN 4680u                     // reg2bin(-1, 0): the bin of a record without a position (SAMv1 section 4.2)
__device__ __forceinline__ uint32_t bm_name_len(const GmDevText& t, uint32_t rd) {
    const unsigned long long nl = t.name_off[rd + 1] - t.name_off[rd];
    return nl > 254ull ? 254u : (uint32_t)nl;
}

__global__ void __launch_bounds__(256) k_bam_sizes(GmDevText t, uint32_t* __restrict__ meta) {
    const unsigned long long k = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (k >= t.n_rows) return;
    unsigned long long rec = 0; uint32_t urd = 0;
    if (!gm_row_is_record(t, k, rec, urd)) {
        // a read without a record: no operation, bin reg2bin(-1, 0) = 4680, one int32 tag (YU); an entry that names no read: nothing
        meta[2ull * k] = 0; meta[2ull * k + 1ull] = BM_UNMAPPED_BIN;
        const uint32_t L = urd != 0xFFFFFFFFu ? t.seq_len[urd] : 0u;
        t.row_len[k] = urd != 0xFFFFFFFFu ? 4u + 32u + bm_name_len(t, urd) + 1u + ((L + 1u) >> 1) + L + 7u : 0u;
        return;
    }
    const GmDevSamRec r = t.recs[rec];
    const uint8_t* slot = t.slots + k * 64ull;
    const uint32_t gout = (uint32_t)slot[58] | ((uint32_t)slot[59] << 8);          // the CIGAR field as the row prints it: bytes [0, gout) of the pool's
    const char* cg = t.pool + r.cigar_off;
    uint32_t n_ops = 0, v = 0;
    unsigned long long ref_len = 0;
    for (uint32_t i = 0; i < gout; ++i) {
        const char c = cg[i];
        if (c >= '0' && c <= '9') v = v * 10u + (uint32_t)(c - '0');
        else { if (bm_op(c)) { ++n_ops; if (c != 'I') ref_len += v; } v = 0; }
    }
    if (!ref_len) ref_len = 1;
    const long long pos0 = (long long)(int32_t)(uint32_t)(r.chr_pos - 1ull);
    const uint32_t L = t.seq_len[r.read];
    meta[2ull * k] = n_ops;
    meta[2ull * k + 1ull] = gm_reg2bin(pos0, pos0 + (long long)ref_len);
    t.row_len[k] = 4u + 32u + bm_name_len(t, r.read) + 1u + 4u * n_ops + ((L + 1u) >> 1) + L + 21u;
}

__device__ __forceinline__ void bm_put32(uint8_t* w, uint32_t v) { w[0] = (uint8_t)v; w[1] = (uint8_t)(v >> 8); w[2] = (uint8_t)(v >> 16); w[3] = (uint8_t)(v >> 24); }
// gm_batch_set_mates: the four core fields a row takes from its mate fields ("=" is the contig's own index; next_pos = PNEXT - 1, -1 for 0)
__device__ __forceinline__ void bm_put_mate(uint8_t* hd, const GmDevMateRow f) {
    hd[18] = (uint8_t)f.flag; hd[19] = (uint8_t)(f.flag >> 8);
    bm_put32(hd + 24, (uint32_t)f.rnext); bm_put32(hd + 28, f.pnext - 1u); bm_put32(hd + 32, (uint32_t)f.tlen);
}

// one wavefront per record, four records per workgroup and step.  TAGS: gm_batch_set_row_tags is on (t.md is there) - an instance of
// its own, so that the walk's registers cost the records without tags no occupancy.  MATES: gm_batch_set_mates is on (t.mate is there):
// flag, next_refID, next_pos and tlen come from the row's fields - instances of their own as well
template <bool TAGS, bool MATES>
__global__ void __launch_bounds__(256) k_bam_rows(GmDevBatch b, GmDevText t, const uint32_t* __restrict__ meta) {
    __shared__ uint8_t s_head[4][64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint8_t* const hd = s_head[wv];
    for (unsigned long long base = (unsigned long long)blockIdx.x * 4ull; base < t.n_rows; base += (unsigned long long)gridDim.x * 4ull) {
        const unsigned long long k = base + wv;
        unsigned long long rec = 0; uint32_t urd = 0;
        const bool is_rec = k < t.n_rows && gm_row_is_record(t, k, rec, urd);
        const bool unm = k < t.n_rows && !is_rec && urd != 0xFFFFFFFFu;        // a read without a record: refID -1, pos -1, flag 4, tag YU
        const bool live = is_rec || unm;
        GmDevSamRec r = {};
        uint32_t n_ops = 0, nl = 0, L = 0;
        if (unm) {
            r.read = urd;
            nl = bm_name_len(t, urd); L = t.seq_len[urd];
            if (lane == 0) {                          // [0, 36) block_size and the core fields, [36, 43) the tag
                const uint32_t size = (uint32_t)(t.row_off[k + 1] - t.row_off[k]);
                bm_put32(hd, size - 4u); bm_put32(hd + 4, 0xFFFFFFFFu); bm_put32(hd + 8, 0xFFFFFFFFu);
                hd[12] = (uint8_t)(nl + 1u); hd[13] = 0;
                hd[14] = (uint8_t)BM_UNMAPPED_BIN; hd[15] = (uint8_t)(BM_UNMAPPED_BIN >> 8); hd[16] = 0; hd[17] = 0;
                hd[18] = 4; hd[19] = 0;
                bm_put32(hd + 20, L); bm_put32(hd + 24, 0xFFFFFFFFu); bm_put32(hd + 28, 0xFFFFFFFFu); bm_put32(hd + 32, 0u);
                hd[36] = 'Y'; hd[37] = 'U'; hd[38] = 'i'; bm_put32(hd + 39, (uint32_t)(int32_t)t.status[urd]);
                if constexpr (MATES) bm_put_mate(hd, t.mate[k]);
            }
        }
        if (is_rec) {
            r = t.recs[rec];
            n_ops = meta[2ull * k]; nl = bm_name_len(t, r.read); L = t.seq_len[r.read];
            if (lane == 0) {                          // [0, 36) block_size and the core fields, [36, 57) the tags
                const uint32_t size = (uint32_t)(t.row_off[k + 1] - t.row_off[k]);
                const int32_t q = r.mapq < 0 ? 0 : r.mapq > 255 ? 255 : r.mapq;
                bm_put32(hd, size - 4u); bm_put32(hd + 4, r.contig); bm_put32(hd + 8, (uint32_t)(r.chr_pos - 1ull));
                hd[12] = (uint8_t)(nl + 1u); hd[13] = (uint8_t)q;
                const uint32_t bin = meta[2ull * k + 1ull];
                hd[14] = (uint8_t)bin; hd[15] = (uint8_t)(bin >> 8); hd[16] = (uint8_t)n_ops; hd[17] = (uint8_t)(n_ops >> 8);
                hd[18] = r.strand ? 16 : 0; hd[19] = 0;
                bm_put32(hd + 20, L); bm_put32(hd + 24, 0xFFFFFFFFu); bm_put32(hd + 28, 0xFFFFFFFFu); bm_put32(hd + 32, 0u);
                hd[36] = 'X'; hd[37] = 'A'; hd[38] = 'f'; bm_put32(hd + 39, __float_as_uint((float)((double)r.a_score * t.inv_adjust)));
                hd[43] = 'X'; hd[44] = 'P'; hd[45] = 'f'; bm_put32(hd + 46, __float_as_uint(r.post_prob));
                hd[50] = 'X'; hd[51] = '0'; hd[52] = 'i'; bm_put32(hd + 53, (uint32_t)r.sim_matches);
                if constexpr (MATES) bm_put_mate(hd, t.mate[k]);
            }
        }
        __syncthreads();
        if (live) {
            const unsigned long long end = t.row_off[k + 1];
            unsigned long long o = t.row_off[k];
            uint8_t* const out = reinterpret_cast<uint8_t*>(t.text);
            const uint8_t* slot = t.slots + k * 64ull;
            const uint32_t gout = (uint32_t)slot[58] | ((uint32_t)slot[59] << 8);      // (0 for a read without a record)
            const uint32_t rd = r.read;
            const unsigned long long n0 = t.name_off[rd];
            const unsigned long long q0 = t.qtail_off ? t.qtail_off[rd] : 0ull;
            const uint32_t TL = t.qtail_off ? (uint32_t)(t.qtail_off[rd + 1] - q0) : 0u, QL = L + TL;
            const bool neg = r.strand != 0;
            // every store stays inside the span the scan gave this record, whatever the lengths say
            if (lane < 36u && o + lane < end) out[o + lane] = hd[lane];
            o += 36u;
            for (uint32_t i = lane; i < nl; i += 64u) if (o + i < end) out[o + i] = (uint8_t)t.names[n0 + i];
            if (lane == 0 && o + nl < end) out[o + nl] = 0;
            o += nl + 1u;
            {   // operation kk of the field in print order; on the reverse strand the row prints the tokens last to first
                const char* cg = t.pool + r.cigar_off;
                uint32_t seen = 0;
                for (uint32_t i0 = 0; i0 < gout; i0 += 64u) {
                    const uint32_t i = i0 + lane;
                    const char c = i < gout ? cg[i] : '0';
                    const bool is_op = bm_op(c);
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(is_op);
                    if (is_op) {
                        const uint32_t kk = seen + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                        uint32_t v = 0, mul = 1;
                        for (uint32_t ts = i, d = 0; ts > 0 && d < 9u && cg[ts - 1u] >= '0' && cg[ts - 1u] <= '9'; --ts, ++d) { v += (uint32_t)(cg[ts - 1u] - '0') * mul; mul *= 10u; }
                        const uint32_t word = (v << 4) | (c == 'M' ? 0u : c == 'I' ? 1u : 2u);
                        const uint32_t j = neg && !t.cigar_forward ? n_ops - 1u - kk : kk;      // GM_CIGAR_FORWARD: operation kk goes to slot kk
                        if (kk < n_ops)
                            for (uint32_t q = 0; q < 4u; ++q) if (o + 4ull * j + q < end) out[o + 4ull * j + q] = (uint8_t)(word >> (8u * q));
                    }
                    seen += (uint32_t)__popcll(m);
                }
            }
            o += 4ull * n_ops;
            const uint8_t* bs = b.bases + (size_t)rd * b.stride; const uint8_t* qs = b.quals + (size_t)rd * b.stride;
            const uint32_t half = (L + 1u) >> 1;
            for (uint32_t i = lane; i < half; i += 64u) {
                const uint32_t j0 = 2u * i, j1 = j0 + 1u;
                const char c0 = neg ? gm_comp_char((char)bs[L - 1u - j0]) : (char)bs[j0];
                uint32_t v = bm_nibble(c0) << 4;
                if (j1 < L) v |= bm_nibble(neg ? gm_comp_char((char)bs[L - 1u - j1]) : (char)bs[j1]);
                if (o + i < end) out[o + i] = (uint8_t)v;
            }
            o += half;
            for (uint32_t i = lane; i < L; i += 64u) {
                const uint32_t si = neg ? QL - 1u - i : i;         // the first L characters of the QUAL field the row prints (k_out_text_rows)
                const uint8_t c = b.fasta ? (uint8_t)(t.fa_qual >> (8u * (((uint32_t)__popc(gm_iupac_mask(bs[si < L ? si : 0u])) - 1u) & 3u)))
                                  : si < L ? qs[si] : (uint8_t)t.qtail[q0 + (si - L)];
                if (o + i < end) out[o + i] = c > 33u ? (uint8_t)(c - 33u) : (uint8_t)0;
            }
            o += L;
            if (lane < (unm ? 7u : 21u) && o + lane < end) out[o + lane] = hd[36u + lane];
            if constexpr (TAGS) if (const uint32_t md_len = is_rec ? t.md[2ull * k + 1ull] : 0u) {
                // gm_batch_set_row_tags, behind X0: NM i <int32>, MD Z <the string of the walk> NUL
                o += 21u;
                if (lane < 10u) {
                    const uint32_t nm = t.md[2ull * k];
                    const uint8_t c[10] = { 'N', 'M', 'i', (uint8_t)nm, (uint8_t)(nm >> 8), (uint8_t)(nm >> 16), (uint8_t)(nm >> 24), 'M', 'D', 'Z' };
                    if (o + lane < end) out[o + lane] = c[lane];
                }
                o += 10u;
                uint32_t nm_w, len_w;
                gm_md_walk<true>(t, r, bs, L, t.pool + r.cigar_off, gout, neg && !t.cigar_forward, lane, out, o, end, &nm_w, &len_w);
                if (lane == 0 && o + md_len < end) out[o + md_len] = 0;
            }
        }
        __syncthreads();
    }
}

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

// ------------------------------------------------------------------------------------------------
// launchers and host code
// ------------------------------------------------------------------------------------------------
int gmk_bam_sizes(const GmDevText& t, uint32_t* meta, void* stream) {
    if (t.n_rows == 0) return 0;
    hipLaunchKernelGGL(k_bam_sizes, dim3(cdiv(t.n_rows, 256)), dim3(256), 0, S_(stream), t, meta);
    return (int)hipGetLastError();
}

int gmk_bam_rows(const GmDevBatch& b, const GmDevText& t, const uint32_t* meta, void* stream) {
    if (t.n_rows == 0) return 0;
    const uint32_t grid = gm_test_grid((uint32_t)std::min<uint64_t>((t.n_rows + 3) / 4, 4096));
    void (*const kern)(GmDevBatch, GmDevText, const uint32_t*) = t.mate ? (t.md ? k_bam_rows<true, true> : k_bam_rows<false, true>)
                                                                        : (t.md ? k_bam_rows<true, false> : k_bam_rows<false, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, S_(stream), b, t, meta);
    return (int)hipGetLastError();
}

void GmBgzfBufs::release() {
    for (DevBuf* d : { &slots, &sizes, &offs, &tmp, &out, &tokens }) d->release();
    for (auto& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
}

uint64_t gm_bgzf_bound(uint64_t n) { return n + (uint64_t)BZ_EXTRA * ((n + BZ_PAYLOAD - 1) / BZ_PAYLOAD); }

// the most input bytes whose worst-case (stored) BGZF form fits in cap
uint64_t gm_bgzf_room(uint64_t cap) {
    const uint64_t per = (uint64_t)BZ_PAYLOAD + BZ_EXTRA, whole = cap / per, rest = cap % per;
    return whole * BZ_PAYLOAD + (rest > BZ_EXTRA ? rest - BZ_EXTRA : 0);
}

std::string gm_bgzf_level_text(int level) {
    return "the level is 0 (stored), 1 (Huffman) or 1 | GM_BGZF_LZ77 (257: Huffman over LZ77 matches), not " + std::to_string(level);
}

// d_in[0, n) in HBM -> whole BGZF blocks side by side in z.out, *total bytes of them; synchronises the stream
int gm_bgzf_device(const void* d_in, uint64_t n, int level, GmBgzfBufs& z, uint64_t* total, void* stream) {
    *total = 0;
    if (!n) return GM_OK;
    if (!gm_bgzf_level_ok(level)) { gm_set_error("BGZF: " + gm_bgzf_level_text(level)); return GM_E_ARG; }
    const uint64_t nb64 = (n + BZ_PAYLOAD - 1) / BZ_PAYLOAD;
    if (nb64 > 0x7FFFFFFFull) { gm_set_error("BGZF: more than 2^31 - 1 blocks in one call"); return GM_E_ARG; }
    const uint32_t nb = (uint32_t)nb64;
    hipStream_t st = S_(stream);
    if (z.slots.ensure((size_t)nb * BZ_SLOT) || z.sizes.ensure((size_t)nb * 4) || z.offs.ensure(((size_t)nb + 1) * 8) || z.tmp.ensure(((size_t)nb / 1024 + 8) * 8) ||
        z.out.ensure((size_t)gm_bgzf_bound(n) + 16)) return GM_E_NOMEM;
    const bool lz = (level & GM_BGZF_LZ77) != 0;
    uint32_t lz_grid = 0;
    if (lz) {
        // one workgroup per compute unit (the LDS holds one), each with room for a payload's tokens
        if (!z.lz_wgs) { int dev = 0, cus = 0; HIPCHK(hipGetDevice(&dev)); HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)); z.lz_wgs = (uint32_t)std::max(cus, 1); }
        lz_grid = std::min(nb, z.lz_wgs);
        if (z.tokens.ensure((size_t)lz_grid * BZ_PAYLOAD * 4)) return GM_E_NOMEM;
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_bgzf_deflate_lz), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BZ_LDS));
    } else
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_bgzf_deflate), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BZ_LDS));
    if (z.timed) { for (auto& e : z.ev) if (!e) HIPCHK(hipEventCreate(&e)); HIPCHK(hipEventRecord(z.ev[0], st)); }
    if (lz)
        hipLaunchKernelGGL(k_bgzf_deflate_lz, dim3(lz_grid), dim3(256), BZ_LDS, st, (const uint8_t*)d_in, (unsigned long long)n, nb, z.slots.as<uint8_t>(), z.sizes.as<uint32_t>(),
                           z.tokens.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_bgzf_deflate, dim3(nb), dim3(256), BZ_LDS, st, (const uint8_t*)d_in, (unsigned long long)n, level, z.slots.as<uint8_t>(), z.sizes.as<uint32_t>());
    HIPCHK(hipGetLastError());
    KCHK(gmk_scan_u32(z.sizes.as<uint32_t>(), nb, z.offs.as<uint64_t>(), z.tmp.as<unsigned long long>(), stream));
    if (z.timed) HIPCHK(hipEventRecord(z.ev[1], st));
    uint64_t sum = 0;
    HIPCHK(hipMemcpyAsync(&sum, z.offs.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (sum > gm_bgzf_bound(n) || sum < 28ull * nb) { gm_set_error("BGZF: the blocks' sizes sum to " + std::to_string(sum) + " bytes for " + std::to_string(n) + " bytes of input"); return GM_E_HIP; }
    if (z.timed) HIPCHK(hipEventRecord(z.ev[2], st));
    hipLaunchKernelGGL(k_bgzf_compact, dim3(nb), dim3(256), 0, st, z.slots.as<uint8_t>(), z.offs.as<unsigned long long>(), z.out.as<uint8_t>());
    HIPCHK(hipGetLastError());
    if (z.timed) {
        float a = 0, b = 0;
        HIPCHK(hipEventRecord(z.ev[3], st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventElapsedTime(&a, z.ev[0], z.ev[1]));
        HIPCHK(hipEventElapsedTime(&b, z.ev[2], z.ev[3]));
        z.ms += (double)a + b; z.in_bytes += n; z.out_bytes += sum;
    }
    *total = sum;
    return GM_OK;
}

extern "C" int gm_bgzf_compress(gm_index* ix, const void* data, uint64_t n, int level, void* out, uint64_t cap, uint64_t* n_out, void* hip_stream) {
    if (!ix || !n_out) return GM_E_ARG;
    *n_out = 0;
    if (!gm_bgzf_level_ok(level)) { gm_set_error("gm_bgzf_compress: " + gm_bgzf_level_text(level)); return GM_E_ARG; }
    if (ix->host_only) { gm_set_error("gm_bgzf_compress: no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (!n) return GM_OK;
    if (!data || (!out && cap)) { gm_set_error("gm_bgzf_compress: data or out is NULL"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(ix->device));
    hipStream_t st = S_(hip_stream);
    Scoped<DevBuf> d_in;
    Scoped<GmBgzfBufs> z;
    if (d_in.ensure((size_t)n + 16)) return GM_E_NOMEM;
    HIPCHK(hipMemcpyAsync(d_in.p, data, (size_t)n, hipMemcpyHostToDevice, st));
    uint64_t total = 0;
    if (const int rc = gm_bgzf_device(d_in.p, n, level, z, &total, hip_stream)) { (void)hipStreamSynchronize(st); return rc; }
    *n_out = total;
    if (total > cap) {
        (void)hipStreamSynchronize(st);
        gm_set_error("gm_bgzf_compress: the blocks take " + std::to_string(total) + " bytes, the buffer holds " + std::to_string(cap));
        return GM_E_CAPACITY;
    }
    HIPCHK(hipMemcpyAsync(out, z.out.p, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GM_OK;
}

extern "C" int gm_bgzf_eof(void* out28) {
    if (!out28) return GM_E_ARG;
    static const uint8_t eof[28] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    memcpy(out28, eof, 28);
    return GM_OK;
}

extern "C" int gm_bam_header(gm_index* ix, const char* sam_header, uint64_t n, void* out, uint64_t cap, uint64_t* n_out) {
    if (!ix || !n_out || (!sam_header && n)) return GM_E_ARG;
    const auto& contigs = ix->h.contigs;
    uint64_t need = 4 + 4 + n + 4;
    for (const auto& c : contigs) need += 4 + c.name.size() + 1 + 4;
    *n_out = need;
    if (n > 0x7FFFFFFFull) { gm_set_error("gm_bam_header: a header text of more than 2^31 - 1 bytes"); return GM_E_ARG; }
    if (need > cap || !out) { gm_set_error("gm_bam_header: the header takes " + std::to_string(need) + " bytes, the buffer holds " + std::to_string(cap)); return GM_E_CAPACITY; }
    uint8_t* w = (uint8_t*)out;
    auto put32 = [&](uint32_t v) { w[0] = (uint8_t)v; w[1] = (uint8_t)(v >> 8); w[2] = (uint8_t)(v >> 16); w[3] = (uint8_t)(v >> 24); w += 4; };
    memcpy(w, "BAM\1", 4); w += 4;
    put32((uint32_t)n);
    if (n) memcpy(w, sam_header, (size_t)n);
    w += n;
    put32((uint32_t)contigs.size());
    for (const auto& c : contigs) {
        put32((uint32_t)c.name.size() + 1u);
        memcpy(w, c.name.c_str(), c.name.size() + 1); w += c.name.size() + 1;
        put32(c.len);
    }
    return GM_OK;
}
