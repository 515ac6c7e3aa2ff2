// gm_nw.hip — k_nw_rows: the banded probabilistic Needleman-Wunsch score (bin_seq::get_align_score, src/bin_seq.cpp:761-850,
// get_val :975-987, max_flt :1013-1026) for blocks whose reads all have ONE length, one LANE per candidate.
//
// Same arithmetic as k_nw_lane (gm_kernels.hip): the 7-cell band row in registers, swept from the bottom-right row by row, cells
// j = i+3 .. i-3, three fp32 adds and the reference's 3-way max per cell, no contraction - the score bits are the reference's.  What
// differs is everything AROUND the adds, which is where k_nw_lane spent its ~170 vector instructions per DP row (it ran at the vector
// issue rate, HBM idle):
//   * the four substitution values of a PWM row, val(row, g) for g = a, c, g, t, depend only on (called base, quality character): they
//     are looked up in a per-workgroup LDS table built once with the reference's own expression (gm_get_val; bit-identical, the same
//     function value looked up instead of recomputed): one ds_read_b128 instead of 28 multiplies / adds + the LUT read;
//   * the read row and the reference window are brought into DP ORDER when they are loaded (forward-strand reads byte-reversed, the
//     2-bit window bit-reversed and funnel-shifted), so that DP row t of EVERY lane - whatever its strand and window start - finds its
//     base, its quality and its new window column at the same register and bit position: compile-time shifts in rows unrolled 8 at a
//     time, no per-row address arithmetic, no 13-way register pick, no strand-dependent indexing;
//   * a band column's base is kept as its byte offset inside a value record (4 x its 2-bit code); a cell's value is ONE ds_read_b32 at
//     record + column offset (the first form picked it out of the row's float4 with three v_cndmask on two lane masks per column: 21 of
//     the 57 instructions of a row; as LDS reads the row is 45 and the kernel 5 % faster - the LDS has the room);
//     sliding the band is register renaming inside the unrolled rows;
//   * PAIRS (the default where it fits): the record of a (quality character, class) holds the values of two adjacent band columns for
//     each of the 16 code pairs, {val(x), val(y)} at byte 8 (4x + y).  An interior row reads cells (0,1), (2,3), (4,5) and (6, -) with
//     one ds_read_b64 each: 4 LDS reads instead of 7.  On gfx950 ds_read_b64 banks over 64 dwords instead of 32, so a half-wave of
//     random entries meets about as many conflicts per instruction as one ds_read_b32 did, for fewer instructions (LDS cycles -29 %,
//     DESIGN.md §4).  The table holds only the quality characters of the block (its range is reduced by the prep kernels into
//     GMK_QUAL_MIN / GMK_QUAL_MAX) and 5 classes, so the host sizes the LDS from that range;
//   * the first 8 and the last 9 .. 16 rows (which touch row L, column L or column -1) run a generic row; the rows between them test nothing.
// The host launches it only for blocks it has checked: one read length L (24 <= L <= 8 NCH), no quality character above 127, -M 3; the
// pair form only with the block's quality range, inside which every quality character of the block lies.
// FASTA blocks (GmDevBatch::fasta): a position's row is its IUPAC letter's, (base mask, p, q) with (p, q) a function of the mask - the
// class axis is the 16 masks (the minus strand's class = the mask with its bits reversed), the quality axis ONE entry: the quality rows
// are neither loaded nor multiplied in (their words stay 0), and the whole pair table is 16 records (2.1 KB), the cells table 256 bytes.
//
// THE LOAD GROUP.  A candidate costs two dependent memory trips: its 16-byte record, then everything the record's fields address,
// requested back to back with no branch and no wait between two loads (the first form went chunk by chunk, one basic block and one
// round trip each: 13 row trips behind the record and the rs_overflow byte, then the window words, then min_score - DESIGN.md section 4):
//   * the read row as NP = (NCH + 1) / 2 pieces of 16 bytes per array (7 for <13>, 10 for <19>), two 8-row chunks each.  Reverse strand:
//     piece m at row offset 16 m.  Forward strand: the row backwards, piece m at L - 16 - 16 m (any byte alignment), byte-reversed as
//     a whole by the v_perm that also splits it into its chunks.  One selector serves both strands;
//   * a row of an ODD number of chunks ends in a piece with one live chunk.  That piece is loaded one chunk lower (reverse strand: at
//     16 m - 8; forward strand: at 0, where the clamp puts it anyway), so that on both strands the live chunk arrives in the piece's
//     upper half and is moved down after the loads; the forward strand's is then shifted by the sh bytes the row falls short of
//     its last chunk.  An EVEN row's last piece on the forward strand starts sh bytes before the row: loaded at 0, both chunks
//     funnel-shifted down by sh bytes.  These fix-ups sit behind the loads, under wave-uniform conditions;
//   * clamps instead of predicates: a piece offset lies in [0, stride - 16], so a piece beyond the row's chunks (L < 8 NCH) loads
//     inside the row and is zeroed by its selector, and nothing is read past the row - the last row of the block ends where the
//     uploaded data does.  Needs stride >= 16 and, for the odd row's 16 m - 8, at least two chunks: the launcher admits 24 <= L <= stride;
//   * the packed window as NWL 16-byte loads (2 / 3) of ASCENDING words ending at word n0 = (begin + L - 1) / 16, n0 clamped to
//     the reference's last word (candidates whose window is refused afterwards load too) and the first word clamped to word 0.  A
//     window within the reference's first NWW - 1 words therefore arrives too low in its registers: its words are moved up by the
//     difference (a rare, divergent branch behind the loads), word 0 filling in, which feeds only columns j < 0;
//   * min_score[r], which the epilogue compares with; and, only when the host says that the retry kernel ran for this launch (sup:
//     rs_overflow is written nowhere else), the flagged candidate's rs_overflow byte, as the last load of the group.
// Only then come the tests: window inside one contig, superseded.  The epilogue writes {step, flags, pad, score} as one 8-byte store.
#include <hip/hip_runtime.h>
#include "gm_device.h"

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define GM_NWR_NCOFF 1024u                  // contig offsets cached in LDS when there are at most this many
#define GM_NWR_QSTRIDE 144u                 // bytes per quality character in the value table: 8 class records of 16 bytes + 16 bytes of skew (banks)
#define GM_NWR_TAB_BYTES (128u * GM_NWR_QSTRIDE)
#define GM_NWR_PAIR_SKEW 8u                 // bytes of skew after each 128-byte pair record (GM_NW_PAIR_SKEW): record r starts 34 r dwords in

// PAIRS: qlo = the block's smallest quality character, nq = the number of characters in its range, rs = bytes per pair record
// FA: a FASTA block (its own instantiation: the FASTQ kernels keep their instructions)
// sup: the host saw the retry kernel (or the heavy path) run for this launch: only then is a flagged candidate's rs_overflow byte loaded
template <int NCH, bool PAIRS, bool FA>
__global__ void __launch_bounds__(256, NCH <= 13 ? 4 : 3) k_nw_rows(GmDevIndex ix, GmDevParams p, GmDevBatch b, const uint32_t L, const uint32_t ntab,
                                                                    const uint32_t qlo, const uint32_t nq, const uint32_t rs, const uint32_t sup) {
    constexpr uint32_t ncls = FA ? 16u : 5u;                                    // class records per quality character (FA: one per base mask)
    constexpr int NHW = (8 * NCH + 3) / 16 + 1;                                // 16-column words of the window stream
    constexpr int NP = (NCH + 1) / 2;                                          // 16-byte pieces of a read row (two chunks each)
    constexpr int NWL = (NHW + 4) / 4, NWW = 4 * NWL;                          // 16-byte loads / words of the packed window (NHW + 1 are used)
    // cells: [ntab][128 quality characters][8 classes] float4 {val(a), val(c), val(g), val(t)};
    // PAIRS: [ntab][nq quality characters][5 classes] 16 x float2 {val(x), val(y)}, records rs bytes apart
    extern __shared__ __attribute__((aligned(16))) unsigned char s_tab[];
    // [phred table][strand][read character] -> byte offset of its class record (+ its table's; PAIRS: - qlo x the quality stride, mod 2^32)
    __shared__ std::conditional_t<PAIRS, uint32_t, uint16_t> s_cls[2][2][256];
    const uint32_t qstride = PAIRS ? ncls * rs : GM_NWR_QSTRIDE, tabb = PAIRS ? nq * qstride : GM_NWR_TAB_BYTES;      // ncls: 5, FASTA 16
    __shared__ uint32_t s_coff[GM_NWR_NCOFF];
    __shared__ uint32_t s_pre[GM_NSHARD + 4];
    {
        float sg[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k) sg[g][k] = p.S256[(size_t)("acgt"[g]) * 4 + k];     // windows are lowercase acgt (GetString)
        if (PAIRS) {
            for (uint32_t e = threadIdx.x; e < ntab * nq * ncls * 16u; e += 256) {     // 16 entries of ncls class records per quality character
                const uint32_t n = e & 15u, rec = e >> 4, tq = rec / ncls, code = rec - ncls * tq;    // class 4: any character outside ACGTacgt
                const uint32_t tab = tq / nq, qi = tq - tab * nq;
                const uint32_t mask = FA ? code : gm_code_mask(code);                            // (FASTA: the class IS the base mask)
                const float2 pq = FA ? p.lut[GM_LUT_FASTA + mask] : p.lut[tab * 256u + qlo + qi];
                float v[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) v[g] = gm_get_val_mask(mask, pq.x, pq.y, sg[g]);
                const uint32_t x = n >> 2, y = n & 3u;
                const float2 o = make_float2(x == 0 ? v[0] : x == 1 ? v[1] : x == 2 ? v[2] : v[3], y == 0 ? v[0] : y == 1 ? v[1] : y == 2 ? v[2] : v[3]);
                *reinterpret_cast<float2*>(s_tab + tab * tabb + qi * qstride + code * rs + 8u * n) = o;
            }
        } else if (FA) {
            if (threadIdx.x < 16u) {                                              // one record per base mask, at "quality" 0
                const uint32_t mask = threadIdx.x;
                const float2 pq = p.lut[GM_LUT_FASTA + mask];
                float4 v;
                v.x = gm_get_val_mask(mask, pq.x, pq.y, sg[0]); v.y = gm_get_val_mask(mask, pq.x, pq.y, sg[1]);
                v.z = gm_get_val_mask(mask, pq.x, pq.y, sg[2]); v.w = gm_get_val_mask(mask, pq.x, pq.y, sg[3]);
                *reinterpret_cast<float4*>(s_tab + mask * 16u) = v;
            }
        } else {
            for (uint32_t e = threadIdx.x; e < ntab * 1024u; e += 256) {
                const uint32_t tab = e >> 10, q = (e >> 3) & 127u, cl = e & 7u;
                const uint32_t code = cl < 4u ? cl : 4u;                         // classes 4 .. 7: any character outside ACGTacgt
                const float2 pq = p.lut[tab * 256u + q];
                float4 v;
                v.x = gm_get_val(code, pq.x, pq.y, sg[0]); v.y = gm_get_val(code, pq.x, pq.y, sg[1]);
                v.z = gm_get_val(code, pq.x, pq.y, sg[2]); v.w = gm_get_val(code, pq.x, pq.y, sg[3]);
                *reinterpret_cast<float4*>(s_tab + tab * GM_NWR_TAB_BYTES + q * GM_NWR_QSTRIDE + cl * 16u) = v;
            }
        }
        const uint32_t ch = threadIdx.x, code = gm_nt4(ch);
#pragma unroll
        for (uint32_t tab = 0; tab < 2; ++tab)
#pragma unroll
            for (uint32_t st = 0; st < 2; ++st) {                                 // the reverse strand reads the complemented PWM row (reverse_comp_cpy)
                const uint32_t cl = FA ? gm_row_mask(1u, ch, st) : (code < 4u && st) ? 3u - code : code;
                const uint32_t tb = (tab < ntab ? tab : 0u) * tabb;
                s_cls[tab][st][ch] = PAIRS ? tb + cl * rs - qlo * qstride : tb + cl * 16u;
            }
    }
    const bool lds_coff = ix.n_seqs + 1 <= GM_NWR_NCOFF;
    if (lds_coff) for (uint32_t q = threadIdx.x; q <= ix.n_seqs; q += 256) s_coff[q] = ix.contig_off[q];
    const uint32_t* coff = lds_coff ? s_coff : ix.contig_off;
    const uint32_t n_cands = gm_cand_prefix(b, s_pre);          // includes the barrier that publishes the tables
    const float gap = p.gap, gap4 = __fmul_rn(p.gap, 4.0f);
    const float ninf_gap = __fadd_rn(GM_NEG_INF, gap);
    const uint32_t* pac32 = reinterpret_cast<const uint32_t*>(ix.pac);
    const int Li = (int)L;
    const int nchunk = (Li + 7) >> 3;
    const uint32_t sh = (uint32_t)(8 * nchunk - Li);            // bytes the reversed row of a forward-strand read is shifted down by
    const int m_last = (nchunk - 1) >> 1;                       // the piece that holds the row's last chunk
    const bool odd = (nchunk & 1) != 0;                         // .. alone: it is loaded one chunk lower, so that both strands find that chunk in its upper half
    // a piece never reaches past its row.  Preconditions (nw_rows_ok: 24 <= L <= stride, stride a multiple of 8): omax >= 8, and the odd
    // row's last piece, loaded at 16 m_last - 8 = 8 nchunk - 16, starts at 8 or beyond and ends inside the row
    const int omax = (int)b.stride - 16;
    const uint32_t nlast = (ix.l_pac - 1u) >> 4;                // the last word of the packed reference that holds a base
    // cells inside the band of one candidate (counter only)
    unsigned long long band_cells = 0;
    if (Li >= 7) band_cells = (unsigned long long)(7 * Li - 12);
    else for (int i = 0; i < Li; ++i) { int lo = i - 3 < 0 ? 0 : i - 3, hi = i + 3 >= Li ? Li - 1 : i + 3; band_cells += (unsigned long long)(hi - lo + 1); }
    uint32_t scored = 0, accepted = 0;                          // this lane's candidates: a grid-stride share of fewer than 2^32
    for (uint32_t wi = blockIdx.x * 256 + threadIdx.x; wi < n_cands; wi += gridDim.x * 256) {
        const size_t ci = gm_cand_slot(b, s_pre, wi);
        GmCand c;
        uint32_t c_hi;                                          // step | flags << 16 | pad << 24: the word the epilogue writes back
        {
            uint4 cw;
            __builtin_memcpy(&cw, &b.cands[ci], 16);
            c.rs = cw.x; c.b = cw.y; c_hi = cw.z;
            c.step = (uint16_t)c_hi; c.flags = (uint8_t)(c_hi >> 16);
        }
        const uint32_t r = c.rs >> 1, strand = c.rs & 1;
        // ---- the load group: everything the candidate's fields address is requested here, back to back - no branch and no wait between
        //      two loads, every address clamped into its allocation instead of predicated.  What is tested (superseded, window inside a
        //      contig) is tested afterwards.  (No overlap is claimed for those tests: coff is an LDS-or-global pointer, its reads are flat
        //      loads, and the first one waits for the whole group) ----
        // the read row in 16-byte pieces, in DP order (element t belongs to DP row i = L - 1 - t).  Reverse strand: t = the read's own
        // index (complemented through s_cls), piece m at 16 m; forward strand: the read backwards, piece m at L - 16 - 16 m, or at 0 when
        // that is before the row (the last piece: put right after the loads).  Pieces beyond the row load inside it and are zeroed
        uint4 TB[NP], TQ[NP];
        {
            unsigned long long row = (unsigned long long)r * b.stride;
            asm("" : "+v"(row));                                            // (the product alone: with a base folded in, both bases wait in vector registers)
            const uint8_t* rb = b.bases + row;
            const uint8_t* rq = b.quals + row;
            uint32_t fwd = strand - 1u;                                     // all ones on the forward strand
            asm("" : "+v"(fwd));                                            // (kept a mask: as a select, the 14 offsets would wait in vector registers)
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                const int orv = 16 * m - ((odd && m == m_last) ? 8 : 0), ofw = Li - 16 - 16 * m;
                const uint32_t orc = (uint32_t)(orv < omax ? orv : omax), ofc = (uint32_t)(ofw > 0 ? ofw : 0);        // (wave-uniform)
                const uint32_t off = orc + (fwd & (ofc - orc));             // (an AND and an add on scalars: a select would keep both in registers)
                __builtin_memcpy(&TB[m], rb + off, 16);
                if (!FA) __builtin_memcpy(&TQ[m], rq + off, 16);
                else TQ[m] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        // the packed window as ascending words ending at word n0 (clamped to the reference's last word for windows that are refused
        // below, and to word 0 at its start)
        const uint32_t g0 = c.b + L - 1u, n0 = g0 >> 4;
        const uint32_t n0c = n0 < nlast ? n0 : nlast;
        uint32_t A[NWW];
        {
            const uint32_t* wp = pac32 + (n0c >= (uint32_t)(NWW - 1) ? n0c - (uint32_t)(NWW - 1) : 0u);
#pragma unroll
            for (int q = 0; q < NWL; ++q) {
                uint4 t;
                __builtin_memcpy(&t, wp + 4 * q, 16);
                A[4 * q] = t.x; A[4 * q + 1] = t.y; A[4 * q + 2] = t.z; A[4 * q + 3] = t.w;
            }
        }
        const double min_score = b.min_score[r];
        uint32_t superseded = 0u;
        if (sup && (c.flags & 4)) superseded = b.rs_overflow[c.rs];         // (the last load of the group)
        const bool ok = gm_window_ok(ix, coff, c.b, L);
        if (superseded) continue;                                           // the retry kernel made this read x strand's candidates again
        float result = 0.0f;
        if (ok && p.nw) {
            // ---- the pieces into chunks: reverse strand as loaded, forward strand byte-reversed (piece and all) ----
            uint2 XB[NCH], XQ[NCH];
            {
                const uint32_t selx = strand ? 0x03020100u : 0x04050607u;
                const uint32_t s8 = strand ? 0u : 8u * sh;                  // the forward strand's last piece was loaded from offset 0: its elements sit sh bytes up
#pragma unroll
                for (int m = 0; m < NP; ++m) {
                    const uint32_t sel = m <= m_last ? selx : 0x0C0C0C0Cu;   // (selector 0x0C: a zero byte)
                    uint2 lo[2], hi[2];
#pragma unroll
                    for (int a = 0; a < (FA ? 1 : 2); ++a) {
                        const uint4 t = a ? TQ[m] : TB[m];
                        lo[a] = make_uint2(__builtin_amdgcn_perm(t.w, t.x, sel), __builtin_amdgcn_perm(t.z, t.y, sel));
                        hi[a] = make_uint2(__builtin_amdgcn_perm(t.y, t.z, sel), __builtin_amdgcn_perm(t.x, t.w, sel));
                        if (m == m_last && (odd || sh != 0u)) {
                            const unsigned long long l64 = ((unsigned long long)lo[a].y << 32) | lo[a].x, h64 = ((unsigned long long)hi[a].y << 32) | hi[a].x;
                            // odd: the one chunk of the piece came in the upper half.  Even: both halves move down by sh bytes
                            const unsigned long long nl = odd ? h64 >> s8 : (l64 >> s8) | ((h64 << 1) << (63u - s8)), nh = odd ? 0ull : h64 >> s8;
                            lo[a] = make_uint2((uint32_t)nl, (uint32_t)(nl >> 32)); hi[a] = make_uint2((uint32_t)nh, (uint32_t)(nh >> 32));
                        }
                    }
                    if (FA) { lo[1] = make_uint2(0u, 0u); hi[1] = make_uint2(0u, 0u); }
                    XB[2 * m] = lo[0]; XQ[2 * m] = lo[1];
                    if (2 * m + 1 < NCH) { XB[2 * m + 1] = hi[0]; XQ[2 * m + 1] = hi[1]; }
                }
            }
            // ---- the window in DP order: H[u] = w[L - 1 - u], 2 bits each, 16 per word, u ascending from bit 0.  The reference packs 4
            //      bases per byte MSB first (_get_pac, src/bntseq.c:225): in a byte-swapped 32-bit word base g sits at bit 30 - 2 (g & 15),
            //      so descending positions are ascending bits and the stream is the words n0, n0 - 1, .. funnel-shifted by 30 - 2 (g0 & 15) ----
            uint32_t HW[NHW];
            {
                if (n0c < (uint32_t)(NWW - 1)) {
                    // the loads started at word 0 instead of n0 - (NWW - 1): the words move up by the difference, word 0 filling in
                    // (below the reference's start only columns j < 0 are fed)
                    const uint32_t up = (uint32_t)(NWW - 1) - n0c;
#pragma unroll
                    for (int bit = 1; bit < NWW; bit <<= 1) {
                        const bool mv = (up & (uint32_t)bit) != 0u;
#pragma unroll
                        for (int q = NWW - 1; q >= 0; --q) A[q] = mv ? A[q >= bit ? q - bit : 0] : A[q];
                    }
                }
                const uint32_t s = 30u - 2u * (g0 & 15u);
                uint32_t W[NHW + 1];
#pragma unroll
                for (int j = 0; j <= NHW; ++j) W[j] = __builtin_amdgcn_perm(A[NWW - 1 - j], A[NWW - 1 - j], 0x00010203u);
#pragma unroll
                for (int m = 0; m < NHW; ++m) HW[m] = __builtin_amdgcn_alignbit(W[m + 1], W[m], s);
            }
            const uint32_t tab = (ntab > 1u && r < b.illumina_until) ? 1u : 0u;
            const auto* const clsrow = s_cls[tab][strand];
            // band row of i + 1: P[d] = nm[i+1][i+1+d-3].  Row L: gGAP * (L - j) for j <= L (bin_seq.cpp:805-808)
            float P[7];
#pragma unroll
            for (int d = 0; d < 7; ++d) P[d] = d <= 3 ? __fmul_rn(gap, (float)(3 - d)) : GM_NEG_INF;
            // the base of band column d (row t: H[t + 3 - d]) as its byte offset in a value record.  cells: 4 x its 2-bit code.  PAIRS: the
            // offset of the pair entry (column d, column d + 1) = 8 x the 4 stream bits of H[t + 2 - d] .. H[t + 3 - d]: the entry's x half
            // is column d's value, a ds_read_b64 there returns columns d and d + 1.  Row L - 1: columns j = L-4+d, valid for d <= 3
            uint32_t cc[7];
#pragma unroll
            for (int d = 0; d < 7; ++d) cc[d] = d > 3 ? 0u : PAIRS ? (((HW[0] << 2) >> (2 * (3 - d))) & 15u) << 3 : ((HW[0] >> (2 * (3 - d))) & 3u) << 2;
            // a row's value record as its LDS byte offset
            auto row_vals = [&](uint32_t bword, uint32_t qword, uint32_t shift) -> uint32_t {
                const uint32_t chv = (bword >> shift) & 255u;
                const uint32_t co = clsrow[chv];
                const uint32_t qv = (qword >> shift) & 255u;
                return __umul24(qv, qstride) + co;                              // (a 24-bit multiply: qstride is a kernel argument in the pair form)
            };
            auto cell_val = [&](const uint32_t v, int d) -> float { return *reinterpret_cast<const float*>(s_tab + v + cc[d]); };
            // band columns of the next row; the new one is H[t + 4] (j = i - 4), at bit pos of hw.  PAIRS: the new entry takes H[t + 3] too,
            // the two bits below pos - from the word before (hwp) when pos = 0
            auto slide = [&](uint32_t hw, uint32_t hwp, uint32_t pos) {
#pragma unroll
                for (int d = 6; d >= 1; --d) cc[d] = cc[d - 1];
                if (PAIRS) cc[0] = (uint32_t)((((unsigned long long)hw << 32) | hwp) >> (27u + pos)) & 0x78u;
                else cc[0] = ((hw >> pos) & 3u) << 2;
            };
            // an interior row (4 <= i <= L - 5): every cell inside the matrix, band edges are NEG_INF
            auto row_int = [&](const uint32_t v, uint32_t hw, uint32_t hwp, uint32_t pos) {
                float val[7], mm[7], g1[7], unused = 0.0f;
                if (PAIRS) {
#pragma unroll
                    for (int d = 0; d < 6; d += 2) {
                        const float2 pv = *reinterpret_cast<const float2*>(s_tab + v + cc[d]);
                        val[d] = pv.x; val[d + 1] = pv.y;
                    }
                    // cell 6 is the x half of its own pair entry, read as the whole entry: an 8-byte-aligned ds_read_b32 would meet only the
                    // even banks of its 32, a ds_read_b64 spreads over all 64 (the y half is kept alive below so that the read stays 8 bytes)
                    const float2 pv = *reinterpret_cast<const float2*>(s_tab + v + cc[6]);
                    val[6] = pv.x; unused = pv.y;
                } else {
#pragma unroll
                    for (int d = 0; d < 7; ++d) val[d] = cell_val(v, d);
                }
#pragma unroll
                for (int d = 0; d < 7; ++d) { mm[d] = __fadd_rn(P[d], val[d]); g1[d] = d > 0 ? __fadd_rn(P[d - 1], gap) : ninf_gap; }
                float left = ninf_gap;                                          // nm[i][j+1] + gGAP beyond the band
#pragma unroll
                for (int d = 6; d >= 0; --d) {
                    const float best = fmaxf(fmaxf(mm[d], g1[d]), left);       // max_flt (:1013-1026) on finite operands = v_max3_f32
                    P[d] = best;
                    left = __fadd_rn(best, gap);
                }
                if (PAIRS) asm volatile("" ::"v"(unused));                       // (no instruction)
                slide(hw, hwp, pos);
            };
            // a row near a matrix edge: exactly k_nw_lane's EDGE row
            auto row_edge = [&](const int t, const uint32_t v, uint32_t hw, uint32_t hwp, uint32_t pos) {
                const int i = Li - 1 - t;
                const float lastcol = __fmul_rn(gap, (float)(unsigned)(Li - i));                  // nm[i][L] = gGAP * (L - i)
#pragma unroll
                for (int d = 6; d >= 0; --d) {
                    const int j = i + d - 3;
                    const float val = cell_val(v, d);
                    const float up = d > 0 ? P[d - 1] : ((i + 1 == Li) ? gap4 : GM_NEG_INF);     // nm[i+1][j]
                    const float left = d < 6 ? P[d + 1] : ((j + 1 == Li) ? gap4 : GM_NEG_INF);   // nm[i][j+1]
                    const float best = fmaxf(fmaxf(__fadd_rn(P[d], val), __fadd_rn(up, gap)), __fadd_rn(left, gap));
                    P[d] = (j >= 0 && j < Li) ? best : (j == Li ? lastcol : GM_NEG_INF);
                }
                slide(hw, hwp, pos);
            };
            auto pick2 = [&](const uint2* X, int k) -> uint2 {                  // k is wave-uniform: a branch tree, one move per word
                uint2 o = X[0];
                switch (k) {
#define GM_NWR_CASE(q) case q: if (q < NCH) o = X[q < NCH ? q : 0]; break;
                    GM_NWR_CASE(1) GM_NWR_CASE(2) GM_NWR_CASE(3) GM_NWR_CASE(4) GM_NWR_CASE(5) GM_NWR_CASE(6) GM_NWR_CASE(7) GM_NWR_CASE(8) GM_NWR_CASE(9)
                    GM_NWR_CASE(10) GM_NWR_CASE(11) GM_NWR_CASE(12) GM_NWR_CASE(13) GM_NWR_CASE(14) GM_NWR_CASE(15) GM_NWR_CASE(16) GM_NWR_CASE(17) GM_NWR_CASE(18)
#undef GM_NWR_CASE
                    default: break;
                }
                return o;
            };
            auto pick_hw = [&](int m) -> uint32_t {
                uint32_t o = HW[0];
                switch (m) {
#define GM_NWR_CASE(q) case q: if (q < NHW) o = HW[q < NHW ? q : 0]; break;
                    GM_NWR_CASE(1) GM_NWR_CASE(2) GM_NWR_CASE(3) GM_NWR_CASE(4) GM_NWR_CASE(5) GM_NWR_CASE(6) GM_NWR_CASE(7) GM_NWR_CASE(8) GM_NWR_CASE(9) GM_NWR_CASE(10)
#undef GM_NWR_CASE
                    default: break;
                }
                return o;
            };
            // rows [t0, t1) of chunk k at run-time positions (the first rows, the tail): EDGE = they touch row L, column L or column -1
            auto tail_rows = [&](const int k, const int t0, const int t1, auto edge_tag) {
                constexpr bool EDGE = decltype(edge_tag)::value;
                const uint2 bw = pick2(XB, k), qw = pick2(XQ, k);
                for (int t = t0; t < t1; ++t) {
                    const uint32_t bsel = (t & 4) ? bw.y : bw.x, qsel = (t & 4) ? qw.y : qw.x;
                    const uint32_t v = row_vals(bsel, qsel, (uint32_t)(t & 3) << 3);
                    const int u = t + 4;
                    const uint32_t hw = pick_hw(u >> 4), hwp = (PAIRS && (u & 15) == 0) ? pick_hw((u >> 4) - 1) : hw;       // (u >= 16 there)
                    if (EDGE) row_edge(t, v, hw, hwp, 2u * (uint32_t)(u & 15));
                    else row_int(v, hw, hwp, 2u * (uint32_t)(u & 15));
                }
            };
            // interior rows [B0, 8) of chunk k at compile-time positions; PAR = k & 1 fixes where the rows' new columns sit in the window
            // stream.  The class offsets of all rows are requested first (one LDS round trip for the chunk)
            auto rows8 = [&](const int k, auto par_tag, auto b0_tag) {
                constexpr int PAR = decltype(par_tag)::value, B0 = decltype(b0_tag)::value;
                const uint2 bw = pick2(XB, k), qw = pick2(XQ, k);
                const int m = (8 * k + 4) >> 4;
                const uint32_t hw_lo = pick_hw(m), hw_hi = PAR ? pick_hw(m + 1) : 0u;
                uint32_t co[8];
#pragma unroll
                for (int bb = B0; bb < 8; ++bb) co[bb] = clsrow[((bb < 4 ? bw.x : bw.y) >> ((bb & 3) << 3)) & 255u];
#pragma unroll
                for (int bb = B0; bb < 8; ++bb) {
                    const uint32_t v = __umul24(((bb < 4 ? qw.x : qw.y) >> ((bb & 3) << 3)) & 255u, qstride) + co[bb];
                    if (PAR) { if (bb < 4) row_int(v, hw_lo, hw_lo, 2u * (12u + bb)); else row_int(v, hw_hi, hw_lo, 2u * (bb - 4u)); }
                    else row_int(v, hw_lo, hw_lo, 2u * (4u + bb));
                }
            };
            if (nchunk >= 4) {
                // rows 0 .. 3 touch row L / column L, rows L - 4 .. L - 1 column -1 (row i = 3 slides column -1 in); all others are interior
                using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I4 = std::integral_constant<int, 4>;
                tail_rows(0, 0, 4, std::true_type{});
                rows8(0, I0{}, I4{});
                const int k_last = nchunk - 3;
                for (int k = 1; k <= k_last; ++k) { if (k & 1) rows8(k, I1{}, I0{}); else rows8(k, I0{}, I0{}); }
                for (int k = k_last + 1; k < nchunk; ++k) {
                    const int lo = 8 * k, hi = (8 * k + 8 < Li) ? 8 * k + 8 : Li, cut = Li - 4;
                    if (lo < cut) tail_rows(k, lo, hi < cut ? hi : cut, std::false_type{});
                    if (hi > cut) tail_rows(k, lo > cut ? lo : cut, hi, std::true_type{});
                }
            } else {
                for (int k = 0; k < nchunk; ++k) tail_rows(k, 8 * k, (8 * k + 8 < Li) ? 8 * k + 8 : Li, std::true_type{});
            }
            ++scored;
            result = P[3];                                                      // nm[0][0]
        } else if (!p.nw) {
            result = (float)c.step;                                             // --no_nw: the score is the vote count (:70-76)
        }
        uint8_t fl = c.flags & 4;
        if (ok) {
            fl |= GMC_VALID;
            if (result > 0.0f) atomicMax(reinterpret_cast<int*>(&b.top_score[r]), __float_as_int(result));   // top_align_score (:95-98)
            if ((double)result >= min_score) {                                 // :102
                fl |= GMC_ACCEPT;
                atomicAdd(&b.hit_count[r], 1u);
                ++accepted;
            }
        }
        // {step, flags, pad, score}: the record's upper 8 bytes, one store
        const uint2 out = make_uint2((c_hi & 0xFF00FFFFu) | ((uint32_t)fl << 16), __float_as_uint(result));
        __builtin_memcpy(reinterpret_cast<unsigned char*>(&b.cands[ci]) + 8, &out, 8);
    }
    gm_count(b, GMK_NW_CELLS, (unsigned long long)scored * band_cells);
    gm_count(b, GMK_ACCEPTED, (unsigned long long)accepted);
}

// bytes per pair record: 128 + a skew of 0 .. 64 bytes in steps of 8 (the entries stay 8-byte aligned for ds_read_b64)
static uint32_t nw_pair_rs() {
    const long long k = gm_opt_ll("GM_NW_PAIR_SKEW", GM_NWR_PAIR_SKEW);
    return 128u + ((k >= 0 && k <= 64 && k % 8 == 0) ? (uint32_t)k : GM_NWR_PAIR_SKEW);
}
// the pair form's dynamic LDS for the quality characters [qlo, qhi] of a block, 0 = none (no valid range)
static size_t nw_pair_lds(uint32_t ntab, uint32_t qlo, uint32_t qhi) {
    return (qlo <= qhi && qhi < 128u) ? (size_t)ntab * (qhi - qlo + 1u) * 5u * nw_pair_rs() : 0;
}
#define GM_NWR_FASTA_CELLS_BYTES 256u       // FASTA blocks, cells form: 16 mask records of 16 bytes

// workgroups per CU: the pair form (lds bytes of table) holds at least as many as the cells form
template <bool FA>
static bool nw_pairs_fit(bool narrow, size_t lds_cells, size_t lds) {
    int per_cells = 0, per_pairs = 0;
    hipError_t e0, e1;
    if (narrow) {
        e0 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cells, k_nw_rows<13, false, FA>, 256, lds_cells);
        e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_pairs, k_nw_rows<13, true, FA>, 256, lds);
    } else {
        e0 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cells, k_nw_rows<19, false, FA>, 256, lds_cells);
        e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_pairs, k_nw_rows<19, true, FA>, 256, lds);
    }
    return e0 == hipSuccess && e1 == hipSuccess && per_pairs > 0 && per_pairs >= per_cells;
}

// the pair table unless it would leave fewer workgroups per CU than the cells table (wide quality ranges, two tables), or GM_NW_CELLS=b32
bool gmk_nw_rows_pairs(const GmDevBatch& b, uint32_t L, uint32_t qlo, uint32_t qhi) {
    if (gm_opt_is("GM_NW_CELLS", "b32")) return false;
    const uint32_t ntab = b.illumina_until ? 2u : 1u;
    const size_t lds = b.fasta ? (size_t)16u * nw_pair_rs() : nw_pair_lds(ntab, qlo, qhi);
    const size_t lds_cells = b.fasta ? (size_t)GM_NWR_FASTA_CELLS_BYTES : (size_t)ntab * GM_NWR_TAB_BYTES;
    if (!lds) return false;
    return b.fasta ? nw_pairs_fit<true>(L <= 104, lds_cells, lds) : nw_pairs_fit<false>(L <= 104, lds_cells, lds);
}

// L = the one read length of the block; [qlo, qhi] = the range of its quality characters (all below 128); illumina = some reads of the
// block use the Phred+64 table (both tables are then resident); any_superseded = the retry kernel or the heavy path ran for this launch (a
// candidate's rs_overflow byte is read only then)
int gmk_nw_rows(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, uint32_t n_cands, uint32_t L, uint32_t qlo, uint32_t qhi, bool any_superseded, void* stream) {
    if (b.n == 0) return 0;
    const uint32_t ntab = (b.illumina_until && !b.fasta) ? 2u : 1u;
    const bool pairs = gmk_nw_rows_pairs(b, L, qlo, qhi);
    const size_t lds = b.fasta ? (pairs ? (size_t)16u * nw_pair_rs() : (size_t)GM_NWR_FASTA_CELLS_BYTES) : pairs ? nw_pair_lds(ntab, qlo, qhi) : (size_t)ntab * GM_NWR_TAB_BYTES;
    const uint32_t nq = b.fasta ? 1u : pairs ? qhi - qlo + 1u : 0u, q0 = (pairs && !b.fasta) ? qlo : 0u;
    // the workgroups stride over the candidates: one resident round of them (4 per CU for <13> with one table; fewer with two tables or
    // for <19>).  The earlier grid of n_cands / 1024 workgroups (10 449 at 10.7 M candidates) left its last round a fifth full and
    // built the value table 10 times per CU: 2.04 -> 1.85 ms
    const uint32_t nw_fixed = (uint32_t)gm_opt_ll("GM_NW_GRID", 0);
    const bool narrow = L <= 104;
#define GM_NWR_LAUNCH_(N, PR, FA, FB)                                                                                                          \
    hipLaunchKernelGGL((k_nw_rows<N, PR, FA>), dim3(nw_fixed ? nw_fixed : resident_grid(k_nw_rows<N, PR, FA>, 256, lds, FB)), dim3(256), lds, \
                       S_(stream), ix, p, b, L, ntab, q0, nq, nw_pair_rs(), any_superseded ? 1u : 0u)
#define GM_NWR_LAUNCH(N, PR, FB) do { if (b.fasta) GM_NWR_LAUNCH_(N, PR, true, FB); else GM_NWR_LAUNCH_(N, PR, false, FB); } while (0)
    if (narrow && pairs) GM_NWR_LAUNCH(13, true, 1024u);
    else if (narrow) GM_NWR_LAUNCH(13, false, 1024u);
    else if (pairs) GM_NWR_LAUNCH(19, true, 768u);
    else GM_NWR_LAUNCH(19, false, 768u);
#undef GM_NWR_LAUNCH_
#undef GM_NWR_LAUNCH
    return (int)hipGetLastError();
}
