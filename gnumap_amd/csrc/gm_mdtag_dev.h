// gm_mdtag_dev.h — NM:i and MD:Z of a row AS PRINTED (gm_batch_set_row_tags, a defined extension: DESIGN.md section 5): what
// `samtools calmd` derives from the row's POS, CIGAR field, SEQ and the reference.  One wave-level walk, written once and used three
// times: k_md_sizes counts (WRITE = false), k_out_text_rows and k_bam_rows write the string (WRITE = true).
//
//   x = POS-1; z = 0; u = 0; nm = 0; md = ""
//   for every token (n, op) of the CIGAR field as printed, read as k_bam_sizes reads it (n = 0 contributes nothing):
//     M: n times: if z >= len(SEQ) or x >= len(contig): the walk ends
//                 if code(SEQ[z]) == code(T[x]) and that code != 15: u += 1
//                 else: md += str(u) + T[x]; u = 0; nm += 1
//                 x += 1; z += 1
//     I: z += n; nm += n
//     D: md += str(u) + "^"; u = 0; nm += n; then n times, while x < len(contig): md += T[x]; x += 1
//   md += str(u)                                   (once, also when the walk ended early)
//
// T is the contig's text - the pac letter, or inside a hole of <fa>.gnumap.amb that hole's character, upper case - and code() the BAM
// nibble of a character (gm_bam_nibble, gm_fmt_dev.h: the function k_bam_rows packs SEQ with).
// The tokens are taken one after the other (a row has a handful), the columns of a token 64 per trip: every
// lane compares its column, one ballot gives every mismatch the run of matches in front of it, a prefix sum over the lanes the place of
// its bytes.  No atomics; every value that steers a loop is the same in all 64 lanes, so the ballots and shuffles see the whole wave.
// The two "walk ends" clamps are memory safety: no load goes past the read's row, the contig or l_pac, and no store past `end`.
#pragma once
#include "gm_internal.h"
#include "gm_fmt_dev.h"

#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t md_digits(uint32_t v) {
    uint32_t d = 1;
    while (v >= 10u) { v /= 10u; ++d; }
    return d;
}
// the decimal digits of v at out[at ...), inside [.., end)
__device__ __forceinline__ void md_put(uint8_t* out, unsigned long long at, unsigned long long end, uint32_t v, uint32_t d) {
    for (uint32_t q = d; q > 0; --q) { if (at + q - 1u < end) out[at + q - 1u] = (uint8_t)('0' + v % 10u); v /= 10u; }
}
// T at concatenated position g (< l_pac).  h0: the first hole that ends behind the row's first column (n_holes: none)
__device__ __forceinline__ char md_ref_char(const GmDevText& t, uint32_t g, uint32_t h0, bool in_reach) {
    char c = "ACGT"[(t.pac[g >> 2] >> ((~g & 3u) << 1)) & 3u];
    if (in_reach) {
        uint32_t h = h0;
        while (h < t.n_holes && g - t.holes[3u * h] >= t.holes[3u * h + 1u] && t.holes[3u * h] <= g) ++h;      // holes that end at or before g
        if (h < t.n_holes && t.holes[3u * h] <= g) c = (char)t.holes[3u * h + 2u];
    }
    return c;
}
// does the row get the two tags: it prints a record whose CIGAR field is neither "*" nor empty (a field of digits alone prints as
// an empty column on the minus strand under GM_CIGAR_GNUMAP: there is no alignment to describe either)
__device__ __forceinline__ bool md_row_has_tags(const char* cg, uint32_t gout) { return gout != 0u && cg[0] != '*'; }

// The row of record r: SEQ is the L characters of bs (reverse-complemented on the minus strand, as the row kernels print it), the
// CIGAR field bytes [0, gout) of cg - its tokens last to first when rev.  WRITE: the string goes to out[o ...), never at or behind
// `end`.  *nm_out, *len_out: NM and the bytes of the string, in every lane.  To be called by all 64 lanes of a wavefront.
template <bool WRITE>
__device__ __forceinline__ void gm_md_walk(const GmDevText& t, const GmDevSamRec& r, const uint8_t* bs, uint32_t L, const char* cg, uint32_t gout, bool rev,
                                           uint32_t lane, uint8_t* out, unsigned long long o, unsigned long long end, uint32_t* nm_out, uint32_t* len_out) {
    const bool neg = r.strand != 0;
    const uint32_t contig = r.contig < t.n_seqs ? r.contig : 0u;
    const uint32_t coff = t.contig_off[contig];
    uint32_t clen = t.contig_off[contig + 1u] - coff;
    if (coff >= t.l_pac) clen = 0; else if (clen > t.l_pac - coff) clen = t.l_pac - coff;
    unsigned long long x = r.chr_pos - 1ull, z = 0;              // columns of the contig and of SEQ (a POS of 0 wraps to a place behind every contig)
    uint32_t u = 0, nm = 0, mdlen = 0;
    // the hole lookup, once per row: the first hole that ends behind the first column
    uint32_t h0 = t.n_holes, hole_at = 0xFFFFFFFFu;
    if (t.n_holes && x < clen) {
        const uint32_t g0 = coff + (uint32_t)x;
        uint32_t lo = 0, hi = t.n_holes;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (t.holes[3u * mid] + t.holes[3u * mid + 1u] <= g0) lo = mid + 1u; else hi = mid; }
        h0 = lo;
        if (h0 < t.n_holes) hole_at = t.holes[3u * h0];
    }
    // the field's bytes: a lane each when they fit (they nearly always do), so that the token loop reads registers
    const bool in_regs = gout <= 64u;
    const int mine = in_regs && lane < gout ? (int)(uint8_t)cg[lane] : 0;
    auto byte_at = [&](uint32_t i) -> char { return in_regs ? (char)__shfl(mine, (int)i) : cg[i]; };
    uint32_t fwd = 0, back = gout;                                  // the bytes not yet taken: [fwd, back)
    bool ended = false;
    while (!ended && fwd < back) {
        // ---- the next token in print order: (n, op); op 0 = a byte that is no operation (its digits count for nothing) ----
        uint32_t n = 0; char op = 0;
        if (!rev) {
            char c = 0;
            while (fwd < back && (c = byte_at(fwd), c >= '0' && c <= '9')) { n = n * 10u + (uint32_t)(c - '0'); ++fwd; }
            if (fwd >= back) break;                                 // digits behind the last operation
            op = c; ++fwd;
        } else {
            const uint32_t te = back - 1u;
            uint32_t ts = te;
            while (ts > fwd) { const char c = byte_at(ts - 1u); if (!(c >= 48 && c <= 58)) break; --ts; }      // ':' counts as a digit of a token (reverse_cigar)
            for (uint32_t j = ts; j < te; ++j) { const char c = byte_at(j); n = (c >= '0' && c <= '9') ? n * 10u + (uint32_t)(c - '0') : 0u; }
            op = byte_at(te); back = ts;
        }
        n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n); op = (char)__builtin_amdgcn_readfirstlane((int)op);      // (the same in every lane)
        if (n == 0) continue;
        if (op == 'M') {
            unsigned long long stop = n;
            const unsigned long long zl = z < L ? L - z : 0ull, xl = x < clen ? clen - x : 0ull;
            if (zl < stop) stop = zl;
            if (xl < stop) stop = xl;
            for (unsigned long long c0 = 0; c0 < stop; c0 += 64ull) {
                const uint32_t cnt = (uint32_t)(stop - c0 < 64ull ? stop - c0 : 64ull);
                const bool act = lane < cnt;
                const uint32_t g = coff + (uint32_t)(x + c0) + lane, zi = (uint32_t)(z + c0) + lane;
                char tch = 'N'; bool mis = false;
                if (act) {
                    tch = md_ref_char(t, g, h0, coff + (uint32_t)(x + c0) + cnt > hole_at);
                    const char sch = neg ? gm_comp_char((char)bs[L - 1u - zi]) : (char)bs[zi];
                    const uint32_t cs = gm_bam_nibble(sch);
                    mis = !(cs == gm_bam_nibble(tch) && cs != 15u);
                }
                const unsigned long long m = __builtin_amdgcn_ballot_w64(mis);
                if (m == 0ull) { u += cnt; continue; }
                const unsigned long long below = m & ((1ull << lane) - 1ull);
                const uint32_t run = below ? lane - 1u - (63u - (uint32_t)__clzll((long long)below)) : u + lane;
                const uint32_t dg = md_digits(run), bytes = mis ? dg + 1u : 0u;
                uint32_t incl = bytes;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const uint32_t v = __shfl_up(incl, off); if ((int)lane >= off) incl += v; }
                if (WRITE && mis) {
                    const unsigned long long at = o + mdlen + (incl - bytes);
                    md_put(out, at, end, run, dg);
                    if (at + dg < end) out[at + dg] = (uint8_t)tch;
                }
                mdlen += (uint32_t)__shfl(incl, 63);
                nm += (uint32_t)__popcll(m);
                u = cnt - 1u - (63u - (uint32_t)__clzll((long long)m));
            }
            if (stop < n) { ended = true; break; }
            x += n; z += n;
        } else if (op == 'I') {
            z += n; nm += n;
        } else if (op == 'D') {
            const uint32_t dg = md_digits(u);
            if (WRITE && lane == 0) { md_put(out, o + mdlen, end, u, dg); if (o + mdlen + dg < end) out[o + mdlen + dg] = (uint8_t)'^'; }
            mdlen += dg + 1u; u = 0; nm += n;
            const unsigned long long xl = x < clen ? clen - x : 0ull;
            const uint32_t cols = (uint32_t)(xl < n ? xl : n);
            if (WRITE) {
                const bool reach = cols && coff + (uint32_t)x + cols > hole_at;
                for (uint32_t c = lane; c < cols; c += 64u) {
                    const unsigned long long at = o + mdlen + c;
                    if (at < end) out[at] = (uint8_t)md_ref_char(t, coff + (uint32_t)x + c, h0, reach);
                }
            }
            mdlen += cols; x += cols;
        }
    }
    const uint32_t dg = md_digits(u);
    if (WRITE && lane == 0) md_put(out, o + mdlen, end, u, dg);
    *nm_out = nm; *len_out = mdlen + dg;
}
#endif
