// gm_output.hip — the device half of what the reference does AFTER a candidate has been scored:
//
//   k_group_*        process_hits' unique-sequence map (inc/align_seq2_raw.cpp:102-165) and the -T / -u exits of
//                    align_sequence (:299-306, :146-152) / set_top_matches (src/Driver.cpp:506-610): the accepted hits of a read
//                    are put in the reference's processing order (POS strand pass, then NEG; seed step; ascending position),
//                    grouped by their window string in READ orientation (2-bit packed compare, no strings), the groups ranked in
//                    std::map<string> (lexicographic) order, and written as gm_match / gm_pos records in HBM.
//   k_out_*          create_match_output (src/Driver.cpp:614-753): SAM rows (TopReadOutput, inc/ScoredSeq.h:375-401) with their
//                    run-length CIGAR built from the traceback operations (src/bin_seq.cpp:578-698, fix_CIGAR_for_deletions
//                    inc/SequenceOperations.h:32-42), and the coverage deposit of every kept sequence
//                    (NormalScoredSeq::score src/NormalScoredSeq.cpp:66-75, BSScoredSeq::score src/BSScoredSeq.cpp:24-88).
//   k_row_*          gm_batch_set_unmapped_rows (a defined extension): the map from row to (record | read without a
//                    record), so that k_out_text_* and k_bam_* (gm_bam.hip) write one flag-4 row for every read the reference drops
//   k_md_sizes       gm_batch_set_row_tags (a defined extension as well): NM:i and MD:Z of every row as printed, sized here and written by
//                    k_out_text_rows / k_bam_rows through the one walk of gm_mdtag_dev.h
//
// What stays on the host (gm_api.cpp) is only the order-dependent fp64 libm work on a flat array of scores:
// denominator += exp(score) in processing order, posterior = exp(score) / denominator, MAPQ = round(-10 log10(1 - p)).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "gm_internal.h"
#include "gm_fmt_dev.h"
#include "gm_mdtag_dev.h"

namespace {

__device__ __forceinline__ uint32_t go_pos2rid(const uint32_t* coff, uint32_t n_seqs, uint32_t pos) {   // bns_pos2rid src/bntseq.c:349-363
    uint32_t lo = 0, hi = n_seqs - 1;
    while (lo < hi) {
        uint32_t mid = (lo + hi + 1) >> 1;
        if (pos >= coff[mid]) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// 32 reference bases starting at g, MSB first (2 bits each); the device pac buffer is padded, bytes past the end are never used
// by a valid window
__device__ __forceinline__ unsigned long long go_ref_word(const uint8_t* pac, uint32_t g) {
    const uint8_t* q = pac + (g >> 2);
    unsigned long long w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w = (w << 8) | q[k];
    const uint32_t sh = (g & 3u) * 2u;
    if (sh) w = (w << sh) | ((unsigned long long)q[8] >> (8u - sh));
    return w;
}

// reverse the order of the 32 two-bit groups of a word
__device__ __forceinline__ unsigned long long go_rev_pairs(unsigned long long x) {
    x = __brevll(x);
    return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
}

// word j (bases 32j .. 32j+31, MSB first, zero padded) of the unique-map key of a hit: the window in READ orientation, i.e. the
// window itself for a POS-strand hit and reverse_comp(window) for a NEG-strand hit (align_seq2_raw.cpp:125-128).  Base codes
// a<c<g<t are 0<1<2<3, so comparing the words as unsigned integers is the std::string comparison of the keys.
__device__ __forceinline__ unsigned long long go_key_word(const uint8_t* pac, uint32_t pos, uint32_t L, uint32_t strand, uint32_t j) {
    const uint32_t done = 32u * j;
    const uint32_t cnt = L - done < 32u ? L - done : 32u;
    unsigned long long k;
    if (!strand) {
        k = go_ref_word(pac, pos + done);
        if (cnt < 32u) k &= ~0ull << (2u * (32u - cnt));
    } else {
        const uint32_t gstart = pos + L - done - cnt;       // lowest reference position of this word's bases
        unsigned long long w = go_ref_word(pac, gstart);    // its top `cnt` groups are the ones wanted
        // the reversal moves them to the low 2*cnt bits in read order; complement (3 - c), then up to the top (zeros shift in)
        k = ~go_rev_pairs(w);
        if (cnt < 32u) k <<= 2u * (32u - cnt);
    }
    return k;
}

// 64-bit hash of a key.  Every word goes through a full-avalanche mixer (the murmur3 finaliser): repeat copies differ from each other
// in a handful of bases, and with a multiply-only step a difference in the top bits of one word stays in the top bits and is cancelled
// by a difference at the same place in the next word - near-identical windows then collide by the dozen (seen on a repeat-rich
// reference: 53 reads of 2424 handed back for "collisions").
__device__ __forceinline__ unsigned long long go_mix64(unsigned long long x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
__device__ __forceinline__ unsigned long long go_key_hash(const uint8_t* pac, uint32_t pos, uint32_t L, uint32_t strand) {
    unsigned long long h = 0x243F6A8885A308D3ull;
    const uint32_t nw = (L + 31u) >> 5;
    for (uint32_t j = 0; j < nw; ++j) h = go_mix64(h ^ go_key_word(pac, pos, L, strand, j)) + 0x9E3779B97F4A7C15ull;
    return h;
}

// <0, 0, >0: key(a) vs key(b) in std::string order
__device__ __forceinline__ int go_key_cmp(const uint8_t* pac, uint32_t L, uint32_t pa, uint32_t sa, uint32_t pb, uint32_t sb) {
    if (pa == pb && sa == sb) return 0;
    const uint32_t nw = (L + 31u) >> 5;
    for (uint32_t j = 0; j < nw; ++j) {
        unsigned long long x = go_key_word(pac, pa, L, sa, j), y = go_key_word(pac, pb, L, sb, j);
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

// the reference's processing order of accepted hits: POS strand pass before NEG (Driver.cpp:506-556); inside a pass the seed step
// at which the position reached -k votes (align_sequence loop), then ascending position (std::map<unsigned long,int>, process_hits).
// --no_nw scores every position of a strand in ONE process_hits call at the end (:317-325): strand, then position.
__device__ __forceinline__ bool go_hit_less(const GmRawHit& a, const GmRawHit& b, int nw) {
    if (a.strand != b.strand) return a.strand < b.strand;
    if (nw && a.step != b.step) return a.step < b.step;
    return a.pos < b.pos;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// grouping, pass 1: reads with 0 or 1 accepted hits are finished by one thread; the others go to a list
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_group_single(GmDevBatch b, GmDevGroup g, int nw, uint32_t max_matches, uint32_t big_min) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b.n) return;
    const uint64_t hb = b.hit_begin[r];
    const uint32_t k = (uint32_t)(b.hit_begin[r + 1] - hb);
    uint32_t nm = 0;
    if (b.status[r] == 0) {
        if (k == 0) b.status[r] = 2;                                     // GM_READ_NONE: the unique map stayed empty (Driver.cpp:595-601)
        else if (k == 1) {
            const GmRawHit h = b.raw_hits[hb];
            g.sorted[hb] = h; g.ord_score[hb] = h.score; g.lead[hb] = 0; g.krank[hb] = 0;
            if (nw && 1u > max_matches) b.status[r] = 1;                  // unique.size() > gMAX_MATCHES (align_seq2_raw.cpp:299-306)
            else nm = 1;
        } else {
            if (k > big_min) { const uint32_t at = atomicAdd(g.n_big, 1u); g.big_list[at] = r; g.big_done[at] = 0; }
            else g.multi_list[atomicAdd(g.n_multi, 1u)] = r;
            return;                                                      // n_match is written by k_group_multi / k_group_big
        }
    }
    g.n_match[r] = nm;
}

// one wavefront per read with >= 2 accepted hits
__global__ void __launch_bounds__(64) k_group_multi(GmDevIndex ix, GmDevBatch b, GmDevGroup g, int nw, int unique_only, uint32_t max_matches) {
    __shared__ uint32_t s_cnt[2];
    const int lane = threadIdx.x;
    const uint32_t n_multi = *g.n_multi;
    for (uint32_t li = blockIdx.x; li < n_multi; li += gridDim.x) {
        const uint32_t r = g.multi_list[li];
        const uint64_t hb = b.hit_begin[r];
        const uint32_t k = (uint32_t)(b.hit_begin[r + 1] - hb);
        const uint32_t L = b.len[r];
        const GmRawHit* raw = b.raw_hits + hb;
        GmRawHit* srt = g.sorted + hb;
        if (lane < 2) s_cnt[lane] = 0;
        // 1. processing order: rank of every hit among the read's hits ((strand, pos) is unique, so the order is total)
        for (uint32_t a = lane; a < k; a += 64) {
            const GmRawHit ha = raw[a];
            uint32_t rank = 0;
            for (uint32_t c = 0; c < k; ++c) rank += go_hit_less(raw[c], ha, nw) ? 1u : 0u;
            srt[rank] = ha;
        }
        __syncthreads();
        // 2. key hash of every hit
        for (uint32_t s = lane; s < k; s += 64) g.khash[hb + s] = go_key_hash(ix.pac, srt[s].pos, L, srt[s].strand);
        __syncthreads();
        // 3. leader = the first hit in processing order with the same key (hash, then the 2-bit words themselves)
        for (uint32_t s = lane; s < k; s += 64) {
            const unsigned long long hs = g.khash[hb + s];
            const GmRawHit h = srt[s];
            uint32_t l = s;
            for (uint32_t t = 0; t < s; ++t)
                if (g.khash[hb + t] == hs && go_key_cmp(ix.pac, L, srt[t].pos, srt[t].strand, h.pos, h.strand) == 0) { l = t; break; }
            g.lead[hb + s] = l;
            g.ord_score[hb + s] = h.score;
        }
        __syncthreads();
        bool too_many = false;
        if (unique_only) {
            if (nw) {
                // -u: an existing key makes align_sequence return false -> READ_TOO_MANY (align_seq2_raw.cpp:146-152, Driver.cpp:512-525)
                bool dup = false;
                for (uint32_t s = lane; s < k; s += 64) dup |= g.lead[hb + s] != s;
                too_many = __ballot(dup) != 0ull;
            } else if (lane == 0) {
                // --no_nw ignores process_hits' return value (:317-325): the rest of THAT strand's single pass is dropped, nothing else
                bool stopped = false; uint32_t cur = 2;
                for (uint32_t s = 0; s < k; ++s) {
                    if (srt[s].strand != cur) { cur = srt[s].strand; stopped = false; }
                    bool drop = stopped;
                    if (!drop) {
                        for (uint32_t t = 0; t < s; ++t)
                            if (g.lead[hb + t] != 0xFFFFFFFFu && g.khash[hb + t] == g.khash[hb + s] &&
                                go_key_cmp(ix.pac, L, srt[t].pos, srt[t].strand, srt[s].pos, srt[s].strand) == 0) { drop = true; stopped = true; break; }
                    }
                    if (drop) { g.lead[hb + s] = 0xFFFFFFFFu; g.ord_score[hb + s] = -INFINITY; }
                    else g.lead[hb + s] = s;
                }
            }
            __syncthreads();
        }
        // 4. number of keys first: a read beyond -T is READ_TOO_MANY whatever the order of its keys is (the map only grows, so the
        //    check after the last seed decides, align_seq2_raw.cpp:299-306) - and ranking thousands of repeat copies would be the
        //    one quadratic step with full key compares
        uint32_t my_leaders = 0;
        for (uint32_t s = lane; s < k; s += 64) my_leaders += g.lead[hb + s] == s ? 1u : 0u;
        if (my_leaders) atomicAdd(&s_cnt[0], my_leaders);
        __syncthreads();
        const uint32_t u = s_cnt[0];
        if (nw && u > max_matches) too_many = true;
        // 5. rank of every key among the read's keys (std::map<string> order): first words first, the whole key only on a tie
        if (!too_many) {
            for (uint32_t s = lane; s < k; s += 64)
                if (g.lead[hb + s] == s) g.khash[hb + s] = go_key_word(ix.pac, srt[s].pos, L, srt[s].strand, 0);      // the hash has done its work
            __syncthreads();
            for (uint32_t s = lane; s < k; s += 64) {
                if (g.lead[hb + s] != s) continue;
                const GmRawHit h = srt[s];
                const unsigned long long w0 = g.khash[hb + s];
                uint32_t rank = 0;
                for (uint32_t t = 0; t < k; ++t) {
                    if (t == s || g.lead[hb + t] != t) continue;
                    const unsigned long long wt = g.khash[hb + t];
                    if (wt < w0 || (wt == w0 && go_key_cmp(ix.pac, L, srt[t].pos, srt[t].strand, h.pos, h.strand) < 0)) ++rank;
                }
                g.krank[hb + s] = rank;
            }
        }
        if (lane == 0) {
            if (too_many) { b.status[r] = 1; g.n_match[r] = 0; }
            else if (u == 0) { b.status[r] = 2; g.n_match[r] = 0; }
            else g.n_match[r] = u;
        }
        __syncthreads();
    }
}


// ------------------------------------------------------------------------------------------------
// grouping of reads with MANY accepted hits (repeat copies: up to 10^5 .. 10^6 per read), linear in the hits instead of the
// all-pairs steps of k_group_multi:
//   * distinct keys are counted in an LDS hash set keyed by the 64-bit key hash, value = the smallest processing-order key among
//     the hits with that hash.  More distinct hashes than -T means more distinct keys than -T: READ_TOO_MANY as soon as the count
//     passes -T, after a few thousand insertions (what the reference finds out seed by seed, align_seq2_raw.cpp:299-306)
//   * otherwise the hits are put in processing order by a wave-level LSD radix sort in HBM, the leader of a hit is found through the
//     set (and verified on the 2-bit windows: a hash collision hands the read back to the all-pairs kernel), the few keys are ranked
//     all-pairs, and a second sort by (key rank, position, strand) lays out the matches' position sets (k_group_write_big)
// ------------------------------------------------------------------------------------------------
#define GO_SET_SLOTS 4096u
#define GO_SET_LIMIT 3000u

// stable LSD radix sort (4-bit digits) of (key, value) pairs by one wavefront, ping-pong between (k0, v0) and (k1, v1); returns 0 / 1 =
// which pair of buffers holds the result.  Needs blockDim.x == 64 (uses __syncthreads between passes).
__device__ int go_wave_sort(unsigned long long* k0, uint32_t* v0, unsigned long long* k1, uint32_t* v1, uint32_t n, int nbits, int lane) {
    unsigned long long* kin = k0; uint32_t* vin = v0; unsigned long long* kout = k1; uint32_t* vout = v1;
    int cur = 0;
    for (int shift = 0; shift < nbits; shift += 4) {
        // histogram: lane d (< 16) ends up with the number of keys whose digit is d
        uint32_t total = 0;
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane;
            const uint32_t dig = i < n ? (uint32_t)(kin[i] >> shift) & 15u : 16u;
#pragma unroll
            for (uint32_t d = 0; d < 16; ++d) {
                const unsigned long long m = __builtin_amdgcn_ballot_w64(dig == d);
                if ((uint32_t)lane == d) total += (uint32_t)__popcll(m);
            }
        }
        // exclusive prefix over the 16 digits (lanes 0..15)
        uint32_t incl = (uint32_t)lane < 16u ? total : 0u;
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) { const uint32_t t = __shfl_up(incl, off); if (lane >= off) incl += t; }
        uint32_t run = incl - ((uint32_t)lane < 16u ? total : 0u);       // lane d: where the next key with digit d goes
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane;
            unsigned long long key = 0; uint32_t val = 0;
            uint32_t dig = 16u;
            if (i < n) { key = kin[i]; val = vin[i]; dig = (uint32_t)(key >> shift) & 15u; }
            uint32_t my_rank = 0;
#pragma unroll
            for (uint32_t d = 0; d < 16; ++d) {
                const unsigned long long m = __builtin_amdgcn_ballot_w64(dig == d);
                const uint32_t start = __shfl(run, (int)d);
                if (dig == d) my_rank = start + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if ((uint32_t)lane == d) run += (uint32_t)__popcll(m);
            }
            if (i < n) { kout[my_rank] = key; vout[my_rank] = val; }
        }
        __syncthreads();
        unsigned long long* tk = kin; kin = kout; kout = tk;
        uint32_t* tv = vin; vin = vout; vout = tv;
        cur ^= 1;
    }
    return cur;
}

__global__ void __launch_bounds__(64) k_group_big(GmDevIndex ix, GmDevBatch b, GmDevGroup g, int nw, int unique_only, uint32_t max_matches) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_big[];
    unsigned long long* s_keys = reinterpret_cast<unsigned long long*>(s_big);           // GO_SET_SLOTS hashes (0 = empty)
    unsigned long long* s_vals = s_keys + GO_SET_SLOTS;                                  // smallest order key of the hash
    uint32_t* s_lead = reinterpret_cast<uint32_t*>(s_vals + GO_SET_SLOTS);               // up to GO_SET_LIMIT leaders (sorted index)
    __shared__ uint32_t s_n[4];                                                          // distinct hashes, leaders, flags
    const int lane = threadIdx.x;
    const uint32_t n_big = *g.n_big;
    for (uint32_t li = blockIdx.x; li < n_big; li += gridDim.x) {
        const uint32_t r = g.big_list[li];
        const uint64_t hb = b.hit_begin[r];
        const uint32_t k = (uint32_t)(b.hit_begin[r + 1] - hb);
        const uint32_t L = b.len[r];
        const GmRawHit* raw = b.raw_hits + hb;
        GmRawHit* srt = g.sorted + hb;
        auto hand_back = [&](int why) { if (lane == 0) { g.multi_list[atomicAdd(g.n_multi, 1u)] = r; atomicAdd(g.n_big + 1 + why, 1u); } };    // the all-pairs kernel runs after this one; n_big[1..3] count the reasons
        if (unique_only && !nw) { hand_back(0); continue; }                // per-strand drop rule of --no_nw -u: rare, all-pairs kernel
        for (uint32_t q = lane; q < GO_SET_SLOTS; q += 64) { s_keys[q] = 0ull; s_vals[q] = ~0ull; }
        if (lane < 4) s_n[lane] = 0;
        __syncthreads();
        const uint32_t limit = nw && max_matches < GO_SET_LIMIT ? max_matches : GO_SET_LIMIT;
        // 1. hash + processing-order key of every hit; distinct hashes into the set (stops as soon as the count passes the limit)
        for (uint32_t base = 0; base < k; base += 64) {
            const uint32_t a = base + lane;
            if (a < k) {
                const GmRawHit h = raw[a];
                const unsigned long long hs = go_key_hash(ix.pac, h.pos, L, h.strand) | 1ull;
                const unsigned long long ok = nw ? ((unsigned long long)h.strand << 48) | ((unsigned long long)h.step << 32) | h.pos
                                                 : ((unsigned long long)h.strand << 48) | h.pos;
                g.khash[hb + a] = hs; g.sk0[hb + a] = ok; g.si0[hb + a] = a;
                uint32_t slot = (uint32_t)(hs >> 17) & (GO_SET_SLOTS - 1u);
                for (uint32_t probe = 0; probe < GO_SET_SLOTS; ++probe) {
                    const unsigned long long old = atomicCAS(&s_keys[slot], 0ull, hs);
                    if (old == 0ull) atomicAdd(&s_n[0], 1u);
                    if (old == 0ull || old == hs) { atomicMin(&s_vals[slot], ok); break; }
                    slot = (slot + 1u) & (GO_SET_SLOTS - 1u);
                }
            }
            __syncthreads();
            if (s_n[0] > limit) break;                                    // uniform: read after the barrier
        }
        __syncthreads();
        const uint32_t distinct = s_n[0];
        if (distinct > limit) {
            if (nw && limit == max_matches) {                             // more distinct keys than -T: READ_TOO_MANY (Driver.cpp:512-525)
                if (lane == 0) { b.status[r] = 1; g.n_match[r] = 0; g.big_done[li] = 1; }
            } else hand_back(1);                                          // more keys than the set holds and no -T to stop at: all-pairs kernel
            continue;
        }
        // 2. processing order
        const int where = go_wave_sort(g.sk0 + hb, g.si0 + hb, g.sk1 + hb, g.si1 + hb, k, 52, lane);
        const unsigned long long* sk = (where ? g.sk1 : g.sk0) + hb;
        const uint32_t* si = (where ? g.si1 : g.si0) + hb;
        unsigned long long* spare_k = (where ? g.sk0 : g.sk1) + hb;
        for (uint32_t i = lane; i < k; i += 64) { const GmRawHit h = raw[si[i]]; srt[i] = h; g.ord_score[hb + i] = h.score; }
        __syncthreads();
        // 3. leader of every hit = the hit with the smallest order key among those with its hash (verified on the windows)
        bool dup = false, collide = false;
        for (uint32_t i = lane; i < k; i += 64) {
            const unsigned long long hs = g.khash[hb + si[i]];
            uint32_t slot = (uint32_t)(hs >> 17) & (GO_SET_SLOTS - 1u);
            while (s_keys[slot] != hs) slot = (slot + 1u) & (GO_SET_SLOTS - 1u);
            const unsigned long long lk = s_vals[slot];
            uint32_t lo = 0, hi = k - 1;                                  // order keys are unique: binary search for the leader's place
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sk[mid] < lk) lo = mid + 1; else hi = mid; }
            const GmRawHit h = srt[i], hl = srt[lo];
            if (lo != i && go_key_cmp(ix.pac, L, hl.pos, hl.strand, h.pos, h.strand) != 0) collide = true;
            g.lead[hb + i] = lo;
            if (lo != i) dup = true;
            else { const uint32_t at = atomicAdd(&s_n[1], 1u); if (at < GO_SET_LIMIT) s_lead[at] = i; }
        }
        __syncthreads();
        if (__builtin_amdgcn_ballot_w64(collide) != 0ull || s_n[1] != distinct) { hand_back(2); continue; }    // two keys under one hash: all-pairs kernel
        if (unique_only && nw && __builtin_amdgcn_ballot_w64(dup) != 0ull) {     // -u: an existing key -> READ_TOO_MANY (align_seq2_raw.cpp:146-152)
            if (lane == 0) { b.status[r] = 1; g.n_match[r] = 0; g.big_done[li] = 1; }
            continue;
        }
        // 4. rank of the (few) keys in std::map<string> order: first words first, the whole key on a tie
        for (uint32_t q = lane; q < distinct; q += 64) { const GmRawHit h = srt[s_lead[q]]; spare_k[q] = go_key_word(ix.pac, h.pos, L, h.strand, 0); }
        __syncthreads();
        for (uint32_t q = lane; q < distinct; q += 64) {
            const uint32_t i = s_lead[q];
            const GmRawHit h = srt[i];
            const unsigned long long w0 = spare_k[q];
            uint32_t rank = 0;
            for (uint32_t t = 0; t < distinct; ++t) {
                if (t == q) continue;
                const unsigned long long wt = spare_k[t];
                if (wt < w0) ++rank;
                else if (wt == w0) { const GmRawHit ht = srt[s_lead[t]]; if (go_key_cmp(ix.pac, L, ht.pos, ht.strand, h.pos, h.strand) < 0) ++rank; }
            }
            g.krank[hb + i] = rank;
        }
        if (lane == 0) { g.n_match[r] = distinct; g.big_done[li] = 1; }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) k_group_write_big(GmDevBatch b, GmDevGroup g) {
    const int lane = threadIdx.x;
    const uint32_t n_big = *g.n_big;
    for (uint32_t li = blockIdx.x; li < n_big; li += gridDim.x) {
        const uint32_t r = g.big_list[li];
        if (!g.big_done[li] || g.n_match[r] == 0) continue;
        const uint64_t hb = b.hit_begin[r], mb = g.match_begin[r];
        const uint32_t k = (uint32_t)(b.hit_begin[r + 1] - hb);
        const GmRawHit* srt = g.sorted + hb;
        // second sort: (key rank, position, strand) = the matches in std::map order, each with its set<(pos,strand)> in order
        for (uint32_t i = lane; i < k; i += 64) {
            const GmRawHit h = srt[i];
            g.sk0[hb + i] = ((unsigned long long)g.krank[hb + g.lead[hb + i]] << 33) | ((unsigned long long)h.pos << 1) | h.strand;
            g.si0[hb + i] = i;
        }
        __syncthreads();
        const int where = go_wave_sort(g.sk0 + hb, g.si0 + hb, g.sk1 + hb, g.si1 + hb, k, 48, lane);
        const unsigned long long* sk = (where ? g.sk1 : g.sk0) + hb;
        const uint32_t* si = (where ? g.si1 : g.si0) + hb;
        for (uint32_t j = lane; j < k; j += 64) {
            const uint32_t i = si[j];
            const GmRawHit h = srt[i];
            const uint32_t grp = (uint32_t)(sk[j] >> 33);
            GmDevPos p; p.pos = h.pos; p.strand = h.strand; for (int q = 0; q < 7; ++q) p.pad[q] = 0;
            g.positions[hb + j] = p;
            GmDevMatch* m = g.matches + mb + grp;
            if (j == 0 || (uint32_t)(sk[j - 1] >> 33) != grp) {
                const uint32_t l = g.lead[hb + i];
                const GmRawHit hl = srt[l];                               // the FIRST hit of a key gives the ScoredSeq its sequence, score and strand
                m->read = b.read_base + r; m->score = hl.score; m->first_pos = hl.pos; m->first_strand = hl.strand;
                m->pad[0] = m->pad[1] = m->pad[2] = 0; m->tail = 0;
                m->pos_begin = (uint32_t)(hb + j);
                g.match_hit[mb + grp] = (uint32_t)(hb + l);
            }
            if (j + 1 == k || (uint32_t)(sk[j + 1] >> 33) != grp) m->pos_end = (uint32_t)(hb + j + 1);
        }
        __syncthreads();
    }
}

// grouping, pass 2 (after the scan of n_match): gm_match records in key order, their positions as the ordered set<(pos,strand)>
__global__ void __launch_bounds__(256) k_group_write_single(GmDevBatch b, GmDevGroup g) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b.n) return;
    const uint64_t hb = b.hit_begin[r];
    if (g.n_match[r] != 1 || b.hit_begin[r + 1] - hb != 1) return;
    const GmRawHit h = g.sorted[hb];
    GmDevMatch m;
    m.read = b.read_base + r; m.score = h.score; m.first_pos = h.pos; m.first_strand = h.strand; m.pad[0] = m.pad[1] = m.pad[2] = 0;
    m.pos_begin = (uint32_t)hb; m.pos_end = (uint32_t)hb + 1u;
    g.matches[g.match_begin[r]] = m;
    g.match_hit[g.match_begin[r]] = (uint32_t)hb;
    GmDevPos p; p.pos = h.pos; p.strand = h.strand; for (int q = 0; q < 7; ++q) p.pad[q] = 0;
    g.positions[hb] = p;
}

__global__ void __launch_bounds__(64) k_group_write_multi(GmDevBatch b, GmDevGroup g) {
    const int lane = threadIdx.x;
    const uint32_t n_multi = *g.n_multi;
    for (uint32_t li = blockIdx.x; li < n_multi; li += gridDim.x) {
        const uint32_t r = g.multi_list[li];
        if (g.n_match[r] == 0) continue;
        const uint64_t hb = b.hit_begin[r], mb = g.match_begin[r];
        const uint32_t k = (uint32_t)(b.hit_begin[r + 1] - hb);
        const GmRawHit* srt = g.sorted + hb;
        for (uint32_t s = lane; s < k; s += 64) {
            const uint32_t l = g.lead[hb + s];
            if (l == 0xFFFFFFFFu) continue;
            const uint32_t grp = g.krank[hb + l];
            const GmRawHit h = srt[s];
            uint32_t within = 0, goff = 0, gsize = 0;
            for (uint32_t t = 0; t < k; ++t) {
                const uint32_t lt = g.lead[hb + t];
                if (lt == 0xFFFFFFFFu) continue;
                if (lt == l) {
                    ++gsize;
                    const GmRawHit ht = srt[t];
                    within += (ht.pos < h.pos || (ht.pos == h.pos && ht.strand < h.strand)) ? 1u : 0u;     // set<pair<pos,strand>> order
                } else if (g.krank[hb + lt] < grp) ++goff;
            }
            GmDevPos p; p.pos = h.pos; p.strand = h.strand; for (int q = 0; q < 7; ++q) p.pad[q] = 0;
            g.positions[hb + goff + within] = p;
            if (s == l) {                                                 // the FIRST hit of a key gives the ScoredSeq its sequence, score and strand
                GmDevMatch m;
                m.read = b.read_base + r; m.score = h.score; m.first_pos = h.pos; m.first_strand = h.strand; m.pad[0] = m.pad[1] = m.pad[2] = 0;
                m.pos_begin = (uint32_t)(hb + goff); m.pos_end = (uint32_t)(hb + goff + gsize);
                g.matches[mb + grp] = m;
                g.match_hit[mb + grp] = (uint32_t)(hb + s);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// output stage
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_out_items(const GmDevMatch* matches, uint32_t n_m, uint32_t read_base, GmCand* items, uint32_t* pos_match) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_m) return;
    const GmDevMatch mm = matches[m];
    GmCand c; c.rs = (mm.read - read_base) * 2u + mm.first_strand; c.b = (uint32_t)mm.first_pos; c.step = 0; c.flags = 0; c.pad = 0; c.score = 0;
    items[m] = c;
    for (uint32_t q = mm.pos_begin; q < mm.pos_end; ++q) pos_match[q] = m;
}

// once the host pass has said which sequences are printed: SAM rows and CIGAR bytes per match (the traceback kernel left the CIGAR
// length of EVERY match, it ran while the host was still computing)
__global__ void __launch_bounds__(256) k_out_sizes(const GmDevMatch* matches, uint32_t n_m, const uint8_t* emit, const uint32_t* cig_all, uint32_t* rec_cnt,
                                                   uint32_t* cig_cnt) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_m) return;
    const bool e = emit[m] != 0;
    rec_cnt[m] = e ? matches[m].pos_end - matches[m].pos_begin : 0u;     // one SAM row per place of a printed sequence (ScoredSeq.h:375-401)
    cig_cnt[m] = e ? cig_all[m] : 0u;
}

// run-length CIGAR text of a traceback (bin_seq.cpp:578-698) from the packed operations (2 bits each: 0 M, 1 I, 2 D); "" -> "*",
// otherwise one trailing run of D is stripped (fix_CIGAR_for_deletions, SequenceOperations.h:32-42).  Returns the length written.
__device__ __forceinline__ uint32_t go_op(const unsigned long long* ops, uint32_t k) { return (uint32_t)(ops[k >> 5] >> (2u * (k & 31u))) & 3u; }

__device__ __forceinline__ uint32_t go_digits(uint32_t v) { return v >= 10000 ? 5u : v >= 1000 ? 4u : v >= 100 ? 3u : v >= 10 ? 2u : 1u; }

__device__ __forceinline__ uint32_t go_cigar(const unsigned long long* ops, uint32_t n_op, char* out) {
    if (n_op == 0) { out[0] = '*'; return 1; }
    uint32_t end = n_op;
    if (go_op(ops, n_op - 1) == 2u) { while (end > 0 && go_op(ops, end - 1) == 2u) --end; }
    uint32_t w = 0, i = 0;
    unsigned long long word = 0;
    while (i < end) {
        if ((i & 31u) == 0 || i == 0) word = ops[i >> 5];
        const uint32_t op = (uint32_t)(word >> (2u * (i & 31u))) & 3u;
        uint32_t j = i + 1;
        while (j < end) {
            if ((j & 31u) == 0) word = ops[j >> 5];
            if (((uint32_t)(word >> (2u * (j & 31u))) & 3u) != op) break;
            ++j;
        }
        const uint32_t run = j - i, digits = go_digits(run);
        uint32_t v = run;
        for (uint32_t d = digits; d > 0; --d) { out[w + d - 1] = (char)('0' + v % 10u); v /= 10u; }
        out[w + digits] = op == 0 ? 'M' : op == 1 ? 'I' : 'D';
        w += digits + 1;
        i = j;
    }
    return w;
}

__global__ void __launch_bounds__(256) k_out_write(GmDevIndex ix, GmDevBatch b, const GmDevMatch* matches, const GmDevPos* positions, uint32_t n_m,
                                                   const uint8_t* emit, const int32_t* mapq, const float* post, const unsigned long long* ops, uint32_t ops_words,
                                                   const uint16_t* ops_len, int nw, const uint64_t* rec_off, const uint64_t* cig_off,
                                                   GmDevSamRec* recs, char* pool) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_m || !emit[m]) return;
    const GmDevMatch mm = matches[m];
    const uint64_t co = cig_off[m];
    char* cg = pool + co;
    uint32_t cl;
    if (nw) cl = go_cigar(ops + (size_t)m * ops_words, ops_len[m], cg);
    else {                                                              // --no_nw: "<L>M" (ScoredSeq.h:330-340)
        uint32_t L = b.len[mm.read - b.read_base], d = go_digits(L), v = L;
        for (uint32_t q = d; q > 0; --q) { cg[q - 1] = (char)('0' + v % 10u); v /= 10u; }
        cg[d] = 'M'; cl = d + 1;
    }
    cg[cl] = 0;
    uint64_t ro = rec_off[m];
    for (uint32_t q = mm.pos_begin; q < mm.pos_end; ++q, ++ro) {
        const GmDevPos p = positions[q];
        GmDevSamRec s;
        s.read = mm.read; s.pad0 = 0; s.pos = p.pos;
        s.contig = go_pos2rid(ix.contig_off, ix.n_seqs, (uint32_t)p.pos); s.pad1 = 0;
        const int base = (int)((uint32_t)p.pos - ix.contig_off[s.contig]);          // int chr_base_pos, GenomeBwt.cpp:632
        s.chr_pos = (unsigned long long)(long long)base + 1ull;
        s.strand = p.strand; s.pad2[0] = s.pad2[1] = s.pad2[2] = 0;
        s.mapq = mapq[m]; s.a_score = mm.score; s.post_prob = post[m];
        s.sim_matches = (int32_t)(mm.pos_end - mm.pos_begin); s.cigar_off = (uint32_t)co;
        recs[ro] = s;
    }
}

// -b / -d: the gapped read string of a kept sequence as g_gen_CONVERSION codes (a,c,g,t,n = 0..4; 6 = the NUL the reference reads one
// past the consensus, which AddSeqScore ignores), built from the traceback operations on the argmax consensus of the read in the
// orientation of the match's first strand (ScoredSeq.h:57-103 max_char, bin_seq.cpp:578-698 incl. the consense[i] quirk at :607)
__device__ __forceinline__ uint32_t go_cons_code(const GmDevBatch& b, const float2* lut, uint32_t r, uint32_t L, uint32_t first_strand, uint32_t i) {
    const uint32_t src = first_strand ? L - 1u - i : i;
    const uint8_t ch = b.bases[(size_t)r * b.stride + src];
    float c[4];
    if (b.fasta) {                                      // the letter's row (get_more_fasta): `lut` is the FASTA table, (p, q) by base mask
        uint32_t mask = gm_iupac_mask(ch);
        if (first_strand) mask = gm_mask_rc(mask);
        const float2 pq = lut[mask];
        for (int k = 0; k < 4; ++k) c[k] = ((mask >> k) & 1u) ? pq.x : pq.y;
    } else {
        const float2 pq = lut[b.quals[(size_t)r * b.stride + src]];
        int code;
        switch (ch) { case 'a': case 'A': code = 0; break; case 'c': case 'C': code = 1; break; case 'g': case 'G': code = 2; break;
                      case 't': case 'T': code = 3; break; default: code = 4; }
        if (first_strand && code < 4) code = 3 - code;
        c[0] = c[1] = c[2] = c[3] = pq.y;
        if (code < 4) c[code] = pq.x;
    }
    if (c[0] == c[1] && c[0] == c[2] && c[0] == c[3]) return 4;        // 'n'
    if (c[0] >= c[1]) { if (c[0] >= c[2]) return c[0] >= c[3] ? 0u : 3u; return c[2] >= c[3] ? 2u : 3u; }
    if (c[1] >= c[2]) return c[1] >= c[3] ? 1u : 3u;
    return c[2] >= c[3] ? 2u : 3u;
}

__global__ void __launch_bounds__(256) k_out_codes(GmDevBatch b, GmDevParams p, const GmDevMatch* matches, uint32_t n_m, const unsigned long long* ops,
                                                   uint32_t ops_words, const uint16_t* ops_len, uint8_t* codes, uint32_t codes_stride) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_m) return;
    const GmDevMatch mm = matches[m];
    const uint32_t r = mm.read - b.read_base, L = b.len[r];
    const float2* lut = p.lut + (b.fasta ? GM_LUT_FASTA : (r < b.illumina_until) ? 256u : 0u);
    const unsigned long long* op = ops + (size_t)m * ops_words;
    uint8_t* out = codes + (size_t)m * codes_stride;
    const uint32_t n_op = ops_len[m];
    uint32_t rr = 0;
    for (uint32_t k = 0; k < n_op; ++k) {
        uint8_t cv;
        const uint32_t o = go_op(op, k);
        if (o == 0) { cv = rr < L ? (uint8_t)go_cons_code(b, lut, r, L, mm.first_strand, rr) : 6; ++rr; }
        else if (o == 1) { cv = rr + 1 < L ? (uint8_t)go_cons_code(b, lut, r, L, mm.first_strand, rr + 1) : 6; ++rr; }
        else cv = 5;                                                    // '-'
        out[k] = cv;
    }
}

// coverage deposit of every kept sequence at every one of its places: amount_genome[(pos+t)/bin] += (float)posterior for t < aligned
// length (GenomeBwt::AddScore src/GenomeBwt.cpp:483-490).  One thread per (place, bin): the bases of a place that fall into one bin
// are added up in a register in base order - exactly the fp32 sequence the reference runs through on an untouched bin - and reach
// HBM as ONE atomic per bin instead of one per base (8 x fewer atomics at the default bin size).  -b / -d (bin size 1) additionally
// reads[base][pos+t] += posterior with the gapped read string reverse-complemented for places on the other strand than the first
// (BSScoredSeq.cpp:50-84).
__global__ void __launch_bounds__(256) k_out_deposit(float* cov, uint64_t bins, uint32_t bin_size, const GmDevMatch* matches, const GmDevPos* positions,
                                                     const uint32_t* pos_match, uint64_t n_p, const uint16_t* ops_len, const float* post, uint32_t bins_per_place,
                                                     float* nuc, const uint8_t* codes, uint32_t codes_stride) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t q = gid / bins_per_place; const uint32_t bi = (uint32_t)(gid % bins_per_place);
    if (q >= n_p) return;
    const uint32_t m = pos_match[q];
    if (m == 0xFFFFFFFFu) return;
    const uint32_t span = ops_len[m];
    const GmDevPos p = positions[q];
    const uint64_t bin = p.pos / bin_size + bi;
    if (bin >= bins || span == 0) return;
    // bases t of this place inside the bin: pos + t in [bin * bin_size, (bin + 1) * bin_size)
    const uint64_t lo = bin * bin_size > p.pos ? bin * bin_size - p.pos : 0;
    uint64_t hi = (bin + 1) * bin_size - p.pos;
    if (hi > span) hi = span;
    if (lo >= hi) return;
    const float w = post[m];
    float acc = 0.0f;
    for (uint64_t t = lo; t < hi; ++t) acc += w;
    atomicAdd(&cov[bin], acc);
    if (nuc) {
        const uint8_t* cd = codes + (size_t)m * codes_stride;
        const bool same = p.strand == matches[m].first_strand;
        for (uint32_t t = (uint32_t)lo; t < (uint32_t)hi; ++t) {
            // codes: 0..3 acgt, 4 'n', 5 '-', 6 the NUL read past the consensus.  Same strand: '-' falls into the N slot (g_gen_CONVERSION
            // default), NUL is ignored.  Other strand: reverse_comp first (SequenceOperations.h:56-96: acgt swapped, everything else 'n')
            uint32_t c;
            if (same) { c = cd[t]; if (c == 5u) c = 4u; }
            else { c = cd[span - 1u - t]; c = c < 4u ? 3u - c : 4u; }
            if (c < 5u) atomicAdd(&nuc[(size_t)c * bins + (p.pos + t) / bin_size], w);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// SAM rows as text (src/Driver.cpp:2146-2217, ScoredSeq::get_SAM inc/ScoredSeq.h:293-404): what the host driver's format_sam writes,
// byte for byte.  Row = name \t flag \t contig \t chr_pos \t mapq \t cigar \t*\t0\t0\t seq \t qual \t XA:f:%g \t XP:f:%g \t X0:i:%d \n
// ------------------------------------------------------------------------------------------------
#define GO_TAIL_MAX 56u
#define GO_NAME_MAX 1023u                                  // MAX_NAME_SZ - 1, inc/const_include.h:46
#define GO_UNMAPPED_HEAD 17u                               // "\t4\t*\t0\t0\t*\t*\t0\t0\t": what a row without a record prints between its name and SEQ

__device__ __forceinline__ uint32_t go_digits64(unsigned long long v) { uint32_t d = 1; while (v >= 10ull) { v /= 10ull; ++d; } return d; }
__device__ __forceinline__ uint32_t go_int_chars(int32_t v) { return v < 0 ? 1u + go_digits64((unsigned long long)(-(long long)v)) : go_digits64((unsigned long long)v); }
__device__ __forceinline__ char* go_put_u64(char* w, unsigned long long v) {
    const uint32_t d = go_digits64(v);
    for (uint32_t q = d; q > 0; --q) { w[q - 1] = (char)('0' + (uint32_t)(v % 10ull)); v /= 10ull; }
    return w + d;
}
__device__ __forceinline__ char* go_put_int(char* w, int32_t v) {
    if (v < 0) { *w++ = '-'; return go_put_u64(w, (unsigned long long)(-(long long)v)); }
    return go_put_u64(w, (unsigned long long)v);
}
__device__ __forceinline__ bool go_cigar_digit(char c) { return c >= 48 && c <= 58; }      // ':' counts as a digit, SequenceOperations.h:109-123

// one lane per record: the numeric tail into the record's slot (through LDS, so that the slots leave as whole 16-byte stores) and
// the length of the row
__global__ void __launch_bounds__(256) k_out_text_sizes(GmDevBatch b, GmDevText t) {
    __shared__ __attribute__((aligned(16))) char s_slot[256][64];
    const unsigned long long k0 = (unsigned long long)blockIdx.x * 256ull, k = k0 + threadIdx.x;
    unsigned long long rec = 0; uint32_t urd = 0;
    const bool is_rec = k < t.n_rows && gm_row_is_record(t, k, rec, urd);
    if (k < t.n_rows && !is_rec) {
        // a read without a record: "YU:i:<status>\n" as the slot's tail, no CIGAR; name, the nine constant columns, SEQ and QUAL as a
        // plus-strand row prints them ("*" and "*" for a read of length 0)
        char* const s = s_slot[threadIdx.x];
        uint32_t len = 0, tail = 0;
        if (urd != 0xFFFFFFFFu) {
            char* w = s;
            w[0] = 'Y'; w[1] = 'U'; w[2] = ':'; w[3] = 'i'; w[4] = ':'; w += 5;
            w = go_put_int(w, (int32_t)t.status[urd]);
            *w++ = '\n';
            tail = (uint32_t)(w - s);                         // <= 5 + 4 + 1
            unsigned long long nl = t.name_off[urd + 1] - t.name_off[urd];
            if (nl > GO_NAME_MAX) nl = GO_NAME_MAX;
            const uint32_t L = t.seq_len[urd];
            const uint32_t QL = L + (t.qtail_off ? (uint32_t)(t.qtail_off[urd + 1] - t.qtail_off[urd]) : 0u);
            len = (uint32_t)nl + GO_UNMAPPED_HEAD + (L ? L + 1u + QL : 3u) + 1u + tail;
        } else atomicMin(t.bad, k);
        s[56] = s[57] = s[58] = s[59] = 0; s[60] = (char)tail;
        t.row_len[k] = len;
    }
    if (is_rec) {
        const GmDevSamRec r = t.recs[rec];
        char* const s = s_slot[threadIdx.x];
        char* w = s;
        bool ok = true;
        w[0] = 'X'; w[1] = 'A'; w[2] = ':'; w[3] = 'f'; w[4] = ':'; w += 5;
        {   // (double)(float)a_score * (1.0 / gADJUST), as format_sam computes it
            char* e = gm_put_g6_hd(w, (double)r.a_score * t.inv_adjust);
            ok &= e != w; w = e;
        }
        w[0] = '\t'; w[1] = 'X'; w[2] = 'P'; w[3] = ':'; w[4] = 'f'; w[5] = ':'; w += 6;
        if (r.post_prob == 1.0f) *w++ = '1';
        else { char* e = gm_put_g6_hd(w, (double)r.post_prob); ok &= e != w; w = e; }
        w[0] = '\t'; w[1] = 'X'; w[2] = '0'; w[3] = ':'; w[4] = 'i'; w[5] = ':'; w += 6;
        w = go_put_int(w, r.sim_matches);
        *w++ = '\n';
        const uint32_t tail = (uint32_t)(w - s);            // <= 5 + 13 + 6 + 13 + 6 + 11 + 1 = 55
        if (!ok) atomicMin(t.bad, k);
        // CIGAR: length in the pool, length in the row
        const char* cg = t.pool + r.cigar_off;
        uint32_t gl = 0, last_op = 0;
        for (char c; gl < 0xFFFFu && (c = cg[gl]) != 0; ++gl) if (!go_cigar_digit(c)) last_op = gl + 1;
        const uint32_t gout = r.strand && !t.cigar_forward ? last_op : gl;      // GM_CIGAR_FORWARD: all gl bytes, as a plus-strand row prints them
        s[56] = (char)(gl & 255u); s[57] = (char)(gl >> 8); s[58] = (char)(gout & 255u); s[59] = (char)(gout >> 8); s[60] = (char)tail;
        const uint32_t rd = r.read;
        unsigned long long nl = t.name_off[rd + 1] - t.name_off[rd];
        if (nl > GO_NAME_MAX) nl = GO_NAME_MAX;
        const uint32_t cl = t.cname_off[r.contig + 1] - t.cname_off[r.contig];
        const uint32_t L = t.seq_len[rd];
        const uint32_t QL = L + (t.qtail_off ? (uint32_t)(t.qtail_off[rd + 1] - t.qtail_off[rd]) : 0u);
        t.row_len[k] = (uint32_t)nl + (r.strand ? 4u : 3u) + cl + 1u + go_digits64(r.chr_pos) + 1u + go_int_chars(r.mapq) + 1u + gout + 7u + L + 1u + QL + 1u + tail;
    }
    __syncthreads();
    // the block's slots are one contiguous stretch of HBM: 16 bytes per lane and step
    const unsigned long long left = t.n_rows - k0;
    const uint32_t chunks = (uint32_t)(left < 256ull ? left : 256ull) * 4u;
    const uint4* src = reinterpret_cast<const uint4*>(&s_slot[0][0]);
    uint4* dst = reinterpret_cast<uint4*>(t.slots + k0 * 64ull);
    for (uint32_t q = threadIdx.x; q < chunks; q += 256u) dst[q] = src[q];
}

// one wavefront per row, four rows per workgroup and step; the grid is one resident round.  TAGS: gm_batch_set_row_tags is on (t.md
// is there) - an instance of its own, so that the walk's registers cost the rows without tags no occupancy.  MATES: gm_batch_set_mates
// is on (t.mate is there) - instances of their own as well, with a head of their own: a flag of up to four digits does not fit
// hd[0, 4), nor a contig name in RNEXT the seven constant bytes.  Its layout: [0, 16) "\t<flag>\t" (a read without a record:
// "\t<flag>\t*\t0\t0\t*"), [16, 50) "\t<chr_pos>\t<mapq>\t", [50, 52) "\t" and "=" / "*" unless RNEXT is a contig's name, [56, 80)
// "\t<PNEXT>\t<TLEN>\t"; the four lengths in [124, 128)
template <bool TAGS, bool MATES>
__global__ void __launch_bounds__(256) k_out_text_rows(GmDevBatch b, GmDevText t) {
    constexpr uint32_t HD = MATES ? 128u : 64u, H2_AT = MATES ? 16u : 4u, LEN1_AT = MATES ? 124u : 62u, LEN2_AT = MATES ? 125u : 63u;
    __shared__ char s_head[4][HD];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    char* const hd = s_head[wv];
    for (unsigned long long base = (unsigned long long)blockIdx.x * 4ull; base < t.n_rows; base += (unsigned long long)gridDim.x * 4ull) {
        const unsigned long long k = base + wv;
        unsigned long long rec = 0; uint32_t urd = 0;
        const bool is_rec = k < t.n_rows && gm_row_is_record(t, k, rec, urd);
        const bool unm = k < t.n_rows && !is_rec && urd != 0xFFFFFFFFu;        // a read without a record: its flag-4 row
        const bool live = is_rec || unm;
        GmDevSamRec r = {};
        GmDevMateRow mf = {};
        if constexpr (MATES) if (live) mf = t.mate[k];
        if (unm) {
            r.read = urd;
            if (lane == 0) {
                if constexpr (MATES) {                        // "\t<flag>\t*\t0\t0\t*": the mate columns follow as on every row
                    char* w = hd;
                    *w++ = '\t'; w = go_put_u64(w, mf.flag); *w++ = '\t'; *w++ = '*'; *w++ = '\t'; *w++ = '0'; *w++ = '\t'; *w++ = '0'; *w++ = '\t'; *w++ = '*';
                    hd[LEN1_AT] = (char)(w - hd); hd[LEN2_AT] = 0;
                } else {                                      // [0, 17) the nine constant columns
                    const char c[GO_UNMAPPED_HEAD + 1] = "\t4\t*\t0\t0\t*\t*\t0\t0\t";
                    for (uint32_t i = 0; i < GO_UNMAPPED_HEAD; ++i) hd[i] = c[i];
                    hd[LEN1_AT] = (char)GO_UNMAPPED_HEAD; hd[LEN2_AT] = 0;
                }
            }
        }
        if (is_rec) {
            r = t.recs[rec];
            if (lane == 0) {                                  // the short head: [0, 4) "\t<flag>\t", [4, ..) "\t<chr_pos>\t<mapq>\t", [48, 55) the constant columns
                char* w = hd;
                *w++ = '\t';
                if constexpr (MATES) w = go_put_u64(w, mf.flag);
                else { if (r.strand) { *w++ = '1'; *w++ = '6'; } else *w++ = '0'; }
                *w++ = '\t';
                hd[LEN1_AT] = (char)(w - hd);
                w = hd + H2_AT;
                *w++ = '\t'; w = go_put_u64(w, r.chr_pos); *w++ = '\t'; w = go_put_int(w, r.mapq); *w++ = '\t';      // <= 1 + 20 + 1 + 11 + 1 = 34
                hd[LEN2_AT] = (char)(w - (hd + H2_AT));
                if constexpr (!MATES) { hd[48] = '\t'; hd[49] = '*'; hd[50] = '\t'; hd[51] = '0'; hd[52] = '\t'; hd[53] = '0'; hd[54] = '\t'; }
            }
        }
        // RNEXT is "=" on the row's own contig, "*" without a mate primary, else that contig's name (from the name pool, like RNAME)
        const bool rn_named = MATES && live && mf.rnext >= 0 && !(is_rec && (uint32_t)mf.rnext == r.contig);
        if constexpr (MATES) if (live && lane == 0) {
            hd[50] = '\t'; hd[51] = mf.rnext < 0 ? '*' : '=';
            hd[126] = rn_named ? 1 : 2;
            char* w = hd + 56;
            *w++ = '\t'; w = go_put_u64(w, mf.pnext); *w++ = '\t'; w = go_put_int(w, mf.tlen); *w++ = '\t';              // <= 1 + 10 + 1 + 11 + 1 = 24
            hd[127] = (char)(w - (hd + 56));
        }
        __syncthreads();
        if (live) {
            const unsigned long long end = t.row_off[k + 1];
            unsigned long long o = t.row_off[k];
            char* const out = t.text;
            const uint8_t* slot = t.slots + k * 64ull;
            const uint32_t gl = (uint32_t)slot[56] | ((uint32_t)slot[57] << 8), gout = (uint32_t)slot[58] | ((uint32_t)slot[59] << 8), tail = slot[60];
            const uint32_t rd = r.read, L = t.seq_len[rd];
            const unsigned long long n0 = t.name_off[rd];
            unsigned long long nl64 = t.name_off[rd + 1] - n0;
            const uint32_t nl = nl64 > GO_NAME_MAX ? GO_NAME_MAX : (uint32_t)nl64;
            const uint32_t c0 = unm ? 0u : t.cname_off[r.contig], cl = unm ? 0u : t.cname_off[r.contig + 1] - c0;
            const unsigned long long q0 = t.qtail_off ? t.qtail_off[rd] : 0ull;
            const uint32_t TL = t.qtail_off ? (uint32_t)(t.qtail_off[rd + 1] - q0) : 0u, QL = L + TL;
            const uint32_t h1 = (uint8_t)hd[LEN1_AT], h2 = (uint8_t)hd[LEN2_AT];
            const bool neg = r.strand != 0;
            const bool star = unm && L == 0u;                    // a read of length 0 without a record: SEQ and QUAL are "*"
            // every store stays inside the row the scan gave this record, whatever the lengths say
            for (uint32_t i = lane; i < nl; i += 64u) if (o + i < end) out[o + i] = t.names[n0 + i];
            o += nl;
            for (uint32_t i = lane; i < h1; i += 64u) if (o + i < end) out[o + i] = hd[i];
            o += h1;
            for (uint32_t i = lane; i < cl; i += 64u) if (o + i < end) out[o + i] = t.cnames[c0 + i];
            o += cl;
            for (uint32_t i = lane; i < h2; i += 64u) if (o + i < end) out[o + i] = hd[H2_AT + i];
            o += h2;
            const char* cg = t.pool + r.cigar_off;
            const bool rev = neg && !t.cigar_forward;            // (GM_CIGAR_FORWARD: gout == gl, the bytes in pool order on either strand)
            if (!rev) { for (uint32_t i = lane; i < gl; i += 64u) if (o + i < end) out[o + i] = cg[i]; }
            else {
                // reverse_cigar: the tokens (digits + operation) in reverse order; byte i of token [ts, te] goes behind the tokens that
                // follow it: (gout - (te + 1)) + (i - ts).  Digits after the last operation belong to no token and are dropped.
                for (uint32_t i = lane; i < gout; i += 64u) {
                    uint32_t te = i; while (te + 1u < gout && go_cigar_digit(cg[te])) ++te;
                    uint32_t ts = i; while (ts > 0 && go_cigar_digit(cg[ts - 1u])) --ts;
                    const uint32_t d = (gout - (te + 1u)) + (i - ts);
                    if (o + d < end) out[o + d] = cg[i];
                }
            }
            o += gout;
            if constexpr (MATES) {
                const uint32_t ha = (uint8_t)hd[126], hb = (uint8_t)hd[127];
                if (lane < ha && o + lane < end) out[o + lane] = hd[50 + lane];
                o += ha;
                if (rn_named) {
                    const uint32_t m0 = t.cname_off[mf.rnext], ml = t.cname_off[mf.rnext + 1] - m0;
                    for (uint32_t i = lane; i < ml; i += 64u) if (o + i < end) out[o + i] = t.cnames[m0 + i];
                    o += ml;
                }
                if (lane < hb && o + lane < end) out[o + lane] = hd[56 + lane];
                o += hb;
            } else if (!unm) {
                for (uint32_t i = lane; i < 7u; i += 64u) if (o + i < end) out[o + i] = hd[48 + i];
                o += 7u;
            }
            const uint8_t* bs = b.bases + (size_t)rd * b.stride; const uint8_t* qs = b.quals + (size_t)rd * b.stride;
            if (!neg) { for (uint32_t i = lane; i < L; i += 64u) if (o + i < end) out[o + i] = (char)bs[i]; }
            else { for (uint32_t i = lane; i < L; i += 64u) if (o + i < end) out[o + i] = gm_comp_char((char)bs[L - 1u - i]); }
            o += L;
            if (star) { if (lane == 0 && o < end) out[o] = '*'; o += 1u; }
            if (lane == 0 && o < end) out[o] = '\t';
            o += 1u;
            if (star) { if (lane == 0 && o < end) out[o] = '*'; o += 1u; }
            else for (uint32_t i = lane; i < QL; i += 64u) {
                const uint32_t si = neg ? QL - 1u - i : i;          // the whole quality line is reversed, its tail included
                // FASTA block: str2qual's character (SequenceOperations.h:193-217) of the letter's row, by the number of bases in its mask
                const char c = b.fasta ? (char)(t.fa_qual >> (8u * (((uint32_t)__popc(gm_iupac_mask(bs[si < L ? si : 0u])) - 1u) & 3u)))
                               : si < L ? (char)qs[si] : t.qtail[q0 + (si - L)];
                if (o + i < end) out[o + i] = c;
            }
            if (!star) o += QL;
            if (lane == 0 && o < end) out[o] = '\t';
            o += 1u;
            const uint32_t md_len = TAGS && is_rec ? t.md[2ull * k + 1ull] : 0u;
            if (!TAGS || !md_len) { for (uint32_t i = lane; i < tail; i += 64u) if (o + i < end) out[o + i] = (char)slot[i]; }
            else if constexpr (TAGS) {
                // gm_batch_set_row_tags: the tail without its newline, "\tNM:i:<nm>\tMD:Z:", the string of the walk, the newline
                const uint32_t body = tail ? tail - 1u : 0u, nm = t.md[2ull * k], dn = md_digits(nm);
                for (uint32_t i = lane; i < body; i += 64u) if (o + i < end) out[o + i] = (char)slot[i];
                o += body;
                if (lane < 12u) {
                    const char c[13] = "\tNM:i:\tMD:Z:";
                    const unsigned long long at = o + lane + (lane < 6u ? 0u : dn);
                    if (at < end) out[at] = c[lane];
                }
                if (lane == 12u) md_put(reinterpret_cast<uint8_t*>(out), o + 6u, end, nm, dn);
                o += 12u + dn;
                uint32_t nm_w, len_w;
                gm_md_walk<true>(t, r, bs, L, cg, gout, rev, lane, reinterpret_cast<uint8_t*>(out), o, end, &nm_w, &len_w);
                o += md_len;
                if (lane == 0 && o < end) out[o] = '\n';
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// gm_batch_set_row_tags: NM:i and MD:Z of the row as printed (the walk: gm_mdtag_dev.h).  The sizes pass, behind k_out_text_sizes /
// k_bam_sizes and in front of the scan of row_len: one wavefront per row, four rows per workgroup and step.  {NM, MD bytes} into t.md
// (0 bytes: the row gets no tags - it prints no record, or a CIGAR of "*"), and the bytes of the two tags added to row_len:
// "\tNM:i:<nm>\tMD:Z:<md>" in SAM text, NM i int32 + MD Z <md> NUL in BAM.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_md_sizes(GmDevBatch b, GmDevText t, int bam) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 4ull; base < t.n_rows; base += (unsigned long long)gridDim.x * 4ull) {
        const unsigned long long k = base + wv;
        if (k >= t.n_rows) continue;                          // (the whole wavefront: k is the same in its 64 lanes, and there is no barrier)
        unsigned long long rec = 0; uint32_t urd = 0;
        uint32_t nm = 0, md_len = 0;
        if (gm_row_is_record(t, k, rec, urd)) {
            const GmDevSamRec r = t.recs[rec];
            const uint8_t* slot = t.slots + k * 64ull;
            const uint32_t gout = (uint32_t)slot[58] | ((uint32_t)slot[59] << 8);
            const char* cg = t.pool + r.cigar_off;
            if (md_row_has_tags(cg, gout)) {
                const uint32_t rd = r.read;                   // (as the row kernels index the block)
                gm_md_walk<false>(t, r, b.bases + (size_t)rd * b.stride, t.seq_len[rd], cg, gout, r.strand != 0 && !t.cigar_forward, lane, nullptr, 0ull, 0ull, &nm, &md_len);
            }
        }
        if (lane == 0) {
            t.md[2ull * k] = nm; t.md[2ull * k + 1ull] = md_len;
            if (md_len) t.row_len[k] += bam ? md_len + 11u : 12u + md_digits(nm) + md_len;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The row source of gm_batch_set_unmapped_rows: which record, or which read without one, every row prints.  The records lie in read
// order (k_out_write: match order, and the matches are a CSR over the reads), so a record's row is its index plus the reads without a
// record in front of its read, and such a read's row is the records plus the reads without one in front of it.  Integer counts and
// two scans: nothing depends on the order the counts arrive in.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_row_count(const GmDevSamRec* __restrict__ recs, unsigned long long n_recs, uint32_t n, uint32_t* __restrict__ cnt) {
    const unsigned long long k = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (k >= n_recs) return;
    const uint32_t rd = recs[k].read;
    if (rd < n) atomicAdd(&cnt[rd], 1u);
}

__global__ void __launch_bounds__(256) k_row_flags(const uint32_t* __restrict__ cnt, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < n) flag[r] = cnt[r] == 0u ? 1u : 0u;
}

// items [0, n_recs): the records; [n_recs, n_recs + n): the reads.  Every row index is checked against the number of rows
__global__ void __launch_bounds__(256) k_row_fill(const GmDevSamRec* __restrict__ recs, unsigned long long n_recs, uint32_t n, const uint32_t* __restrict__ cnt,
                                                  const uint64_t* __restrict__ first, const uint64_t* __restrict__ ucum, unsigned long long* __restrict__ row_src) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const unsigned long long n_rows = n_recs + ucum[n];
    if (i < n_recs) {
        const uint32_t rd = recs[i].read;
        const unsigned long long row = i + ucum[rd < n ? rd : n];
        if (row < n_rows) row_src[row] = i;
    } else if (i - n_recs < n) {
        const uint32_t r = (uint32_t)(i - n_recs);
        const unsigned long long row = first[r] + ucum[r];
        if (cnt[r] == 0u && row < n_rows) row_src[row] = GM_ROW_UNMAPPED | r;
    }
}

__global__ void __launch_bounds__(256) k_fmt_g6(const double* v, uint32_t n, char* out, uint8_t* len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    char* w = out + (size_t)i * 16;
    len[i] = (uint8_t)(gm_put_g6_hd(w, v[i]) - w);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

int gmk_group_count(const GmDevIndex& ix, const GmDevBatch& b, const GmDevGroup& g, int nw, int unique_only, uint32_t max_matches, void* stream) {
    if (b.n == 0) return 0;
    const uint32_t big_min = (uint32_t)gm_opt_ll("GM_GROUP_BIG_MIN", GM_GROUP_BIG);     // test switch
    hipLaunchKernelGGL(k_group_single, dim3(cdiv(b.n, 256)), dim3(256), 0, S_(stream), b, g, nw, max_matches, big_min);
    {   // reads with many accepted hits first: what this kernel cannot finish goes to the all-pairs kernel's list
        const size_t lds = (size_t)GO_SET_SLOTS * 16 + (size_t)GO_SET_LIMIT * 4 + 64;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_group_big), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        hipLaunchKernelGGL(k_group_big, dim3(gm_test_grid(std::min<uint32_t>(b.n, 4096u))), dim3(64), lds, S_(stream), ix, b, g, nw, unique_only, max_matches);
    }
    hipLaunchKernelGGL(k_group_multi, dim3(gm_test_grid(std::min<uint32_t>(b.n, 16384u))), dim3(64), 0, S_(stream), ix, b, g, nw, unique_only, max_matches);
    return (int)hipGetLastError();
}

int gmk_group_write(const GmDevBatch& b, const GmDevGroup& g, void* stream) {
    if (b.n == 0) return 0;
    hipLaunchKernelGGL(k_group_write_single, dim3(cdiv(b.n, 256)), dim3(256), 0, S_(stream), b, g);
    hipLaunchKernelGGL(k_group_write_multi, dim3(gm_test_grid(std::min<uint32_t>(b.n, 16384u))), dim3(64), 0, S_(stream), b, g);
    hipLaunchKernelGGL(k_group_write_big, dim3(gm_test_grid(std::min<uint32_t>(b.n, 4096u))), dim3(64), 0, S_(stream), b, g);
    return (int)hipGetLastError();
}

int gmk_out_items(const GmDevMatch* matches, uint32_t n_m, uint32_t read_base, GmCand* items, uint32_t* pos_match, void* stream) {
    if (n_m == 0) return 0;
    hipLaunchKernelGGL(k_out_items, dim3(cdiv(n_m, 256)), dim3(256), 0, S_(stream), matches, n_m, read_base, items, pos_match);
    return (int)hipGetLastError();
}

int gmk_out_sizes(const GmDevMatch* matches, uint32_t n_m, const uint8_t* emit, const uint32_t* cig_all, uint32_t* rec_cnt, uint32_t* cig_cnt, void* stream) {
    if (n_m == 0) return 0;
    hipLaunchKernelGGL(k_out_sizes, dim3(cdiv(n_m, 256)), dim3(256), 0, S_(stream), matches, n_m, emit, cig_all, rec_cnt, cig_cnt);
    return (int)hipGetLastError();
}

int gmk_out_write(const GmDevIndex& ix, const GmDevBatch& b, const GmDevMatch* matches, const GmDevPos* positions, uint32_t n_m, const uint8_t* emit,
                  const int32_t* mapq, const float* post, const unsigned long long* ops, uint32_t ops_words, const uint16_t* ops_len, int nw,
                  const uint64_t* rec_off, const uint64_t* cig_off, GmDevSamRec* recs, char* pool, void* stream) {
    if (n_m == 0) return 0;
    hipLaunchKernelGGL(k_out_write, dim3(cdiv(n_m, 256)), dim3(256), 0, S_(stream), ix, b, matches, positions, n_m, emit, mapq, post, ops, ops_words, ops_len,
                       nw, rec_off, cig_off, recs, pool);
    return (int)hipGetLastError();
}

int gmk_out_codes(const GmDevBatch& b, const GmDevParams& p, const GmDevMatch* matches, uint32_t n_m, const unsigned long long* ops, uint32_t ops_words,
                  const uint16_t* ops_len, uint8_t* codes, uint32_t codes_stride, void* stream) {
    if (n_m == 0) return 0;
    hipLaunchKernelGGL(k_out_codes, dim3(cdiv(n_m, 256)), dim3(256), 0, S_(stream), b, p, matches, n_m, ops, ops_words, ops_len, codes, codes_stride);
    return (int)hipGetLastError();
}

int gmk_out_deposit(float* cov, uint64_t bins, uint32_t bin_size, const GmDevMatch* matches, const GmDevPos* positions, const uint32_t* pos_match,
                    uint64_t n_p, const uint16_t* ops_len, const float* post, uint32_t max_span, float* nuc, const uint8_t* codes, uint32_t codes_stride,
                    void* stream) {
    if (n_p == 0 || max_span == 0) return 0;
    const uint32_t bins_per_place = (max_span + bin_size - 1) / bin_size + 1;          // a place may start in the middle of a bin
    const uint64_t total = n_p * bins_per_place;
    hipLaunchKernelGGL(k_out_deposit, dim3(cdiv(total, 256)), dim3(256), 0, S_(stream), cov, bins, bin_size, matches, positions, pos_match, n_p, ops_len,
                       post, bins_per_place, nuc, codes, codes_stride);
    return (int)hipGetLastError();
}

int gmk_out_text_sizes(const GmDevBatch& b, const GmDevText& t, void* stream) {
    if (t.n_rows == 0) return 0;
    hipLaunchKernelGGL(k_out_text_sizes, dim3(cdiv(t.n_rows, 256)), dim3(256), 0, S_(stream), b, t);
    return (int)hipGetLastError();
}

int gmk_out_text_rows(const GmDevBatch& b, const GmDevText& t, void* stream) {
    if (t.n_rows == 0) return 0;
    // one resident round: as many workgroups of 4 waves as the device holds at once
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    void (*const kern)(GmDevBatch, GmDevText) = t.mate ? (t.md ? k_out_text_rows<true, true> : k_out_text_rows<false, true>)
                                                       : (t.md ? k_out_text_rows<true, false> : k_out_text_rows<false, false>);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, 0) != hipSuccess || per_cu <= 0) per_cu = 4;
    const uint32_t grid = gm_test_grid((uint32_t)std::min<uint64_t>((t.n_rows + 3) / 4, (uint64_t)cus * (uint64_t)per_cu));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, S_(stream), b, t);
    return (int)hipGetLastError();
}

int gmk_md_sizes(const GmDevBatch& b, const GmDevText& t, int bam, void* stream) {
    if (t.n_rows == 0) return 0;
    const uint32_t grid = gm_test_grid((uint32_t)std::min<uint64_t>((t.n_rows + 3) / 4, 4096));
    hipLaunchKernelGGL(k_md_sizes, dim3(grid), dim3(256), 0, S_(stream), b, t, bam);
    return (int)hipGetLastError();
}

int gmk_row_source(const GmDevSamRec* recs, uint64_t n_recs, uint32_t n, uint32_t* cnt, uint32_t* flag, uint64_t* first, uint64_t* ucum, unsigned long long* tmp,
                   unsigned long long* row_src, void* stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)n * 4, S_(stream));
    if (e == hipSuccess) e = hipMemsetAsync(row_src, 0xFF, (size_t)(n_recs + n) * 8, S_(stream));       // (an entry nothing fills names no row)
    if (e != hipSuccess) return (int)e;
    if (n_recs) hipLaunchKernelGGL(k_row_count, dim3(cdiv(n_recs, 256)), dim3(256), 0, S_(stream), recs, (unsigned long long)n_recs, n, cnt);
    hipLaunchKernelGGL(k_row_flags, dim3(cdiv(n, 256)), dim3(256), 0, S_(stream), cnt, n, flag);
    if (const int rc = gmk_scan_u32(cnt, n, first, tmp, stream)) return rc;
    if (const int rc = gmk_scan_u32(flag, n, ucum, tmp, stream)) return rc;
    hipLaunchKernelGGL(k_row_fill, dim3(cdiv(n_recs + n, 256)), dim3(256), 0, S_(stream), recs, (unsigned long long)n_recs, n, cnt, first, ucum, row_src);
    return (int)hipGetLastError();
}

int gmk_fmt_g6(const double* v, uint32_t n, char* out, uint8_t* len, void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_fmt_g6, dim3(cdiv(n, 256)), dim3(256), 0, S_(stream), v, n, out, len);
    return (int)hipGetLastError();
}
