// gm_readtext.hip — a chunk of FASTQ text cut into read rows where the kernels read them (gm_batch_upload_text).  The contract is the
// chunk mode of the driver's host parser (FastqScanner::parse_range, gnumap_main.cpp), byte for byte:
//
//   lines    a line starts at 0 and behind every '\n' that is not the text's last byte; it runs to the next '\n' or to the end.  No other
//            byte is special ('\r' and NUL are data)
//   records  in order; blank lines are skipped BEFORE a name line and nowhere else; the three lines behind a name are sequence, plus and
//            quality whatever they hold
//   good     four lines, '@' first in the name, a non-empty plus line with '+' first, sequence no longer than quality
//   the first record that is not good (RT_BAD_FORM), or is good but longer than 2048 (RT_BAD_LONG), ends the block: n = its index
//
// The phase 0 .. 3 of a line depends on the lines before it only because blank lines are skipped in phase 0: a line is a map on the four
// phases (blank: 0 -> 0, p -> p + 1 otherwise; anything else: p -> p + 1, modulo 4), eight bits, and maps compose associatively, so the
// phases are a scan.
//
// Passes, ordered by kernel boundaries (nothing waits for another workgroup; the tile sums are scanned by ONE workgroup in between, as in
// gm_tracktext.hip):
//   k_rt_count        newlines per tile of RT_TILE bytes, 16 bytes per lane
//   k_rt_scan         exclusive scan of the tile counts; the number of lines
//   k_rt_lines        the offsets of the line starts
//   k_rt_phase_tiles  per tile of RT_WG lines: the composed map, and the records it starts for each of the four phases it may be entered in
//   k_rt_phase_scan   scan of the maps -> the phase every tile is entered in; scan of the record counts that follow from it
//   k_rt_records      phase and record index of every line; the lane of a name line checks its record, writes its gm_text_rec and
//                     atomicMin()s the first record that ends the block
//   k_rt_finish       over the n records in front of that one: lengths, longest / shortest, name and tail bytes
//   -- one read-back: n, the longest read, the first bad record with its kind and offset, the lengths --
//   k_rt_rows         bases and qualities as zero-padded rows of `stride` bytes: whole 8- or 16-byte stores, the text side read as aligned
//                     8-byte words and shifted into place
//   k_rt_names        names (cut to 1023 bytes) and quality tails into the pools k_out_text_sizes / k_out_text_rows read
//   k_rt_illumina     --illumina's fallback index: the smallest read with a quality character below 64 (a signed char) in its kept length
#include <hip/hip_runtime.h>
#include "gm_internal.h"

static inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

#define RT_WG 256u
#define RT_TILE (RT_WG * 16u)

// phase maps: phase s -> bits [2s, 2s + 2)
#define RT_MAP_ID 0xE4u
#define RT_MAP_NEXT 0x39u           // 0 -> 1, 1 -> 2, 2 -> 3, 3 -> 0
#define RT_MAP_BLANK 0x38u          // 0 -> 0, 1 -> 2, 2 -> 3, 3 -> 0
__device__ __forceinline__ uint32_t rt_apply(uint32_t m, uint32_t s) { return (m >> (2u * s)) & 3u; }
// a, then b
__device__ __forceinline__ uint32_t rt_compose(uint32_t a, uint32_t b) {
    return rt_apply(b, a & 3u) | (rt_apply(b, (a >> 2) & 3u) << 2) | (rt_apply(b, (a >> 4) & 3u) << 4) | (rt_apply(b, (a >> 6) & 3u) << 6);
}

// sum over the workgroup (every lane gets it) and the exclusive prefix of the lane
__device__ __forceinline__ uint32_t rt_block_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < RT_WG / 64u; ++w) { const uint32_t x = s_wave[w]; if (w < wave) before += x; all += x; }
    total = all;
    return before + inc - v;
}

// bit j: text[at + j] is a newline that a line starts behind (at + j + 1 < bytes); `at` a multiple of 16.  One 16-byte load: the buffer
// is 16-byte aligned and padded, what lies beyond `bytes` is masked here
__device__ __forceinline__ uint32_t rt_nl_mask(const uint8_t* text, uint64_t bytes, uint64_t at) {
    if (at >= bytes) return 0u;
    const uint4 v = *reinterpret_cast<const uint4*>(text + at);
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = w[q] ^ 0x0A0A0A0Au;
        const uint32_t y = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      // 0x80 in every byte of x that is zero, exactly
        m |= ((((y >> 7) * 0x01020408u) >> 24) & 15u) << (4 * q);                       // bits 0, 8, 16, 24 -> 0 .. 3
    }
    const uint64_t left = bytes - at;                                                   // >= 1
    if (left <= 16u) m &= (1u << (uint32_t)(left - 1u)) - 1u;
    return m;
}

__global__ void __launch_bounds__(RT_WG) k_rt_count(GmDevReadText t) {
    __shared__ uint32_t s_wave[RT_WG / 64u];
    const uint64_t at = (uint64_t)blockIdx.x * RT_TILE + threadIdx.x * 16u;
    uint32_t total;
    (void)rt_block_scan(__popc(rt_nl_mask(t.text, t.bytes, at)), s_wave, total);
    if (threadIdx.x == 0) t.tile_cnt[blockIdx.x] = total;
}

// exclusive scan of the tile sums by one workgroup; off[nt] = the sum, meta[slot] = the sum + plus
__global__ void __launch_bounds__(1024) k_rt_scan(const uint32_t* cnt, uint32_t nt, uint32_t* off, unsigned long long* meta, uint32_t slot, uint32_t plus) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, per = (nt + 1023u) / 1024u;
    const uint32_t a = (uint64_t)t * per < nt ? t * per : nt, b = (uint64_t)a + per < nt ? a + per : nt;
    uint32_t s = 0;
    for (uint32_t j = a; j < b; ++j) s += cnt[j];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint32_t j = a; j < b; ++j) { off[j] = run; run += cnt[j]; }
    if (t == 1023u) { off[nt] = part[1023]; meta[slot] = (unsigned long long)part[1023] + plus; }
}

// line k starts at line_at[k]; line 0 at 0.  The last line's end is not a line start: it goes to meta[RT_META_END]
__global__ void __launch_bounds__(RT_WG) k_rt_lines(GmDevReadText t) {
    __shared__ uint32_t s_wave[RT_WG / 64u];
    const uint64_t at = (uint64_t)blockIdx.x * RT_TILE + threadIdx.x * 16u;
    uint32_t m = rt_nl_mask(t.text, t.bytes, at), total;
    uint32_t k = 1u + t.tile_off[blockIdx.x] + rt_block_scan(__popc(m), s_wave, total);
    while (m) {
        const uint32_t j = (uint32_t)__ffs(m) - 1u;
        m &= m - 1u;
        if (k < t.n_lines) t.line_at[k] = (uint32_t)(at + j + 1u);
        ++k;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) t.line_at[0] = 0u;
    if (at < t.bytes && t.bytes - at <= 16u)                                             // the lane that holds the text's last byte
        t.meta[RT_META_END] = t.text[t.bytes - 1u] == '\n' ? t.bytes - 1u : t.bytes;
}

// line k without its newline
__device__ __forceinline__ uint32_t rt_line_len(const GmDevReadText& t, uint32_t k) {
    const uint64_t end = k + 1u < t.n_lines ? (uint64_t)t.line_at[k + 1u] - 1u : (uint64_t)t.meta[RT_META_END];
    return (uint32_t)(end - t.line_at[k]);
}

// the map of the lines in front of the lane's line within its tile (exclusive), and the tile's whole map
__device__ __forceinline__ uint32_t rt_map_scan(uint32_t f, uint32_t* s_wave, uint32_t& all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = f;
    for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc = rt_compose(o, inc); }
    if (lane == 63u) s_wave[wave] = inc;
    uint32_t exc = __shfl_up(inc, 1, 64);
    if (lane == 0u) exc = RT_MAP_ID;
    __syncthreads();
    uint32_t before = RT_MAP_ID, whole = RT_MAP_ID;
    for (uint32_t w = 0; w < RT_WG / 64u; ++w) { const uint32_t x = s_wave[w]; if (w < wave) before = rt_compose(before, x); whole = rt_compose(whole, x); }
    all = whole;
    return rt_compose(before, exc);
}

__global__ void __launch_bounds__(RT_WG) k_rt_phase_tiles(GmDevReadText t) {
    __shared__ uint32_t s_wave[RT_WG / 64u];
    __shared__ uint32_t s_cnt[4];
    if (threadIdx.x < 4u) s_cnt[threadIdx.x] = 0u;
    const uint64_t k = (uint64_t)blockIdx.x * RT_WG + threadIdx.x;
    const bool valid = k < t.n_lines;
    const bool blank = valid && rt_line_len(t, (uint32_t)k) == 0u;
    uint32_t all;
    const uint32_t exc = rt_map_scan(!valid ? RT_MAP_ID : blank ? RT_MAP_BLANK : RT_MAP_NEXT, s_wave, all);     // its barrier also publishes s_cnt = 0
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        const unsigned long long starts = __ballot(valid && !blank && rt_apply(exc, e) == 0u);
        if ((threadIdx.x & 63u) == 0u && starts) atomicAdd(&s_cnt[e], (uint32_t)__popcll(starts));
    }
    __syncthreads();
    if (threadIdx.x == 0) t.ltile_sum[(size_t)blockIdx.x * 8u] = all;
    if (threadIdx.x < 4u) t.ltile_sum[(size_t)blockIdx.x * 8u + 1u + threadIdx.x] = s_cnt[threadIdx.x];
}

// one workgroup: the phase every tile of lines is entered in (scan over map composition), then the records in front of it
__global__ void __launch_bounds__(1024) k_rt_phase_scan(GmDevReadText t) {
    __shared__ uint32_t part[1024];
    const uint32_t nt = t.n_ltiles, th = threadIdx.x, per = (nt + 1023u) / 1024u;
    const uint32_t a = (uint64_t)th * per < nt ? th * per : nt, b = (uint64_t)a + per < nt ? a + per : nt;
    uint32_t m = RT_MAP_ID;
    for (uint32_t j = a; j < b; ++j) m = rt_compose(m, t.ltile_sum[(size_t)j * 8u]);
    part[th] = m;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t v = th >= d ? part[th - d] : RT_MAP_ID;
        __syncthreads();
        part[th] = rt_compose(v, part[th]);
        __syncthreads();
    }
    const uint32_t in0 = th ? part[th - 1u] & 3u : 0u;                       // the text starts in phase 0
    __syncthreads();
    uint32_t ph = in0, s = 0;
    for (uint32_t j = a; j < b; ++j) { s += t.ltile_sum[(size_t)j * 8u + 1u + ph]; ph = rt_apply(t.ltile_sum[(size_t)j * 8u], ph); }
    part[th] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t v = th >= d ? part[th - d] : 0u;
        __syncthreads();
        part[th] += v;
        __syncthreads();
    }
    uint32_t run = part[th] - s;
    ph = in0;
    for (uint32_t j = a; j < b; ++j) {
        t.ltile_in[(size_t)j * 2u] = ph; t.ltile_in[(size_t)j * 2u + 1u] = run;
        run += t.ltile_sum[(size_t)j * 8u + 1u + ph]; ph = rt_apply(t.ltile_sum[(size_t)j * 8u], ph);
    }
    if (th == 1023u) t.meta[RT_META_RECS] = part[1023];
}

__global__ void __launch_bounds__(RT_WG) k_rt_records(GmDevReadText t) {
    __shared__ uint32_t s_wave[RT_WG / 64u];
    __shared__ uint32_t s_sum[RT_WG / 64u];
    const uint64_t k64 = (uint64_t)blockIdx.x * RT_WG + threadIdx.x;
    const bool valid = k64 < t.n_lines;
    const uint32_t k = (uint32_t)k64;
    const uint32_t nl = valid ? rt_line_len(t, k) : 0u;
    uint32_t all;
    const uint32_t exc = rt_map_scan(!valid ? RT_MAP_ID : nl == 0u ? RT_MAP_BLANK : RT_MAP_NEXT, s_wave, all);
    const bool start = valid && nl != 0u && rt_apply(exc, t.ltile_in[(size_t)blockIdx.x * 2u]) == 0u;
    uint32_t total;
    const uint32_t r = t.ltile_in[(size_t)blockIdx.x * 2u + 1u] + rt_block_scan(start ? 1u : 0u, s_sum, total);
    if (!start || r >= t.rec_cap) return;
    // the record whose name line this is
    const uint32_t name_at = t.line_at[k];
    GmDevTextRec rec;
    rec.name_off = name_at + 1u; rec.name_len = nl - 1u;
    rec.seq_off = rec.qual_off = 0u; rec.seq_len = rec.qual_len = 0u;
    bool good = (uint64_t)k + 3u < t.n_lines && t.text[name_at] == '@';
    if ((uint64_t)k + 1u < t.n_lines) { rec.seq_off = t.line_at[k + 1u]; rec.seq_len = rt_line_len(t, k + 1u); }
    if ((uint64_t)k + 3u < t.n_lines) {
        const uint32_t pl = rt_line_len(t, k + 2u);
        rec.qual_off = t.line_at[k + 3u]; rec.qual_len = rt_line_len(t, k + 3u);
        good = good && pl != 0u && t.text[t.line_at[k + 2u]] == '+' && rec.seq_len <= rec.qual_len;
    }
    t.recs[r] = rec;
    if (!good || rec.seq_len > 2048u)
        atomicMin(&t.meta[RT_META_BAD], ((unsigned long long)r << 2) | (good ? (unsigned long long)RT_BAD_LONG : (unsigned long long)RT_BAD_FORM));
}

__device__ __forceinline__ uint32_t rt_wave_max(uint32_t v) { for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; } return v; }
__device__ __forceinline__ uint32_t rt_wave_min(uint32_t v) { for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(v, d, 64); v = o < v ? o : v; } return v; }
__device__ __forceinline__ uint32_t rt_wave_sum(uint32_t v) { for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64); return v; }

// the block = the records in front of the first one that ends it
__global__ void __launch_bounds__(RT_WG) k_rt_finish(GmDevReadText t) {
    const unsigned long long bad = t.meta[RT_META_BAD], all = t.meta[RT_META_RECS];
    const unsigned long long n = bad != ~0ull && (bad >> 2) < all ? bad >> 2 : all;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        t.meta[RT_META_N] = n;
        t.meta[RT_META_BAD_AT] = n < all && n < t.rec_cap ? (unsigned long long)t.recs[n].name_off - 1u : 0ull;
    }
    const uint64_t r = (uint64_t)blockIdx.x * RT_WG + threadIdx.x;
    const bool in = r < n && r < t.rec_cap;
    uint32_t len = 0, nlen = 0, tlen = 0;
    if (in) {
        const GmDevTextRec rec = t.recs[r];
        len = rec.seq_len; nlen = rec.name_len < 1023u ? rec.name_len : 1023u; tlen = rec.qual_len - rec.seq_len;
        t.len[r] = (uint16_t)len; t.name_len[r] = nlen; t.tail_len[r] = tlen;
    }
    const uint32_t mx = rt_wave_max(len), mn = rt_wave_min(in ? len : 0xFFFFFFFFu), ns = rt_wave_sum(nlen), ts = rt_wave_sum(tlen);     // a wave: at most 64 x 1023 name bytes, tails below 2^32 in all
    if ((threadIdx.x & 63u) == 0u && __ballot(in) != 0ull) {
        atomicMax(&t.meta[RT_META_MAXLEN], (unsigned long long)mx);
        atomicMin(&t.meta[RT_META_MINLEN], (unsigned long long)mn);
        if (ns) atomicAdd(&t.meta[RT_META_NAME_BYTES], (unsigned long long)ns);
        if (ts) atomicAdd(&t.meta[RT_META_TAIL_BYTES], (unsigned long long)ts);
    }
}

// bytes [off, off + 8) of the text: two aligned words shifted into place (the buffer is padded: the second word may lie behind `bytes`)
__device__ __forceinline__ unsigned long long rt_load8(const uint8_t* text, uint32_t off) {
    const unsigned long long* w = reinterpret_cast<const unsigned long long*>(text + (off & ~7u));
    const uint32_t sh = (off & 7u) * 8u;
    const unsigned long long lo = w[0];
    return sh ? (lo >> sh) | (w[1] << (64u - sh)) : lo;
}
// bytes [c, c + 8) of a row whose `len` bytes start at text[off]: zero behind len
__device__ __forceinline__ unsigned long long rt_row8(const uint8_t* text, uint32_t off, uint32_t len, uint32_t c) {
    if (c >= len) return 0ull;
    const unsigned long long v = rt_load8(text, off + c);
    const uint32_t keep = len - c;
    return keep >= 8u ? v : v & ((1ull << (8u * keep)) - 1ull);
}

// one lane per W bytes of a row (W = 16 when the stride allows, else 8): both rows of a read
template <uint32_t W> __global__ void __launch_bounds__(RT_WG) k_rt_rows(GmDevReadText t, uint32_t n, uint32_t stride, uint8_t* bases, uint8_t* quals) {
    const uint32_t per = stride / W;
    const uint64_t p = (uint64_t)blockIdx.x * RT_WG + threadIdx.x;
    const uint64_t r = p / per;
    if (r >= n) return;
    const uint32_t c = (uint32_t)(p - r * per) * W;
    const GmDevTextRec rec = t.recs[r];
    const size_t at = (size_t)r * stride + c;
    if (W == 16u) {
        ulonglong2 b, q;
        b.x = rt_row8(t.text, rec.seq_off, rec.seq_len, c); b.y = rt_row8(t.text, rec.seq_off, rec.seq_len, c + 8u);
        q.x = rt_row8(t.text, rec.qual_off, rec.seq_len, c); q.y = rt_row8(t.text, rec.qual_off, rec.seq_len, c + 8u);
        *reinterpret_cast<ulonglong2*>(bases + at) = b;
        *reinterpret_cast<ulonglong2*>(quals + at) = q;
    } else {
        *reinterpret_cast<unsigned long long*>(bases + at) = rt_row8(t.text, rec.seq_off, rec.seq_len, c);
        *reinterpret_cast<unsigned long long*>(quals + at) = rt_row8(t.text, rec.qual_off, rec.seq_len, c);
    }
}

// 16 lanes per read: its name (cut) and what its quality line holds behind the sequence's length
__global__ void __launch_bounds__(RT_WG) k_rt_names(GmDevReadText t, uint32_t n, char* names, const uint64_t* name_off, char* tails, const uint64_t* tail_off) {
    const uint64_t g = (uint64_t)blockIdx.x * RT_WG + threadIdx.x;
    const uint64_t r = g >> 4;
    const uint32_t j0 = (uint32_t)g & 15u;
    if (r >= n) return;
    const GmDevTextRec rec = t.recs[r];
    const uint64_t no = name_off[r], nn = name_off[r + 1u] - no;
    for (uint64_t j = j0; j < nn; j += 16u) names[no + j] = (char)t.text[rec.name_off + j];
    const uint64_t to = tail_off[r], tn = tail_off[r + 1u] - to;
    for (uint64_t j = j0; j < tn; j += 16u) tails[to + j] = (char)t.text[(uint64_t)rec.qual_off + rec.seq_len + j];
}

// SeqReader.cpp:1155, 1171-1180: `int Q = (int)fastq[i]` of a signed char below 64 within the kept length; one lane per read, 8 bytes at a time
__global__ void __launch_bounds__(RT_WG) k_rt_illumina(const uint8_t* quals, uint32_t stride, const uint16_t* len, uint32_t n, uint32_t* until) {
    const uint64_t r = (uint64_t)blockIdx.x * RT_WG + threadIdx.x;
    bool low = false;
    if (r < n) {
        const unsigned long long* q = reinterpret_cast<const unsigned long long*>(quals + (size_t)r * stride);
        const uint32_t L = len[r] < stride ? len[r] : stride;
        for (uint32_t c = 0; c < L && !low; c += 8u) {
            unsigned long long v = q[c >> 3];
            const uint32_t keep = L - c;
            if (keep < 8u) v |= 0x4040404040404040ull << (8u * keep);                   // padding is not a quality
            const unsigned long long top = v & 0xC0C0C0C0C0C0C0C0ull;                    // a byte is 64 .. 127 iff its top bits are 01
            low = keep < 8u ? ((top ^ 0x4040404040404040ull) & ((1ull << (8u * keep)) - 1ull)) != 0ull : top != 0x4040404040404040ull;
        }
    }
    const unsigned long long any = __ballot(low);
    if (any && (threadIdx.x & 63u) == 0u) atomicMin(until, (uint32_t)(r + (uint32_t)__ffsll((long long)any) - 1u));
}

uint32_t gmk_readtext_tile_bytes() { return RT_TILE; }
uint32_t gmk_readtext_tiles(uint64_t bytes) { return (uint32_t)((bytes + RT_TILE - 1u) / RT_TILE); }
uint32_t gmk_readtext_line_tiles(uint64_t lines) { return (uint32_t)((lines + RT_WG - 1u) / RT_WG); }

int gmk_readtext_count(const GmDevReadText& t, void* stream) {
    if (t.bytes == 0) return 0;
    hipLaunchKernelGGL(k_rt_count, dim3(t.n_tiles), dim3(RT_WG), 0, S_(stream), t);
    hipLaunchKernelGGL(k_rt_scan, dim3(1), dim3(1024), 0, S_(stream), t.tile_cnt, t.n_tiles, t.tile_off, t.meta, (uint32_t)RT_META_LINES, 1u);
    return (int)hipGetLastError();
}

int gmk_readtext_records(const GmDevReadText& t, void* stream) {
    if (t.bytes == 0 || t.n_lines == 0) return 0;
    hipLaunchKernelGGL(k_rt_lines, dim3(t.n_tiles), dim3(RT_WG), 0, S_(stream), t);
    hipLaunchKernelGGL(k_rt_phase_tiles, dim3(t.n_ltiles), dim3(RT_WG), 0, S_(stream), t);
    hipLaunchKernelGGL(k_rt_phase_scan, dim3(1), dim3(1024), 0, S_(stream), t);
    hipLaunchKernelGGL(k_rt_records, dim3(t.n_ltiles), dim3(RT_WG), 0, S_(stream), t);
    hipLaunchKernelGGL(k_rt_finish, dim3((t.rec_cap + RT_WG - 1u) / RT_WG), dim3(RT_WG), 0, S_(stream), t);
    return (int)hipGetLastError();
}

int gmk_readtext_rows(const GmDevReadText& t, uint32_t n, uint32_t stride, uint8_t* bases, uint8_t* quals, void* stream) {
    if (n == 0) return 0;
    if (stride % 16u == 0u) {
        const uint64_t lanes = (uint64_t)n * (stride / 16u);
        hipLaunchKernelGGL(k_rt_rows<16u>, dim3((uint32_t)((lanes + RT_WG - 1u) / RT_WG)), dim3(RT_WG), 0, S_(stream), t, n, stride, bases, quals);
    } else {
        const uint64_t lanes = (uint64_t)n * (stride / 8u);
        hipLaunchKernelGGL(k_rt_rows<8u>, dim3((uint32_t)((lanes + RT_WG - 1u) / RT_WG)), dim3(RT_WG), 0, S_(stream), t, n, stride, bases, quals);
    }
    return (int)hipGetLastError();
}

int gmk_readtext_names(const GmDevReadText& t, uint32_t n, char* names, const uint64_t* name_off, char* tails, const uint64_t* tail_off, void* stream) {
    if (n == 0) return 0;
    const uint64_t lanes = (uint64_t)n * 16u;
    hipLaunchKernelGGL(k_rt_names, dim3((uint32_t)((lanes + RT_WG - 1u) / RT_WG)), dim3(RT_WG), 0, S_(stream), t, n, names, name_off, tails, tail_off);
    return (int)hipGetLastError();
}

int gmk_readtext_illumina(const uint8_t* quals, uint32_t stride, const uint16_t* len, uint32_t n, uint32_t* until, void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_rt_illumina, dim3((n + RT_WG - 1u) / RT_WG), dim3(RT_WG), 0, S_(stream), quals, stride, len, n, until);
    return (int)hipGetLastError();
}
