// gm_samsort.hip — coordinate-sorted SAM without a host sort: the rows gm_output_batch_sorted formats stay in HBM, in an arena of
// fixed-size pieces, with one (key, place, length) entry per row; when the input is exhausted the keys are sorted once and the rows
// are gathered in key order, slab by slab, for the download.
//
//   k_ss_rows     per block: key = contig << 32 | chr_pos of every ROW's record (~0 without a contig, and for the row of a read without a
//                 record, gm_batch_set_unmapped_rows), where the row lies in the arena, its length
//   k_ss_prepare  at finish, per block in sequence order: the sort key (contig and position packed into the bits in use, so the radix
//                 sort runs over those only), the row ordinal, and the block's places / lengths into the run's tables
//   rocprim::radix_sort_pairs (stable: equal keys keep ordinal = input order), k_ss_permute (places / lengths in sorted order),
//   rocprim::exclusive_scan (the sorted rows' offsets in the output)
//   k_ss_bound    one thread: how many whole rows fit in a byte budget (the block split at a piece's end; the rows of a slab)
//   k_ss_spans    per slab: the row that holds the first byte of every 4 KiB span of the slab
//   k_ss_gather   per slab, the hot path: one wavefront per span, a lane per 16 destination bytes - the few rows of the span go into LDS
//                 once, the row that owns a lane's bytes is found by a binary search there, the source is read with one unaligned
//                 16-byte load and stored with one aligned 16-byte store; only the 16 bytes across a row boundary are put together
//                 byte by byte
// With BAM rows, gm_sam_sorter_index_begin / gm_sam_sorter_bai (below) build the .bai of the file the slabs make: kernels in gm_bai.hip
#include "gm_lib.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <algorithm>
#include <chrono>
#include <memory>

namespace {

constexpr uint32_t SS_SPAN = 4096;                  // destination bytes one wavefront of k_ss_gather moves: 64 lanes x 16 bytes x 4

// rows [row_a, row_a + n) of the block; row_src (null: row k is record k) as gmk_row_source left it, for the whole block
__global__ void __launch_bounds__(256) k_ss_rows(const GmDevSamRec* recs, const unsigned long long* row_src, unsigned long long n_recs, unsigned long long row_a,
                                                 const uint64_t* row_off, uint32_t n, uint32_t n_seqs, uint32_t piece, long long delta,
                                                 unsigned long long* key, unsigned long long* place, uint32_t* len) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned long long src = row_src ? row_src[row_a + i] : row_a + i;
    GmDevSamRec r = {}; r.contig = 0xFFFFFFFFu;                  // a read without a record: no contig, sorts last
    if (src < n_recs) r = recs[src];
    key[i] = r.contig < n_seqs ? (unsigned long long)r.contig << 32 | (r.chr_pos & 0xFFFFFFFFull) : ~0ull;
    const unsigned long long a = row_off[i], b = row_off[i + 1];
    place[i] = (unsigned long long)piece << 32 | (unsigned long long)((long long)a + delta);
    len[i] = (uint32_t)(b - a);
}

__global__ void __launch_bounds__(256) k_ss_prepare(const unsigned long long* key, const unsigned long long* place, const uint32_t* len, uint32_t n, uint32_t base,
                                                    uint32_t n_seqs, uint32_t pos_bits, unsigned long long* skey, uint32_t* ord, unsigned long long* place_cat,
                                                    uint32_t* len_cat) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i], pos_max = (1ull << pos_bits) - 1;
    const unsigned long long pos = k & 0xFFFFFFFFull;
    skey[base + i] = k == ~0ull ? (unsigned long long)n_seqs << pos_bits : (k >> 32) << pos_bits | (pos < pos_max ? pos : pos_max);
    ord[base + i] = base + i;
    place_cat[base + i] = place[i];
    len_cat[base + i] = len[i];
}

__global__ void __launch_bounds__(256) k_ss_permute(const uint32_t* ord, const unsigned long long* place_cat, const uint32_t* len_cat, uint32_t n,
                                                    unsigned long long* splace, uint32_t* slen) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    if (i == n) { slen[n] = 0; return; }
    const uint32_t o = ord[i];
    splace[i] = place_cat[o];
    slen[i] = len_cat[o];
}

// out[0] = the largest b in [lo, hi] with off[b] - off[lo] <= room, out[1] = off[b], out[2] = off[lo + 1] - off[lo] (lo < hi)
__global__ void k_ss_bound(const unsigned long long* off, unsigned long long lo, unsigned long long hi, unsigned long long room, unsigned long long* out) {
    const unsigned long long base = off[lo];
    unsigned long long a = lo, b = hi;
    while (a < b) {
        const unsigned long long m = a + (b - a + 1) / 2;
        if (off[m] - base <= room) a = m; else b = m - 1;
    }
    out[0] = a; out[1] = off[a]; out[2] = lo < hi ? off[lo + 1] - base : 0;
}

// rows [r0, r1) of the sorted order make the slab; base = soff[r0].  span_first[s] = the row that holds byte s * SS_SPAN of the slab,
// span_first[n_spans] = r1 - 1
__global__ void __launch_bounds__(256) k_ss_spans(const unsigned long long* soff, uint32_t r0, uint32_t r1, uint32_t n_spans, uint32_t* span_first) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= r1 - r0) return;
    const uint32_t r = r0 + (uint32_t)i;
    const unsigned long long base = soff[r0], a = soff[r] - base, b = soff[r + 1] - base;
    for (unsigned long long s = (a + SS_SPAN - 1) / SS_SPAN; s * SS_SPAN < b; ++s) span_first[s] = r;
    if (i == 0) span_first[n_spans] = r1 - 1;
}

__device__ __forceinline__ const char* ss_src(const char* const* pieces, unsigned long long place) { return pieces[place >> 32] + (place & 0xFFFFFFFFull); }

// One wavefront per span.  The few rows that hold the span's bytes (span_first[span] .. span_first[span + 1]) are loaded once, side by
// side, into the wavefront's part of LDS - their offsets in the slab and their addresses in the arena - so that a lane's way from
// its 16 destination bytes to their source is one trip to global memory and a search in LDS; the four source loads of a lane are
// issued before the first of them is stored.  A span of more than SS_ROWS rows (rows under 64 bytes on average) searches soff itself.
constexpr uint32_t SS_ROWS = 63;

__global__ void __launch_bounds__(256) k_ss_gather(const unsigned long long* __restrict__ soff, const unsigned long long* __restrict__ splace,
                                                   const char* const* __restrict__ pieces, const uint32_t* __restrict__ span_first, uint32_t r0, uint32_t n_spans,
                                                   unsigned long long bytes, char* __restrict__ slab) {
    __shared__ unsigned long long s_off[4][SS_ROWS + 1];
    __shared__ const char* s_src[4][SS_ROWS + 1];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t span = blockIdx.x * 4u + w;
    const bool live = span < n_spans;
    const unsigned long long base = soff[r0];
    uint32_t lo = 0, n_rows = 0;
    if (live) {
        lo = span_first[span];
        n_rows = span_first[span + 1] - lo + 1;
        if (n_rows <= SS_ROWS && lane <= n_rows) {                     // entry n_rows: where the last row ends
            s_off[w][lane] = soff[lo + lane] - base;
            if (lane < n_rows) s_src[w][lane] = ss_src(pieces, splace[lo + lane]);
        }
    }
    __syncthreads();
    if (!live) return;
    const bool in_lds = n_rows <= SS_ROWS;
    auto off_of = [&](uint32_t k) -> unsigned long long { return in_lds ? s_off[w][k] : soff[lo + k] - base; };      // k in [0, n_rows]
    auto src_of = [&](uint32_t k) -> const char* { return in_lds ? s_src[w][k] : ss_src(pieces, splace[lo + k]); };
    uint4 v[4];
    uint32_t row[4];
    bool fast[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
        const unsigned long long c = (unsigned long long)span * SS_SPAN + u * 1024u + lane * 16u;
        fast[u] = false; row[u] = 0;
        if (c >= bytes) continue;
        uint32_t a = 0, b = n_rows - 1;              // the last row of the span's that starts at or before c
        while (a < b) {
            const uint32_t m = a + (b - a + 1) / 2;
            if (off_of(m) <= c) a = m; else b = m - 1;
        }
        row[u] = a;
        fast[u] = off_of(a + 1) - c >= 16;
        if (fast[u]) __builtin_memcpy(&v[u], src_of(a) + (c - off_of(a)), 16);
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
        const unsigned long long c = (unsigned long long)span * SS_SPAN + u * 1024u + lane * 16u;
        if (c >= bytes) continue;
        if (!fast[u]) {                              // the chunk crosses into the next row(s), or the slab ends inside it
            uint32_t x[4] = { 0, 0, 0, 0 };
            uint32_t r = row[u];
            unsigned long long at = off_of(r), end = off_of(r + 1);
            const char* src = src_of(r);
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const unsigned long long d = c + k;
                if (d < bytes) {
                    while (d >= end) { ++r; at = end; end = off_of(r + 1); src = src_of(r); }
                    x[k >> 2] |= (uint32_t)(unsigned char)src[d - at] << ((k & 3u) * 8u);
                }
            }
            v[u] = make_uint4(x[0], x[1], x[2], x[3]);
        }
        *reinterpret_cast<uint4*>(slab + c) = v[u];
    }
}

struct U32ToU64 { __host__ __device__ unsigned long long operator()(uint32_t v) const { return v; } };

struct SsBlock { uint64_t n_rows = 0; void* tab = nullptr; };
struct SsSeg { uint64_t row_a, row_b, src_off, bytes; uint32_t piece; uint64_t dst_off; };

uint32_t bits_for(uint64_t v) { uint32_t b = 0; while (v >> b && b < 64) ++b; return b ? b : 1; }

}   // namespace

struct gm_sam_sorter {
    gm_index* ix = nullptr;
    int device = -1;                                    // ix->device, kept: gm_sam_sorter_destroy may run after the index was closed
    std::mutex mu;
    size_t piece_bytes = (size_t)1 << 30;
    std::vector<char*> pieces; size_t used = 0;         // used: bytes of the last piece that hold rows
    std::map<uint64_t, SsBlock> blocks;                 // by sequence number
    uint64_t table_bytes = 0;
    int rows = GM_ROWS_TEXT;                            // what the blocks put into the arena: SAM rows as text or BAM records (gm_sam_sorter_set_rows)
    GmBgzfBufs bz;                                      // gm_sam_sorter_read_bgzf: the slab's blocks
    bool closed = false, finished = false;              // closed: finish was called, no more blocks; finished: it succeeded, the rows can be read
    int failed = GM_OK; std::string fail_text;          // finish failed: every later finish / read returns this
    uint64_t n_rows = 0, text_bytes = 0, next_row = 0, next_off = 0;
    DevBuf bound, soff, splace, d_pieces, slab, spans;
    hipEvent_t ev[2] = { nullptr, nullptr };
    // gm_sam_sorter_index_begin: the per-row table of the .bai, filled slab by slab as gm_sam_sorter_read_bgzf hands the rows out
    bool bai_on = false;
    int bai_level = -1;                                 // the level of the reads so far (-1: none yet)
    uint64_t bai_off = 0;                               // where the next block read_bgzf returns will lie in the file
    void* bai_tab = nullptr;
    GmBaiRows bai{};
    void* bai_file = nullptr;                           // the finished index in HBM (gm_sam_sorter_bai builds it once)
    hipEvent_t bai_ev[2] = { nullptr, nullptr };
    gm_sam_sort_stats st{};
    uint64_t held() const { return (uint64_t)pieces.size() * piece_bytes + table_bytes; }
};

// free HBM is checked before every growth: the index, its tables and the batches come first, the sorter takes what is left
static int ss_alloc(gm_sam_sorter* s, void** p, size_t bytes, const char* what) {
    size_t free_b = 0, total_b = 0;
    hipError_t e = hipMemGetInfo(&free_b, &total_b);
    if (e == hipSuccess && free_b >= bytes) e = hipMalloc(p, bytes);
    else if (e == hipSuccess) e = hipErrorOutOfMemory;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        gm_set_error(std::string("SAM sorter: out of HBM for ") + what + ": it holds " + std::to_string(s->held()) + " bytes and asked for " + std::to_string(bytes) +
                     " more (" + std::to_string(free_b) + " free)");
        return GM_E_NOMEM;
    }
    return GM_OK;
}

extern "C" int gm_sam_sorter_create(gm_index* ix, gm_sam_sorter** out) {
    if (!ix || !out) return GM_E_ARG;
    *out = nullptr;
    if (ix->host_only) { gm_set_error("gm_sam_sorter_create: no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(ix->device));
    std::unique_ptr<gm_sam_sorter> s(new gm_sam_sorter());
    s->ix = ix; s->device = ix->device;
    const long long want = gm_opt_ll("GM_SORT_PIECE", 1ll << 30);
    s->piece_bytes = (size_t)std::min<long long>(std::max<long long>(want, 64 << 10), 0xFFFF0000ll) & ~(size_t)15;    // a row's offset in its piece fits 32 bits
    if (s->bound.ensure(32)) return GM_E_NOMEM;
    for (auto& e : s->ev) HIPCHK(hipEventCreate(&e));
    s->st.piece_bytes = s->piece_bytes;
    *out = s.release();
    return GM_OK;
}

extern "C" void gm_sam_sorter_destroy(gm_sam_sorter* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);                  // not through s->ix: a sorter may outlive its index (one a garbage collector frees late), and a failing call here is what the next hipGetLastError of the thread reports
    for (char* p : s->pieces) (void)hipFree(p);
    for (auto& b : s->blocks) if (b.second.tab) (void)hipFree(b.second.tab);
    for (DevBuf* d : { &s->bound, &s->soff, &s->splace, &s->d_pieces, &s->slab, &s->spans }) d->release();
    s->bz.release();
    for (auto e : s->ev) if (e) (void)hipEventDestroy(e);
    for (auto e : s->bai_ev) if (e) (void)hipEventDestroy(e);
    if (s->bai_tab) (void)hipFree(s->bai_tab);
    if (s->bai_file) (void)hipFree(s->bai_file);
    delete s;
}

extern "C" int gm_sam_sorter_set_rows(gm_sam_sorter* s, int rows) {
    if (!s) return GM_E_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (rows != GM_ROWS_TEXT && rows != GM_ROWS_BAM) { gm_set_error("gm_sam_sorter_set_rows: GM_ROWS_TEXT or GM_ROWS_BAM"); return GM_E_ARG; }
    if (!s->blocks.empty() || s->closed) { gm_set_error("gm_sam_sorter_set_rows: the sorter holds blocks already"); return GM_E_ARG; }
    s->rows = rows;
    return GM_OK;
}

int gm_samsort_rows(gm_sam_sorter* s) { std::lock_guard<std::mutex> lk(s->mu); return s->rows; }

// the sequence number is taken before anything of the block is computed: a seq used twice or an add after finish deposits nothing
int gm_samsort_claim(gm_sam_sorter* s, const gm_index* ix, uint64_t seq) {
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->ix != ix) { gm_set_error("SAM sorter: it belongs to another index"); return GM_E_ARG; }
    if (s->closed) { gm_set_error("SAM sorter: a block added after gm_sam_sorter_finish"); return GM_E_ARG; }
    if (!s->blocks.emplace(seq, SsBlock{}).second) { gm_set_error("SAM sorter: sequence number " + std::to_string(seq) + " used twice"); return GM_E_ARG; }
    return GM_OK;
}

// ... and given back when the call that took it fails before any row of the block is in the arena (GM_E_BATCH_TOO_LARGE: the caller
// adds the block again in halves, the first of which may carry the same number)
void gm_samsort_release(gm_sam_sorter* s, uint64_t seq) {
    std::lock_guard<std::mutex> lk(s->mu);
    auto it = s->blocks.find(seq);
    if (it != s->blocks.end() && !it->second.n_rows && !it->second.tab) s->blocks.erase(it);
}

// the rows of a block as k_out_text_rows left them (text, n_rows + 1 offsets, the records), all in HBM, into the arena on `stream`.
// The keys are per row: row_src (null: row k is record k) names the record of a row, or says that it has none - key ~0, behind every
// contig, and among themselves such rows keep input order like all rows of one key
int gm_samsort_add(gm_sam_sorter* s, uint64_t seq, const GmDevSamRec* recs, const unsigned long long* row_src, uint64_t n_recs, uint64_t n_rows, const char* d_text,
                   const uint64_t* d_rowoff, uint64_t text_len, void* stream) {
    if (!n_rows) return GM_OK;
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = S_(stream);
    const uint32_t n_seqs = (uint32_t)s->ix->h.contigs.size();
    std::vector<SsSeg> segs;
    void* tab = nullptr;
    {
        // The arena's tail is handed out under the sorter's mutex, and so is its growth: the hipMalloc of a piece and, where a block
        // has to be cut at a piece's end, k_ss_bound with its wait run with the mutex held, and the other workers' adds and claims wait
        // meanwhile.  With pieces of 1 GiB that is once per several blocks.
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->closed) { gm_set_error("SAM sorter: a block added after gm_sam_sorter_finish"); return GM_E_ARG; }
        const size_t pieces0 = s->pieces.size(), used0 = s->used;
        if (s->n_rows + n_rows > 0xFFFFFFFFull) { gm_set_error("SAM sorter: more than 2^32 - 1 rows (row ordinals are 32-bit)"); return GM_E_UNSUPPORTED; }
        const size_t tab_bytes = (size_t)n_rows * 20 + 64;
        if (const int rc = ss_alloc(s, &tab, tab_bytes, "a block's row table")) return rc;
        auto grow = [&]() -> int {
            void* p = nullptr;
            if (const int rc = ss_alloc(s, &p, s->piece_bytes + 64, "a piece of the text arena")) return rc;
            s->pieces.push_back((char*)p); s->used = 0;
            return GM_OK;
        };
        uint64_t a = 0, at = 0;                     // rows [0, a) are placed; at = row_off[a]
        int rc = GM_OK;
        while (a < n_rows && rc == GM_OK) {
            if (s->pieces.empty() || s->used >= s->piece_bytes) { rc = grow(); continue; }
            const uint64_t room = s->piece_bytes - s->used, rest = text_len - at;
            if (rest <= room) { segs.push_back({ a, n_rows, at, rest, (uint32_t)s->pieces.size() - 1, s->used }); s->used += rest; a = n_rows; break; }
            // the block does not fit: cut it at the last row boundary the piece has room for
            unsigned long long res[3] = { 0, 0, 0 };
            hipLaunchKernelGGL(k_ss_bound, dim3(1), dim3(1), 0, st, (const unsigned long long*)d_rowoff, (unsigned long long)a, (unsigned long long)n_rows, (unsigned long long)room,
                               s->bound.as<unsigned long long>());
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(res, s->bound.p, 24, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { gm_set_error(std::string("SAM sorter: k_ss_bound: ") + hipGetErrorString(e)); rc = GM_E_HIP; break; }
            const uint64_t b = res[0];
            if (b < a || b > n_rows || res[1] < at || res[1] - at > room) { gm_set_error("SAM sorter: row offsets of the block do not ascend"); rc = GM_E_ARG; break; }
            if (b == a) {
                if (s->used == 0) { gm_set_error("SAM sorter: a row of " + std::to_string(res[2]) + " bytes is longer than a piece of the arena (GM_SORT_PIECE)"); rc = GM_E_UNSUPPORTED; break; }
                rc = grow();
                continue;
            }
            segs.push_back({ a, b, at, res[1] - at, (uint32_t)s->pieces.size() - 1, s->used });
            s->used += res[1] - at; a = b; at = res[1];
        }
        if (rc != GM_OK) {                          // nothing of the block stays: the pieces it made grow go back, the tail is where it was
            (void)hipFree(tab);
            while (s->pieces.size() > pieces0) { (void)hipFree(s->pieces.back()); s->pieces.pop_back(); }
            s->used = used0;
            return rc;
        }
        SsBlock& blk = s->blocks[seq];
        blk.n_rows = n_rows; blk.tab = tab;
        s->table_bytes += tab_bytes;
        s->n_rows += n_rows; s->text_bytes += text_len;
    }
    unsigned long long* key = (unsigned long long*)tab;
    unsigned long long* place = key + n_rows;
    uint32_t* len = (uint32_t*)(place + n_rows);
    for (const SsSeg& g : segs) {
        char* dst = nullptr;
        { std::lock_guard<std::mutex> lk(s->mu); dst = s->pieces[g.piece]; }
        HIPCHK(hipMemcpyAsync(dst + g.dst_off, d_text + g.src_off, (size_t)g.bytes, hipMemcpyDeviceToDevice, st));
        const uint32_t n = (uint32_t)(g.row_b - g.row_a);
        hipLaunchKernelGGL(k_ss_rows, dim3((n + 255u) / 256u), dim3(256), 0, st, recs, row_src, (unsigned long long)n_recs, (unsigned long long)g.row_a, d_rowoff + g.row_a, n, n_seqs, g.piece,
                           (long long)g.dst_off - (long long)g.src_off, key + g.row_a, place + g.row_a, len + g.row_a);
        HIPCHK(hipGetLastError());
    }
    {
        std::lock_guard<std::mutex> lk(s->mu);
        s->st.add_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return GM_OK;
}

static int ss_sort(gm_sam_sorter* s, void* stream);

extern "C" int gm_sam_sorter_finish(gm_sam_sorter* s, uint64_t* n_rows, uint64_t* text_bytes, void* stream) {
    if (!s) return GM_E_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (n_rows) *n_rows = s->n_rows;
    if (text_bytes) *text_bytes = s->text_bytes;
    if (s->failed) { gm_set_error(s->fail_text); return s->failed; }
    if (s->finished) return GM_OK;
    s->closed = true;
    const int rc = ss_sort(s, stream);
    if (rc != GM_OK) {                              // remembered: the tables are incomplete, nothing may be read
        s->failed = rc; s->fail_text = std::string("gm_sam_sorter_finish failed earlier: ") + gm_last_error();
        s->soff.release(); s->splace.release();
        return rc;
    }
    s->finished = true;
    return GM_OK;
}

// the sort proper, under the sorter's mutex
static int ss_sort(gm_sam_sorter* s, void* stream) {
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(s->ix->device));
    hipStream_t st = S_(stream);
    s->st.rows = s->n_rows; s->st.text_bytes = s->text_bytes; s->st.pieces = s->pieces.size();
    const uint64_t N = s->n_rows;
    if (!N) return GM_OK;
    const uint32_t n = (uint32_t)N;
    // the key bits in use: the contig index (n_seqs itself for a row without a contig) above the widest position
    const auto& contigs = s->ix->h.contigs;
    uint64_t max_len = 1;
    for (const auto& c : contigs) max_len = std::max<uint64_t>(max_len, c.len);
    const uint32_t n_seqs = (uint32_t)contigs.size(), pos_bits = std::min<uint32_t>(32, bits_for(max_len + 1)), end_bit = pos_bits + bits_for(n_seqs);
    Scoped<DevBuf> k0, k1, v0, v1, place_cat, len_cat, slen, tmp;
    size_t tmp_sort = 0, tmp_scan = 0;
    {
        rocprim::double_buffer<unsigned long long> kb(nullptr, nullptr);
        rocprim::double_buffer<uint32_t> vb(nullptr, nullptr);
        auto in = rocprim::make_transform_iterator((const uint32_t*)nullptr, U32ToU64());
        if (rocprim::radix_sort_pairs(nullptr, tmp_sort, kb, vb, (size_t)N, 0u, end_bit, st) != hipSuccess ||
            rocprim::exclusive_scan(nullptr, tmp_scan, in, (unsigned long long*)nullptr, 0ull, (size_t)N + 1, rocprim::plus<unsigned long long>(), st) != hipSuccess) {
            gm_set_error("SAM sorter: rocPRIM could not size its scratch"); return GM_E_HIP;
        }
    }
    void* big[8]; size_t big_bytes[8] = { N * 8, N * 8, N * 4, N * 4, N * 8, N * 4, (N + 1) * 4, std::max(tmp_sort, tmp_scan) + 64 };
    DevBuf* bufs[8] = { &k0, &k1, &v0, &v1, &place_cat, &len_cat, &slen, &tmp };
    for (int i = 0; i < 8; ++i) {
        if (const int rc = ss_alloc(s, &big[i], big_bytes[i] + 64, "the sort")) return rc;
        bufs[i]->p = big[i]; bufs[i]->cap = big_bytes[i] + 64;
    }
    void* keep[2];
    if (const int rc = ss_alloc(s, &keep[0], (N + 1) * 8 + 64, "the sorted rows' offsets")) return rc;
    s->soff.p = keep[0]; s->soff.cap = (N + 1) * 8 + 64;
    if (const int rc = ss_alloc(s, &keep[1], N * 8 + 64, "the sorted rows' places")) return rc;
    s->splace.p = keep[1]; s->splace.cap = N * 8 + 64;
    uint32_t base = 0;
    for (auto& kv : s->blocks) {                    // ascending sequence number
        const SsBlock& b = kv.second;
        if (!b.n_rows) continue;
        const uint32_t bn = (uint32_t)b.n_rows;
        const unsigned long long* key = (const unsigned long long*)b.tab;
        const unsigned long long* place = key + bn;
        const uint32_t* len = (const uint32_t*)(place + bn);
        hipLaunchKernelGGL(k_ss_prepare, dim3((bn + 255u) / 256u), dim3(256), 0, st, key, place, len, bn, base, n_seqs, pos_bits, k0.as<unsigned long long>(), v0.as<uint32_t>(),
                           place_cat.as<unsigned long long>(), len_cat.as<uint32_t>());
        HIPCHK(hipGetLastError());
        base += bn;
    }
    rocprim::double_buffer<unsigned long long> kb(k0.as<unsigned long long>(), k1.as<unsigned long long>());
    rocprim::double_buffer<uint32_t> vb(v0.as<uint32_t>(), v1.as<uint32_t>());
    HIPCHK(rocprim::radix_sort_pairs(tmp.p, tmp_sort, kb, vb, (size_t)N, 0u, end_bit, st));
    hipLaunchKernelGGL(k_ss_permute, dim3(n / 256u + 1u), dim3(256), 0, st, (const uint32_t*)vb.current(), place_cat.as<unsigned long long>(), len_cat.as<uint32_t>(), n,
                       s->splace.as<unsigned long long>(), slen.as<uint32_t>());
    HIPCHK(hipGetLastError());
    auto in = rocprim::make_transform_iterator((const uint32_t*)slen.as<uint32_t>(), U32ToU64());
    HIPCHK(rocprim::exclusive_scan(tmp.p, tmp_scan, in, s->soff.as<unsigned long long>(), 0ull, (size_t)N + 1, rocprim::plus<unsigned long long>(), st));
    if (s->d_pieces.ensure(s->pieces.size() * sizeof(char*))) return GM_E_NOMEM;
    HIPCHK(hipMemcpyAsync(s->d_pieces.p, s->pieces.data(), s->pieces.size() * sizeof(char*), hipMemcpyHostToDevice, st));
    unsigned long long total = 0;
    HIPCHK(hipMemcpyAsync(&total, s->soff.as<unsigned long long>() + N, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total != s->text_bytes) { gm_set_error("SAM sorter: the sorted rows' lengths sum to " + std::to_string(total) + " bytes, the arena holds " + std::to_string(s->text_bytes)); return GM_E_HIP; }
    for (auto& kv : s->blocks) if (kv.second.tab) { (void)hipFree(kv.second.tab); kv.second.tab = nullptr; }
    s->table_bytes = 0;
    s->st.sort_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return GM_OK;
}

// the next whole rows that fit in `room` bytes, gathered into s->slab on `st` (not waited for): *bytes of them, 0 when none is left;
// GM_E_CAPACITY with *bytes = the next row's length when that row alone is longer.  Under the sorter's mutex
static int ss_gather_next(gm_sam_sorter* s, const char* who, uint64_t room, uint64_t* bytes_out, uint64_t* r1_out, uint64_t* off1_out, hipStream_t st) {
    *bytes_out = 0;
    if (s->failed) { gm_set_error(s->fail_text); return s->failed; }
    if (!s->finished) { gm_set_error(std::string(who) + ": call gm_sam_sorter_finish first"); return GM_E_ARG; }
    *r1_out = s->next_row; *off1_out = s->next_off;
    if (s->next_row >= s->n_rows) return GM_OK;
    HIPCHK(hipSetDevice(s->ix->device));
    unsigned long long res[3] = { 0, 0, 0 };
    hipLaunchKernelGGL(k_ss_bound, dim3(1), dim3(1), 0, st, s->soff.as<unsigned long long>(), (unsigned long long)s->next_row, (unsigned long long)s->n_rows, (unsigned long long)room,
                       s->bound.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(res, s->bound.p, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t r0 = s->next_row, r1 = res[0];
    if (r1 < r0 || r1 > s->n_rows || res[1] < s->next_off || res[1] - s->next_off > room) { gm_set_error(std::string(who) + ": the sorted offsets do not ascend"); return GM_E_HIP; }
    if (r1 == r0) { *bytes_out = res[2]; return GM_E_CAPACITY; }
    const uint64_t bytes = res[1] - s->next_off;
    const uint64_t n_spans64 = (bytes + SS_SPAN - 1) / SS_SPAN;
    if (n_spans64 > 0x7FFFFFF0ull) { gm_set_error(std::string(who) + ": a slab of more than 8 TB"); return GM_E_ARG; }
    const uint32_t n_spans = (uint32_t)n_spans64;
    // the last lane's store may reach up to 15 bytes past `bytes`: the slab is a whole number of spans
    if (s->slab.ensure((size_t)n_spans * SS_SPAN + 64) || s->spans.ensure(((size_t)n_spans + 1) * 4)) return GM_E_NOMEM;
    HIPCHK(hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(k_ss_spans, dim3((uint32_t)((r1 - r0 + 255) / 256)), dim3(256), 0, st, s->soff.as<unsigned long long>(), (uint32_t)r0, (uint32_t)r1, n_spans, s->spans.as<uint32_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_ss_gather, dim3((n_spans + 3u) / 4u), dim3(256), 0, st, s->soff.as<unsigned long long>(), s->splace.as<unsigned long long>(),
                       (const char* const*)s->d_pieces.p, s->spans.as<uint32_t>(), (uint32_t)r0, n_spans, (unsigned long long)bytes, s->slab.as<char>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[1], st));
    *bytes_out = bytes; *r1_out = r1; *off1_out = res[1];
    return GM_OK;
}

// the gather has run and has been waited for: its time, and the rows count as read
static int ss_consumed(gm_sam_sorter* s, uint64_t bytes, uint64_t r1, uint64_t off1) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    s->st.gather_ms += ms; s->st.gather_bytes += bytes;
    s->next_row = r1; s->next_off = off1;
    return GM_OK;
}

extern "C" int gm_sam_sorter_read(gm_sam_sorter* s, char* text, uint64_t cap, uint64_t* n_out, void* stream) {
    if (!s || !n_out) return GM_E_ARG;
    *n_out = 0;
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->bai_on) { gm_set_error("gm_sam_sorter_read: after gm_sam_sorter_index_begin the rows leave through gm_sam_sorter_read_bgzf"); return GM_E_ARG; }
    if (!text && cap && s->finished && s->next_row < s->n_rows) { gm_set_error("gm_sam_sorter_read: text is NULL"); return GM_E_ARG; }
    hipStream_t st = S_(stream);
    uint64_t bytes = 0, r1 = 0, off1 = 0;
    const int rc = ss_gather_next(s, "gm_sam_sorter_read", cap, &bytes, &r1, &off1, st);
    if (rc == GM_E_CAPACITY) {
        *n_out = bytes;
        gm_set_error("gm_sam_sorter_read: the next row is " + std::to_string(bytes) + " bytes long, the buffer holds " + std::to_string(cap));
        return rc;
    }
    if (rc != GM_OK || !bytes) return rc;
    HIPCHK(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpyAsync(text, s->slab.p, (size_t)bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->st.download_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (const int r = ss_consumed(s, bytes, r1, off1)) return r;
    *n_out = bytes;
    return GM_OK;
}

extern "C" int gm_sam_sorter_read_bgzf(gm_sam_sorter* s, int level, void* out, uint64_t cap, uint64_t* n_out, void* stream) {
    if (!s || !n_out) return GM_E_ARG;
    *n_out = 0;
    if (!gm_bgzf_level_ok(level)) { gm_set_error("gm_sam_sorter_read_bgzf: " + gm_bgzf_level_text(level)); return GM_E_ARG; }
    std::lock_guard<std::mutex> lk(s->mu);
    if (!out && cap && s->finished && s->next_row < s->n_rows) { gm_set_error("gm_sam_sorter_read_bgzf: out is NULL"); return GM_E_ARG; }
    if (s->bai_on && s->bai_level >= 0 && level != s->bai_level) {
        gm_set_error("gm_sam_sorter_read_bgzf: level " + std::to_string(level) + " after reads at level " + std::to_string(s->bai_level) + ": one indexed file, one level");
        return GM_E_ARG;
    }
    hipStream_t st = S_(stream);
    uint64_t bytes = 0, r1 = 0, off1 = 0;
    const int rc = ss_gather_next(s, "gm_sam_sorter_read_bgzf", gm_bgzf_room(cap), &bytes, &r1, &off1, st);
    if (rc == GM_E_CAPACITY) {
        *n_out = gm_bgzf_bound(bytes);
        gm_set_error("gm_sam_sorter_read_bgzf: the next row is " + std::to_string(bytes) + " bytes long and may take " + std::to_string(*n_out) + " as BGZF, the buffer holds " + std::to_string(cap));
        return rc;
    }
    if (rc != GM_OK || !bytes) return rc;
    uint64_t total = 0;
    if (const int r = gm_bgzf_device(s->slab.p, bytes, level, s->bz, &total, stream)) return r;
    if (total > cap) { gm_set_error("gm_sam_sorter_read_bgzf: the blocks outgrew their worst case"); return GM_E_HIP; }
    if (s->bai_on) {                                 // the slab and the scan of its blocks' sizes are still in place: where its rows lie in the file
        HIPCHK(hipEventRecord(s->bai_ev[0], st));
        KCHK(gmk_bai_rows(s->slab.p, s->soff.as<uint64_t>(), s->next_row, r1, bytes, s->bz.offs.as<uint64_t>(), (uint32_t)gm_bai_blocks(bytes), s->bai_off,
                          (uint32_t)s->ix->h.contigs.size(), s->bai, stream));
        HIPCHK(hipEventRecord(s->bai_ev[1], st));
    }
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpyAsync(out, s->bz.out.p, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->st.download_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (s->bai_on) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, s->bai_ev[0], s->bai_ev[1]));
        s->st.bai_ms += ms;
        s->bai_off += total; s->bai_level = level;
    }
    if (const int r = ss_consumed(s, bytes, r1, off1)) return r;
    *n_out = total;
    return GM_OK;
}

// ---- the .bai beside a sorted BAM (kernels: gm_bai.hip) ----
extern "C" int gm_sam_sorter_index_begin(gm_sam_sorter* s, uint64_t file_offset) {
    if (!s) return GM_E_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->failed) { gm_set_error(s->fail_text); return s->failed; }
    if (s->rows != GM_ROWS_BAM) { gm_set_error("gm_sam_sorter_index_begin: the sorter holds SAM rows as text, a .bai indexes BAM records (gm_sam_sorter_set_rows)"); return GM_E_ARG; }
    if (!s->finished) { gm_set_error("gm_sam_sorter_index_begin: call gm_sam_sorter_finish first"); return GM_E_ARG; }
    if (s->bai_on) { gm_set_error("gm_sam_sorter_index_begin: called twice"); return GM_E_ARG; }
    if (s->next_row || s->next_off) { gm_set_error("gm_sam_sorter_index_begin: rows have been read already, their places in the file are not known"); return GM_E_ARG; }
    if (file_offset >> 47) { gm_set_error("gm_sam_sorter_index_begin: a file offset of 2^47 or more does not fit a virtual offset"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(s->ix->device));
    const size_t n = (size_t)s->n_rows, bytes = n * 28 + 16 + 64;
    if (const int rc = ss_alloc(s, &s->bai_tab, bytes, "the index's row table")) return rc;
    char* p = (char*)s->bai_tab;
    s->bai.vbeg = (unsigned long long*)p; p += n * 8;
    s->bai.vend = (unsigned long long*)p; p += n * 8;
    s->bai.ref = (uint32_t*)p; p += n * 4;
    s->bai.pos = (int32_t*)p; p += n * 4;
    s->bai.pk = (uint32_t*)p; p += n * 4;
    s->bai.err = (uint32_t*)p;
    hipError_t e = hipMemset(s->bai.err, 0xFF, 16);
    for (auto& ev : s->bai_ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) {
        for (auto& ev : s->bai_ev) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
        (void)hipFree(s->bai_tab); s->bai_tab = nullptr;
        gm_set_error(std::string("gm_sam_sorter_index_begin: ") + hipGetErrorString(e)); return GM_E_HIP;
    }
    s->table_bytes += bytes;
    s->bai_on = true; s->bai_off = file_offset; s->bai_level = -1;
    return GM_OK;
}

extern "C" int gm_sam_sorter_bai(gm_sam_sorter* s, void* out, uint64_t cap, uint64_t* n_out, void* stream) {
    if (!s || !n_out) return GM_E_ARG;
    *n_out = 0;
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->failed) { gm_set_error(s->fail_text); return s->failed; }
    if (!s->bai_on) { gm_set_error("gm_sam_sorter_bai: call gm_sam_sorter_index_begin before the first gm_sam_sorter_read_bgzf"); return GM_E_ARG; }
    if (s->next_row < s->n_rows) {
        gm_set_error("gm_sam_sorter_bai: " + std::to_string(s->n_rows - s->next_row) + " of " + std::to_string(s->n_rows) + " rows are still unread: their places in the file are not known");
        return GM_E_ARG;
    }
    HIPCHK(hipSetDevice(s->ix->device));
    hipStream_t st = S_(stream);
    if (!s->bai_file) {
        uint64_t bytes = 0, chunks = 0;
        HIPCHK(hipEventRecord(s->bai_ev[0], st));
        const int rc = gm_bai_build(s->ix, s->bai, s->n_rows, [s](void** p, size_t b, const char* what) { return ss_alloc(s, p, b, what); }, &s->bai_file, &bytes, &chunks, stream);
        if (rc != GM_OK) { (void)hipStreamSynchronize(st); return rc; }
        float ms = 0;
        HIPCHK(hipEventRecord(s->bai_ev[1], st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventElapsedTime(&ms, s->bai_ev[0], s->bai_ev[1]));
        s->st.bai_ms += ms; s->st.bai_bytes = bytes; s->st.bai_chunks = chunks;
    }
    *n_out = s->st.bai_bytes;
    if (s->st.bai_bytes > cap || !out) {
        gm_set_error("gm_sam_sorter_bai: the index takes " + std::to_string(s->st.bai_bytes) + " bytes, the buffer holds " + std::to_string(cap));
        return GM_E_CAPACITY;
    }
    HIPCHK(hipMemcpyAsync(out, s->bai_file, (size_t)s->st.bai_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GM_OK;
}

// unit level: rows of the caller's under keys of the caller's, through the same claim / add as a block of gm_output_batch_sorted
extern "C" int gm_sam_sorter_add_rows(gm_sam_sorter* s, uint64_t seq, const char* text, const uint64_t* row_off, const uint32_t* contig, const uint64_t* chr_pos,
                                      uint64_t n_rows, void* stream) {
    if (!s || (n_rows && (!text || !row_off || !contig || !chr_pos))) return GM_E_ARG;
    if (n_rows > 0x7FFFFFFFull) { gm_set_error("gm_sam_sorter_add_rows: more than 2^31 - 1 rows in one call"); return GM_E_ARG; }
    for (uint64_t i = 0; i < n_rows; ++i)
        if (row_off[i + 1] < row_off[i]) { gm_set_error("gm_sam_sorter_add_rows: row offsets do not ascend"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(s->ix->device));
    if (const int rc = gm_samsort_claim(s, s->ix, seq)) return rc;
    if (!n_rows) return GM_OK;
    hipStream_t st = S_(stream);
    const uint64_t off0 = row_off[0], text_len = row_off[n_rows] - off0;
    std::vector<GmDevSamRec> recs(n_rows);
    std::vector<uint64_t> off(n_rows + 1);
    for (uint64_t i = 0; i < n_rows; ++i) { recs[i] = GmDevSamRec{}; recs[i].contig = contig[i]; recs[i].chr_pos = chr_pos[i]; }
    for (uint64_t i = 0; i <= n_rows; ++i) off[i] = row_off[i] - off0;
    Scoped<DevBuf> d_recs, d_off, d_text;
    int rc = GM_OK;
    if (d_recs.ensure(n_rows * sizeof(GmDevSamRec)) || d_off.ensure((n_rows + 1) * 8) || d_text.ensure((size_t)text_len + 16)) rc = GM_E_NOMEM;
    auto run = [&]() -> int {
        HIPCHK(hipMemcpyAsync(d_recs.p, recs.data(), n_rows * sizeof(GmDevSamRec), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off.p, off.data(), (n_rows + 1) * 8, hipMemcpyHostToDevice, st));
        if (text_len) HIPCHK(hipMemcpyAsync(d_text.p, text + off0, (size_t)text_len, hipMemcpyHostToDevice, st));
        if (const int r = gm_samsort_add(s, seq, d_recs.as<GmDevSamRec>(), nullptr, n_rows, n_rows, d_text.as<char>(), d_off.as<uint64_t>(), text_len, stream)) return r;
        HIPCHK(hipStreamSynchronize(st));
        return GM_OK;
    };
    if (rc == GM_OK) rc = run();
    if (rc != GM_OK) { (void)hipStreamSynchronize(st); gm_samsort_release(s, seq); }
    return rc;
}

extern "C" int gm_sam_sorter_stats(gm_sam_sorter* s, gm_sam_sort_stats* out) {
    if (!s || !out) return GM_E_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    *out = s->st;
    out->rows = s->n_rows; out->text_bytes = s->text_bytes; out->pieces = s->pieces.size();
    return GM_OK;
}
