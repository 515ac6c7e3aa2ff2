// gm_lib.h — what the host files of libgnumap_hip.so that hold a gm_index share (gm_api.cpp, gm_tracks.cpp): the error macros, the
// device / page-locked buffers, and the index itself.  Not part of the public ABI.
#pragma once
#include "gm_host.h"
#include <functional>
#include <map>
#include <mutex>

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            gm_set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                                  \
            return GM_E_HIP;                                                                                  \
        }                                                                                                     \
    } while (0)
#define KCHK(expr)                                                                                            \
    do {                                                                                                      \
        int e_ = (expr);                                                                                      \
        if (e_ != 0) {                                                                                        \
            gm_set_error(std::string(#expr) + ": " + hipGetErrorString((hipError_t)e_));                      \
            return GM_E_HIP;                                                                                  \
        }                                                                                                     \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return GM_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { gm_set_error(std::string("hipMalloc: ") + hipGetErrorString(e)); p = nullptr; return GM_E_NOMEM; }
        cap = want;
        return GM_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct PinBuf {                              // page-locked host staging: device <-> host copies at link rate, no zero fill
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return GM_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) { gm_set_error(std::string("hipHostMalloc: ") + hipGetErrorString(e)); p = nullptr; return GM_E_NOMEM; }
        cap = want;
        return GM_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

template <class B> struct Scoped : B { ~Scoped() { this->release(); } };       // a DevBuf / PinBuf that lives as long as one call

inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

struct gm_index {
    GmHostIndex h;
    int device = -1;
    bool host_only = false;
    bool full_sa = false;
    DevBuf d_bwt, d_sa, d_full, d_pac, d_contig, d_cov, d_ptab, d_planes, d_nuc;
    DevBuf d_cnames, d_cname_off;           // contig names back to back + n_seqs + 1 offsets: what k_out_text_rows prints (uploaded by the first gm_output_batch_text)
    bool cnames_on = false;
    DevBuf d_holes;                         // GmHostIndex::holes in HBM, for the walk of gm_batch_set_row_tags (uploaded by the first output call with the setting on)
    bool holes_on = false;
    bool nuc_on = false;
    GmDevIndex dev{};
    uint64_t cov_bins = 0;
    uint32_t cov_bin_size = 0;
    // parameter tables resident in HBM: S256 (256x4 floats) + lut (512 float2)
    std::map<std::vector<float>, DevBuf> ptabs;   // by content
    std::map<int, DevBuf> kmer_tabs;        // memoised backward search of the last T characters of a seed, per T
    std::map<int, DevBuf> kmer_ctabs;       // its compact form (16 B per 8 codes), per T
    std::map<int, DevBuf> buckets;          // k-mer -> positions records (128 B per code; gm_bucket.hip), per T; empty DevBuf = tried, no room
    std::mutex mu;
    uint64_t hbm_bytes = 0;
    int probe_format = GM_READS_FASTQ;      // gm_index_set_probe_format: how the unit probes read their gm_reads
    gm_track_text_stats tt_stats{};         // of the last gm_coverage_write_*_device / gm_coverage_text / gm_coverage_calls_text
};

unsigned host_threads();                                        // these three: gm_api.cpp.  GM_HOST_THREADS, else min(16, hardware threads); read once per process
uint32_t host_pos2rid(const GmHostIndex& h, uint64_t pos);      // the contig that holds a concatenated position
int index_cnames(gm_index* ix);                                 // contig names + offsets into HBM (d_cnames / d_cname_off), once per index
int index_holes(gm_index* ix);                                  // the holes of <fa>.gnumap.amb into HBM (d_holes), once per index
// gm_samsort.hip: what gm_output_batch_sorted (gm_api.cpp) does with a block besides gm_output_batch_text's work.  claim: the sequence number,
// before anything of the block is computed (GM_E_ARG: used before, the sorter is finished or belongs to another index).  add: the rows
// as k_out_text_rows left them in HBM - the records, n_rows + 1 offsets, the text - into the arena, on `stream` (GM_E_NOMEM, GM_E_UNSUPPORTED)
int gm_samsort_claim(gm_sam_sorter* s, const gm_index* ix, uint64_t seq);
void gm_samsort_release(gm_sam_sorter* s, uint64_t seq);     // the claim back, when the call failed before a row of the block was added
// row_src null: row k is record k.  Else GmDevText::row_src of the block: a row of a read without a record gets the key of a row without a contig
int gm_samsort_add(gm_sam_sorter* s, uint64_t seq, const GmDevSamRec* recs, const unsigned long long* row_src, uint64_t n_recs, uint64_t n_rows, const char* d_text,
                   const uint64_t* d_rowoff, uint64_t text_len, void* stream);
int gm_samsort_rows(gm_sam_sorter* s);                       // GM_ROWS_TEXT / GM_ROWS_BAM: what the blocks put into the arena

// gm_bam.hip and gm_bai.hip share these two.  The bytes of input per BGZF block, and the bin of [beg, end) (SAMv1 section 5.3)
constexpr uint32_t GM_BGZF_PAYLOAD = 65280;
__host__ __device__ inline uint32_t gm_reg2bin(long long beg, long long end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
// gm_bam.hip.  The record kernels run behind gmk_out_text_sizes on the same GmDevText: sizes overwrites row_len with the records' sizes
// and leaves (operations, bin) per record in meta; rows writes the records at row_off into t.text.
int gmk_bam_sizes(const GmDevText& t, uint32_t* meta, void* stream);
int gmk_bam_rows(const GmDevBatch& b, const GmDevText& t, const uint32_t* meta, void* stream);
// BGZF: the worst-case slots of the blocks, their sizes and the scan of those, and the blocks side by side
struct GmBgzfBufs {
    DevBuf slots, sizes, offs, tmp, out;
    DevBuf tokens;                          // GM_BGZF_LZ77: a payload's tokens per resident workgroup of k_bgzf_deflate_lz, from the first such call on
    uint32_t lz_wgs = 0;                    // those workgroups: the device's compute units (0: not asked yet)
    bool timed = false;                     // HIP events around k_bgzf_deflate + the scan and around k_bgzf_compact, summed into ms (one more wait per call)
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    double ms = 0; uint64_t in_bytes = 0, out_bytes = 0;
    void release();
};
uint64_t gm_bgzf_bound(uint64_t n);                          // the most bytes the blocks of n input bytes take: n + 31 per started 65280
uint64_t gm_bgzf_room(uint64_t cap);                         // the most input bytes whose blocks are sure to fit in cap
// d_in[0, n) in HBM -> z.out[0, *total); synchronises the stream.  level 0 stored, 1 Huffman, 1 | GM_BGZF_LZ77 Huffman over LZ77 matches
inline bool gm_bgzf_level_ok(int level) { return level == 0 || level == 1 || level == (1 | GM_BGZF_LZ77); }
std::string gm_bgzf_level_text(int level);                   // "the level is ..., not <level>", for the GM_E_ARG of every entry point that takes one
int gm_bgzf_device(const void* d_in, uint64_t n, int level, GmBgzfBufs& z, uint64_t* total, void* stream);

// gm_bai.hip.  The per-row table of a sorted BAM's index, one entry per row of the sorted order: the virtual offsets of the record's
// first byte and of the byte behind it, its reference (~0: none), its position, and bin | last 16 kbp window << 16 | unmapped << 31.
// err[0 .. 3]: the first row that is no whole record / names no reference of the index / ends beyond 2^29 / breaks the order (~0: none)
struct GmBaiRows {
    unsigned long long* vbeg; unsigned long long* vend;
    uint32_t* ref; int32_t* pos; uint32_t* pk; uint32_t* err;
};
using GmBaiAlloc = std::function<int(void** p, size_t bytes, const char* what)>;      // the sorter's ss_alloc
uint64_t gm_bai_blocks(uint64_t bytes);                      // the BGZF blocks of a slab of that many bytes
// rows [r0, r1) of the sorted order lie in slab[0, bytes), compressed into nb blocks at offs[] (nb + 1 entries) from file_off: their entries
int gmk_bai_rows(const void* slab, const uint64_t* soff, uint64_t r0, uint64_t r1, uint64_t bytes, const uint64_t* offs, uint32_t nb, uint64_t file_off, uint32_t n_ref,
                 const GmBaiRows& t, void* stream);
// the finished file in HBM (*out, the caller's to hipFree); GM_E_ARG / GM_E_UNSUPPORTED for what err[] holds.  Synchronises the stream
int gm_bai_build(const gm_index* ix, const GmBaiRows& t, uint64_t n_rows, const GmBaiAlloc& alloc, void** out, uint64_t* out_bytes, uint64_t* n_chunks, void* stream);
