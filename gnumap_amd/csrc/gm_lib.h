// gm_lib.h — what the host files of libgnumap_hip.so that hold a gm_index share (gm_api.cpp, gm_tracks.cpp): the error macros, the
// device / page-locked buffers, and the index itself.  Not part of the public ABI.
#pragma once
#include "gm_host.h"
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
// gm_samsort.hip: what gm_output_batch_sorted (gm_api.cpp) does with a block besides gm_output_batch_text's work.  claim: the sequence number,
// before anything of the block is computed (GM_E_ARG: used before, the sorter is finished or belongs to another index).  add: the rows
// as k_out_text_rows left them in HBM - the records, n_rows + 1 offsets, the text - into the arena, on `stream` (GM_E_NOMEM, GM_E_UNSUPPORTED)
int gm_samsort_claim(gm_sam_sorter* s, const gm_index* ix, uint64_t seq);
void gm_samsort_release(gm_sam_sorter* s, uint64_t seq);     // the claim back, when the call failed before a row of the block was added
int gm_samsort_add(gm_sam_sorter* s, uint64_t seq, const GmDevSamRec* recs, uint64_t n_rows, const char* d_text, const uint64_t* d_rowoff, uint64_t text_len, void* stream);
