// gm_bai.hip — the .bai (SAMv1 section 5.2) of a coordinate-sorted BAM, built where the sorter's slabs and their BGZF offsets are.
//
//   k_bai_rows    per slab, behind k_bgzf_deflate and the scan of the blocks' sizes: one lane per record - refID, pos, flag and the CIGAR
//                 are read from the record's bytes in the slab; the lane leaves the record's tuple in the per-row table: reference,
//                 position, bin | last window | unmapped bit, and the virtual offsets of its first byte and of the byte behind it
//   k_bai_order   at build time: the rows ascend in (refID as unsigned, pos)
//   k_bai_refs    the rows of every reference (its first and last row write), and where the rows without a reference start
//   k_bai_keys    per row: reference << 32 | last window (an inclusive max-scan of these is, the references ascending, the running
//                 maximum of the last window inside the reference), and whether (reference, bin) differs from the row before
//   k_bai_runs    the runs of equal (reference, bin): first row and sort key; a stable radix sort on reference << 16 | bin puts the
//                 runs of a bin side by side in file order; k_bai_sorted fetches their offsets, k_bai_flags marks bin heads and
//                 chunk heads (a run starts a chunk unless it begins in the compressed block in which the run before ends, or before)
//   k_bai_bins    first chunk of every bin, first bin / chunk of every reference
//   k_bai_sizes   per reference: n_intv from the running maximum of its last row, its bytes in the file
//   k_bai_lin     a row writes its own offset into the windows it is the first to cover; an inclusive max-scan fills the gaps
//   k_bai_write_refs / _runs / _lin   the little-endian file, every word at the offset the scans gave it
//
// Every kernel writes its row's own slot or a slot a scan assigned; the only atomics are integer minima (the first offending row).
// The bytes are a function of the records, the level and the file offset alone.
#include "gm_lib.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <algorithm>

namespace {

constexpr long long BAI_MAX_END = 1ll << 29;
constexpr uint32_t BAI_NONE = 0xFFFFFFFFu;          // the reference of a row without one
constexpr uint32_t BAI_PSEUDO_BIN = 37450;

__device__ __forceinline__ uint32_t bai_rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
__device__ __forceinline__ uint32_t bai_rd16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ void bai_put64(uint8_t* o, unsigned long long v) {          // o is 4-byte aligned
    reinterpret_cast<uint32_t*>(o)[0] = (uint32_t)v; reinterpret_cast<uint32_t*>(o)[1] = (uint32_t)(v >> 32);
}
__device__ __forceinline__ void bai_put32(uint8_t* o, uint32_t v) { *reinterpret_cast<uint32_t*>(o) = v; }

// rows [r0, r1) of the sorted order are the slab's bytes [0, bytes); offs[b] = where block b of the slab's nb starts among them
// compressed, offs[nb] = their total; file_off = where block 0 lies in the file
__global__ void __launch_bounds__(256) k_bai_rows(const uint8_t* __restrict__ slab, const unsigned long long* __restrict__ soff, uint32_t r0, uint32_t r1,
                                                  unsigned long long bytes, const unsigned long long* __restrict__ offs, uint32_t nb, unsigned long long file_off,
                                                  uint32_t n_ref, GmBaiRows t) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g >= r1 - r0) return;
    const uint32_t i = r0 + (uint32_t)g;
    const unsigned long long base = soff[r0], u = soff[i] - base, e = soff[i + 1] - base, len = e - u;
    const uint8_t* const p = slab + u;
    uint32_t ref = BAI_NONE, pk = 0;
    int32_t pos = -1;
    bool ok = len >= 36 && e <= bytes;
    if (ok) {
        const uint32_t l_name = p[12], n_ops = bai_rd16(p + 16), flag = bai_rd16(p + 18);
        ok = (unsigned long long)bai_rd32(p) + 4ull == len && 36ull + l_name + 4ull * n_ops <= len;
        if (ok) {
            const int32_t ref_id = (int32_t)bai_rd32(p + 4);
            pos = (int32_t)bai_rd32(p + 8);
            if (ref_id >= 0) {
                ref = (uint32_t)ref_id;
                unsigned long long ref_len = 0;
                const uint8_t* cg = p + 36 + l_name;
                for (uint32_t k = 0; k < n_ops; ++k) {
                    const uint32_t w = bai_rd32(cg + 4u * k), op = w & 15u;
                    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += w >> 4;       // M D N = X
                }
                const long long end = (long long)pos + (long long)(ref_len ? ref_len : 1ull);
                if (ref >= n_ref) atomicMin(&t.err[1], i);
                else if (pos < 0 || end > BAI_MAX_END) atomicMin(&t.err[2], i);
                else pk = gm_reg2bin(pos, end) | (uint32_t)((end - 1) >> 14) << 16 | ((flag & 4u) ? 0x80000000u : 0u);
            }
        }
    }
    if (!ok) atomicMin(&t.err[0], i);
    const uint32_t blk = (uint32_t)(u / GM_BGZF_PAYLOAD);
    const unsigned long long eb = e / GM_BGZF_PAYLOAD;
    t.vbeg[i] = (file_off + offs[blk < nb ? blk : nb]) << 16 | (u % GM_BGZF_PAYLOAD);
    t.vend[i] = e >= bytes || eb >= nb ? (file_off + offs[nb]) << 16 : (file_off + offs[eb]) << 16 | (e % GM_BGZF_PAYLOAD);
    t.ref[i] = ref; t.pos[i] = pos; t.pk[i] = pk;
}

__global__ void __launch_bounds__(256) k_bai_order(GmBaiRows t, uint32_t n) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g == 0 || g >= n) return;
    const uint32_t i = (uint32_t)g, a = t.ref[i - 1], b = t.ref[i];
    if (a > b || (a == b && a != BAI_NONE && t.pos[i - 1] > t.pos[i])) atomicMin(&t.err[3], i);
}

// row0[r], row1[r]: the rows of reference r (both 0: none); *placed = the first row without a reference (n: none)
__global__ void __launch_bounds__(256) k_bai_refs(const uint32_t* __restrict__ ref, uint32_t n, uint32_t n_ref, uint32_t* row0, uint32_t* row1, uint32_t* placed) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const uint32_t i = (uint32_t)g, r = ref[i];
    if (i == 0 || ref[i - 1] != r) { if (r < n_ref) row0[r] = i; else if (r == BAI_NONE) *placed = i; }
    if ((i + 1 == n || ref[i + 1] != r) && r < n_ref) row1[r] = i + 1;
}

// rows [0, m) have a reference.  head has m + 1 entries, the last one 0 (its exclusive scan ends in the number of runs)
__global__ void __launch_bounds__(256) k_bai_keys(GmBaiRows t, uint32_t m, unsigned long long* kx, uint32_t* head) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g > m) return;
    const uint32_t i = (uint32_t)g;
    if (i == m) { head[m] = 0; return; }
    const uint32_t r = t.ref[i], pk = t.pk[i];
    kx[i] = (unsigned long long)r << 32 | ((pk >> 16) & 0x7FFFu);
    head[i] = i == 0 || t.ref[i - 1] != r || ((t.pk[i - 1] ^ pk) & 0xFFFFu) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_bai_runs(GmBaiRows t, uint32_t m, const uint32_t* __restrict__ head, const uint32_t* __restrict__ run_ex, uint32_t n_runs,
                                                  uint32_t* run_row, unsigned long long* key, uint32_t* ord) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g >= m) return;
    const uint32_t i = (uint32_t)g;
    if (i == 0) run_row[n_runs] = m;
    if (!head[i]) return;
    const uint32_t q = run_ex[i];
    if (q >= n_runs) return;
    run_row[q] = i; ord[q] = q;
    key[q] = (unsigned long long)t.ref[i] << 16 | (t.pk[i] & 0xFFFFu);
}

__global__ void __launch_bounds__(256) k_bai_sorted(GmBaiRows t, uint32_t m, const uint32_t* __restrict__ ord, const uint32_t* __restrict__ run_row, uint32_t n_runs,
                                                    unsigned long long* sbeg, unsigned long long* send) {
    const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_runs) return;
    const uint32_t q = ord[k];
    if (q >= n_runs) return;
    const uint32_t a = run_row[q], b = run_row[q + 1];
    if (a >= b || b > m) return;
    sbeg[k] = t.vbeg[a]; send[k] = t.vend[b - 1];
}

// n_runs + 1 entries each, the last one 0
__global__ void __launch_bounds__(256) k_bai_flags(const unsigned long long* __restrict__ key, const unsigned long long* __restrict__ sbeg,
                                                   const unsigned long long* __restrict__ send, uint32_t n_runs, uint32_t* bin_head, uint32_t* chunk_head) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g > n_runs) return;
    const uint32_t k = (uint32_t)g;
    if (k == n_runs) { bin_head[k] = chunk_head[k] = 0; return; }
    const bool bh = k == 0 || key[k - 1] != key[k];
    bin_head[k] = bh ? 1u : 0u;
    chunk_head[k] = bh || (send[k - 1] >> 16) < (sbeg[k] >> 16) ? 1u : 0u;
}

struct BaiRefs {                                    // per reference; n_ref + 1 entries where a scan runs over them
    uint32_t *row0, *row1, *bin0, *bin1, *chunk0, *chunk1;
    unsigned long long *n_intv, *size, *lin_off, *ref_off;
};

// bin_ex / chunk_ex: the exclusive scans of the flags (n_runs + 1 entries): run k lies in bin bin_ex[k + 1] - 1, chunk chunk_ex[k + 1] - 1
__global__ void __launch_bounds__(256) k_bai_bins(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ bin_head, const uint32_t* __restrict__ bin_ex,
                                                  const uint32_t* __restrict__ chunk_ex, uint32_t n_runs, uint32_t n_ref, uint32_t* bin_chunk0, BaiRefs f) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g >= n_runs) return;
    const uint32_t k = (uint32_t)g, bid = bin_ex[k + 1] - 1u, cid = chunk_ex[k + 1] - 1u;
    const uint32_t r = (uint32_t)(key[k] >> 16);
    if (bid >= n_runs || r >= n_ref) return;
    if (bin_head[k]) bin_chunk0[bid] = cid;
    if (k + 1 == n_runs) bin_chunk0[bid + 1] = chunk_ex[n_runs];
    if (k == 0 || (uint32_t)(key[k - 1] >> 16) != r) { f.bin0[r] = bid; f.chunk0[r] = cid; }
    if (k + 1 == n_runs || (uint32_t)(key[k + 1] >> 16) != r) { f.bin1[r] = bid + 1u; f.chunk1[r] = cid + 1u; }
}

__global__ void __launch_bounds__(256) k_bai_sizes(BaiRefs f, uint32_t n_ref, const unsigned long long* __restrict__ rmax) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g > n_ref) return;
    const uint32_t r = (uint32_t)g;
    if (r == n_ref) { f.n_intv[r] = 0; f.size[r] = 0; return; }
    const bool has = f.row1[r] > f.row0[r];
    const unsigned long long ni = has ? (rmax[f.row1[r] - 1u] & 0xFFFFFFFFull) + 1ull : 0ull;
    f.n_intv[r] = ni;
    f.size[r] = 8ull + 8ull * (f.bin1[r] - f.bin0[r]) + 16ull * (f.chunk1[r] - f.chunk0[r]) + (has ? 40ull : 0ull) + 8ull * ni;
}

// rmax: the running maximum of the last window inside the reference (low 32 bits).  The rows ascend in pos, so the first row in file
// order that overlaps window w is the one at which the running maximum first reaches w - unless that row starts behind w
__global__ void __launch_bounds__(256) k_bai_lin(GmBaiRows t, uint32_t m, uint32_t n_ref, const unsigned long long* __restrict__ rmax, BaiRefs f,
                                                 unsigned long long n_win, unsigned long long* lin) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g >= m) return;
    const uint32_t i = (uint32_t)g, r = t.ref[i];
    if (r >= n_ref) return;
    const long long prev = i > f.row0[r] ? (long long)(rmax[i - 1] & 0xFFFFFFFFull) : -1ll;
    const long long w0 = t.pos[i] >> 14, w1 = (t.pk[i] >> 16) & 0x7FFFu;
    const unsigned long long at = f.lin_off[r], v = t.vbeg[i];
    for (long long w = prev + 1 > w0 ? prev + 1 : w0; w <= w1; ++w)
        if (at + (unsigned long long)w < n_win) lin[at + (unsigned long long)w] = v;
}

__global__ void __launch_bounds__(256) k_bai_write_refs(GmBaiRows t, BaiRefs f, uint32_t n_ref, const uint32_t* __restrict__ unm_incl, unsigned long long n_no_coor,
                                                        unsigned long long total, uint8_t* out) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g > n_ref) return;
    const uint32_t r = (uint32_t)g;
    if (r == n_ref) {
        bai_put32(out, 0x01494142u);                 // "BAI\1"
        bai_put32(out + 4, n_ref);
        bai_put64(out + total - 8, n_no_coor);
        return;
    }
    const uint32_t a = f.row0[r], b = f.row1[r], nb = f.bin1[r] - f.bin0[r], nc = f.chunk1[r] - f.chunk0[r];
    const bool has = b > a;
    if (8ull + f.ref_off[r] + f.size[r] + 8ull > total) return;
    uint8_t* o = out + 8 + f.ref_off[r];
    bai_put32(o, nb + (has ? 1u : 0u));
    o += 4ull + 8ull * nb + 16ull * nc;
    if (has) {
        const unsigned long long unm = unm_incl[b - 1] - (a ? unm_incl[a - 1] : 0u);
        bai_put32(o, BAI_PSEUDO_BIN); bai_put32(o + 4, 2u);
        bai_put64(o + 8, t.vbeg[a]); bai_put64(o + 16, t.vend[b - 1]);
        bai_put64(o + 24, (unsigned long long)(b - a) - unm); bai_put64(o + 32, unm);
        o += 40;
    }
    bai_put32(o, (uint32_t)f.n_intv[r]);
}

__global__ void __launch_bounds__(256) k_bai_write_runs(const unsigned long long* __restrict__ key, const unsigned long long* __restrict__ sbeg,
                                                        const unsigned long long* __restrict__ send, const uint32_t* __restrict__ bin_head,
                                                        const uint32_t* __restrict__ chunk_head, const uint32_t* __restrict__ bin_ex, const uint32_t* __restrict__ chunk_ex,
                                                        const uint32_t* __restrict__ bin_chunk0, uint32_t n_runs, uint32_t n_ref, BaiRefs f, unsigned long long total,
                                                        uint8_t* out) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g >= n_runs) return;
    const uint32_t k = (uint32_t)g, bid = bin_ex[k + 1] - 1u, cid = chunk_ex[k + 1] - 1u;
    const uint32_t r = (uint32_t)(key[k] >> 16);
    if (bid >= n_runs || r >= n_ref || bid < f.bin0[r] || cid < f.chunk0[r]) return;
    // the bin's 8-byte header lies in front of its first chunk
    const unsigned long long chunk_at = 8ull + f.ref_off[r] + 4ull + 8ull * (bid - f.bin0[r] + 1u) + 16ull * (cid - f.chunk0[r]);
    if (chunk_at + 16ull + 8ull > total) return;
    if (bin_head[k]) {
        bai_put32(out + chunk_at - 8, (uint32_t)(key[k] & 0xFFFFu));
        bai_put32(out + chunk_at - 4, bin_chunk0[bid + 1] - bin_chunk0[bid]);
    }
    if (chunk_head[k]) bai_put64(out + chunk_at, sbeg[k]);
    if (chunk_head[k + 1] || k + 1 == n_runs) bai_put64(out + chunk_at + 8, send[k]);
}

// lin is the gap-filled array of every reference's windows side by side: the windows in front of a reference's first record hold 0
__global__ void __launch_bounds__(256) k_bai_write_lin(GmBaiRows t, BaiRefs f, uint32_t n_ref, const unsigned long long* __restrict__ lin, unsigned long long n_win,
                                                       unsigned long long total, uint8_t* out) {
    const unsigned long long w = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (w >= n_win) return;
    uint32_t a = 0, b = n_ref;                       // the last reference whose windows start at or before w
    while (b - a > 1u) { const uint32_t mid = a + (b - a) / 2u; if (f.lin_off[mid] <= w) a = mid; else b = mid; }
    const unsigned long long local = w - f.lin_off[a];
    if (local >= f.n_intv[a] || f.row1[a] <= f.row0[a]) return;
    const unsigned long long at = 8ull + f.ref_off[a] + f.size[a] - 8ull * f.n_intv[a] + 8ull * local;
    if (at + 16ull > total) return;
    const unsigned long long first = (unsigned long long)(t.pos[f.row0[a]] >> 14);
    bai_put64(out + at, local < first ? 0ull : lin[w]);
}

struct BaiUnmapped { __host__ __device__ uint32_t operator()(uint32_t pk) const { return pk >> 31; } };

inline uint32_t bai_grid(uint64_t n) { return (uint32_t)((n + 255) / 256); }
uint32_t bai_bits(uint64_t v) { uint32_t b = 0; while (v >> b && b < 64) ++b; return b ? b : 1; }

struct BaiBuf {                                     // device memory from the caller's allocator, freed with the build
    void* p = nullptr; size_t cap = 0;
    ~BaiBuf() { if (p) (void)hipFree(p); }
    int get(const GmBaiAlloc& alloc, size_t bytes, const char* what) {
        if (bytes <= cap) return GM_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        if (const int rc = alloc(&p, bytes + 64, what)) return rc;
        cap = bytes + 64;
        return GM_OK;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// a rocPRIM call in its two steps: the size of its scratch, then the run
template <class F> int bai_prim(const GmBaiAlloc& alloc, BaiBuf& tmp, F&& call) {
    size_t need = 0;
    if (call(nullptr, need) != hipSuccess) { (void)hipGetLastError(); gm_set_error("BAM index: rocPRIM could not size its scratch"); return GM_E_HIP; }
    if (const int rc = tmp.get(alloc, need + 64, "the index's scans")) return rc;
    HIPCHK(call(tmp.p, need));
    return GM_OK;
}

}  // namespace

int gmk_bai_rows(const void* slab, const uint64_t* soff, uint64_t r0, uint64_t r1, uint64_t bytes, const uint64_t* offs, uint32_t nb, uint64_t file_off, uint32_t n_ref,
                 const GmBaiRows& t, void* stream) {
    if (r1 <= r0) return 0;
    hipLaunchKernelGGL(k_bai_rows, dim3(bai_grid(r1 - r0)), dim3(256), 0, S_(stream), (const uint8_t*)slab, (const unsigned long long*)soff, (uint32_t)r0, (uint32_t)r1,
                       (unsigned long long)bytes, (const unsigned long long*)offs, nb, (unsigned long long)file_off, n_ref, t);
    return (int)hipGetLastError();
}

uint64_t gm_bai_blocks(uint64_t bytes) { return (bytes + GM_BGZF_PAYLOAD - 1) / GM_BGZF_PAYLOAD; }

int gm_bai_build(const gm_index* ix, const GmBaiRows& t, uint64_t n_rows, const GmBaiAlloc& alloc, void** out, uint64_t* out_bytes, uint64_t* n_chunks, void* stream) {
    *out = nullptr; *out_bytes = 0; *n_chunks = 0;
    hipStream_t st = S_(stream);
    const auto& contigs = ix->h.contigs;
    const uint32_t n_ref = (uint32_t)contigs.size(), n = (uint32_t)n_rows;
    // ---- what k_bai_rows found, and the order ----
    if (n > 1) { hipLaunchKernelGGL(k_bai_order, dim3(bai_grid(n)), dim3(256), 0, st, t, n); HIPCHK(hipGetLastError()); }
    uint32_t err[4];
    HIPCHK(hipMemcpyAsync(err, t.err, sizeof err, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < 4; ++k) {
        if (err[k] == BAI_NONE) continue;
        uint32_t ref = 0; int32_t pos = 0;
        HIPCHK(hipMemcpy(&ref, t.ref + err[k], 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&pos, t.pos + err[k], 4, hipMemcpyDeviceToHost));
        const std::string where = "row " + std::to_string(err[k]) + " of the sorted order";
        const std::string rname = ref < n_ref ? contigs[ref].name : ref == BAI_NONE ? std::string("*") : "#" + std::to_string(ref);
        if (k == 0) { gm_set_error("BAM index: " + where + " is not a whole BAM record"); return GM_E_ARG; }
        if (k == 1) { gm_set_error("BAM index: " + where + " names reference " + std::to_string(ref) + ", the index has " + std::to_string(n_ref)); return GM_E_ARG; }
        if (k == 2) {
            gm_set_error("BAM index: the record of " + where + " on " + rname + " at position " + std::to_string((long long)pos + 1) +
                         " lies outside the .bai coordinate space: a record ends at or below 2^29 = " + std::to_string(BAI_MAX_END) + " (a .csi index is not written)");
            return GM_E_UNSUPPORTED;
        }
        gm_set_error("BAM index: the records are not in coordinate order: " + where + " (" + rname + ", position " + std::to_string((long long)pos + 1) +
                     ") sorts before the row in front of it - the sort keys disagree with the records");
        return GM_E_ARG;
    }
    // ---- per reference: its rows ----
    BaiBuf refs32, refs64, small, tmp;
    const size_t nr1 = (size_t)n_ref + 1;
    if (const int rc = refs32.get(alloc, nr1 * 6 * 4, "the index's per-reference counts")) return rc;
    if (const int rc = refs64.get(alloc, nr1 * 4 * 8, "the index's per-reference offsets")) return rc;
    if (const int rc = small.get(alloc, 64, "the index's totals")) return rc;
    HIPCHK(hipMemsetAsync(refs32.p, 0, nr1 * 6 * 4, st));
    HIPCHK(hipMemsetAsync(refs64.p, 0, nr1 * 4 * 8, st));
    BaiRefs f;
    f.row0 = refs32.as<uint32_t>(); f.row1 = f.row0 + nr1; f.bin0 = f.row1 + nr1; f.bin1 = f.bin0 + nr1; f.chunk0 = f.bin1 + nr1; f.chunk1 = f.chunk0 + nr1;
    f.n_intv = refs64.as<unsigned long long>(); f.size = f.n_intv + nr1; f.lin_off = f.size + nr1; f.ref_off = f.lin_off + nr1;
    uint32_t* const d_placed = small.as<uint32_t>();
    uint32_t m = n;                                  // rows [0, m) have a reference
    HIPCHK(hipMemcpyAsync(d_placed, &m, 4, hipMemcpyHostToDevice, st));
    if (n) {
        hipLaunchKernelGGL(k_bai_refs, dim3(bai_grid(n)), dim3(256), 0, st, (const uint32_t*)t.ref, n, n_ref, f.row0, f.row1, d_placed);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&m, d_placed, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (m > n) { gm_set_error("BAM index: the rows without a reference start behind the last row"); return GM_E_HIP; }
    }
    // ---- running maxima of the last window, unmapped counts, runs of equal (reference, bin) ----
    BaiBuf kx, unm, head, run_ex, run_row, key0, key1, ord0, ord1, sbeg, send, bin_head, chunk_head, bin_ex, chunk_ex, bin_chunk0;
    uint32_t n_runs = 0;
    if (m) {
        if (const int rc = kx.get(alloc, (size_t)m * 8, "the index's window maxima")) return rc;
        if (const int rc = unm.get(alloc, (size_t)m * 4, "the index's unmapped counts")) return rc;
        if (const int rc = head.get(alloc, ((size_t)m + 1) * 4, "the index's run heads")) return rc;
        if (const int rc = run_ex.get(alloc, ((size_t)m + 1) * 4, "the index's run numbers")) return rc;
        hipLaunchKernelGGL(k_bai_keys, dim3(bai_grid((uint64_t)m + 1)), dim3(256), 0, st, t, m, kx.as<unsigned long long>(), head.as<uint32_t>());
        HIPCHK(hipGetLastError());
        if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
                return rocprim::inclusive_scan(p, b, kx.as<unsigned long long>(), kx.as<unsigned long long>(), (size_t)m, rocprim::maximum<unsigned long long>(), st); })) return rc;
        if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
                return rocprim::inclusive_scan(p, b, rocprim::make_transform_iterator((const uint32_t*)t.pk, BaiUnmapped()), unm.as<uint32_t>(), (size_t)m, rocprim::plus<uint32_t>(), st); })) return rc;
        if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
                return rocprim::exclusive_scan(p, b, head.as<uint32_t>(), run_ex.as<uint32_t>(), 0u, (size_t)m + 1, rocprim::plus<uint32_t>(), st); })) return rc;
        HIPCHK(hipMemcpyAsync(&n_runs, run_ex.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!n_runs || n_runs > m) { gm_set_error("BAM index: " + std::to_string(n_runs) + " runs of bins for " + std::to_string(m) + " rows"); return GM_E_HIP; }
        const size_t R = n_runs;
        if (const int rc = run_row.get(alloc, (R + 1) * 4, "the index's runs")) return rc;
        if (const int rc = key0.get(alloc, R * 8, "the index's runs")) return rc;
        if (const int rc = key1.get(alloc, R * 8, "the index's runs")) return rc;
        if (const int rc = ord0.get(alloc, R * 4, "the index's runs")) return rc;
        if (const int rc = ord1.get(alloc, R * 4, "the index's runs")) return rc;
        if (const int rc = sbeg.get(alloc, R * 8, "the index's runs")) return rc;
        if (const int rc = send.get(alloc, R * 8, "the index's runs")) return rc;
        if (const int rc = bin_head.get(alloc, (R + 1) * 4, "the index's runs")) return rc;
        if (const int rc = chunk_head.get(alloc, (R + 1) * 4, "the index's runs")) return rc;
        if (const int rc = bin_ex.get(alloc, (R + 1) * 4, "the index's runs")) return rc;
        if (const int rc = chunk_ex.get(alloc, (R + 1) * 4, "the index's runs")) return rc;
        if (const int rc = bin_chunk0.get(alloc, (R + 1) * 4, "the index's runs")) return rc;
        HIPCHK(hipMemsetAsync(sbeg.p, 0, R * 8, st));
        HIPCHK(hipMemsetAsync(send.p, 0, R * 8, st));
        HIPCHK(hipMemsetAsync(bin_chunk0.p, 0, (R + 1) * 4, st));
        hipLaunchKernelGGL(k_bai_runs, dim3(bai_grid(m)), dim3(256), 0, st, t, m, (const uint32_t*)head.as<uint32_t>(), (const uint32_t*)run_ex.as<uint32_t>(), n_runs,
                           run_row.as<uint32_t>(), key0.as<unsigned long long>(), ord0.as<uint32_t>());
        HIPCHK(hipGetLastError());
        // stable: the runs of a bin keep file order
        if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
                return rocprim::radix_sort_pairs(p, b, key0.as<unsigned long long>(), key1.as<unsigned long long>(), ord0.as<uint32_t>(), ord1.as<uint32_t>(), R, 0u,
                                                 16u + bai_bits(n_ref), st); })) return rc;
        const unsigned long long* const key = key1.as<unsigned long long>();
        hipLaunchKernelGGL(k_bai_sorted, dim3(bai_grid(R)), dim3(256), 0, st, t, m, (const uint32_t*)ord1.as<uint32_t>(), (const uint32_t*)run_row.as<uint32_t>(), n_runs,
                           sbeg.as<unsigned long long>(), send.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_bai_flags, dim3(bai_grid(R + 1)), dim3(256), 0, st, key, (const unsigned long long*)sbeg.as<unsigned long long>(),
                           (const unsigned long long*)send.as<unsigned long long>(), n_runs, bin_head.as<uint32_t>(), chunk_head.as<uint32_t>());
        HIPCHK(hipGetLastError());
        if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
                return rocprim::exclusive_scan(p, b, bin_head.as<uint32_t>(), bin_ex.as<uint32_t>(), 0u, R + 1, rocprim::plus<uint32_t>(), st); })) return rc;
        if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
                return rocprim::exclusive_scan(p, b, chunk_head.as<uint32_t>(), chunk_ex.as<uint32_t>(), 0u, R + 1, rocprim::plus<uint32_t>(), st); })) return rc;
        hipLaunchKernelGGL(k_bai_bins, dim3(bai_grid(R)), dim3(256), 0, st, key, (const uint32_t*)bin_head.as<uint32_t>(), (const uint32_t*)bin_ex.as<uint32_t>(),
                           (const uint32_t*)chunk_ex.as<uint32_t>(), n_runs, n_ref, bin_chunk0.as<uint32_t>(), f);
        HIPCHK(hipGetLastError());
    }
    // ---- per reference: n_intv and its bytes; where its bytes and its windows start ----
    hipLaunchKernelGGL(k_bai_sizes, dim3(bai_grid(nr1)), dim3(256), 0, st, f, n_ref, (const unsigned long long*)kx.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
            return rocprim::exclusive_scan(p, b, f.size, f.ref_off, 0ull, nr1, rocprim::plus<unsigned long long>(), st); })) return rc;
    if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
            return rocprim::exclusive_scan(p, b, f.n_intv, f.lin_off, 0ull, nr1, rocprim::plus<unsigned long long>(), st); })) return rc;
    unsigned long long refs_bytes = 0, n_win = 0;
    uint32_t chunks = 0;
    HIPCHK(hipMemcpyAsync(&refs_bytes, f.ref_off + n_ref, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&n_win, f.lin_off + n_ref, 8, hipMemcpyDeviceToHost, st));
    if (n_runs) HIPCHK(hipMemcpyAsync(&chunks, chunk_ex.as<uint32_t>() + n_runs, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // what the counts allow at most: 32768 windows per reference, a bin and a chunk per run
    if (n_win > (unsigned long long)n_ref << 15 || refs_bytes > 48ull * n_ref + 24ull * n_runs + 8ull * n_win || refs_bytes < 8ull * n_ref || (refs_bytes & 3ull)) {
        gm_set_error("BAM index: the references' sizes sum to " + std::to_string(refs_bytes) + " bytes with " + std::to_string(n_win) + " windows"); return GM_E_HIP;
    }
    const unsigned long long total = 8ull + refs_bytes + 8ull;
    // ---- the linear index ----
    BaiBuf lin, file;
    if (n_win) {
        if (const int rc = lin.get(alloc, (size_t)n_win * 8, "the index's windows")) return rc;
        HIPCHK(hipMemsetAsync(lin.p, 0, (size_t)n_win * 8, st));
        hipLaunchKernelGGL(k_bai_lin, dim3(bai_grid(m)), dim3(256), 0, st, t, m, n_ref, (const unsigned long long*)kx.as<unsigned long long>(), f, n_win, lin.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        if (const int rc = bai_prim(alloc, tmp, [&](void* p, size_t& b) {
                return rocprim::inclusive_scan(p, b, lin.as<unsigned long long>(), lin.as<unsigned long long>(), (size_t)n_win, rocprim::maximum<unsigned long long>(), st); })) return rc;
    }
    // ---- the file ----
    if (const int rc = file.get(alloc, (size_t)total, "the index file")) return rc;
    HIPCHK(hipMemsetAsync(file.p, 0, (size_t)total, st));
    uint8_t* const o = file.as<uint8_t>();
    hipLaunchKernelGGL(k_bai_write_refs, dim3(bai_grid(nr1)), dim3(256), 0, st, t, f, n_ref, (const uint32_t*)unm.as<uint32_t>(), (unsigned long long)(n - m), total, o);
    HIPCHK(hipGetLastError());
    if (n_runs) {
        hipLaunchKernelGGL(k_bai_write_runs, dim3(bai_grid(n_runs)), dim3(256), 0, st, (const unsigned long long*)key1.as<unsigned long long>(),
                           (const unsigned long long*)sbeg.as<unsigned long long>(), (const unsigned long long*)send.as<unsigned long long>(),
                           (const uint32_t*)bin_head.as<uint32_t>(), (const uint32_t*)chunk_head.as<uint32_t>(), (const uint32_t*)bin_ex.as<uint32_t>(),
                           (const uint32_t*)chunk_ex.as<uint32_t>(), (const uint32_t*)bin_chunk0.as<uint32_t>(), n_runs, n_ref, f, total, o);
        HIPCHK(hipGetLastError());
    }
    if (n_win) {
        hipLaunchKernelGGL(k_bai_write_lin, dim3(bai_grid(n_win)), dim3(256), 0, st, t, f, n_ref, (const unsigned long long*)lin.as<unsigned long long>(), n_win, total, o);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));
    *out = file.p; file.p = nullptr;                 // the caller's from here on
    *out_bytes = total; *n_chunks = chunks;
    return GM_OK;
}
