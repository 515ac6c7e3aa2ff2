// gm_tracks.cpp — the coverage track of an index and the files written from it: <out>.sgr, the eight- and nine-column <out>.gmp and
// <out>.vcf (GenomeBwt::PrintFinalSGR / PrintFinalBisulfite / PrintFinalSNP / PrintSNPCall src/GenomeBwt.cpp:930-1273, Genome::PrintFinalVCF
// src/Genome.cpp:1142-1245).  The host writers format with one row emitter (TrackRows); the device writers run the kernels of
// gm_tracktext.hip, whose contract is that emitter's bytes, and hand a slab they cannot print to it.  No kernel lives here.
#include "gm_lib.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <thread>
#include <fcntl.h>
#include <unistd.h>

extern "C" int gm_coverage_reset(gm_index* ix, uint32_t bin_size) {
    if (!ix || bin_size == 0) return GM_E_ARG;
    const uint64_t bins = ix->h.l_pac / bin_size + 64;  // the reference allocates l_pac/gGEN_SIZE floats and writes a little past it
    if (!ix->host_only) {                               // host-only: no track in HBM, only the geometry the text writers need (CPU-side tests of gm_coverage_write_*)
        HIPCHK(hipSetDevice(ix->device));
        if (ix->d_cov.ensure(bins * 4)) return GM_E_NOMEM;
        HIPCHK(hipMemset(ix->d_cov.p, 0, bins * 4));
    }
    ix->cov_bins = bins; ix->cov_bin_size = bin_size;
    return GM_OK;
}

extern "C" uint64_t gm_coverage_bins(const gm_index* ix) { return ix ? ix->cov_bins : 0; }
extern "C" void* gm_coverage_device_ptr(gm_index* ix) { return ix ? ix->d_cov.p : nullptr; }

extern "C" int gm_coverage_add(gm_index* ix, const uint64_t* pos, const uint32_t* span, const float* w, uint32_t n, void* stream) {
    if (!ix || !pos || !span || !w) return GM_E_ARG;
    if (!ix->cov_bins) { gm_set_error("coverage track not initialised (gm_coverage_reset)"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(ix->device));
    if (n == 0) return GM_OK;
    Scoped<DevBuf> dp_, ds_, dw_;
    if (dp_.ensure((size_t)n * 8) || ds_.ensure((size_t)n * 4) || dw_.ensure((size_t)n * 4)) return GM_E_NOMEM;
    uint32_t max_span = 0;
    for (uint32_t i = 0; i < n; ++i) max_span = std::max(max_span, span[i]);
    hipStream_t st = S_(stream);
    if (hipMemcpyAsync(dp_.p, pos, (size_t)n * 8, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(ds_.p, span, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(dw_.p, w, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        gmk_coverage_add(ix->d_cov.as<float>(), ix->cov_bins, ix->cov_bin_size, dp_.as<uint64_t>(), ds_.as<uint32_t>(), dw_.as<float>(), n, max_span, nullptr, nullptr, nullptr, st) ||
        hipStreamSynchronize(st) != hipSuccess) { gm_set_error("gm_coverage_add: HIP failure"); return GM_E_HIP; }
    return GM_OK;
}

extern "C" int gm_coverage_download(gm_index* ix, float* host) {
    if (!ix || !host || !ix->cov_bins) return GM_E_ARG;
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemcpy(host, ix->d_cov.p, ix->cov_bins * 4, hipMemcpyDeviceToHost));
    return GM_OK;
}

extern "C" int gm_coverage_enable_nuc(gm_index* ix) {
    if (!ix || !ix->cov_bins) { gm_set_error("gm_coverage_reset first"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(ix->device));
    if (ix->d_nuc.ensure(5 * ix->cov_bins * 4)) return GM_E_NOMEM;
    HIPCHK(hipMemset(ix->d_nuc.p, 0, 5 * ix->cov_bins * 4));
    ix->nuc_on = true;
    return GM_OK;
}

extern "C" void* gm_coverage_nuc_device_ptr(gm_index* ix) { return ix && ix->nuc_on ? ix->d_nuc.p : nullptr; }

extern "C" int gm_coverage_download_nuc(gm_index* ix, float* host) {
    if (!ix || !host || !ix->nuc_on) return GM_E_ARG;
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemcpy(host, ix->d_nuc.p, 5 * ix->cov_bins * 4, hipMemcpyDeviceToHost));
    return GM_OK;
}

namespace {
// GM_TRACK_SLICE: the one size option of every writer below, read here and nowhere else.  Tests set it small to take a small index through
// several slices, slabs and launches; unset, every use keeps the default it was measured with:
//   host_slice_bins        bins one host thread formats and writes at a time (write_track_text); default 2^20.  x host_threads() = the bins
//                          of one round of write_track_text, which is the slab gm_coverage_write_gmp_calls brings down
//   snp_launch_positions   x 16: positions per k_snp_call / k_snp_gather launch of snp_calls_range
//   vcf_stretch_positions  positions gm_coverage_write_vcf asks snp_calls_range for at a time: one launch's worth
//   device_slab_bins       bins per slab of the device writers (TrackTextRun); default 2^24, never above 2^26
uint64_t track_slice(long long dflt) { return (uint64_t)std::max<long long>(1, gm_opt_ll("GM_TRACK_SLICE", dflt)); }
uint64_t host_slice_bins() { return track_slice(1ll << 20); }
uint64_t snp_launch_positions() { return host_slice_bins() * 16; }
uint64_t vcf_stretch_positions() { return snp_launch_positions(); }
uint64_t device_slab_bins() { return std::min<uint64_t>(track_slice(1ll << 24), 1ull << 26); }

std::string call_prefix(const char* call) { return call ? std::string(call) + ": " : std::string(); }      // errors under the caller's name, where it has one

// ---- track text at memory speed ------------------------------------------------------------------------------------------------------
// printf("%.Nf") of a float bin, N = 5 or 6, without printf: a float has 24 significant bits, so value x 10^N is exact in a double for
// every value below 2^53 / 10^N x 2^-17 (far beyond any coverage), and rint() of an exact number in the default rounding mode is the
// correctly rounded decimal glibc's printf prints (ties to even included).  Larger or non-finite values take snprintf.
// This is the specification of tt_fixed (gm_tracktext.hip).
inline char* put_fixed(char* w, float v, int decimals) {
    const double scale = decimals == 5 ? 100000.0 : 1000000.0;
    if (!(v >= 0.0f) || !(v < 1.0e9f)) return w + snprintf(w, 64, decimals == 5 ? "%.5f" : "%f", v);
    const uint64_t q = (uint64_t)rint((double)v * scale);
    const uint64_t ip = q / (uint64_t)scale; uint32_t fp = (uint32_t)(q % (uint64_t)scale);
    char tmp[24]; int k = 0;
    uint64_t t = ip;
    do { tmp[k++] = (char)('0' + t % 10); t /= 10; } while (t);
    while (k) *w++ = tmp[--k];
    *w++ = '.';
    for (int d = decimals - 1; d >= 0; --d) { w[d] = (char)('0' + fp % 10); fp /= 10; }
    return w + decimals;
}
inline char* put_long(char* w, long v) {
    if (v < 0) { *w++ = '-'; v = -v; }
    char tmp[24]; int k = 0;
    do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) *w++ = tmp[--k];
    return w;
}

// PrintSNPCall's column (src/GenomeBwt.cpp:1011-1090) of position `count` from k_snp_call's code byte cd and p-value
inline char* put_call(char* w, const GmHostIndex& h, uint64_t count, unsigned cd, double pval) {
    const unsigned at = (h.pac[count >> 2] >> ((~count & 3) << 1)) & 3, p1 = cd & 7u, dip = (cd >> 5) & 1u, r2 = (cd >> 3) & 3u;
    *w++ = '\t'; *w++ = (cd & 0x40) ? 'Y' : 'N';
    if (p1 != at || dip) {                                                // :1065-1085
        *w++ = ':'; *w++ = "acgt"[at]; *w++ = '-'; *w++ = '>'; *w++ = "acgtn"[p1];
        if (dip) { *w++ = '/'; *w++ = "acgtn"[r2 + (r2 >= p1 ? 1u : 0u)]; }
        w += snprintf(w, 40, " p_val=%.2e", pval);
    }
    return w;
}

// The rows of a track file, kind = GM_TRACK_*: the emitter of every host writer and of the device writers' fallback.  bins[k - base] is
// bin k, nuc[q * nuc_stride + k - base] its sum q, code / pval[k - base] its call (GM_TRACK_CALLS only); a writer that holds one slab of the
// tracks passes the slab's first bin as base.  want: the reference base of GM_TRACK_BASE
struct TrackRows {
    const GmHostIndex* h; uint64_t bs; int kind; char want;
    const float* bins; const float* nuc; uint64_t nuc_stride, base;
    const uint8_t* code; const double* pval;
    // the row of bin k, if it has one; i = the contig cursor of the run of bins that k continues
    char* row(uint64_t k, char* w, int& i) const {
        // the reference walks `count` over the concatenated coordinate in steps of bin_size without resetting it per contig,
        // so bin k is printed under the contig that holds k * bin_size
        const uint64_t count = k * bs;
        while ((size_t)i + 1 < h->contigs.size() && count >= h->contigs[(size_t)i + 1].offset) ++i;
        const float total = bins[k - base];
        if (kind == GM_TRACK_SGR) { if (!((double)total > 0.001)) return w; }       // MIN_PRINT, GenomeBwt.cpp:928
        else if (kind != GM_TRACK_BASE) { if (!(total > 0.001f)) return w; }        // --snp, with and without the call column
        else {
            const char at = "acgt"[(h->pac[count >> 2] >> ((~count & 3) << 1)) & 3];
            if (at != want || !(total > 0.0f)) return w;
        }
        const GmContig& cg = h->contigs[(size_t)i];
        memcpy(w, cg.name.data(), cg.name.size()); w += cg.name.size();
        *w++ = '\t'; w = put_long(w, (long)(count - cg.offset) + 1); *w++ = '\t';
        w = put_fixed(w, total, kind == GM_TRACK_BASE ? 6 : 5);                     // "%f" of the total in the base-filtered .gmp
        if (kind != GM_TRACK_SGR) for (int q = 0; q < 5; ++q) { *w++ = '\t'; w = put_fixed(w, nuc[(uint64_t)q * nuc_stride + k - base], 5); }
        if (kind == GM_TRACK_CALLS) w = put_call(w, *h, count, code[k - base], pval[k - base]);
        *w++ = '\n';
        return w;
    }
    // the rows of bins [lo, hi) into w, which has max_line() bytes per bin; the end of the text.  rows, if given, counts them
    char* range(uint64_t lo, uint64_t hi, char* w, uint64_t* rows = nullptr) const {
        int i = (int)host_pos2rid(*h, lo * bs);
        for (uint64_t k = lo; k < hi; ++k) { char* const w2 = row(k, w, i); if (rows) *rows += w2 != w; w = w2; }
        return w;
    }
    // Bytes of buffer per bin: the contig name and, with 22 = tab, a position of up to 20 digits, tab; 16 = put_fixed's longest own
    // number (9 digits below 1e9, the point, 6 decimals); 24 = the longest call column "\tY:a->c/g p_val=1.00e-05" (26: three-digit exponent)
    //   .sgr 48 >= 22 + 16 + newline = 39     .gmp 160 >= 22 + 6 x 16 + 5 tabs + newline = 124     calls 208 = 160 + 48 >= 124 + 26 = 150
    // The rest (9, 36, 58 bytes) is for numbers that take snprintf: "inf" / "nan" fit anywhere, a finite float of 1e9 and more has up to 46
    // bytes ("%f" of FLT_MAX; 47 with a sign).  The buffer holds the budget for EVERY bin of a slice, printed or not, so such rows fit as
    // long as they are few; a slice whose every number is that large would not, and sums of alignment posteriors never come near it.
    size_t max_line() const {
        size_t name = 0;
        for (const auto& c : h->contigs) name = std::max(name, c.name.size());
        return name + (kind == GM_TRACK_SGR ? 48 : kind == GM_TRACK_CALLS ? 208 : 160);
    }
};
char gmp_want(int mode) { return mode == GM_MODE_BS ? 'c' : mode == GM_MODE_BS2 ? 'g' : mode == GM_MODE_ATOG ? 'a' : 't'; }

// fn(0 .. parts - 1) at the same time: parts - 1 threads and the caller
template <class F> void run_parts(unsigned parts, F&& fn) {
    std::vector<std::thread> th;
    for (unsigned c = 1; c < parts; ++c) th.emplace_back(std::ref(fn), c);
    fn(0u);
    for (auto& x : th) x.join();
}

// where the text goes: a file at a running offset, or the first cap bytes into the caller's buffer; `total` counts everything
struct TrackSink {
    int fd = -1; uint64_t file_off = 0;
    char* mem = nullptr; uint64_t cap = 0, total = 0;
    ~TrackSink() { if (fd >= 0) ::close(fd); }
    // no O_APPEND: on Linux pwrite() on an O_APPEND descriptor ignores its offset, and write_track_text writes its slices concurrently
    bool open(const char* path, int append) {
        fd = ::open(path, O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0644);
        if (fd >= 0 && append) file_off = (uint64_t)lseek(fd, 0, SEEK_END);
        return fd >= 0;
    }
    bool write_at(const char* q, uint64_t n, uint64_t at) const {          // any thread, any offset
        while (n) { const ssize_t k = ::pwrite(fd, q, (size_t)n, (off_t)at); if (k <= 0) return false; q += k; n -= (uint64_t)k; at += (uint64_t)k; }
        return true;
    }
    uint64_t room() const { return fd >= 0 ? ~0ull : (cap > total ? cap - total : 0); }
    bool put(const char* q, uint64_t n) {                    // host text, behind what is there
        if (fd >= 0) { if (!write_at(q, n, file_off)) return false; file_off += n; }
        else if (const uint64_t m = std::min(n, room())) memcpy(mem + total, q, (size_t)m);
        total += n;
        return true;
    }
};

// bins [0, nb) through e in rounds: host_threads() threads format one slice of host_slice_bins() each and write it at its offset.
// slab(lo, hi) runs before the bins [lo, hi) of a round are formatted (a writer fetches them from HBM there and points e at them); non-zero ends the file
template <class Slab> int write_track_text(const char* path, int append, uint64_t nb, const TrackRows& e, Slab&& slab) {
    TrackSink out;
    if (!out.open(path, append)) { gm_set_error(std::string("cannot write ") + path); return GM_E_IO; }
    const unsigned T = host_threads();
    const uint64_t per = host_slice_bins();
    const size_t max_line = e.max_line();
    std::vector<std::vector<char>> buf(T);
    std::vector<size_t> used(T), off(T);
    std::atomic<int> bad{ 0 };
    for (uint64_t s0 = 0; s0 < nb && !bad; s0 += per * T) {
        const unsigned parts = (unsigned)std::min<uint64_t>(T, (nb - s0 + per - 1) / per);
        if (const int rc = slab(s0, std::min<uint64_t>(nb, s0 + per * T))) return rc;
        run_parts(parts, [&](unsigned c) {
            const uint64_t lo = s0 + c * per, hi = std::min<uint64_t>(nb, lo + per);
            std::vector<char>& o = buf[c];
            if (o.size() < (size_t)(hi - lo) * max_line) o.resize((size_t)(hi - lo) * max_line);
            used[c] = (size_t)(e.range(lo, hi, o.data()) - o.data());
        });
        for (unsigned c = 0; c < parts; ++c) { off[c] = out.file_off; out.file_off += used[c]; }
        run_parts(parts, [&](unsigned c) { if (!out.write_at(buf[c].data(), used[c], off[c])) bad = 1; });
    }
    if (bad) { gm_set_error(std::string("write failed: ") + path); return GM_E_IO; }
    return GM_OK;
}
}  // namespace

extern "C" int gm_coverage_write_sgr(gm_index* ix, const float* bins, const char* path, int append) {
    // GenomeBwt::PrintFinalSGR src/GenomeBwt.cpp:1212-1273: bins run over the CONCATENATED coordinate
    if (!ix || !bins || !path || !ix->cov_bin_size) return GM_E_ARG;
    const uint64_t bs = ix->cov_bin_size;
    const TrackRows e{ &ix->h, bs, GM_TRACK_SGR, 0, bins, nullptr, 0, 0, nullptr, nullptr };
    return write_track_text(path, append, (ix->h.l_pac + bs - 1) / bs, e, [](uint64_t, uint64_t) { return 0; });
}

extern "C" int gm_coverage_write_gmp(gm_index* ix, const gm_params* p, const float* bins, const float* nuc, const char* path, int append) {
    // GenomeBwt::PrintFinalBisulfite src/GenomeBwt.cpp:1092-1210
    if (!ix || !p || !bins || !nuc || !path || !ix->cov_bin_size || p->mode == GM_MODE_NORMAL) return GM_E_ARG;
    const uint64_t bs = ix->cov_bin_size;
    // GM_MODE_SNP: GenomeBwt::PrintFinalSNP src/GenomeBwt.cpp:930-1090 up to the per-nucleotide columns: every position whose total is above MIN_PRINT,
    // "%.5f" for all six numbers.  The line ends here; gm_coverage_write_gmp_calls writes the same rows with PrintSNPCall's column behind them.
    const TrackRows e{ &ix->h, bs, p->mode == GM_MODE_SNP ? GM_TRACK_SNP : GM_TRACK_BASE, gmp_want(p->mode), bins, nuc, ix->cov_bins, 0, nullptr, nullptr };
    return write_track_text(path, append, (ix->h.l_pac + bs - 1) / bs, e, [](uint64_t, uint64_t) { return 0; });
}

// ------------------------------------------------------------------------------------------------
// --snp: the likelihood-ratio column (gm_snpcall.hip)
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(gm_snp_rec) == sizeof(GmDevSnpRec) && sizeof(gm_snp_rec) == 64 && offsetof(gm_snp_rec, chr_pos) == offsetof(GmDevSnpRec, chr_pos) &&
              offsetof(gm_snp_rec, total) == offsetof(GmDevSnpRec, total) && offsetof(gm_snp_rec, nuc) == offsetof(GmDevSnpRec, nuc) &&
              offsetof(gm_snp_rec, p_val) == offsetof(GmDevSnpRec, p_val) && offsetof(gm_snp_rec, ref) == offsetof(GmDevSnpRec, ref) &&
              offsetof(gm_snp_rec, diploid) == offsetof(GmDevSnpRec, diploid), "gm_snp_rec layout");

namespace {
// what every entry point that calls SNPs asks of the tracks: bin size 1 (Driver.cpp:3207-3211 forces it with --snp), the five sums
// enabled, a device.  call = the name the error carries, null for gm_snp_calls and gm_coverage_write_gmp_calls, which carry none
int snp_tracks_ready(gm_index* ix, const char* call) {
    if (!ix->cov_bins || ix->cov_bin_size != 1) { gm_set_error(call_prefix(call) + "SNP calls need the coverage track with bin size 1 (gm_coverage_reset(ix, 1))"); return GM_E_ARG; }
    if (!ix->host_only && !ix->nuc_on) { gm_set_error(call_prefix(call) + "SNP calls read the per-nucleotide tracks: call gm_coverage_enable_nuc first"); return GM_E_ARG; }
    if (ix->host_only) { gm_set_error(call_prefix(call) + "no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    return GM_OK;
}

// the 'Y' rows of the positions [p_lo, p_hi) (clamped to the reference): gm_snp_calls is the whole range, gm_coverage_write_vcf fetches in pieces
int snp_calls_range(gm_index* ix, float snp_pval, int monop, uint64_t p_lo, uint64_t p_hi, gm_snp_rec* out, uint64_t cap, uint64_t* n_out, void* stream) {
    HIPCHK(hipSetDevice(ix->device));
    hipStream_t st = S_(stream);
    const uint64_t l_pac = std::min<uint64_t>(ix->h.l_pac, p_hi), bins = ix->cov_bins;
    const uint64_t per = snp_launch_positions();
    const uint32_t groups = gmk_snp_call_groups(std::min(per, l_pac));
    Scoped<DevBuf> d_code, d_pval, d_cnt, d_off, d_out;
    if (d_code.ensure(per) || d_pval.ensure(per * 8) || d_cnt.ensure((size_t)groups * 4 + 4) || d_off.ensure(((size_t)groups + 1) * 8) ||
        d_out.ensure((size_t)std::max<uint64_t>(cap, 1) * sizeof(GmDevSnpRec))) return GM_E_NOMEM;
    unsigned long long total = 0;
    for (uint64_t lo = p_lo; lo < l_pac; lo += per) {
        const uint64_t n = std::min(per, l_pac - lo);
        KCHK(gmk_snp_call(ix->d_cov.as<float>(), ix->d_nuc.as<float>(), bins, ix->dev, lo, n, snp_pval, monop ? 1 : 0, d_code.as<uint8_t>(), d_pval.as<double>(),
                          d_cnt.as<uint32_t>(), st));
        KCHK(gmk_snp_gather(ix->d_cov.as<float>(), ix->d_nuc.as<float>(), bins, ix->dev, lo, n, d_code.as<uint8_t>(), d_pval.as<double>(), d_cnt.as<uint32_t>(),
                            d_off.as<unsigned long long>(), total, cap, d_out.as<GmDevSnpRec>(), st));
        unsigned long long got = 0;
        HIPCHK(hipMemcpyAsync(&got, d_off.as<unsigned long long>() + gmk_snp_call_groups(n), 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        total += got;
    }
    const uint64_t have = std::min<uint64_t>(total, cap);
    if (have) HIPCHK(hipMemcpy(out, d_out.p, (size_t)have * sizeof(gm_snp_rec), hipMemcpyDeviceToHost));
    *n_out = total;
    if (total > cap) { gm_set_error("gm_snp_calls: out[] too small"); return GM_E_CAPACITY; }
    return GM_OK;
}
}  // namespace

extern "C" int gm_snp_calls(gm_index* ix, float snp_pval, int monop, gm_snp_rec* out, uint64_t cap, uint64_t* n_out, void* stream) {
    if (!ix || !n_out || (cap && !out)) return GM_E_ARG;
    if (const int rc = snp_tracks_ready(ix, nullptr)) return rc;
    return snp_calls_range(ix, snp_pval, monop, 0, ~0ull, out, cap, n_out, stream);
}

extern "C" int gm_dev_snp_stat(gm_index* ix, const float* counts, uint32_t n, int monop, double* p_val, int8_t* pos1, int8_t* pos2, uint8_t* dip) {
    if (!ix || !counts || !p_val || !pos1 || !pos2 || !dip) return GM_E_ARG;
    if (ix->host_only) { gm_set_error("no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (n == 0) return GM_OK;
    HIPCHK(hipSetDevice(ix->device));
    Scoped<DevBuf> d_in, d_p, d_1, d_2, d_d;
    if (d_in.ensure((size_t)n * 20) || d_p.ensure((size_t)n * 8) || d_1.ensure(n) || d_2.ensure(n) || d_d.ensure(n)) return GM_E_NOMEM;
    HIPCHK(hipMemcpy(d_in.p, counts, (size_t)n * 20, hipMemcpyHostToDevice));
    KCHK(gmk_snp_stat(d_in.as<float>(), n, monop ? 1 : 0, d_p.as<double>(), d_1.as<int8_t>(), d_2.as<int8_t>(), d_d.as<uint8_t>(), nullptr));
    HIPCHK(hipMemcpy(p_val, d_p.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pos1, d_1.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pos2, d_2.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dip, d_d.p, n, hipMemcpyDeviceToHost));
    return GM_OK;
}

namespace {
// what a writer that reads the tracks in HBM prints: the kind of row, the reference base of GM_TRACK_BASE, k_snp_call's settings of GM_TRACK_CALLS
struct TrackJob { int kind; char want; float snp_pval; int monop; };

// One slab of the tracks on the host, bins [lo, lo + n): the total with the sums behind it (n floats apart; none for an .sgr) and, for
// GM_TRACK_CALLS, k_snp_call's code bytes and p-values, which call() leaves in HBM.  Page-locked and kept from slab to slab:
// gm_coverage_write_gmp_calls streams the whole reference through it.
struct HostSlab {
    Scoped<DevBuf> d_code, d_pval, d_cnt;
    Scoped<PinBuf> h_f, h_code, h_pval;
    uint64_t lo = 0, n = 0;
    int reserve(uint64_t len) { return d_code.ensure(len) || d_pval.ensure(len * 8) || d_cnt.ensure((size_t)gmk_snp_call_groups(len) * 4 + 4) ? GM_E_NOMEM : GM_OK; }
    // k_snp_call over the slab that fetch() is to bring down
    int call(gm_index* ix, const TrackJob& job, uint64_t s0, uint64_t len, hipStream_t s) {
        if (const int rc = reserve(len)) return rc;
        KCHK(gmk_snp_call(ix->d_cov.as<float>(), ix->d_nuc.as<float>(), ix->cov_bins, ix->dev, s0, len, job.snp_pval, job.monop ? 1 : 0, d_code.as<uint8_t>(), d_pval.as<double>(),
                          d_cnt.as<uint32_t>(), s));
        return GM_OK;
    }
    int fetch(gm_index* ix, int kind, uint64_t s0, uint64_t len) {
        const uint64_t cols = kind == GM_TRACK_SGR ? 1 : 6;
        if (h_f.ensure(len * 4 * cols)) return GM_E_NOMEM;
        lo = s0; n = len;
        HIPCHK(hipMemcpy(h_f.p, ix->d_cov.as<float>() + lo, n * 4, hipMemcpyDeviceToHost));
        for (uint64_t q = 1; q < cols; ++q) HIPCHK(hipMemcpy(h_f.as<float>() + q * n, ix->d_nuc.as<float>() + (q - 1) * ix->cov_bins + lo, n * 4, hipMemcpyDeviceToHost));
        if (kind != GM_TRACK_CALLS) return GM_OK;
        if (h_code.ensure(n) || h_pval.ensure(n * 8)) return GM_E_NOMEM;
        HIPCHK(hipMemcpy(h_code.p, d_code.p, n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_pval.p, d_pval.p, n * 8, hipMemcpyDeviceToHost));
        return GM_OK;
    }
    TrackRows rows(const gm_index* ix, const TrackJob& job) const {
        return TrackRows{ &ix->h, ix->cov_bin_size, job.kind, job.want, h_f.as<float>(), h_f.as<float>() + n, n, lo, h_code.as<uint8_t>(), h_pval.as<double>() };
    }
};
}  // namespace

extern "C" int gm_coverage_write_gmp_calls(gm_index* ix, float snp_pval, int monop, const char* path, int append) {
    // GenomeBwt::PrintFinalSNP src/GenomeBwt.cpp:930-1009 with PrintSNPCall's column (:1011-1090).  A slab of the six tracks comes down from
    // HBM together with k_snp_call's code byte and p-value per position; the first eight columns are gm_coverage_write_gmp's, byte for byte
    if (!ix || !path) return GM_E_ARG;
    if (const int rc = snp_tracks_ready(ix, nullptr)) return rc;
    HIPCHK(hipSetDevice(ix->device));
    const TrackJob job{ GM_TRACK_CALLS, 0, snp_pval, monop };
    HostSlab hs;
    TrackRows e = hs.rows(ix, job);
    return write_track_text(path, append, ix->h.l_pac, e, [&](uint64_t lo, uint64_t hi) -> int {
        if (const int rc = hs.call(ix, job, lo, hi - lo, nullptr)) return rc;
        if (const int rc = hs.fetch(ix, job.kind, lo, hi - lo)) return rc;
        e = hs.rows(ix, job);
        return GM_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// track files formatted on the device (gm_tracktext.hip)
// ------------------------------------------------------------------------------------------------
namespace {
struct ScopedEvents {
    hipEvent_t a = nullptr, b = nullptr;
    ~ScopedEvents() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// bins [lo, hi) as rows: per slab of device_slab_bins() bins the sizes pass and its scan, the 32 bytes of `meta` read back, a text buffer
// of exactly that size, the rows pass, and the text down in pieces of 32 MB through two page-locked buffers (the copy of one piece runs
// while the one before it is written).  A slab whose meta says that a printed value needs snprintf is formatted here from its own tracks.
// GM_TRACK_CALLS (the nine-column .gmp): k_snp_call runs first on every slab and its code bytes / p-values stay in HBM for the two passes.
struct TrackTextRun {
    gm_index* const ix; const char* const call; const TrackJob job; TrackSink& out;
    gm_track_text_stats st{};
    GmDevTrack t{};
    Scoped<DevBuf> d_len, d_off, d_meta, d_text;
    Scoped<PinBuf> h_meta, h_txt[2];
    ScopedEvents ev;
    HostSlab hs;                                             // GM_TRACK_CALLS: the slab's calls in HBM; any kind: a slab the host formats
    std::vector<char> hbuf;                                  // and its text
    const hipStream_t s = nullptr;
    bool nine() const { return job.kind == GM_TRACK_CALLS; }
    const unsigned long long* meta() const { return h_meta.as<unsigned long long>(); }
    int fail_io() const { gm_set_error(std::string(call) + ": write failed"); return GM_E_IO; }
    int read_meta() {
        HIPCHK(hipMemcpyAsync(h_meta.p, d_meta.p, TT_META_N * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return GM_OK;
    }
    // k_snp_call for the nine-column file, then k_track_sizes and its scan: meta() holds the slab's bytes, rows and host flag
    int sizes_pass(uint64_t s0, uint64_t n) {
        float ms = 0;
        t.lo = s0; t.n = n; t.text = nullptr;
        if (nine()) { if (const int rc = hs.reserve(n)) return rc; }        // not between the events: kernel_ms is the kernels' time
        HIPCHK(hipMemsetAsync(d_meta.p, 0, TT_META_N * 8, s));
        HIPCHK(hipEventRecord(ev.a, s));
        if (nine()) {
            if (const int rc = hs.call(ix, job, s0, n, s)) return rc;
            t.code = hs.d_code.as<uint8_t>(); t.pval = hs.d_pval.as<double>();
        }
        KCHK(gmk_track_sizes(t, s));
        HIPCHK(hipEventRecord(ev.b, s));
        if (const int rc = read_meta()) return rc;
        HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
        st.kernel_ms += ms; st.launches += nine() ? 3 : 2; ++st.slabs;
        return GM_OK;
    }
    // the host emitter over this slab's tracks only, 65 536 bins of text at a time
    int host_slab(uint64_t s0, uint64_t n) {
        ++st.host_slabs;
        if (const int rc = hs.fetch(ix, job.kind, s0, n)) return rc;
        const TrackRows e = hs.rows(ix, job);
        const size_t max_line = e.max_line();
        for (uint64_t k0 = s0; k0 < s0 + n; k0 += 65536) {
            const uint64_t k1 = std::min(s0 + n, k0 + 65536);
            hbuf.resize((size_t)(k1 - k0) * max_line);
            char* const w = e.range(k0, k1, hbuf.data(), &st.rows);
            if (!out.put(hbuf.data(), (uint64_t)(w - hbuf.data()))) return fail_io();
        }
        return GM_OK;
    }
    // k_track_rows into a buffer of the slab's `bytes`, and the first `need` of them to the sink.  host = true: nothing was written, the
    // rows pass met a p-value that only the host prints (k_track_rows<true> flags what gm_put_e2_hd refused inside its domain)
    int rows_pass(uint64_t bytes, uint64_t need, bool& host) {
        float ms = 0;
        if (d_text.ensure((size_t)bytes + 16)) return GM_E_NOMEM;
        t.text = d_text.as<char>();
        HIPCHK(hipEventRecord(ev.a, s));
        KCHK(gmk_track_rows(t, s));
        HIPCHK(hipEventRecord(ev.b, s));
        ++st.launches;
        if (nine()) {
            if (const int rc = read_meta()) return rc;
            if ((host = meta()[TT_META_HOST] != 0)) return GM_OK;
        }
        if (out.fd < 0) {
            HIPCHK(hipMemcpy(out.mem + out.total, t.text, (size_t)need, hipMemcpyDeviceToHost));
            out.total += bytes;
        } else {
            const char* prev = nullptr; size_t prev_n = 0; int c = 0;
            for (uint64_t done = 0; done < bytes; c ^= 1) {
                const size_t m = (size_t)std::min<uint64_t>((size_t)32 << 20, bytes - done);
                if (h_txt[c].ensure(m)) return GM_E_NOMEM;
                HIPCHK(hipMemcpyAsync(h_txt[c].p, t.text + done, m, hipMemcpyDeviceToHost, s));
                if (prev && !out.put(prev, prev_n)) return fail_io();
                HIPCHK(hipStreamSynchronize(s));
                prev = h_txt[c].as<char>(); prev_n = m; done += m;
            }
            if (prev && !out.put(prev, prev_n)) return fail_io();
        }
        HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
        st.kernel_ms += ms;
        return GM_OK;
    }
    int run(uint64_t lo, uint64_t hi) {
        HIPCHK(hipSetDevice(ix->device));
        if (const int rc = index_cnames(ix)) return rc;
        const uint64_t bs = ix->cov_bin_size, nbk = (ix->h.l_pac + bs - 1) / bs;      // the files print the bins that start below l_pac
        hi = std::min(hi, nbk); lo = std::min(lo, hi);
        const uint64_t per = device_slab_bins();
        ix->tt_stats = st;
        const uint32_t tiles_max = gmk_track_tiles(std::min(per, hi - lo));
        if (d_len.ensure((size_t)tiles_max * 4 + 4) || d_off.ensure(((size_t)tiles_max + 1) * 8) || d_meta.ensure(TT_META_N * 8) || h_meta.ensure(TT_META_N * 8)) return GM_E_NOMEM;
        HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.b));
        t.cov = ix->d_cov.as<float>(); t.nuc = job.kind == GM_TRACK_SGR ? nullptr : ix->d_nuc.as<float>(); t.nuc_stride = ix->cov_bins;
        t.pac = ix->dev.pac; t.contig_off = ix->dev.contig_off; t.n_seqs = ix->dev.n_seqs;
        t.cnames = ix->d_cnames.as<char>(); t.cname_off = ix->d_cname_off.as<uint32_t>();
        t.bin_size = (uint32_t)bs; t.kind = (uint32_t)job.kind; t.want = job.want == 'a' ? 0u : job.want == 'c' ? 1u : job.want == 'g' ? 2u : 3u;
        t.tile_len = d_len.as<uint32_t>(); t.tile_off = d_off.as<unsigned long long>(); t.meta = d_meta.as<unsigned long long>();
        for (uint64_t s0 = lo; s0 < hi; s0 += per) {
            const uint64_t n = std::min(per, hi - s0);
            if (const int rc = sizes_pass(s0, n)) return rc;
            const uint64_t bytes = meta()[TT_META_BYTES], rows = meta()[TT_META_ROWS];
            bool host = meta()[TT_META_HOST] != 0;
            if (!host) {
                const uint64_t need = std::min(bytes, out.room());   // what has to come down
                if (!need) out.total += bytes;
                else if (const int rc = rows_pass(bytes, need, host)) return rc;
            }
            if (!host) st.rows += rows;
            else if (const int rc = host_slab(s0, n)) return rc;
        }
        st.bytes = out.total;
        ix->tt_stats = st;
        return GM_OK;
    }
};

// The job of a device entry point, and whether the tracks are ready for it: k_snp_call's settings (calls) mean the nine-column rows, else
// the mode of p decides (null: the .sgr)
int track_job(gm_index* ix, const char* call, const gm_params* p, const TrackJob* calls, TrackJob& job) {
    if (calls) { job = *calls; return snp_tracks_ready(ix, call); }
    if (!ix->cov_bins || !ix->cov_bin_size) { gm_set_error(std::string(call) + ": no coverage track (gm_coverage_reset)"); return GM_E_ARG; }
    const int mode = p ? p->mode : GM_MODE_NORMAL;
    job = TrackJob{ mode == GM_MODE_NORMAL ? GM_TRACK_SGR : mode == GM_MODE_SNP ? GM_TRACK_SNP : GM_TRACK_BASE, gmp_want(mode), 0.0f, 0 };
    if (ix->host_only) { gm_set_error(std::string(call) + ": no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (job.kind != GM_TRACK_SGR && !ix->nuc_on) { gm_set_error(std::string(call) + ": the .gmp rows read the per-nucleotide tracks: call gm_coverage_enable_nuc first"); return GM_E_ARG; }
    return GM_OK;
}

// every bin of the track into a file
int track_text_file(gm_index* ix, const char* call, const gm_params* p, const TrackJob* calls, const char* path, int append) {
    TrackJob job;
    if (const int rc = track_job(ix, call, p, calls, job)) return rc;
    TrackSink out;
    if (!out.open(path, append)) { gm_set_error(std::string(call) + ": cannot write " + path); return GM_E_IO; }
    return TrackTextRun{ ix, call, job, out }.run(0, ix->cov_bins);
}

// the bins [bin_lo, bin_hi) into text[0, cap); *n_out = the bytes they take
int track_text_mem(gm_index* ix, const char* call, const gm_params* p, const TrackJob* calls, uint64_t bin_lo, uint64_t bin_hi, char* text, uint64_t cap, uint64_t* n_out) {
    if (!ix || !n_out || (cap && !text)) { gm_set_error(std::string(call) + ": null argument"); return GM_E_ARG; }
    if (!ix->cov_bins || !ix->cov_bin_size) { gm_set_error(std::string(call) + ": no coverage track (gm_coverage_reset)"); return GM_E_ARG; }
    if (bin_lo > bin_hi || bin_hi > ix->cov_bins) { gm_set_error(std::string(call) + ": bins [bin_lo, bin_hi) are not a range of the track"); return GM_E_ARG; }
    TrackJob job;
    if (const int rc = track_job(ix, call, p, calls, job)) return rc;
    TrackSink out;
    out.mem = text; out.cap = cap;
    if (const int rc = TrackTextRun{ ix, call, job, out }.run(bin_lo, bin_hi)) return rc;
    *n_out = out.total;
    if (out.total > cap) { gm_set_error(std::string(call) + ": text[] too small"); return GM_E_CAPACITY; }
    return GM_OK;
}
}  // namespace

extern "C" int gm_coverage_write_sgr_device(gm_index* ix, const char* path, int append) {
    // GenomeBwt::PrintFinalSGR src/GenomeBwt.cpp:1212-1273, from the track in HBM
    if (!ix || !path) { gm_set_error("gm_coverage_write_sgr_device: null argument"); return GM_E_ARG; }
    return track_text_file(ix, "gm_coverage_write_sgr_device", nullptr, nullptr, path, append);
}

extern "C" int gm_coverage_write_gmp_device(gm_index* ix, const gm_params* p, const char* path, int append) {
    // GenomeBwt::PrintFinalBisulfite src/GenomeBwt.cpp:1092-1210, PrintFinalSNP :930-1009 (eight columns), from the tracks in HBM
    if (!ix || !p || !path) { gm_set_error("gm_coverage_write_gmp_device: null argument"); return GM_E_ARG; }
    if (p->mode == GM_MODE_NORMAL) { gm_set_error("gm_coverage_write_gmp_device: GM_MODE_NORMAL writes an .sgr (gm_coverage_write_sgr_device)"); return GM_E_ARG; }
    return track_text_file(ix, "gm_coverage_write_gmp_device", p, nullptr, path, append);
}

extern "C" int gm_coverage_text(gm_index* ix, const gm_params* p, uint64_t bin_lo, uint64_t bin_hi, char* text, uint64_t cap, uint64_t* n_out) {
    return track_text_mem(ix, "gm_coverage_text", p, nullptr, bin_lo, bin_hi, text, cap, n_out);
}

extern "C" int gm_coverage_write_gmp_calls_device(gm_index* ix, float snp_pval, int monop, const char* path, int append) {
    // the file of gm_coverage_write_gmp_calls from the tracks in HBM: k_snp_call, then k_track_sizes<true> / k_track_rows<true> per slab
    if (!ix || !path) { gm_set_error("gm_coverage_write_gmp_calls_device: null argument"); return GM_E_ARG; }
    const TrackJob calls{ GM_TRACK_CALLS, 0, snp_pval, monop };
    return track_text_file(ix, "gm_coverage_write_gmp_calls_device", nullptr, &calls, path, append);
}

extern "C" int gm_coverage_calls_text(gm_index* ix, float snp_pval, int monop, uint64_t bin_lo, uint64_t bin_hi, char* text, uint64_t cap, uint64_t* n_out) {
    const TrackJob calls{ GM_TRACK_CALLS, 0, snp_pval, monop };
    return track_text_mem(ix, "gm_coverage_calls_text", nullptr, &calls, bin_lo, bin_hi, text, cap, n_out);
}

extern "C" int gm_coverage_write_vcf(gm_index* ix, float snp_pval, int monop, const char* path, int append) {
    // Genome::PrintFinalVCF src/Genome.cpp:1142-1245 over gm_snp_calls' records.  The rows are few (one per called SNP), so they are
    // formatted here: a count pass, then the records of one stretch of positions at a time
    const char* const call = "gm_coverage_write_vcf";
    if (!ix || !path) { gm_set_error(std::string(call) + ": null argument"); return GM_E_ARG; }
    if (const int rc = snp_tracks_ready(ix, call)) return rc;
    uint64_t total = 0;
    int rc = snp_calls_range(ix, snp_pval, monop, 0, ~0ull, nullptr, 0, &total, nullptr);
    if (rc != GM_OK && rc != GM_E_CAPACITY) return rc;
    FILE* f = fopen(path, append ? "a" : "w");
    if (!f) { gm_set_error(std::string(call) + ": cannot write " + path); return GM_E_IO; }
    if (!append) {
        char date[16] = "";
        const time_t now = time(nullptr);
        struct tm tmv;
        if (localtime_r(&now, &tmv)) strftime(date, sizeof date, "%Y%m%d", &tmv);
        fprintf(f, "##fileformat=VCFv4.0\n##fileDate=%s\n##source=%s\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n", date, gm_version());
    }
    const GmHostIndex& h = ix->h;
    const uint64_t step = vcf_stretch_positions();
    std::vector<gm_snp_rec> recs((size_t)std::min<uint64_t>(std::max<uint64_t>(total, 1), 1u << 16));
    unsigned long long id = 0;
    for (uint64_t lo = 0; total && lo < h.l_pac; lo += step) {
        uint64_t got = 0;
        rc = snp_calls_range(ix, snp_pval, monop, lo, lo + step, recs.data(), recs.size(), &got, nullptr);
        if (rc == GM_E_CAPACITY) {                           // a denser stretch: once more with room for it
            recs.resize((size_t)got);
            rc = snp_calls_range(ix, snp_pval, monop, lo, lo + step, recs.data(), recs.size(), &got, nullptr);
        }
        if (rc != GM_OK) { fclose(f); return rc; }
        auto base = [](unsigned b) { return b < 5u ? b : 4u; };
        for (uint64_t r = 0; r < got; ++r) {
            const gm_snp_rec& c = recs[(size_t)r];
            const unsigned a1 = base(c.alt1), a2 = base(c.alt2);
            const char* name = h.contigs[c.contig].name.c_str();
            if (c.diploid)
                fprintf(f, "%s\t%llu\tsnp%llu\t%c\t%c%c\t.\t.\tDiploid;pval=%.5f;coverage=%.5f;ratio=%.2f\n", name, (unsigned long long)c.chr_pos, id++, "acgtn"[base(c.ref)],
                        "acgtn"[a1], "acgtn"[a2], c.p_val, c.total, c.nuc[a2] / c.nuc[a1]);
            else
                fprintf(f, "%s\t%llu\tsnp%llu\t%c\t%c\t.\t.\tMonoploid;pval=%.5f;coverage=%.5f\n", name, (unsigned long long)c.chr_pos, id++, "acgtn"[base(c.ref)], "acgtn"[a1], c.p_val,
                        c.total);
        }
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) { gm_set_error(std::string(call) + ": write failed: " + path); return GM_E_IO; }
    return GM_OK;
}

extern "C" int gm_coverage_text_stats(gm_index* ix, gm_track_text_stats* out) {
    if (!ix || !out) return GM_E_ARG;
    *out = ix->tt_stats;
    return GM_OK;
}
