// gm_api.cpp — the C ABI of libgnumap_hip.so (include/gnumap_hip.h): index residency in HBM, batch staging,
// the kernel pipeline, and the host-side mirror of the reference's per-read bookkeeping
// (unique-sequence map, denominator, posterior, MAPQ: src/Driver.cpp:432-753, inc/align_seq2_raw.cpp:102-165,
// inc/ScoredSeq.h:293-404).  There is NO CPU fallback for the device work: without a usable gfx950 device every
// compute entry point fails with GM_E_NO_DEVICE.
#include "gm_lib.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <thread>
#include <unistd.h>

static thread_local std::string g_err;
// ---- run-time switches: gm_set_option() overrides, else the environment; never latched (see gm_internal.h) ----
namespace { std::mutex g_opt_mu; std::map<std::string, const char*> g_opts; }      // values are interned (never freed): a reader may still hold one
const char* gm_opt(const char* name) {
    const char* v = nullptr; bool have = false;
    {
        std::lock_guard<std::mutex> lk(g_opt_mu);
        auto it = g_opts.find(name);
        if (it != g_opts.end()) { v = it->second; have = true; }
    }
    if (!have) v = getenv(name);
    return v && *v ? v : nullptr;                              // an empty value counts as unset
}
extern "C" int gm_set_option(const char* name, const char* value) {
    if (!name || strncmp(name, "GM_", 3) != 0) return GM_E_ARG;
    std::lock_guard<std::mutex> lk(g_opt_mu);
    if (value) g_opts[name] = strdup(value); else g_opts.erase(name);       // null: back to the environment
    return GM_OK;
}
static bool gm_trace_on() { return gm_opt_ll("GM_TRACE", 0) != 0; }
static double gm_trace_ms() { static const auto t0 = std::chrono::steady_clock::now(); return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
#define GM_TRACE(...) do { if (gm_trace_on()) { fprintf(stderr, "[gm_trace %9.1f ms] ", gm_trace_ms()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)
void gm_set_error(const std::string& s) { g_err = s; }
extern "C" const char* gm_last_error(void) { return g_err.c_str(); }
extern "C" const char* gm_version(void) { return "gnumap-mi355x 0.2 (gfx950)"; }

struct gm_batch {
    gm_index* ix = nullptr;
    uint32_t max_reads = 0, max_len = 0;
    uint32_t len_max = 0;                 // longest read of the uploaded block
    uint32_t len_min = 0;                 // and the shortest
    uint32_t n = 0, stride = 0, max_seeds = 0, illumina_until = 0;
    int up_illumina = 0;                  // gm_params.illumina of the upload that left the block resident: illumina_until was scanned under it
    DevBuf bases, quals, len, status, self_score, min_score, top_score, seeds, n_seeds, n_entries, entry_off, coords,
        rs_overflow, retry_list, retry_off, gtab_keys, gtab_vals, cands, fixed_cands, fixed_cnt, heavy_list, heavy_off, heavy_k0, heavy_k1, heavy_tmp, hit_count, hit_begin, hit_cursor, raw_hits, counters, small, shards, big_list,
        tb_items, tb_ops, tb_len, band_moves, pack,
        // grouping (process_hits' unique map) and output stage, gm_output.hip
        g_sorted, g_ord, g_lead, g_krank, g_khash, g_nmatch, g_mbegin, g_multi, g_big, g_bigdone, g_sk0, g_sk1, g_si0, g_si1, g_matches, g_mhit, g_positions, scan_tmp,
        o_small, o_posmatch, o_post, o_mapq, o_emit, o_reccnt, o_cigcnt, o_cigall, o_recoff, o_cigoff, o_recs, o_pool, o_codes,
        pair_fb, pair_list,             // k_vote_pair: the reads it leaves to k_vote_bucket (one byte each), their list + its counter
        snp_scratch, snp_hmm,           // --snp: forward matrices of a chunk of kept sequences, their 5 floats per window position
        t_names, t_nameoff, t_qtail, t_qtailoff, t_slots, t_rowlen, t_rowoff, t_text, t_bad,     // gm_output_batch_text: the block's names, tails and row offsets, the text
        t_bammeta,                      // gm_output_batch_bam: operations and bin of every record (k_bam_sizes)
        t_status, t_rowcnt, t_rowflag, t_rowfirst, t_rowucum, t_rowsrc,        // gm_batch_set_unmapped_rows: the reads' status bytes and the row source (gmk_row_source)
        t_md,                           // gm_batch_set_row_tags: {NM, MD bytes} of every row (k_md_sizes)
        m_span, m_first, m_end, m_prim, m_proper, m_meta, m_fields,            // gm_batch_set_mates: what the k_mate_* kernels leave (GmDevMates), the fields of every row
        m_namelen, m_nameoff, m_names,  // ... and the names after the QNAME rule's cuts, a pool of their own
        full_len, d_adaptor,            // -A: the lengths as uploaded (`len` then holds what k_adaptor_trim keeps), the adaptor's characters
        rt_text, rt_tilecnt, rt_tileoff, rt_lineat, rt_lsum, rt_lin, rt_recs, rt_nlen, rt_tlen, rt_meta;      // gm_batch_upload_text: the FASTQ text and what k_rt_* make of it
    GmBgzfBufs bz;                      // gm_output_batch_bam: the BGZF blocks of the block's records
    hipEvent_t bam_ev[4] = { nullptr, nullptr, nullptr, nullptr };      // while profiling is on: around k_bam_sizes and around k_bam_rows (gm_batch_bam_times)
    double bam_rows_ms = 0; uint64_t bam_raw_bytes = 0;
    bool text_block = false;            // the block that is resident was cut from text by gm_batch_upload_text: t_names / t_qtail hold its names and tails
    bool text_pools = false;            // ... and still do (gm_output_batch_text with a caller's gm_read_text overwrites them)
    uint64_t text_name_bytes = 0, text_tail_bytes = 0;
    PinBuf h_rt;                        // its read-backs
    std::string adaptor;                // gm_batch_set_adaptor; empty = none (no launch, no copy, no wait in gm_batch_upload)
    int read_format = GM_READS_FASTQ;   // gm_batch_set_read_format: the blocks uploaded from now on
    bool unmapped_rows = false;         // gm_batch_set_unmapped_rows: a read without a record gets a flag-4 row from the row-producing output calls
    uint64_t n_unmapped = 0;            // ... and how many the last output call wrote (gm_batch_unmapped_rows)
    uint32_t row_tags = 0;              // gm_batch_set_row_tags: GM_ROW_TAG_MD = the rows of the row-producing output calls carry NM:i and MD:Z
    bool mates = false;                 // gm_batch_set_mates: reads 2i and 2i + 1 are the mates of pair i in every output call
    uint32_t mate_min = 0, mate_max = 500;      // ... the insert limits of a concordant combination, both inclusive
    uint64_t mate_n_rows = 0;           // ... the rows the last output call left fields for in m_fields (gm_batch_mate_rows)
    gm_mate_stats mate_stats{};         // ... and its pair counters (gm_batch_mate_stats)
    int cigar_order = GM_CIGAR_GNUMAP;  // gm_batch_set_cigar_order: GM_CIGAR_FORWARD = a minus-strand row prints its CIGAR in reference order
    bool fasta = false;                 // the block that is resident was uploaded as FASTA (GmDevBatch::fasta)
    bool adaptor_dirty = false;         // d_adaptor does not hold `adaptor` yet
    PinBuf h_top, h_hbegin, h_ord, h_post, h_mapq, h_emit, h_mhit, h_stat;      // h_stat: the small status words a phase reads back (page-locked: one short DMA)
    std::vector<double> h_exp;          // exp(score) of every accepted hit of the last gm_map_batch (reused by gm_output_batch)
    uint64_t cache_hits = 0, cache_matches = 0;
    uint32_t epoch_ctr = 0;             // launch stamps handed out so far for the own-slot candidates of k_vote_bucket (map_vote_attempt takes the next one)
    uint64_t stamp = 0;                 // names the gm_map_batch result resident in g_matches / g_positions (gm_hits::stamp); 0 = none
    std::string path;                   // which kernels the last gm_map_batch_device chose (gm_batch_path)
    uint32_t pair_flagged = 0;          // reads k_vote_pair handed to the list in it (gm_batch_pair_flagged): pair_list[0] as the status words brought it
    // gm_*_enqueue / gm_batch_wait: the batch's own service thread runs the queued calls in order, the caller goes on
    struct Service {
        std::thread th; std::mutex mu; std::condition_variable cv;
        std::deque<std::function<int()>> q;
        bool busy = false, quit = false;
        int rc = GM_OK; std::string err;
    } svc;
    const void* resume_ptr = nullptr;   // set when gm_map_batch returned GM_E_CAPACITY: the next call with the same reads resumes at the copies
    uint32_t cand_cap = 0;
    uint64_t raw_cap = 0;
    uint32_t n_cands = 0;
    uint64_t n_raw = 0;
    bool mapped = false;
    unsigned long long counters_host[GMK_N] = { 0 };
    GmDevBatch dev{};
    std::vector<uint16_t> len_host;     // the lengths `len` holds in HBM: as uploaded, or with an adaptor set what k_adaptor_trim kept
    double adaptor_ms = 0; uint64_t adaptor_launches = 0;      // k_adaptor_trim while profiling is on (gm_batch_adaptor_time)
    // sub-batch pipeline (gm_map_batch_device on large batches): streams + per-stream retry tables + host counter sums
    static const int NS = 3;
    hipStream_t sub_streams[NS] = { nullptr, nullptr, nullptr };
    hipEvent_t sub_ready = nullptr;
    DevBuf sub_gk[NS], sub_gv[NS], sub_counters, sub_small, sub_shards;
    bool counters_on_host = false;
    // HIP-event profiling of the kernels of gm_map_batch_device
    bool profiling = false;
    struct Ev { int which; hipEvent_t a, b; };
    std::vector<Ev> pending;
    std::vector<hipEvent_t> pool;
    double k_ms[GM_K_COUNT] = { 0 };
    uint64_t k_launches[GM_K_COUNT] = { 0 };
};

namespace {
struct KTimer {     // brackets one kernel (or one small group of launches) with events on its stream
    gm_batch* b; int which; hipStream_t st; hipEvent_t a = nullptr, e = nullptr; bool on;
    KTimer(gm_batch* b_, int w, hipStream_t s) : b(b_), which(w), st(s), on(b_->profiling) {
        if (!on) return;
        auto get = [&]() { hipEvent_t ev = nullptr; if (!b->pool.empty()) { ev = b->pool.back(); b->pool.pop_back(); } else if (hipEventCreate(&ev) != hipSuccess) ev = nullptr; return ev; };
        a = get(); e = get();
        if (!a || !e) { on = false; return; }
        (void)hipEventRecord(a, st);
    }
    ~KTimer() {
        if (!on) return;
        (void)hipEventRecord(e, st);
        b->pending.push_back({ which, a, e });
    }
};
}  // namespace

// ------------------------------------------------------------------------------------------------
// parameters (const_define.h:29-131, a_matrices.c:55-83, Driver.cpp:1206,1260-1313,2805-2816)
// ------------------------------------------------------------------------------------------------
extern "C" void gm_params_default(gm_params* p) {
    memset(p, 0, sizeof *p);
    p->mer = 10; p->jump = 0; p->min_seed_hits = 2; p->max_kmer_hits = 0; p->max_matches = 1000; p->max_gap = 3;
    p->nw = 1; p->fast = 0; p->unique_only = 0; p->pos_strand = 1; p->neg_strand = 1; p->mode = GM_MODE_NORMAL;
    p->align_score = 0.9f; p->align_is_fraction = 1; p->cutoff = 0.0f;
    p->adjust = 0.25f; p->match = 3; p->transition = -2; p->transversion = -3; p->gap = -4;
    p->bin_size = 8; p->print_all_sam = 0; p->illumina = 0; p->finalized = 0;
}

extern "C" int gm_params_finalize(gm_params* p) {
    if (!p) return GM_E_ARG;
    if (p->finalized) return GM_OK;
    if (p->mer < 1 || p->mer > 32) { gm_set_error("-m/--mer_size: must be 1..32 (MAX_MER_SIZE)"); return GM_E_ARG; }
    if (p->min_seed_hits < 1) { gm_set_error("-k/--num_seed: Invalid matching seed number"); return GM_E_ARG; }
    if (p->max_gap < 1 || p->max_gap > 7) { gm_set_error("-M/--max_gap: 1 .. 7 (band rows of up to 17 cells)"); return GM_E_UNSUPPORTED; }
    if (p->jump <= 0) p->jump = p->mer / 2;
    if (p->jump < 1) p->jump = 1;
    p->match *= p->adjust; p->transition *= p->adjust; p->transversion *= p->adjust; p->gap *= p->adjust;
    for (int i = 0; i < 256; ++i) for (int j = 0; j < 4; ++j) p->S[i][j] = p->transversion;
    static const char lo[4] = { 'a', 'c', 'g', 't' }, up[4] = { 'A', 'C', 'G', 'T' };
    for (int g = 0; g < 4; ++g)
        for (int b = 0; b < 4; ++b) {
            float v = g == b ? p->match : ((g ^ b) == 2 ? p->transition : p->transversion);
            p->S[(int)lo[g]][b] = v;
            p->S[(int)up[g]][b] = v;
        }
    if (p->mode == GM_MODE_BS) p->S['c'][3] = p->match;
    if (p->mode == GM_MODE_BS2) p->S['g'][0] = p->match;
    if (p->mode == GM_MODE_ATOG) p->S['a'][2] = p->match;
    if (p->mode == GM_MODE_ATOG2) p->S['t'][1] = p->match;
    if (p->mode != GM_MODE_NORMAL) p->bin_size = 1;
    if (p->bin_size < 1) { gm_set_error("--bin_size: must be >= 1"); return GM_E_ARG; }
    p->finalized = 1;
    return GM_OK;
}

extern "C" int gm_params_load_subst(gm_params* p, const char* path) {
    if (!p || !path || !p->finalized) { gm_set_error("gm_params_load_subst: finalize the parameters first"); return GM_E_ARG; }
    FILE* f = fopen(path, "r");
    if (!f) { gm_set_error(std::string("cannot open substitution file ") + path); return GM_E_IO; }
    float t[5][4];
    char line[100], l0[100], l1[100], l2[100], l3[100];
    int count = 0; bool labels = false;
    auto next_line = [&]() -> bool {                           // ifstream::getline(buf, 100): at most 99 characters of a line
        if (!fgets(line, sizeof line, f)) return false;
        size_t n = strlen(line);
        if (n && line[n - 1] == '\n') line[n - 1] = 0;
        return true;
    };
    while (count < 5 && next_line()) {
        if (sscanf(line, "%99s %99s %99s %99s", l0, l1, l2, l3) == 4 && tolower((unsigned char)l0[0]) == 'a' && tolower((unsigned char)l1[0]) == 'c') {
            if (!next_line()) break;                           // the label line: rows carry a label from here on
            labels = true;
        }
        float a, c, g, tt;
        const int got = labels ? sscanf(line, "%99s %f %f %f %f", l0, &a, &c, &g, &tt) - 1 : sscanf(line, "%f %f %f %f", &a, &c, &g, &tt);
        if (got != 4) { fclose(f); gm_set_error(std::string("Error in Score File: ") + line); return GM_E_IO; }
        t[count][0] = a; t[count][1] = c; t[count][2] = g; t[count][3] = tt;
        ++count;
    }
    fclose(f);
    if (count < 5) { gm_set_error("Error in Score File:  Not enough lines"); return GM_E_IO; }
    static const char rows[5] = { 'a', 'c', 'g', 't', 'n' };
    for (int r = 0; r < 5; ++r) for (int b = 0; b < 4; ++b) p->S[(int)rows[r]][b] = t[r][b];
    p->adjust = 1.0f;                                          // gADJUST = 1: "don't adjust the scores" (XA:f: prints score * 1 / gADJUST)
    return GM_OK;
}

// Q -> (p, (1-p)/3) in fp32 exactly as SeqReader::get_more_fastq computes them (fp64 libm, then one cast):
// Q2Prb_std src/SeqReader.cpp:623-627, Q2Prb_ill :618-622.  Negative p is stored as NaN.
// the FASTA rows of SeqReader::get_more_fasta (src/SeqReader.cpp:875-979, cast to float at :996) as (p, q) by base mask: a row holds the
// fp64 constant 1.0, 0.5, 1.0 / 3.0 or 0.25 at the 1, 2, 3 or 4 bases of its mask and 0.0 elsewhere.  Mask 0 (no IUPAC letter) is all zero.
static void build_fasta_lut(float* lut /* 16 x 2 */) {
    static const double by_count[5] = { 0.0, 1.0, 0.5, 1.0 / 3.0, 0.25 };
    for (int m = 0; m < 16; ++m) { lut[2 * m] = (float)by_count[__builtin_popcount(m)]; lut[2 * m + 1] = (float)0.0; }
}
// str2qual (inc/SequenceOperations.h:193-217) of a FASTA row whose largest entry is pmax: the quality character a SAM row prints there
static char fasta_qual_char(float pmax) {
    const double MAX_PRB = 0.9999;
    if (pmax > MAX_PRB) return (char)((-10 * log(1 - MAX_PRB) / log(10.)) + 33);
    return (char)((-10 * log(1 - pmax) / log(10)) + 33);
}
// ... for the rows with 1, 2, 3, 4 bases in their mask, in bytes 0 .. 3 (GmDevText::fa_qual)
static uint32_t fasta_qual_word() {
    float l[32]; build_fasta_lut(l);
    return (uint32_t)(uint8_t)fasta_qual_char(l[2 * 1]) | ((uint32_t)(uint8_t)fasta_qual_char(l[2 * 3]) << 8) | ((uint32_t)(uint8_t)fasta_qual_char(l[2 * 7]) << 16) |
           ((uint32_t)(uint8_t)fasta_qual_char(l[2 * 15]) << 24);
}

static void build_lut(float* lut /* 512 x 2 */) {
    for (int which = 0; which < 2; ++which)
        for (int ch = 0; ch < 256; ++ch) {
            double p;
            const int sc = ch >= 128 ? ch - 256 : ch;                // `int Q = (int)fastq[i]` (SeqReader.cpp:1155): the character is a signed char,
            if (which == 0) { int Q = sc - 33; p = 1 - exp((-(double)Q / 10.0) * log(10.0)); }       // a byte above 127 a negative quality -> "Invalid Fastq Character"
            else { int Q = sc - 64; p = 1.0 - 1.0 / (pow(10.0, ((double)Q / 10.0))); }
            if (p > 1.0) p = 1.0;
            double other = (1 - p) / 3;
            float* o = lut + ((size_t)which * 256 + ch) * 2;
            if (p < 0) { o[0] = NAN; o[1] = NAN; } else { o[0] = (float)p; o[1] = (float)other; }
        }
}

// want_bucket: the caller may use the bucket table of gm_bucket.hip (gm_map_batch_device): built on first use when it applies
static int sync_params(gm_index* ix, const gm_params* p, GmDevParams& dp, hipStream_t st, bool want_bucket = false) {
    std::vector<float> tab(256 * 4 + GM_LUT_ENTRIES * 2);
    memcpy(tab.data(), p->S, sizeof(float) * 1024);
    build_lut(tab.data() + 1024);
    build_fasta_lut(tab.data() + 1024 + 2 * GM_LUT_FASTA);
    // parameter tables are kept per CONTENT and never overwritten: batches of one index may run concurrently with different
    // gm_params (e.g. --illumina switched off from some block on) without one call rewriting what another call's kernels read
    const float* d_tab = nullptr;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        auto it = ix->ptabs.find(tab);
        if (it == ix->ptabs.end()) {
            if (ix->ptabs.size() >= 64) { gm_set_error("more than 64 distinct parameter tables on one index"); return GM_E_NOMEM; }
            DevBuf nb;
            int rc = nb.ensure(tab.size() * sizeof(float));
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(nb.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
            it = ix->ptabs.emplace(tab, nb).first;
        }
        d_tab = it->second.as<float>();
    }
    dp.mer = p->mer; dp.jump = p->jump; dp.kmin = p->min_seed_hits; dp.nw = p->nw; dp.fast = p->fast;
    dp.pos_strand = p->pos_strand; dp.neg_strand = p->neg_strand; dp.align_is_fraction = p->align_is_fraction; dp.max_gap = p->max_gap;
    dp.fused = 0; dp.heavy_min = 0xFFFFFFFFu;
    dp.dbg = (int)gm_opt_ll("GM_DBG", 0);
    // k-mer interval table: the last T characters of every seed are one lookup (GM_KMER_TABLE=0 keeps the pure occ walk;
    // GM_KMER_TABLE=<T> picks another suffix length, at most 16)
    dp.kmer_tab = nullptr; dp.kmer_T = 0; dp.kmer_ctab = nullptr; dp.bucket = nullptr; dp.bucket_T = 0; dp.bucket_ctx = 0;
    dp.bucket_ecap = (uint32_t)std::min<long long>(384, gm_opt_ll("GM_BUCKET_ECAP", 384)); dp.bucket_ovcap = (uint32_t)std::min<long long>(16, gm_opt_ll("GM_BUCKET_OVCAP", 16));
    {
        // up to 12 characters by default; more for longer seeds on references where the extra occ steps are HBM misses anyway
        // (>= 50 Mbp): 14 characters = 2 GB + 0.5 GB compact,
        // 15 / 16 characters (8.6 + 2.1 GB / 34 + 8.6 GB: what 288 GB of HBM is for) when the seeds are that long: a 16-mer is then
        // ONE random 16-byte probe instead of a probe + two search steps
        int T = std::min(p->mer, ix->h.seq_len >= 50000000ull ? 16 : 12);
        if (const char* e = gm_opt("GM_KMER_TABLE")) { if (*e) T = std::min(std::min(atoi(e), p->mer), 16); }
        const long long bucket_opt = gm_opt_ll("GM_SEED_BUCKET", -1);
        if (T >= 4) {
            std::lock_guard<std::mutex> lk(ix->mu);
            // the 15- / 16-character tables are bought with free HBM: step down while table + previous level + compact form (+ 8 GB
            // for the batches) do not fit what is free right now
            while (T > 14 && !ix->kmer_tabs.count(T)) {
                size_t fr = 0, tot = 0;
                const size_t need = (((size_t)1 << (2 * T)) + ((size_t)1 << (2 * T - 2))) * 8 + ((size_t)1 << (2 * T - 3)) * 16 + ((size_t)8 << 30);
                if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr >= need) break;
                --T;
            }
            DevBuf& tb = ix->kmer_tabs[T];
            if (!tb.p) {
                if (tb.ensure(((size_t)1 << (2 * T)) * 8)) return GM_E_NOMEM;
                if (T <= 12) {
                    KCHK(gmk_build_kmer_table(ix->dev, tb.as<uint2>(), T, st));
                } else {                             // 12 characters directly, then one character (one search step per entry) at a time
                    DevBuf cur, nxt;
                    if (cur.ensure(((size_t)1 << 24) * 8)) return GM_E_NOMEM;
                    int e2 = gmk_build_kmer_table(ix->dev, cur.as<uint2>(), 12, st);
                    for (int tt = 13; tt <= T && !e2; ++tt) {
                        uint2* dst = tb.as<uint2>();
                        if (tt < T) { if (nxt.ensure(((size_t)1 << (2 * tt)) * 8)) { cur.release(); return GM_E_NOMEM; } dst = nxt.as<uint2>(); }
                        e2 = gmk_extend_kmer_table(ix->dev, cur.as<uint2>(), dst, tt, st);
                        if (hipStreamSynchronize(st) != hipSuccess) e2 = 1;
                        if (tt < T) { cur.release(); cur = nxt; nxt = DevBuf(); }
                    }
                    cur.release(); nxt.release();
                    if (e2) { gm_set_error("k-mer table construction failed"); return GM_E_HIP; }
                }
                HIPCHK(hipStreamSynchronize(st));
                ix->hbm_bytes += tb.cap;
            }
            dp.kmer_tab = tb.as<uint2>(); dp.kmer_T = T;
            const bool compact = !gm_opt_is("GM_KMER_COMPACT", "0");
            if (compact) {
                DevBuf& cb = ix->kmer_ctabs[T];
                if (!cb.p) {
                    if (cb.ensure(((size_t)1 << (2 * T - 3)) * 16)) return GM_E_NOMEM;
                    KCHK(gmk_build_kmer_compact(tb.as<uint2>(), cb.as<uint4>(), T, st));
                    HIPCHK(hipStreamSynchronize(st));
                    ix->hbm_bytes += cb.cap;
                }
                dp.kmer_ctab = cb.as<uint4>();
            }
            // k-mer -> positions records (gm_bucket.hip): full SA, the table covering the whole seed, a k-mer expected between a
            // fraction of a time and ~20 times in the reference (a record holds 28 positions; more go through the suffix array),
            // and 128 bytes per code have to fit beside everything else: -m 14 = 34 GB of the 288.  GM_SEED_BUCKET=0 / 1: never /
            // whenever the table can be built.
            const double occ = (double)ix->h.seq_len / pow(4.0, (double)std::min(p->mer, 31));
            if (want_bucket && bucket_opt != 0 && ix->full_sa && T <= 15 && ix->h.seq_len < 0xFFFFE000ull &&
                T == p->mer && (bucket_opt > 0 || (occ >= 1.0 && occ <= 20.0))) {
                auto it = ix->buckets.find(T);
                if (it == ix->buckets.end()) {
                    DevBuf bb;
                    const size_t need = (((size_t)1 << (2 * T)) + 1) * 128;            // + the all-zero record behind the last code
                    size_t fr = 0, tot = 0;
                    if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr >= need + ((size_t)24 << 30) && bb.ensure(need) == GM_OK) {
                        const auto t0 = std::chrono::steady_clock::now();
                        // a failed build: the memory goes back and the empty entry is recorded, so that it is neither leaked nor tried again on every call
                        if (gmk_build_bucket(tb.as<uint2>(), ix->d_full.as<uint32_t>(), ix->dev.pac, bb.as<uint4>(), T, 0, st) != 0 || hipStreamSynchronize(st) != hipSuccess) {
                            bb.release();
                            ix->buckets.emplace(T, DevBuf());
                            gm_set_error("k-mer -> positions table construction failed");
                            return GM_E_HIP;
                        }
                        ix->hbm_bytes += bb.cap;
                        GM_TRACE("bucket table: %d-mers%s, %.1f GB, built in %.0f ms", T, "", need / 1e9, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                    }
                    it = ix->buckets.emplace(T, bb).first;     // an empty entry = does not fit: not tried again
                }
                dp.bucket = it->second.as<uint4>(); dp.bucket_T = T; dp.bucket_ctx = 0;
            }
        }
    }
    dp.hcap = p->max_kmer_hits; dp.gap = p->gap; dp.align_score = p->align_score; dp.cutoff = p->cutoff;
    dp.S256 = d_tab;
    dp.lut = reinterpret_cast<const float2*>(d_tab + 1024);
    return GM_OK;
}

// ------------------------------------------------------------------------------------------------
// index
// ------------------------------------------------------------------------------------------------
extern "C" int gm_index_build_on(const char* fasta_path, int where, int device_id) {
    if (!fasta_path || where < GM_BUILD_AUTO || where > GM_BUILD_DEVICE || device_id < 0) return GM_E_ARG;
    std::string err;
    int rc = gm_host_index_build(fasta_path, where, device_id, err);
    if (rc) gm_set_error(err);
    return rc;
}

extern "C" int gm_index_build(const char* fasta_path) { return gm_index_build_on(fasta_path, GM_BUILD_AUTO, 0); }

extern "C" int gm_index_open(const char* fasta_path, int device_id, int flags, gm_index** out) {
    if (!fasta_path || !out) return GM_E_ARG;
    *out = nullptr;
    std::string fa = fasta_path, err;
    if (!gm_host_index_files_exist(fa)) {
        if (!(flags & GM_INDEX_BUILD)) { gm_set_error("fail to locate the index files for " + fa); return GM_E_IO; }
        int rc = gm_host_index_build(fa, GM_BUILD_AUTO, device_id < 0 ? 0 : device_id, err);   // GenomeBwt::LoadGenome: "Could not find reference genome index! Building now."
        if (rc) { gm_set_error(err); return rc; }
    }
    gm_index* ix = new gm_index();
    int rc = gm_host_index_load(fa, ix->h, err);
    if (rc) { gm_set_error(err); delete ix; return rc; }
    if (ix->h.seq_len >= 0xFFFFFFFEull) {
        gm_set_error("reference too long for 32-bit ranks");
        delete ix;
        return GM_E_UNSUPPORTED;
    }
    ix->host_only = (flags & GM_INDEX_HOST_ONLY) != 0;
    if (ix->host_only) { *out = ix; return GM_OK; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) {
        gm_set_error("no usable HIP device (libgnumap_hip needs an MI355X / gfx950; there is no CPU fallback)");
        delete ix;
        return GM_E_NO_DEVICE;
    }
    ix->device = device_id;
    auto fail = [&](int code) { gm_index_close(ix); return code; };
    if (hipSetDevice(device_id) != hipSuccess) { gm_set_error("hipSetDevice failed"); return fail(GM_E_NO_DEVICE); }
    const GmHostIndex& h = ix->h;
    // stage the index into HBM once
    if (ix->d_bwt.ensure(h.bwt.size() * 4)) return fail(GM_E_NOMEM);
    if (hipMemcpy(ix->d_bwt.p, h.bwt.data(), h.bwt.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { gm_set_error("bwt upload failed"); return fail(GM_E_HIP); }
    std::vector<uint32_t> sa32(h.n_sa);
    for (uint64_t i = 0; i < h.n_sa; ++i) sa32[i] = (uint32_t)h.sa[i];      // sa[0] = (u64)-1 -> 0xFFFFFFFF
    if (ix->d_sa.ensure(sa32.size() * 4)) return fail(GM_E_NOMEM);
    if (hipMemcpy(ix->d_sa.p, sa32.data(), sa32.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { gm_set_error("sa upload failed"); return fail(GM_E_HIP); }
    if (ix->d_pac.ensure(h.pac.size())) return fail(GM_E_NOMEM);
    if (hipMemcpy(ix->d_pac.p, h.pac.data(), h.pac.size(), hipMemcpyHostToDevice) != hipSuccess) { gm_set_error("pac upload failed"); return fail(GM_E_HIP); }
    std::vector<uint32_t> coff(h.contigs.size() + 1);
    for (size_t i = 0; i < h.contigs.size(); ++i) coff[i] = (uint32_t)h.contigs[i].offset;
    coff[h.contigs.size()] = (uint32_t)h.l_pac;
    if (ix->d_contig.ensure(coff.size() * 4)) return fail(GM_E_NOMEM);
    if (hipMemcpy(ix->d_contig.p, coff.data(), coff.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { gm_set_error("contig upload failed"); return fail(GM_E_HIP); }
    GmDevIndex& d = ix->dev;
    d.bwt = ix->d_bwt.as<uint32_t>(); d.sa_samples = ix->d_sa.as<uint32_t>(); d.full_sa = nullptr;
    d.pac = ix->d_pac.as<uint8_t>(); d.contig_off = ix->d_contig.as<uint32_t>();
    d.seq_len = (uint32_t)h.seq_len; d.primary = (uint32_t)h.primary; d.l_pac = (uint32_t)h.l_pac; d.n_seqs = (uint32_t)h.contigs.size();
    d.sa_mask = h.sa_intv - 1; d.sa_shift = 0;
    while ((1u << d.sa_shift) < h.sa_intv) ++d.sa_shift;
    for (int i = 0; i < 5; ++i) d.L2[i] = (uint32_t)h.L2[i];
    {   // derive the bit-plane rank structure (one 16-byte load per rank query) from the reference-format BWT, once
        d.occ_nblk = (uint32_t)((h.seq_len + 95) / 96) + 1;
        if (ix->d_planes.ensure((size_t)4 * d.occ_nblk * 16)) return fail(GM_E_NOMEM);
        if (hipMemset(ix->d_planes.p, 0, (size_t)4 * d.occ_nblk * 16) != hipSuccess) { gm_set_error("plane memset failed"); return fail(GM_E_HIP); }
        int e = gmk_build_occ_planes(d, ix->d_planes.as<uint4>(), d.occ_nblk, nullptr);
        if (e || hipDeviceSynchronize() != hipSuccess) { gm_set_error("occ plane construction failed"); return fail(GM_E_HIP); }
        d.occ_planes = ix->d_planes.as<uint4>();
    }
    if (flags & GM_INDEX_FULL_SA) {
        if (ix->d_full.ensure(((size_t)h.seq_len + 1) * 4)) return fail(GM_E_NOMEM);
        int e = gmk_expand_full_sa(d, ix->d_full.as<uint32_t>(), nullptr);
        if (e || hipDeviceSynchronize() != hipSuccess) { gm_set_error("full SA expansion failed"); return fail(GM_E_HIP); }
        d.full_sa = ix->d_full.as<uint32_t>();
        ix->full_sa = true;
    }
    ix->hbm_bytes = ix->d_bwt.cap + ix->d_sa.cap + ix->d_pac.cap + ix->d_contig.cap + ix->d_full.cap + ix->d_planes.cap;
    *out = ix;
    return GM_OK;
}

// the tables the mapping kernels need for these parameters (memoised backward search of the seed, its compact form, the k-mer ->
// positions records) are built on the first gm_map_batch_device otherwise: a driver that wants its first block at full rate stages
// them with the index
extern "C" int gm_index_prepare(gm_index* ix, const gm_params* p) {
    if (!ix || !p || !p->finalized) return GM_E_ARG;
    if (ix->host_only) return GM_E_NO_DEVICE;
    HIPCHK(hipSetDevice(ix->device));
    GmDevParams dp;
    return sync_params(ix, p, dp, nullptr, true);
}

extern "C" void gm_index_close(gm_index* ix) {
    if (!ix) return;
    if (!ix->host_only && ix->device >= 0) {
        (void)hipSetDevice(ix->device);
        ix->d_bwt.release(); ix->d_sa.release(); ix->d_full.release(); ix->d_pac.release(); ix->d_contig.release();
        ix->d_cov.release(); ix->d_ptab.release(); ix->d_planes.release(); ix->d_nuc.release(); ix->d_cnames.release(); ix->d_cname_off.release();
        ix->d_holes.release();
        for (auto& kv : ix->ptabs) kv.second.release();
        for (auto& kv : ix->kmer_tabs) kv.second.release();
        for (auto& kv : ix->kmer_ctabs) kv.second.release();
        for (auto& kv : ix->buckets) kv.second.release();
    }
    delete ix;
}

extern "C" int gm_index_get_info(const gm_index* ix, gm_index_info* o) {
    if (!ix || !o) return GM_E_ARG;
    o->l_pac = ix->h.l_pac; o->seq_len = ix->h.seq_len; o->primary = ix->h.primary; o->bwt_words = ix->h.bwt_words; o->n_sa = ix->h.n_sa;
    o->sa_intv = ix->h.sa_intv; o->n_seqs = (uint32_t)ix->h.contigs.size(); o->device_id = ix->device; o->full_sa = ix->full_sa;
    o->hbm_bytes = ix->hbm_bytes;
    return GM_OK;
}

extern "C" const char* gm_index_contig_name(const gm_index* ix, uint32_t i) {
    if (!ix || i >= ix->h.contigs.size()) return nullptr;
    return ix->h.contigs[i].name.c_str();
}

extern "C" uint64_t gm_index_contig_offset(const gm_index* ix, uint32_t i) {
    if (!ix) return 0;
    if (i >= ix->h.contigs.size()) return ix->h.l_pac;
    return ix->h.contigs[i].offset;
}

// contig names back to back + n_seqs + 1 offsets in HBM, once per index: what k_out_text_rows and k_track_rows print
int index_cnames(gm_index* ix) {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->cnames_on) return GM_OK;
    const uint32_t n_seqs = (uint32_t)ix->h.contigs.size();
    std::string all; std::vector<uint32_t> off(n_seqs + 1, 0);
    for (uint32_t i = 0; i < n_seqs; ++i) { off[i] = (uint32_t)all.size(); all += ix->h.contigs[i].name; }
    off[n_seqs] = (uint32_t)all.size();
    if (ix->d_cnames.ensure(all.size() + 16) || ix->d_cname_off.ensure(off.size() * 4)) return GM_E_NOMEM;
    HIPCHK(hipMemcpy(ix->d_cnames.p, all.data(), all.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_cname_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    ix->cnames_on = true;
    return GM_OK;
}

// the holes of <fa>.gnumap.amb in HBM, once per index: what the walk of gm_batch_set_row_tags looks a row's first column up in
int index_holes(gm_index* ix) {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->holes_on) return GM_OK;
    if (ix->d_holes.ensure(ix->h.holes.size() * 4 + 16)) return GM_E_NOMEM;
    if (!ix->h.holes.empty()) HIPCHK(hipMemcpy(ix->d_holes.p, ix->h.holes.data(), ix->h.holes.size() * 4, hipMemcpyHostToDevice));
    ix->holes_on = true;
    return GM_OK;
}

uint32_t host_pos2rid(const GmHostIndex& h, uint64_t pos) {      // bns_pos2rid src/bntseq.c:349-363
    uint32_t lo = 0, hi = (uint32_t)h.contigs.size() - 1;
    while (lo < hi) {
        uint32_t mid = (lo + hi + 1) >> 1;
        if (pos >= h.contigs[mid].offset) lo = mid; else hi = mid - 1;
    }
    return lo;
}

static bool host_window(const GmHostIndex& h, uint64_t begin, uint32_t L, char* out) {   // GenomeBwt::GetString src/GenomeBwt.cpp:384-415
    if (L == 0 || begin >= h.l_pac || begin + L > h.l_pac) return false;
    if (host_pos2rid(h, begin) != host_pos2rid(h, begin + L - 1)) return false;
    for (uint32_t t = 0; t < L; ++t) {
        uint64_t p = begin + t;
        out[t] = "acgt"[(h.pac[p >> 2] >> ((~p & 3) << 1)) & 3];
    }
    return true;
}

extern "C" int gm_index_window(const gm_index* ix, uint64_t begin, uint32_t L, char* out) {
    if (!ix || !out) return 0;
    out[0] = 0;
    if (!host_window(ix->h, begin, L, out)) return 0;
    out[L] = 0;
    return (int)L;
}

// ------------------------------------------------------------------------------------------------
// batches
// ------------------------------------------------------------------------------------------------
extern "C" int gm_batch_create(gm_index* ix, uint32_t max_reads, uint32_t max_len, gm_batch** out) {
    if (!ix || !out || max_reads == 0 || max_len == 0) return GM_E_ARG;
    if (max_len > 2048) { gm_set_error("gm_batch_create: reads of at most 2048 bases (LDS budget of the seed and DP kernels)"); return GM_E_ARG; }
    // the vote kernels run one workgroup of 128 threads per read x strand and HIP refuses launches of 2^32 threads or more
    if (max_reads > 16000000u) { gm_set_error("gm_batch_create: at most 16 000 000 reads per batch (2 x reads x 128 threads per launch must stay below 2^32); use several batches"); return GM_E_ARG; }
    if (ix->host_only) { gm_set_error("index opened host-only"); return GM_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(ix->device));
    gm_batch* b = new gm_batch();
    b->ix = ix; b->max_reads = max_reads; b->max_len = max_len;
    *out = b;
    return GM_OK;
}

extern "C" void gm_batch_destroy(gm_batch* b) {
    if (!b) return;
    if (b->svc.th.joinable()) {
        { std::lock_guard<std::mutex> lk(b->svc.mu); b->svc.quit = true; }
        b->svc.cv.notify_all();
        b->svc.th.join();
    }
    (void)hipSetDevice(b->ix->device);
    DevBuf* all[] = { &b->bases, &b->quals, &b->len, &b->status, &b->self_score, &b->min_score, &b->top_score, &b->seeds, &b->n_seeds,
                      &b->n_entries, &b->entry_off, &b->coords, &b->rs_overflow, &b->retry_list, &b->retry_off, &b->gtab_keys, &b->gtab_vals,
                      &b->cands, &b->fixed_cands, &b->fixed_cnt, &b->heavy_list, &b->heavy_off, &b->heavy_k0, &b->heavy_k1, &b->heavy_tmp, &b->hit_count, &b->hit_begin, &b->hit_cursor, &b->raw_hits, &b->counters, &b->small, &b->shards, &b->big_list, &b->tb_items, &b->tb_ops,
                      &b->tb_len, &b->band_moves, &b->pack,
                      &b->g_sorted, &b->g_ord, &b->g_lead, &b->g_krank, &b->g_khash, &b->g_nmatch, &b->g_mbegin, &b->g_multi, &b->g_big, &b->g_bigdone, &b->g_sk0, &b->g_sk1, &b->g_si0, &b->g_si1, &b->g_matches, &b->g_mhit, &b->g_positions,
                      &b->scan_tmp, &b->o_small, &b->o_posmatch, &b->o_post, &b->o_mapq, &b->o_emit, &b->o_reccnt, &b->o_cigcnt, &b->o_cigall, &b->o_recoff, &b->o_cigoff,
                      &b->o_recs, &b->o_pool, &b->o_codes, &b->snp_scratch, &b->snp_hmm, &b->pair_fb, &b->pair_list,
                      &b->t_names, &b->t_nameoff, &b->t_qtail, &b->t_qtailoff, &b->t_slots, &b->t_rowlen, &b->t_rowoff, &b->t_text, &b->t_bad, &b->t_bammeta, &b->full_len, &b->d_adaptor,
                      &b->t_status, &b->t_rowcnt, &b->t_rowflag, &b->t_rowfirst, &b->t_rowucum, &b->t_rowsrc,
                      &b->m_span, &b->m_first, &b->m_end, &b->m_prim, &b->m_proper, &b->m_meta, &b->m_fields, &b->m_namelen, &b->m_nameoff, &b->m_names,
                      &b->rt_text, &b->rt_tilecnt, &b->rt_tileoff, &b->rt_lineat, &b->rt_lsum, &b->rt_lin, &b->rt_recs, &b->rt_nlen, &b->rt_tlen, &b->rt_meta };
    for (DevBuf* d : all) d->release();
    b->bz.release();
    for (auto e : b->bam_ev) if (e) (void)hipEventDestroy(e);
    PinBuf* pins[] = { &b->h_top, &b->h_hbegin, &b->h_ord, &b->h_post, &b->h_mapq, &b->h_emit, &b->h_mhit, &b->h_stat, &b->h_rt };
    for (PinBuf* d : pins) d->release();
    for (int i = 0; i < gm_batch::NS; ++i) { if (b->sub_streams[i]) (void)hipStreamDestroy(b->sub_streams[i]); b->sub_gk[i].release(); b->sub_gv[i].release(); }
    if (b->sub_ready) (void)hipEventDestroy(b->sub_ready);
    b->sub_counters.release(); b->sub_small.release(); b->sub_shards.release();
    for (auto& ev : b->pending) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto ev : b->pool) (void)hipEventDestroy(ev);
    delete b;
}

// rows of the seed table: what one strand of a row of `stride` characters can yield under these -m / -j
static uint32_t seed_rows(uint32_t stride, const gm_params* p) {
    const uint32_t last = stride > (uint32_t)p->mer ? stride - (uint32_t)p->mer : 0;
    return last / (uint32_t)p->jump + 2;
}

static int ensure_batch_buffers(gm_batch* b, const gm_params* p) {
    const size_t n = b->n, n2 = 2 * (size_t)b->n;
    b->max_seeds = seed_rows(b->stride, p);
    int rc = 0;
    rc |= b->status.ensure(n); rc |= b->self_score.ensure(n * 4); rc |= b->min_score.ensure(n * 8); rc |= b->top_score.ensure(n * 4);
    rc |= b->seeds.ensure(n2 * b->max_seeds * sizeof(GmSeed)); rc |= b->n_seeds.ensure(n2 * 2); rc |= b->n_entries.ensure(n2 * 4);
    rc |= b->entry_off.ensure((n2 + 1) * 8); rc |= b->rs_overflow.ensure(n2); rc |= b->retry_list.ensure(n2 * 4);
    rc |= b->retry_off.ensure((n2 + 1024) * 8); rc |= b->big_list.ensure(n2 * 4 + 64);
    rc |= b->hit_count.ensure(n * 4); rc |= b->hit_begin.ensure((n + 1) * 8); rc |= b->hit_cursor.ensure(n * 4);
    rc |= b->counters.ensure(GMK_N * 8); rc |= b->small.ensure(64); rc |= b->shards.ensure((size_t)GM_NSHARD * GM_SHARD_STRIDE * 4);
    if (b->cand_cap < 16 * n + 64 * GM_NSHARD) { b->cand_cap = (uint32_t)std::min<size_t>(16 * n + 64 * GM_NSHARD, 0x7FFFFFFF); }
    rc |= b->cands.ensure((size_t)b->cand_cap * sizeof(GmCand));
    return rc ? GM_E_NOMEM : GM_OK;
}

// what the resident block defines.  The kernel form of a map call (pack, fixed_cands, fixed_cnt, fixed_epoch) is not the batch's: it
// stays null / 0 here, and map_fill_dev puts it on top for the length of that call
static void fill_dev_batch(gm_batch* b) {
    GmDevBatch& d = b->dev;
    d.n = b->n; d.stride = b->stride; d.max_seeds = b->max_seeds; d.illumina_until = b->illumina_until; d.read_base = 0; d.fasta = b->fasta ? 1u : 0u;
    d.bases = b->bases.as<uint8_t>(); d.quals = b->quals.as<uint8_t>(); d.len = b->len.as<uint16_t>();
    d.status = b->status.as<int8_t>(); d.self_score = b->self_score.as<float>(); d.min_score = b->min_score.as<double>();
    d.top_score = b->top_score.as<float>(); d.seeds = b->seeds.as<GmSeed>(); d.n_seeds = b->n_seeds.as<uint16_t>();
    d.n_entries = b->n_entries.as<uint32_t>(); d.entry_off = b->entry_off.as<uint64_t>(); d.coords = b->coords.as<uint32_t>();
    d.rs_overflow = b->rs_overflow.as<uint8_t>(); d.retry_list = b->retry_list.as<uint32_t>(); d.retry_off = b->retry_off.as<uint64_t>();
    d.gtab_keys = b->gtab_keys.as<uint32_t>(); d.gtab_vals = b->gtab_vals.as<uint32_t>();
    d.cands = b->cands.as<GmCand>(); d.cand_cap = b->cand_cap; d.cand_region = b->cand_cap / GM_NSHARD;
    d.shard_cnt = b->shards.as<uint32_t>();
    d.fixed_cands = nullptr; d.fixed_cnt = nullptr; d.fixed_epoch = 0;
    d.hit_count = b->hit_count.as<uint32_t>(); d.hit_begin = b->hit_begin.as<uint64_t>(); d.hit_cursor = b->hit_cursor.as<uint32_t>();
    d.raw_hits = b->raw_hits.as<GmRawHit>(); d.raw_cap = b->raw_cap;
    d.counters = b->counters.as<unsigned long long>();
    d.n_retry = b->small.as<uint32_t>() + 1; d.n_big = b->small.as<uint32_t>() + 2; d.big_list = b->big_list.as<uint32_t>();
    d.band_moves = b->band_moves.as<unsigned long long>(); d.band_moves_words = b->band_moves.cap / 8;
    d.pack = nullptr; d.pack_w2 = gm_pack_w2(b->stride); d.pack_words = gm_pack_words(b->stride);
}

extern "C" int gm_batch_upload(gm_batch* b, const gm_params* p, const gm_reads* r, void* stream) {
    if (!b || !p || !r || !p->finalized) return GM_E_ARG;
    if (r->n > b->max_reads || r->stride > 2048) { gm_set_error("batch larger than gm_batch_create allowed, or reads longer than 2048 bases"); return GM_E_ARG; }
    if (r->stride % 8 != 0) { gm_set_error("gm_reads.stride must be a multiple of 8"); return GM_E_ARG; }
    const bool fasta = b->read_format == GM_READS_FASTA;
    if (fasta && !b->adaptor.empty()) { gm_set_error("a FASTA block with an adaptor set: the reference trims FASTA reads with the PWM-based FixReads, which is not built (gm_batch_set_adaptor(NULL) first)"); return GM_E_UNSUPPORTED; }
    if (r->n && (!r->bases || !r->len || (!fasta && !r->quals))) { gm_set_error("gm_reads: bases, len" + std::string(fasta ? "" : ", quals") + " must not be NULL"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(b->ix->device));
    hipStream_t st = S_(stream);
    b->n = r->n; b->stride = r->stride; b->mapped = false; b->cache_hits = b->cache_matches = 0; b->resume_ptr = nullptr; b->stamp = 0;
    b->fasta = fasta; b->text_block = b->text_pools = false;
    size_t bytes = (size_t)r->n * r->stride;
    if (b->bases.ensure(bytes + 16) || (!fasta && b->quals.ensure(bytes + 16)) || b->len.ensure((size_t)r->n * 2 + 16)) return GM_E_NOMEM;
    b->len_host.assign(r->len, r->len + r->n);
    b->len_max = 0; b->len_min = r->n ? 0xFFFFFFFFu : 0u;
    for (uint32_t i = 0; i < r->n; ++i) {
        if (r->len[i] > r->stride) { gm_set_error("read longer than stride"); return GM_E_ARG; }
        b->len_max = std::max<uint32_t>(b->len_max, r->len[i]);
        b->len_min = std::min<uint32_t>(b->len_min, r->len[i]);
    }
    const bool trim = !b->adaptor.empty() && r->n != 0;
    if (bytes) {
        HIPCHK(hipMemcpyAsync(b->bases.p, r->bases, bytes, hipMemcpyHostToDevice, st));
        if (!fasta) HIPCHK(hipMemcpyAsync(b->quals.p, r->quals, bytes, hipMemcpyHostToDevice, st));      // (a FASTA block is its letters: half the bytes)
        if (!trim) HIPCHK(hipMemcpyAsync(b->len.p, r->len, (size_t)r->n * 2, hipMemcpyHostToDevice, st));
    }
    if (trim) {
        // -A (SeqReader.cpp:1146-1150): the lengths as uploaded stay in full_len (SEQ / QUAL of a SAM row are the whole lines, :1264-1265),
        // `len` - what every kernel downstream reads - takes what FixReads2 keeps, and the host's copy follows: one small wait per upload
        if (b->full_len.ensure((size_t)r->n * 2 + 16) || b->d_adaptor.ensure(GM_ADAPTOR_MAX)) return GM_E_NOMEM;
        if (b->adaptor_dirty) { HIPCHK(hipMemcpyAsync(b->d_adaptor.p, b->adaptor.data(), b->adaptor.size(), hipMemcpyHostToDevice, st)); b->adaptor_dirty = false; }
        HIPCHK(hipMemcpyAsync(b->full_len.p, r->len, (size_t)r->n * 2, hipMemcpyHostToDevice, st));
        hipEvent_t ea = nullptr, ee = nullptr;
        if (b->profiling) { if (hipEventCreate(&ea) != hipSuccess || hipEventCreate(&ee) != hipSuccess) { if (ea) (void)hipEventDestroy(ea); ea = ee = nullptr; } }
        if (ea) (void)hipEventRecord(ea, st);
        const int krc = gmk_adaptor_trim(b->bases.as<uint8_t>(), r->stride, b->full_len.as<uint16_t>(), r->n, b->d_adaptor.as<uint8_t>(), (uint32_t)b->adaptor.size(),
                                         b->len.as<uint16_t>(), st);
        if (ea) (void)hipEventRecord(ee, st);
        hipError_t e1 = krc ? (hipError_t)krc : hipMemcpyAsync(b->len_host.data(), b->len.p, (size_t)r->n * 2, hipMemcpyDeviceToHost, st);
        if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
        if (ea) { float ms = 0.0f; if (e1 == hipSuccess && hipEventElapsedTime(&ms, ea, ee) == hipSuccess) { b->adaptor_ms += ms; ++b->adaptor_launches; } (void)hipEventDestroy(ea); (void)hipEventDestroy(ee); }
        if (e1 != hipSuccess) { gm_set_error(std::string("k_adaptor_trim: ") + hipGetErrorString(e1)); return GM_E_HIP; }
        b->len_max = 0; b->len_min = 0xFFFFFFFFu;                 // a block whose reads all keep one length takes the one-length DP / prep kernels
        for (uint32_t i = 0; i < r->n; ++i) { b->len_max = std::max<uint32_t>(b->len_max, b->len_host[i]); b->len_min = std::min<uint32_t>(b->len_min, b->len_host[i]); }
    }
    // --illumina with automatic fallback (SeqReader.cpp:1171-1180): reads before the first one that shows a
    // quality below '@' keep Phred+64, that read and all later ones use Phred+33 (with -A only the kept characters are looked at, :1152)
    b->illumina_until = 0; b->up_illumina = p->illumina != 0;
    if (p->illumina && !fasta) {                                   // (--illumina is accepted and ignored for FASTA, as in the reference)
        uint32_t until = r->n;
        for (uint32_t i = 0; i < r->n && until == r->n; ++i) {
            const uint8_t* q = r->quals + (size_t)i * r->stride;
            for (uint32_t t = 0; t < b->len_host[i]; ++t) if ((int8_t)q[t] < 64) { until = i; break; }      // `int Q = (int)fastq[i]` (SeqReader.cpp:1155): a signed char
        }
        b->illumina_until = until;
    }
    int rc = ensure_batch_buffers(b, p);
    if (rc) return rc;
    fill_dev_batch(b);
    return GM_OK;
}

// ------------------------------------------------------------------------------------------------
// gm_batch_upload_text = gm_batch_upload for reads that are still FASTQ text: the text goes up as it stands and the kernels of
// gm_readtext.hip cut it into the rows, lengths, names and quality tails the other kernels read.  Two small waits: the number of
// lines (sizes the line and record tables), then n / longest read / first bad record / byte sums together with the lengths (size the
// rows and the pools).  With -A or --illumina one more, for what the trim kept and the fallback index.
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(gm_text_rec) == sizeof(GmDevTextRec) && offsetof(gm_text_rec, name_off) == offsetof(GmDevTextRec, name_off) &&
              offsetof(gm_text_rec, seq_off) == offsetof(GmDevTextRec, seq_off) && offsetof(gm_text_rec, qual_off) == offsetof(GmDevTextRec, qual_off) &&
              offsetof(gm_text_rec, name_len) == offsetof(GmDevTextRec, name_len) && offsetof(gm_text_rec, seq_len) == offsetof(GmDevTextRec, seq_len) &&
              offsetof(gm_text_rec, qual_len) == offsetof(GmDevTextRec, qual_len), "gm_text_rec layout");

extern "C" int gm_batch_upload_text(gm_batch* b, const gm_params* p, const char* text, uint64_t bytes, gm_text_info* info, gm_text_rec* recs, uint64_t recs_cap,
                                    void* stream) {
    if (!b) { gm_set_error("gm_batch_upload_text: batch is NULL"); return GM_E_ARG; }
    if (b->ix->host_only) { gm_set_error("gm_batch_upload_text: no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (!p || !p->finalized || !info || (bytes && !text)) { gm_set_error("gm_batch_upload_text: params (finalized), info and text must not be NULL"); return GM_E_ARG; }
    memset(info, 0, sizeof *info);
    if (b->read_format == GM_READS_FASTA) { gm_set_error("gm_batch_upload_text: the batch is set to GM_READS_FASTA; FASTQ text only"); return GM_E_UNSUPPORTED; }
    HIPCHK(hipSetDevice(b->ix->device));
    hipStream_t st = S_(stream);
    // until the end of this call nothing is resident
    b->n = 0; b->mapped = false; b->cache_hits = b->cache_matches = 0; b->resume_ptr = nullptr; b->stamp = 0; b->fasta = false;
    b->text_block = b->text_pools = false; b->text_name_bytes = b->text_tail_bytes = 0; b->len_host.clear(); b->len_max = b->len_min = 0; b->illumina_until = 0;
    if (bytes >= (1ull << 32)) {
        gm_set_error("gm_batch_upload_text: " + std::to_string(bytes) + " bytes of text; the limit is bytes < 2^32 per call (offsets are 32 bits): cut the text at a record start");
        return GM_E_ARG;
    }
    const bool adaptor = !b->adaptor.empty();
    uint32_t n = 0, maxlen = 0, minlen = 0;
    GmDevReadText t{};
    if (bytes) {
        if (b->h_rt.ensure((RT_META_N_WORDS + 2) * 8)) return GM_E_NOMEM;
        unsigned long long* const hm = b->h_rt.as<unsigned long long>();
        t.n_tiles = gmk_readtext_tiles(bytes);
        if (b->rt_text.ensure((size_t)bytes + 64) || b->rt_tilecnt.ensure((size_t)t.n_tiles * 4) || b->rt_tileoff.ensure(((size_t)t.n_tiles + 1) * 4) ||
            b->rt_meta.ensure(RT_META_N_WORDS * 8)) return GM_E_NOMEM;
        t.text = b->rt_text.as<uint8_t>(); t.bytes = bytes; t.tile_cnt = b->rt_tilecnt.as<uint32_t>(); t.tile_off = b->rt_tileoff.as<uint32_t>();
        t.meta = b->rt_meta.as<unsigned long long>();
        for (int i = 0; i < RT_META_N_WORDS; ++i) hm[i] = 0ull;
        hm[RT_META_BAD] = ~0ull; hm[RT_META_MINLEN] = ~0ull;
        HIPCHK(hipMemcpyAsync(b->rt_meta.p, hm, RT_META_N_WORDS * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b->rt_text.p, text, (size_t)bytes, hipMemcpyHostToDevice, st));
        KCHK(gmk_readtext_count(t, st));
        HIPCHK(hipMemcpyAsync(&hm[RT_META_N_WORDS], t.meta + RT_META_LINES, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const unsigned long long lines = hm[RT_META_N_WORDS];
        if (lines == 0 || lines > bytes) { gm_set_error("internal: gm_batch_upload_text counted " + std::to_string(lines) + " lines in " + std::to_string(bytes) + " bytes"); return GM_E_HIP; }
        t.n_lines = (uint32_t)lines; t.n_ltiles = gmk_readtext_line_tiles(lines); t.rec_cap = (uint32_t)(lines / 4 + 1);
        DevBuf& len_as_read = adaptor ? b->full_len : b->len;       // with -A the lengths as they stand in the text go to full_len, as in gm_batch_upload
        if (b->rt_lineat.ensure((size_t)lines * 4) || b->rt_lsum.ensure((size_t)t.n_ltiles * 32) || b->rt_lin.ensure((size_t)t.n_ltiles * 8) ||
            b->rt_recs.ensure((size_t)t.rec_cap * sizeof(GmDevTextRec)) || len_as_read.ensure((size_t)t.rec_cap * 2 + 16) ||
            b->rt_nlen.ensure((size_t)t.rec_cap * 4) || b->rt_tlen.ensure((size_t)t.rec_cap * 4)) return GM_E_NOMEM;
        t.line_at = b->rt_lineat.as<uint32_t>(); t.ltile_sum = b->rt_lsum.as<uint32_t>(); t.ltile_in = b->rt_lin.as<uint32_t>();
        t.recs = b->rt_recs.as<GmDevTextRec>(); t.len = len_as_read.as<uint16_t>(); t.name_len = b->rt_nlen.as<uint32_t>(); t.tail_len = b->rt_tlen.as<uint32_t>();
        KCHK(gmk_readtext_records(t, st));
        b->len_host.resize(t.rec_cap);
        HIPCHK(hipMemcpyAsync(hm, t.meta, RT_META_N_WORDS * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(b->len_host.data(), t.len, (size_t)t.rec_cap * 2, hipMemcpyDeviceToHost, st));     // n is not known yet: the table's bound, n x 2 bytes for a well-formed text
        HIPCHK(hipStreamSynchronize(st));
        const unsigned long long all = hm[RT_META_RECS], nn = hm[RT_META_N];
        if (nn > all || all > t.rec_cap) { b->len_host.clear(); gm_set_error("internal: gm_batch_upload_text found more records than four lines each allow"); return GM_E_HIP; }
        n = (uint32_t)nn;
        info->n = n;
        if (nn < all) { info->status = (hm[RT_META_BAD] & 3ull) == RT_BAD_LONG ? GM_TEXT_TOO_LONG : GM_TEXT_MALFORMED; info->bad_at = hm[RT_META_BAD_AT]; }
        if (n) { maxlen = (uint32_t)hm[RT_META_MAXLEN]; minlen = (uint32_t)hm[RT_META_MINLEN]; }
        b->text_name_bytes = hm[RT_META_NAME_BYTES]; b->text_tail_bytes = hm[RT_META_TAIL_BYTES];
        b->len_host.resize(n);
    }
    info->max_len = maxlen; info->stride = std::max<uint32_t>(8u, (maxlen + 7u) & ~7u);
    if (n > b->max_reads) {
        b->len_host.clear();
        gm_set_error("gm_batch_upload_text: " + std::to_string(n) + " records in the text; the limit is gm_batch_create's max_reads = " + std::to_string(b->max_reads));
        return GM_E_ARG;
    }
    if (recs && n > recs_cap) { b->len_host.clear(); gm_set_error("gm_batch_upload_text: recs has room for fewer records than the text holds"); return GM_E_CAPACITY; }
    const uint32_t stride = info->stride;
    if (n) {
        const size_t row_bytes = (size_t)n * stride;
        unsigned long long* const hm = b->h_rt.as<unsigned long long>();
        if (b->bases.ensure(row_bytes + 16) || b->quals.ensure(row_bytes + 16) || b->len.ensure((size_t)n * 2 + 16) || b->t_names.ensure((size_t)b->text_name_bytes + 16) ||
            b->t_nameoff.ensure(((size_t)n + 1) * 8) || b->t_qtail.ensure((size_t)b->text_tail_bytes + 16) || b->t_qtailoff.ensure(((size_t)n + 1) * 8) ||
            b->scan_tmp.ensure(((size_t)n / 1024 + 8) * 8)) return GM_E_NOMEM;
        KCHK(gmk_scan_u32(t.name_len, n, b->t_nameoff.as<uint64_t>(), b->scan_tmp.as<unsigned long long>(), st));
        KCHK(gmk_scan_u32(t.tail_len, n, b->t_qtailoff.as<uint64_t>(), b->scan_tmp.as<unsigned long long>(), st));
        KCHK(gmk_readtext_rows(t, n, stride, b->bases.as<uint8_t>(), b->quals.as<uint8_t>(), st));
        KCHK(gmk_readtext_names(t, n, b->t_names.as<char>(), b->t_nameoff.as<uint64_t>(), b->t_qtail.as<char>(), b->t_qtailoff.as<uint64_t>(), st));
        if (recs) HIPCHK(hipMemcpyAsync(recs, t.recs, (size_t)n * sizeof(gm_text_rec), hipMemcpyDeviceToHost, st));
        if (adaptor) {                                             // as gm_batch_upload: `len` takes what FixReads2 keeps, the host's copy follows
            if (b->d_adaptor.ensure(GM_ADAPTOR_MAX)) return GM_E_NOMEM;
            if (b->adaptor_dirty) { HIPCHK(hipMemcpyAsync(b->d_adaptor.p, b->adaptor.data(), b->adaptor.size(), hipMemcpyHostToDevice, st)); b->adaptor_dirty = false; }
            KCHK(gmk_adaptor_trim(b->bases.as<uint8_t>(), stride, b->full_len.as<uint16_t>(), n, b->d_adaptor.as<uint8_t>(), (uint32_t)b->adaptor.size(), b->len.as<uint16_t>(), st));
            HIPCHK(hipMemcpyAsync(b->len_host.data(), b->len.p, (size_t)n * 2, hipMemcpyDeviceToHost, st));
        }
        uint32_t* const h_until = reinterpret_cast<uint32_t*>(&hm[RT_META_N_WORDS + 1]);
        uint32_t* const d_until = reinterpret_cast<uint32_t*>(t.meta + RT_META_N_WORDS - 1);
        if (p->illumina) {                                         // the smallest read with a quality below '@' in what is kept of it (SeqReader.cpp:1152-1180)
            *h_until = n;
            HIPCHK(hipMemcpyAsync(d_until, h_until, 4, hipMemcpyHostToDevice, st));
            KCHK(gmk_readtext_illumina(b->quals.as<uint8_t>(), stride, b->len.as<uint16_t>(), n, d_until, st));
            HIPCHK(hipMemcpyAsync(h_until, d_until, 4, hipMemcpyDeviceToHost, st));
        }
        if (recs || adaptor || p->illumina) HIPCHK(hipStreamSynchronize(st));
        if (p->illumina) b->illumina_until = *h_until;
        if (adaptor) {
            maxlen = 0; minlen = 0xFFFFFFFFu;
            for (uint32_t i = 0; i < n; ++i) { maxlen = std::max<uint32_t>(maxlen, b->len_host[i]); minlen = std::min<uint32_t>(minlen, b->len_host[i]); }
        }
    }
    b->n = n; b->stride = stride; b->len_max = maxlen; b->len_min = minlen; b->up_illumina = p->illumina != 0;
    const int rc = ensure_batch_buffers(b, p);
    if (rc) { b->n = 0; b->len_host.clear(); return rc; }
    fill_dev_batch(b);
    b->text_block = b->text_pools = true;
    return GM_OK;
}

// gm_batch_set_row_tags with gm_batch_set_adaptor: with -A a row's SEQ is the whole read and its CIGAR covers the kept part, so a tag
// of the row as printed would describe nothing.  Whichever setter comes second refuses, so no output call meets the two together
static std::string row_tags_adaptor_text(const char* who) {
    return std::string(who) + ": GM_ROW_TAG_MD (gm_batch_set_row_tags) and an adaptor (gm_batch_set_adaptor) on one batch: with an adaptor SEQ is the whole read and the "
           "CIGAR covers the kept part, so NM / MD of the row as printed would describe nothing";
}

// -A / --adaptor (Driver.cpp:2793-2798: the string exactly as given).  Takes effect with the next upload; NULL or "" clears it.
extern "C" int gm_batch_set_adaptor(gm_batch* b, const char* adaptor) {
    if (!b) { gm_set_error("gm_batch_set_adaptor: batch is NULL"); return GM_E_ARG; }
    const size_t n = adaptor ? strlen(adaptor) : 0;
    if (n > GM_ADAPTOR_MAX) { gm_set_error("gm_batch_set_adaptor: an adaptor of at most 256 characters"); return GM_E_ARG; }
    if (n && b->row_tags) { gm_set_error(row_tags_adaptor_text("gm_batch_set_adaptor")); return GM_E_UNSUPPORTED; }
    b->adaptor.assign(adaptor ? adaptor : "", n);
    b->adaptor_dirty = n != 0;
    return GM_OK;
}

// which of SeqReader::find_type's formats (src/SeqReader.cpp:175-244) the blocks uploaded from now on are in
extern "C" int gm_batch_set_read_format(gm_batch* b, int format) {
    if (!b) { gm_set_error("gm_batch_set_read_format: batch is NULL"); return GM_E_ARG; }
    if (format != GM_READS_FASTQ && format != GM_READS_FASTA) { gm_set_error("gm_batch_set_read_format: GM_READS_FASTQ or GM_READS_FASTA"); return GM_E_ARG; }
    b->read_format = format;
    return GM_OK;
}

// A defined extension: the reference prints no row for a read that does not map.  Takes effect with the next
// row-producing output call; gm_output_batch (records) does not read it.
extern "C" int gm_batch_set_unmapped_rows(gm_batch* b, int on) {
    if (!b) { gm_set_error("gm_batch_set_unmapped_rows: batch is NULL"); return GM_E_ARG; }
    b->unmapped_rows = on != 0;
    return GM_OK;
}

extern "C" int gm_batch_unmapped_rows(gm_batch* b, uint64_t* n) {
    if (!b || !n) { gm_set_error("gm_batch_unmapped_rows: batch or n is NULL"); return GM_E_ARG; }
    *n = b->n_unmapped;
    return GM_OK;
}

// Two more defined extensions, read by the six row-producing output calls from the next call on; gm_output_batch
// (records) reads neither.  Row tags: NM:i and MD:Z of the row as printed, behind X0, on every row whose CIGAR field is not "*".
// gm_batch_set_mates: the setting is only stored here; an odd block and limits the wrong way round are refused by the output call
extern "C" int gm_batch_set_mates(gm_batch* b, int on, uint32_t min_insert, uint32_t max_insert) {
    if (!b) { gm_set_error("gm_batch_set_mates: batch is NULL"); return GM_E_ARG; }
    b->mates = on != 0; b->mate_min = min_insert; b->mate_max = max_insert;
    return GM_OK;
}

static_assert(sizeof(gm_mate_row) == 16 && sizeof(GmDevMateRow) == 16 && offsetof(gm_mate_row, rnext) == offsetof(GmDevMateRow, rnext) &&
              offsetof(gm_mate_row, pnext) == offsetof(GmDevMateRow, pnext) && offsetof(gm_mate_row, tlen) == offsetof(GmDevMateRow, tlen), "gm_mate_row layout");
extern "C" int gm_batch_mate_rows(gm_batch* b, gm_mate_row* out, uint64_t cap, uint64_t* n) {
    if (!b || !n) { gm_set_error("gm_batch_mate_rows: batch or n is NULL"); return GM_E_ARG; }
    *n = b->mate_n_rows;
    if (b->mate_n_rows > cap) { gm_set_error("gm_batch_mate_rows: room for " + std::to_string(cap) + " rows, the last output call left " + std::to_string(b->mate_n_rows)); return GM_E_CAPACITY; }
    if (!b->mate_n_rows) return GM_OK;
    if (!out) { gm_set_error("gm_batch_mate_rows: out is NULL"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(b->ix->device));
    HIPCHK(hipMemcpy(out, b->m_fields.p, (size_t)b->mate_n_rows * sizeof(gm_mate_row), hipMemcpyDeviceToHost));
    return GM_OK;
}

extern "C" int gm_batch_mate_stats(gm_batch* b, gm_mate_stats* out) {
    if (!b || !out) { gm_set_error("gm_batch_mate_stats: batch or out is NULL"); return GM_E_ARG; }
    *out = b->mate_stats;
    return GM_OK;
}

extern "C" int gm_batch_set_row_tags(gm_batch* b, uint32_t tags) {
    if (!b) { gm_set_error("gm_batch_set_row_tags: batch is NULL"); return GM_E_ARG; }
    if (tags & ~(uint32_t)GM_ROW_TAG_MD) { gm_set_error("gm_batch_set_row_tags: GM_ROW_TAG_MD or 0, not " + std::to_string(tags)); return GM_E_ARG; }
    if (tags && !b->adaptor.empty()) { gm_set_error(row_tags_adaptor_text("gm_batch_set_row_tags")); return GM_E_UNSUPPORTED; }
    if (tags && !b->ix->h.amb_found) {
        gm_set_error("gm_batch_set_row_tags: cannot read or parse " + b->ix->h.amb_path + ": MD:Z prints the reference's own letter where the FASTA holds another than ACGT");
        return GM_E_IO;
    }
    b->row_tags = tags;
    return GM_OK;
}

// Minus-strand rows: GM_CIGAR_GNUMAP prints the tokens last to first, as the reference does; GM_CIGAR_FORWARD prints the pool's bytes as
// a plus-strand row does - the order the traceback computed them in, against the forward window
extern "C" int gm_batch_set_cigar_order(gm_batch* b, int order) {
    if (!b) { gm_set_error("gm_batch_set_cigar_order: batch is NULL"); return GM_E_ARG; }
    if (order != GM_CIGAR_GNUMAP && order != GM_CIGAR_FORWARD) { gm_set_error("gm_batch_set_cigar_order: GM_CIGAR_GNUMAP or GM_CIGAR_FORWARD, not " + std::to_string(order)); return GM_E_ARG; }
    b->cigar_order = order;
    return GM_OK;
}

extern "C" int gm_index_set_probe_format(gm_index* ix, int format) {
    if (!ix) { gm_set_error("gm_index_set_probe_format: index is NULL"); return GM_E_ARG; }
    if (format != GM_READS_FASTQ && format != GM_READS_FASTA) { gm_set_error("gm_index_set_probe_format: GM_READS_FASTQ or GM_READS_FASTA"); return GM_E_ARG; }
    ix->probe_format = format;
    return GM_OK;
}

// a kernel form that only an A/B switch selects and that was not taught FASTA blocks: the DP score kernel k_nw.  Such a block with the
// switch set is refused, by name.  (GM_PREP=tile and GM_TRACEBACK=group are no such forms: k_prep and k_traceback are what blocks with
// rows beyond 152 / 511 bytes take, FASTA included.)
// Every way into gmk_nw passes here first: gm_map_batch_device (before its pipelined and its single-pass form) and gm_dev_nw_score;
// gmk_nw itself fails the launch for a FASTA block in the wave form, should a new caller forget.
static int fasta_forced_form(const gm_batch* b) {
    if (!b->fasta) return GM_OK;
    const char* sw = gm_opt_is("GM_NW", "wave") ? "GM_NW=wave" : nullptr;
    if (!sw) return GM_OK;
    gm_set_error(std::string("a FASTA block with ") + sw + ": that kernel form takes FASTQ blocks only (unset the switch)");
    return GM_E_UNSUPPORTED;
}

extern "C" int gm_batch_trimmed_len(gm_batch* b, uint16_t* out) {
    if (!b || (b->n && !out)) return GM_E_ARG;
    if (b->len_host.size() < b->n) { gm_set_error("gm_batch_trimmed_len: no block uploaded"); return GM_E_ARG; }
    if (b->n) memcpy(out, b->len_host.data(), (size_t)b->n * 2);
    return GM_OK;
}

extern "C" int gm_batch_adaptor_time(gm_batch* b, double* ms, uint64_t* launches) {
    if (!b || !ms || !launches) return GM_E_ARG;
    *ms = b->adaptor_ms; *launches = b->adaptor_launches;
    b->adaptor_ms = 0; b->adaptor_launches = 0;
    return GM_OK;
}

// k_adaptor_trim on a caller's block (unit level, parity tests): out_len[i] = what FixReads2 keeps of read i; only bases and len are read
extern "C" int gm_dev_adaptor_trim(gm_index* ix, const gm_reads* reads, const char* adaptor, uint16_t* out_len) {
    if (!ix || !reads || (reads->n && (!reads->bases || !reads->len || !out_len))) return GM_E_ARG;
    const size_t a_len = adaptor ? strlen(adaptor) : 0;
    if (a_len > GM_ADAPTOR_MAX) { gm_set_error("gm_dev_adaptor_trim: an adaptor of at most 256 characters"); return GM_E_ARG; }
    if (reads->stride % 8 != 0 || reads->stride > 2048) { gm_set_error("gm_reads.stride must be a multiple of 8, at most 2048"); return GM_E_ARG; }
    for (uint32_t i = 0; i < reads->n; ++i) if (reads->len[i] > reads->stride) { gm_set_error("read longer than stride"); return GM_E_ARG; }
    if (ix->host_only) { gm_set_error("no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (reads->n == 0) return GM_OK;
    if (a_len == 0) { memcpy(out_len, reads->len, (size_t)reads->n * 2); return GM_OK; }      // no adaptor: every read keeps its length
    HIPCHK(hipSetDevice(ix->device));
    DevBuf db, dl, da, dout;
    const size_t bytes = (size_t)reads->n * reads->stride;
    int rc = GM_OK;
    if (db.ensure(bytes + 16) || dl.ensure((size_t)reads->n * 2) || da.ensure(GM_ADAPTOR_MAX) || dout.ensure((size_t)reads->n * 2)) rc = GM_E_NOMEM;
    auto run = [&]() -> int {
        if (bytes) HIPCHK(hipMemcpy(db.p, reads->bases, bytes, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dl.p, reads->len, (size_t)reads->n * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(da.p, adaptor, a_len, hipMemcpyHostToDevice));
        KCHK(gmk_adaptor_trim(db.as<uint8_t>(), reads->stride, dl.as<uint16_t>(), reads->n, da.as<uint8_t>(), (uint32_t)a_len, dout.as<uint16_t>(), nullptr));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out_len, dout.p, (size_t)reads->n * 2, hipMemcpyDeviceToHost));
        return GM_OK;
    };
    if (rc == GM_OK) rc = run();
    db.release(); dl.release(); da.release(); dout.release();
    return rc;
}

// ------------------------------------------------------------------------------------------------
// gm_map_batch_device: prep -> seed -> vote -> NW -> compaction of the resident block, as named steps
//
// MapForm: which kernels one call runs.  map_choose_form decides it once, from the index, this call's parameters, the resident block
// and the GM_* switches; it is a value of the call, never stored in the batch.
struct MapForm {
    int use_full = 0;                   // the index holds the full suffix array (no sampled-SA locate pass)
    int dense = 0;                      // gmk_vote's kernel class: 0 = sparse, 1 = k_vote_slots / k_vote_tiny*, 2 = the 64-slot form, 3 = k_vote_block
    int slots_hint = 40;                // expected 64-lane slots per read x strand (picks the k_vote_slots form; 0 / -1: k_vote_tiny / k_vote_tiny2)
    int fused = 0;                      // the vote kernels look their seeds up themselves: no k_seed launch (GmDevParams::fused)
    bool use_bucket = false;            // ... in the bucket table: k_vote_bucket + the list kernel instead of gmk_vote
    uint32_t bucket_reg = 0;            // its seed positions per strand (the kernel's template size)
    bool use_pair = false;              // k_vote_pair in front of k_vote_bucket: two reads per wavefront
    bool pair_direct = false;           // ... handing its results straight to the shards and the flagged reads' list
    bool use_fixed = false;             // candidates in own slots per read x strand, gathered by k_cand_gather
    bool use_pack = false;              // k_prep writes the 2-bit read forms of the fused seed lookup
    uint32_t heavy_min = 0;             // read x strands with more SA hits go to the sorted-key path of gm_heavy.hip
    uint64_t heavy_budget = 0;          // keys per chunk of that path
    uint32_t sub_n = 0;                 // GM_PIPELINE: the sub-batch size asked for
    bool pipeline = false;              // ... and the block is large enough for map_pipelined to be tried first
};

// Decides, and nothing else: no launch, no memset, no ensure().
static MapForm map_choose_form(const gm_index* ix, const gm_params* p, const gm_batch* b, const GmDevParams& dp) {
    MapForm f;
    f.use_full = ix->full_sa ? 1 : 0;
    // which vote kernel: expected SA hits per seed ~ reference length / 4^mer (capped by -h), expected seeds per strand from the
    // longest read.  0 = sparse (<= 16 hits per read x strand fit a 16-lane group), 1 = k_vote_slots (its hits fit 40 slots of
    // 64 lanes), 2 = its 64-slot form, 3 = k_vote_block (more: rounds of 2048 hits).  GM_VOTE=wave|block|big|rounds forces 0..3, GM_VOTE_KERNEL the dense form.
    {
        double per_seed = (double)ix->h.seq_len / pow(4.0, (double)std::min(p->mer, 31));
        if (p->max_kmer_hits > 0) per_seed = std::min(per_seed, (double)p->max_kmer_hits);
        const double L = (double)b->stride;
        double ns = L > p->mer ? floor((L - p->mer - 1) / std::max(1, p->jump)) + 1 : 1;
        if (p->nw && p->fast) ns = 1;
        ns = std::min(ns, (double)b->max_seeds);
        const double e_exp = ns * (1.0 + per_seed);                                      // the true locus + chance hits
        const double slots_exp = ns * ceil((per_seed + 3.0 * sqrt(per_seed) + 1.0) / 64.0);
        f.dense = e_exp > 14.0 ? (slots_exp <= 38.0 ? 1 : slots_exp <= 60.0 ? 2 : 3) : 0;
        f.slots_hint = (int)std::min(1000.0, slots_exp);
        // few hits in many short runs (long seeds on a large reference): one wave per read x strand, 16-rank groups (k_vote_tiny)
        const double groups_exp = ns * ceil((per_seed + 3.0 * sqrt(per_seed) + 1.0) / 16.0);
        if (f.dense == 1 && p->min_seed_hits >= 2 && e_exp + 4.0 * sqrt(e_exp) <= 230.0 && groups_exp <= 28.0) f.slots_hint = 0;
        else if (f.dense == 1 && p->min_seed_hits >= 2 && e_exp + 4.0 * sqrt(e_exp) <= 350.0 && groups_exp <= 56.0) f.slots_hint = -1;      // k_vote_tiny2
        if (const char* ev = gm_opt("GM_VOTE_SLOTS")) { if (*ev) f.slots_hint = atoi(ev); }
        if (const char* ev = gm_opt("GM_VOTE")) f.dense = !strcmp(ev, "block") ? 1 : !strcmp(ev, "big") ? 2 : !strcmp(ev, "rounds") ? 3 : !strcmp(ev, "wave") ? 0 : f.dense;
    }
    // optional sub-batch pipeline over several streams for large full-SA batches (GM_PIPELINE=<sub-batch size>).  Measured
    // +4 % at configs[1]: three vote kernels end up sharing the LDS rather than hiding seed / NW work, and per-kernel
    // timings stop being attributable, so it is off by default.
    f.sub_n = (uint32_t)gm_opt_ll("GM_PIPELINE", 0);
    f.pipeline = f.use_full && f.sub_n >= 4096 && b->n >= 3 * (uint64_t)f.sub_n;
    // read x strands with very many SA hits (repeat seeds without -h) leave the ordinary vote kernels before they start: sorted-key
    // path of gm_heavy.hip, routed by the seed search's own hit count.  GM_HEAVY_MIN / GM_HEAVY_BUDGET (keys per chunk) are test switches.
    f.heavy_min = (uint32_t)gm_opt_ll("GM_HEAVY_MIN", 16384);
    f.heavy_budget = (uint64_t)gm_opt_ll("GM_HEAVY_BUDGET", 1ll << 27);
    // seed lookup inside the vote kernels that take one read x strand per wave / workgroup (full SA, the k-mer table covering the
    // whole seed): no k_seed launch, no seed rows through HBM.  A k-mer that does not occur changes the positions of all later ones;
    // the wave then walks again round by round (gm_seed_rewalk_ool), one probe round trip per failing k-mer.  That stays rare while
    // even a k-mer with a sequencing error still occurs somewhere by chance - every k-mer expected >= 4 times in the reference
    // (measured on 100 Mbp: -m 12, 6 per k-mer: 21.0 ms fused against 27.7; -m 14, 0.4 per k-mer: an erroneous k-mer dies one or two
    // characters before its end, the walk creeps past the error in ~9 rounds, 207 against 29.5 ms - k_seed amortises those serial
    // steps over 64 lanes).  GM_SEED_FUSED=0 / 1: never / whenever possible.
    const bool no_kernel_env = !gm_opt("GM_VOTE_KERNEL");
    const int fused_env = (int)gm_opt_ll("GM_SEED_FUSED", -1);
    const double occ = (double)ix->h.seq_len / pow(4.0, (double)std::min(p->mer, 31));
    // -h: on a real reference the k-mers of repeats exceed any cap, and each of them makes the walk slide base by base (:213-217) in
    // one lane - not measurable on the synthetic references of bench.py, so a capped run keeps k_seed unless forced
    const bool pays = occ >= 4.0 && p->max_kmer_hits == 0;
    f.fused = (fused_env < 0 ? pays : fused_env != 0) && f.use_full && (f.dense == 1 || f.dense == 2) && no_kernel_env && b->max_seeds <= 64 && dp.kmer_tab &&
              dp.kmer_ctab && dp.kmer_T == p->mer && p->mer <= 16 && p->jump >= 1 && !(dp.dbg & 128);
    // ... or in the bucket table (one read per wave, both strands; handles -h and k-mers that do not occur by walking again):
    // every seed is ONE random line
    const uint32_t lastmax = b->len_max > (uint32_t)p->mer ? b->len_max - (uint32_t)p->mer : 0;      // (the longest read of the block, not the row stride)
    const uint32_t max_reg = (lastmax + (uint32_t)p->jump - 1) / (uint32_t)p->jump;
    f.use_bucket = dp.bucket && f.use_full && dp.kmer_tab && dp.kmer_T == dp.bucket_T && dp.bucket_T == p->mer && p->min_seed_hits >= 2 && max_reg <= 32 && b->max_seeds <= 34 && no_kernel_env &&
                   !gm_opt("GM_VOTE") && f.sub_n == 0 && !(dp.dbg & 128) && fused_env != 0;
    // -A: the minus strand's k-mers come from another stretch of the row than its DP (see k_seed): only k_seed knows that form
    if (!b->adaptor.empty()) { f.fused = 0; f.use_bucket = false; }
    if (f.use_bucket) { f.fused = 1; f.bucket_reg = max_reg; }
    // ... two reads per wavefront (gm_pair.hip) where a strand has at most 16 seeds; GM_VOTE_PAIR=0: one read per wavefront always
    f.use_pair = f.use_bucket && !dp.bucket_ctx && max_reg <= 16 && !(p->nw && p->fast) && !gm_opt_is("GM_VOTE_PAIR", "0") && !(dp.dbg & (64 | 256 | 512 | 1024 | 2048));       // (GM_DBG 4096 .. 32768: timing experiments of k_vote_pair)
    // hand-off of k_vote_pair's results: straight into the candidate shards and the flagged reads' list at each 16-pair flush (default),
    // or GM_PAIR_HANDOFF=gather: own candidate slots + one flag byte per read, read back by k_cand_gather / k_pair_collect / k_heavy_collect
    f.pair_direct = f.use_pair && !gm_opt_is("GM_PAIR_HANDOFF", "gather");
    f.use_pack = f.fused != 0;
    // the one-wave vote kernels leave their candidates in per read x strand slots (no bump counter on the wave's critical path)
    f.use_fixed = !gm_opt_is("GM_VOTE_FIXED", "0") && !f.pair_direct && (f.use_bucket || ((f.dense == 1 || f.dense == 2) && no_kernel_env));      // k_vote_bucket, k_vote_tiny*, k_vote_slots (all forms)
    return f;
}

// the buffers only some forms use
static int map_form_buffers(gm_batch* b, const MapForm& f, hipStream_t st) {
    if (f.use_pair && b->pair_list.ensure(((size_t)b->n + 16) * 4)) return GM_E_NOMEM;
    if (f.use_pair && !f.pair_direct && b->pair_fb.ensure((size_t)b->n + 64)) return GM_E_NOMEM;
    if (f.use_pack && b->pack.ensure((size_t)b->n * gm_pack_words(b->stride) * 4 + 64)) return GM_E_NOMEM;
    if (f.use_fixed) {
        const size_t cap_before = b->fixed_cands.cap;       // by CAPACITY: hipFree + a larger hipMalloc may hand back the same base address
        if (b->fixed_cands.ensure(((2 * (size_t)b->n + 63) / 64) * 64 * GM_FIXED_C * sizeof(GmCand)) || b->fixed_cnt.ensure(2 * (size_t)b->n + 64)) return GM_E_NOMEM;
        // new memory: no stale launch stamps.  (TEST switch GM_TEST_EPOCH=<start>: the counter starts there, so that a few calls reach the
        // NaN / inf / denormal bit patterns of the stamp and the 32-bit wrap)
        if (b->fixed_cands.cap != cap_before) { HIPCHK(hipMemsetAsync(b->fixed_cands.p, 0, b->fixed_cands.cap, st)); b->epoch_ctr = (uint32_t)gm_opt_ll("GM_TEST_EPOCH", 0); }
    }
    return GM_OK;
}

// what path() says of the form.  gmk_vote's own branches are copied here: more than 64 seeds per strand leave the one-workgroup kernels
// for the ordered k_vote, GM_VOTE_KERNEL picks the dense form whatever `dense` says, GM_VOTE_SPARSE=0 runs k_vote_fast for every read x strand
static std::string map_form_name(const MapForm& f, const gm_batch* b, const GmDevParams& dp) {
    char buf[224];
    const int pp_env = (int)gm_opt_ll("GM_SLOTS_PIPE", -1);                                               // (gmk_vote's condition for the pipelined form of k_vote_slots)
    const bool slots_pp = f.use_full && !gm_opt("GM_VOTE_KERNEL") && (pp_env < 0 ? f.dense == 2 : pp_env != 0) && !(dp.dbg & 64);
    const char* kenv = gm_opt("GM_VOTE_KERNEL"); if (kenv && !*kenv) kenv = nullptr;
    const bool wg_form = f.dense != 0 && b->max_seeds <= 64;
    const bool slots_form = wg_form && (kenv ? !strcmp(kenv, "slots") : f.dense <= 2);
    const uint32_t reg = f.bucket_reg;
    snprintf(buf, sizeof buf, "seeds=%s vote=%s locate=%s cands=%s", f.use_bucket ? "bucket-table (in the vote kernel)" : f.fused ? "k-mer table (in the vote kernel)" : "k_seed",
             f.use_pair ? (reg <= 8 ? "k_vote_pair<4> + k_vote_bucket<2>" : reg <= 14 ? "k_vote_pair<7> + k_vote_bucket<4>" : "k_vote_pair<8> + k_vote_bucket<4>")
             : f.use_bucket ? (reg <= 8 ? "k_vote_bucket<2>" : reg <= 16 ? "k_vote_bucket<4>" : reg <= 24 ? "k_vote_bucket<6>" : "k_vote_bucket<8>")
                            : !wg_form ? (b->max_seeds > 64 ? "k_vote" : gm_opt_is("GM_VOTE_SPARSE", "0") ? "k_vote_fast" : "sparse") : !slots_form ? "k_vote_block"
                            : f.dense == 2 ? (slots_pp ? "k_vote_slots_pp<64>" : "k_vote_slots<64>") : f.slots_hint == 0 ? "k_vote_tiny" : f.slots_hint < 0 ? "k_vote_tiny2" : slots_pp ? "k_vote_slots_pp" : "k_vote_slots",
             f.use_full ? "full-SA" : "sampled-SA", f.use_fixed ? "own-slots" : "shards");
    return buf;
}

// shared by the single pass and the sub-batch pipeline: k_prep counted the quality characters below the offset ...
static int map_check_quals(const gm_batch* b, const unsigned long long* ctr) {
    if (ctr[GMK_BAD_QUAL] && !b->fasta) { gm_set_error("Invalid Fastq Character? (negative base probability)"); return GM_E_BAD_QUAL; }
    return GM_OK;
}

// ... and those above 127: one read length in the block and none of them (a FASTA block has no quality characters) is what the DP kernel
// with the rows in DP order takes, 0 = another form
static uint32_t map_nw_rows_len(const gm_batch* b, const unsigned long long* ctr) {
    return (b->len_min == b->len_max && (b->fasta || ctr[GMK_HIGH_QUAL] == 0)) ? b->len_max : 0u;
}

// ... and the tables of gmk_vote_retry, all handed out at once: `slots` empty keys and zero counts
static int map_retry_tables(DevBuf& keys, DevBuf& vals, size_t slots, hipStream_t st) {
    if (keys.ensure(slots * 4) || vals.ensure(slots * 4)) return GM_E_NOMEM;
    HIPCHK(hipMemsetAsync(keys.p, 0xFF, slots * 4, st));
    HIPCHK(hipMemsetAsync(vals.p, 0, slots * 4, st));
    return GM_OK;
}

// Large batches in full-SA mode: the batch is cut into sub-batches that go through prep -> seed -> vote -> NW on NS
// streams, so that the LDS-bound vote kernel of one sub-batch runs beside the seed / NW kernels of its neighbours.
// Returns 1 when a candidate shard overflowed (the caller then takes the single-pass path, which can grow the list).
// Of the form it takes dense, slots_hint and sub_n: the sub-batches run k_prep -> k_seed -> gmk_vote on shard candidates, and their views
// are cut from a b->dev that carries no form (no 2-bit read forms, no own slots).
static int map_pipelined(gm_index* ix, const GmDevParams& dp, gm_batch* b, const MapForm& form, hipStream_t st) {
    const uint32_t n = b->n, sub_n = form.sub_n;
    const uint32_t nsb = (n + sub_n - 1) / sub_n;
    for (int i = 0; i < gm_batch::NS; ++i)
        if (!b->sub_streams[i]) HIPCHK(hipStreamCreateWithFlags(&b->sub_streams[i], hipStreamNonBlocking));
    if (!b->sub_ready) HIPCHK(hipEventCreateWithFlags(&b->sub_ready, hipEventDisableTiming));
    const size_t shard_bytes = (size_t)GM_NSHARD * GM_SHARD_STRIDE * 4;
    if (b->sub_counters.ensure((size_t)nsb * GMK_N * 8) || b->sub_small.ensure((size_t)nsb * 64) || b->sub_shards.ensure((size_t)nsb * shard_bytes)) return GM_E_NOMEM;
    fill_dev_batch(b);
    const uint32_t region = (b->cand_cap / nsb) / GM_NSHARD;          // per sub-batch, per shard
    if (region < 16) return 1;
    HIPCHK(hipEventRecord(b->sub_ready, st));                          // the upload / earlier work on the caller's stream
    std::vector<GmDevBatch> view(nsb);
    std::vector<uint32_t> ncand(nsb, 0);
    std::vector<uint32_t> shard_host((size_t)GM_NSHARD * GM_SHARD_STRIDE);
    bool overflow = false;
    auto make_view = [&](uint32_t i) {
        GmDevBatch v = b->dev;
        const uint32_t lo = i * sub_n, cnt = std::min(sub_n, n - lo);
        v.n = cnt; v.read_base = lo;
        v.illumina_until = b->illumina_until > lo ? std::min(b->illumina_until - lo, cnt) : 0;
        v.bases += (size_t)lo * b->stride; v.quals += (size_t)lo * b->stride; v.len += lo;
        v.status += lo; v.self_score += lo; v.min_score += lo; v.top_score += lo;
        v.seeds += (size_t)2 * lo * b->max_seeds; v.n_seeds += 2 * (size_t)lo; v.n_entries += 2 * (size_t)lo;
        v.rs_overflow += 2 * (size_t)lo; v.retry_list += 2 * (size_t)lo; v.retry_off += 2 * (size_t)lo;
        v.cands += (size_t)i * region * GM_NSHARD; v.cand_cap = region * GM_NSHARD; v.cand_region = region;
        v.shard_cnt = b->sub_shards.as<uint32_t>() + (size_t)i * GM_NSHARD * GM_SHARD_STRIDE;
        v.hit_count += lo; v.hit_begin += lo; v.hit_cursor += lo;
        v.counters = b->sub_counters.as<unsigned long long>() + (size_t)i * GMK_N;
        v.n_retry = b->sub_small.as<uint32_t>() + (size_t)i * 16 + 1; v.n_big = b->sub_small.as<uint32_t>() + (size_t)i * 16 + 2;
        v.big_list += 2 * (size_t)lo;
        return v;
    };
    auto finish = [&](uint32_t i) -> int {                            // vote(i) is done: size check, retry, then NW
        const int s = (int)(i % gm_batch::NS);
        hipStream_t ss = b->sub_streams[s];
        uint32_t small[2]; unsigned long long ctr[GMK_N];
        HIPCHK(hipMemcpyAsync(small, b->sub_small.as<uint32_t>() + (size_t)i * 16, 8, hipMemcpyDeviceToHost, ss));
        HIPCHK(hipMemcpyAsync(ctr, view[i].counters, sizeof ctr, hipMemcpyDeviceToHost, ss));
        HIPCHK(hipMemcpyAsync(shard_host.data(), view[i].shard_cnt, shard_bytes, hipMemcpyDeviceToHost, ss));
        HIPCHK(hipStreamSynchronize(ss));
        if (int rc = map_check_quals(b, ctr)) return rc;
        auto tally = [&](uint64_t& total, uint32_t& mx) { total = 0; mx = 0; for (int q = 0; q < GM_NSHARD; ++q) { uint32_t c = shard_host[(size_t)q * GM_SHARD_STRIDE]; total += c; mx = std::max(mx, c); } };
        uint64_t total; uint32_t mx;
        tally(total, mx);
        if (small[1] && mx <= region) {
            if (int rc = map_retry_tables(b->sub_gk[s], b->sub_gv[s], (size_t)ctr[GMK_HEAVY_SLOTS], ss)) return rc;
            view[i].gtab_keys = b->sub_gk[s].as<uint32_t>(); view[i].gtab_vals = b->sub_gv[s].as<uint32_t>();
            { KTimer t(b, GM_K_VOTE_RETRY, ss); KCHK(gmk_vote_retry(ix->dev, dp, view[i], 1, 0, small[1], ss)); }
            HIPCHK(hipMemcpyAsync(shard_host.data(), view[i].shard_cnt, shard_bytes, hipMemcpyDeviceToHost, ss));
            HIPCHK(hipStreamSynchronize(ss));
            tally(total, mx);
        }
        if (mx > region) { overflow = true; return GM_OK; }
        ncand[i] = (uint32_t)total;
        { KTimer t(b, GM_K_NW, ss); KCHK(gmk_nw(ix->dev, dp, view[i], ncand[i], map_nw_rows_len(b, ctr), gm_qual_lo(ctr), gm_qual_hi(ctr), small[1] != 0, ss)); }
        return GM_OK;
    };
    uint32_t next_finish = 0;
    for (uint32_t i = 0; i < nsb && !overflow; ++i) {
        view[i] = make_view(i);
        hipStream_t ss = b->sub_streams[i % gm_batch::NS];
        if (i < (uint32_t)gm_batch::NS) HIPCHK(hipStreamWaitEvent(ss, b->sub_ready, 0));
        HIPCHK(hipMemsetAsync(view[i].counters, 0, GMK_N * 8, ss));
        HIPCHK(hipMemsetAsync(b->sub_small.as<uint32_t>() + (size_t)i * 16, 0, 64, ss));
        HIPCHK(hipMemsetAsync(view[i].shard_cnt, 0, shard_bytes, ss));
        HIPCHK(hipMemsetAsync(view[i].rs_overflow, 0, 2 * (size_t)view[i].n, ss));
        { KTimer t(b, GM_K_PREP, ss); KCHK(gmk_prep(ix->dev, dp, view[i], ss)); }
        { KTimer t(b, GM_K_SEED, ss); KCHK(gmk_seed(ix->dev, dp, view[i], ss, b->adaptor.empty() ? nullptr : b->full_len.as<uint16_t>() + view[i].read_base)); }
        { KTimer t(b, GM_K_VOTE, ss); KCHK(gmk_vote(ix->dev, dp, view[i], 1, form.dense, form.slots_hint, ss)); }
        if (i + 1 >= (uint32_t)gm_batch::NS) { int rc = finish(next_finish++); if (rc) return rc; }
    }
    while (next_finish < nsb && !overflow) { int rc = finish(next_finish++); if (rc) return rc; }
    for (int s = 0; s < gm_batch::NS; ++s) HIPCHK(hipStreamSynchronize(b->sub_streams[s]));
    if (overflow) return 1;
    // counters of all sub-batches, summed on the host
    std::vector<unsigned long long> all((size_t)nsb * GMK_N);
    HIPCHK(hipMemcpy(all.data(), b->sub_counters.p, all.size() * 8, hipMemcpyDeviceToHost));
    memset(b->counters_host, 0, sizeof b->counters_host);
    for (uint32_t i = 0; i < nsb; ++i) for (int q = 0; q < GMK_N; ++q) b->counters_host[q] += all[(size_t)i * GMK_N + q];
    b->counters_on_host = true;
    uint64_t total_c = 0;
    for (uint32_t i = 0; i < nsb; ++i) total_c += ncand[i];
    b->n_cands = (uint32_t)std::min<uint64_t>(total_c, 0xFFFFFFFFull);
    if (b->raw_cap < total_c + 16ull) b->raw_cap = total_c + 16ull;
    if (b->raw_hits.ensure(b->raw_cap * sizeof(GmRawHit))) return GM_E_NOMEM;
    fill_dev_batch(b);
    { KTimer t(b, GM_K_COMPACT, st); KCHK(gmk_scan_hits(b->dev, st)); }
    for (uint32_t i = 0; i < nsb; ++i) {
        view[i].raw_hits = b->dev.raw_hits; view[i].raw_cap = b->dev.raw_cap;
        uint32_t grid = std::max<uint32_t>(64, std::min<uint32_t>(2048, (ncand[i] + 255) / 256));
        KTimer t(b, GM_K_COMPACT, st);
        KCHK(gmk_scatter(view[i], grid, st));
    }
    b->mapped = true;
    return GM_OK;
}

// what the steps of the single pass hand each other
struct MapState {
    GmDevParams dp;
    MapForm form;
    uint32_t epoch = 0;                             // the attempt's launch stamp for the own slots of k_vote_bucket; 0 = the count array form
    unsigned long long ctr[GMK_N];                  // the work counters as the last vote attempt's wait brought them
    std::vector<uint32_t> heavy;                    // {rs, n_seeds, SA hits} triples of the heavy path
    // status words of a phase come back in ONE short DMA into page-locked memory (b->h_stat): [0..15] = b->small (n_retry, n_big, n_heavy,
    // shard total, shard maximum), [16..] = the work counters
    uint32_t* hs_small = nullptr;
    unsigned long long* hs_ctr = nullptr;
    uint64_t total = 0; uint32_t mx = 0;            // candidates in all shards and in the fullest one (gmk_shard_stats)
    // of the last attempt: k_nw_rows loads rs_overflow bytes only when this is set.  The bytes are written by the vote kernels next to
    // n_retry alone; the heavy path does not write them and is included only to stay on the safe side
    bool any_superseded = false;
};

// b->dev for the launches of this call: the resident block, this call's form and the attempt's stamp on top.  Every ensure() inside the
// call that may move a buffer is followed by this before the next launch (never by fill_dev_batch alone), and so is every vote attempt.
static void map_fill_dev(gm_batch* b, const MapState& s) {
    fill_dev_batch(b);
    if (s.form.use_pack) b->dev.pack = b->pack.as<uint32_t>();
    if (s.form.use_fixed) { b->dev.fixed_cands = b->fixed_cands.as<GmCand>(); b->dev.fixed_cnt = b->fixed_cnt.as<uint8_t>(); b->dev.fixed_epoch = s.epoch; }
}

// ... and off again however the call ends
struct MapFormScope {
    gm_batch* b;
    ~MapFormScope() { b->dev.pack = nullptr; b->dev.fixed_cands = nullptr; b->dev.fixed_cnt = nullptr; b->dev.fixed_epoch = 0; }
};

// nothing is launched: the counters and the path are this call's (all zero, no kernel), not the last block's
static int map_empty_block(gm_batch* b) {
    b->n_cands = 0; b->n_raw = 0; b->mapped = true; memset(b->counters_host, 0, sizeof b->counters_host); b->counters_on_host = true;
    b->path = std::string("reads=") + (b->fasta ? "fasta" : "fastq") + " (empty block: no kernel)";
    return GM_OK;
}

// what the upload bound and what it did not (gnumap_hip.h at gm_batch_upload): the fallback scan of --illumina read the host's
// quality rows then, so `illumina` cannot change; the seed rows follow THIS call's -m / -j, whatever the upload sized them for
static int map_check_binding(const gm_params* p, gm_batch* b) {
    if (!b->fasta && (p->illumina != 0) != (b->up_illumina != 0)) {
        gm_set_error(std::string("gm_params.illumina = ") + (p->illumina ? "1" : "0") + " for a block uploaded with illumina = " + (b->up_illumina ? "1" : "0") +
                     ": the upload binds this field (its fallback scan read the quality rows); upload the block again under the other value");
        return GM_E_ARG;
    }
    if (const uint32_t ms = seed_rows(b->stride, p); ms != b->max_seeds) {
        b->max_seeds = ms;
        if (b->seeds.ensure(2 * (size_t)b->n * ms * sizeof(GmSeed))) return GM_E_NOMEM;      // (map_fill_dev comes before the first launch)
    }
    return GM_OK;
}

// k_prep, k_seed unless the vote kernels look the seeds up, and on a sampled-SA index the locate pass with its one wait
static int map_prep_seed(gm_index* ix, gm_batch* b, MapState& s, hipStream_t st) {
    map_fill_dev(b, s);
    HIPCHK(hipMemsetAsync(b->counters.p, 0, GMK_N * 8, st));
    { KTimer t(b, GM_K_PREP, st); KCHK(gmk_prep(ix->dev, s.dp, b->dev, st)); }
    if (!s.form.fused) { KTimer t(b, GM_K_SEED, st); KCHK(gmk_seed(ix->dev, s.dp, b->dev, st, b->adaptor.empty() ? nullptr : b->full_len.as<uint16_t>())); }
    if (!s.form.use_full) {
        // faithful mode: locate every SA hit by LF walks into coords[] first (exact size from the seed kernel)
        HIPCHK(hipMemcpyAsync(s.ctr, b->counters.p, sizeof s.ctr, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (b->coords.ensure((size_t)s.ctr[GMK_SA_HITS] * 4 + 64)) return GM_E_NOMEM;
        map_fill_dev(b, s);
        KCHK(gmk_scan_entries(b->dev, st));
        { KTimer t(b, GM_K_LOCATE, st); KCHK(gmk_locate_sampled(ix->dev, b->dev, s.ctr[GMK_SA_HITS], st)); }
    }
    if (b->heavy_list.ensure(3 * 2 * (size_t)b->n * 4 + 64) || b->h_stat.ensure(64 + GMK_N * 8 + 64)) return GM_E_NOMEM;
    s.hs_small = b->h_stat.as<uint32_t>();
    s.hs_ctr = reinterpret_cast<unsigned long long*>(b->h_stat.as<uint8_t>() + 64);
    return GM_OK;
}

// the list of the heavy path: collected right after k_seed, or (fused form) after the first vote launch, which left those read x strands
// alone.  Enqueued here; the count comes back with the phase's status words, then the triples are fetched
static int map_heavy_enqueue(gm_batch* b, const MapState& s, hipStream_t st) {
    const bool direct = s.form.pair_direct;
    HIPCHK(hipMemsetAsync(b->small.as<uint32_t>() + 3, 0, 4, st));
    KCHK(gmk_heavy_collect(b->dev, s.form.heavy_min, b->small.as<uint32_t>() + 3, b->heavy_list.as<uint32_t>(), s.form.fused,
                           direct ? b->pair_list.as<uint32_t>() + 4 : nullptr, direct ? b->pair_list.as<uint32_t>() : nullptr, st));
    return GM_OK;
}

static int map_heavy_fetch(gm_batch* b, MapState& s) {
    const uint32_t nh = s.hs_small[3];
    GM_TRACE("map_device: %u reads, seeds done, %u read x strands on the heavy path (> %u SA hits)", b->n, nh, s.form.heavy_min);
    s.heavy.clear();
    if (nh) {
        s.heavy.resize(3 * (size_t)nh);
        HIPCHK(hipMemcpy(s.heavy.data(), b->heavy_list.p, s.heavy.size() * 4, hipMemcpyDeviceToHost));
    }
    return GM_OK;
}

static int map_heavy_after_seed(gm_batch* b, MapState& s, hipStream_t st) {      // the two-kernel form
    if (int rc = map_heavy_enqueue(b, s, st)) return rc;
    HIPCHK(hipMemcpyAsync(s.hs_small, b->small.p, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return map_heavy_fetch(b, s);
}

// candidates per shard: total and maximum are reduced on the device (gmk_shard_stats -> small[4], small[5]) and come back with the
// status words and the counters in one wait
static int map_read_status(gm_batch* b, MapState& s, hipStream_t st) {
    KCHK(gmk_shard_stats(b->dev, b->small.as<uint32_t>() + 4, s.form.use_pair ? b->pair_list.as<uint32_t>() : nullptr, st));
    HIPCHK(hipMemcpyAsync(s.hs_small, b->small.p, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s.hs_ctr, b->counters.p, GMK_N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s.total = s.hs_small[4]; s.mx = s.hs_small[5]; b->pair_flagged = s.hs_small[6];
    return GM_OK;
}

// one attempt at the vote: the per-attempt clears, the launch group, the heavy list when fused, and the ONE wait of the vote phase
static int map_vote_attempt(gm_index* ix, gm_batch* b, MapState& s, hipStream_t st) {
    const MapForm& f = s.form;
    HIPCHK(hipMemsetAsync(b->small.p, 0, 64, st));
    HIPCHK(hipMemsetAsync(b->shards.p, 0, (size_t)GM_NSHARD * GM_SHARD_STRIDE * 4, st));
    HIPCHK(hipMemsetAsync(b->rs_overflow.p, 0, 2 * (size_t)b->n, st));
    HIPCHK(hipMemsetAsync(b->counters.as<unsigned long long>() + GMK_HEAVY_SLOTS, 0, 8, st));
    HIPCHK(hipMemsetAsync(b->counters.as<unsigned long long>() + GMK_OVERFLOW_RS, 0, 8, st));
    if (f.use_fixed && f.use_bucket) {          // own-slot candidates carry the launch's stamp: nothing to zero but the flags "goes to the list kernel"
        HIPCHK(hipMemsetAsync(b->fixed_cnt.p, 0, 2 * (size_t)b->n + 32, st));
        if (++b->epoch_ctr == 0) { HIPCHK(hipMemsetAsync(b->fixed_cands.p, 0, b->fixed_cands.cap, st)); b->epoch_ctr = 1; }
        s.epoch = b->epoch_ctr;
    } else if (f.use_fixed) HIPCHK(hipMemsetAsync(b->fixed_cnt.p, 0, 2 * (size_t)b->n, st));
    map_fill_dev(b, s);                          // every attempt starts from b->dev filled anew: the stamp, and the list map_grow_cands moved
    if (f.fused) {                               // the seed search runs inside the vote launch: its work counters start over with it
        HIPCHK(hipMemsetAsync(b->counters.as<unsigned long long>() + GMK_KMERS, 0, 4 * 8, st));            // KMERS, OCC, SEEDS, SA_HITS
        HIPCHK(hipMemsetAsync(b->counters.as<unsigned long long>() + GMK_OCC_BLOCKS, 0, 2 * 8, st));       // OCC_BLOCKS, TAB_LOOKUPS
    }
    {
        KTimer t(b, GM_K_VOTE, st);
        uint32_t* const plist = b->pair_list.as<uint32_t>();
        if (f.use_bucket && f.use_pair) {
            // two reads per wavefront for the reads without complications; the flagged ones go through k_vote_bucket (direct hand-off:
            // no own slots - k_vote_bucket and the list kernel append their candidates and list entries as they go)
            if (!f.pair_direct) HIPCHK(hipMemsetAsync(b->pair_fb.p, 0, (size_t)b->n + 16, st));
            HIPCHK(hipMemsetAsync(b->pair_list.p, 0, 16, st));
            KCHK(gmk_vote_pair(ix->dev, s.dp, b->dev, f.bucket_reg, f.pair_direct ? nullptr : b->pair_fb.as<uint8_t>(), plist + 4, plist, st));
            KCHK(gmk_vote_bucket(ix->dev, s.dp, b->dev, f.bucket_reg, plist + 4, plist, st));
            KCHK(gmk_vote_list(ix->dev, s.dp, b->dev, f.use_full, st));
        } else if (f.use_bucket) { KCHK(gmk_vote_bucket(ix->dev, s.dp, b->dev, f.bucket_reg, nullptr, nullptr, st)); KCHK(gmk_vote_list(ix->dev, s.dp, b->dev, f.use_full, st)); }
        else KCHK(gmk_vote(ix->dev, s.dp, b->dev, f.use_full, f.dense, f.slots_hint, st));
        KCHK(gmk_cand_gather(b->dev, st));
    }
    if (f.fused) { if (int rc = map_heavy_enqueue(b, s, st)) return rc; }
    if (int rc = map_read_status(b, s, st)) return rc;
    memcpy(s.ctr, s.hs_ctr, sizeof s.ctr);
    return f.fused ? map_heavy_fetch(b, s) : GM_OK;
}

// GM_DBG 64: sampled phase clocks of the vote kernel (cycles of one lane per sampled workgroup)
static void map_print_vote_phases(const MapState& s) {
    const unsigned long long* ctr = s.ctr;
    const double ns = (double)std::max<unsigned long long>(1, ctr[GMK_DBG8]);
    if (s.form.use_bucket) fprintf(stderr, "[gm_dbg] k_vote_bucket phases (mean clock ticks of lane 0 per sampled read, %llu samples; reads that leave early do not reach the later marks): forms + codes %.0f, "
                    "records %.0f, first walk %.0f, routing %.0f, filter pass %.0f, sweeps %.0f, store %.0f\n", ctr[GMK_DBG8], ctr[GMK_DBG0] / ns, ctr[GMK_DBG1] / ns, ctr[GMK_DBG2] / ns,
                    ctr[GMK_DBG3] / ns, ctr[GMK_DBG4] / ns, ctr[GMK_DBG5] / ns, ctr[GMK_DBG6] / ns);
    else
    fprintf(stderr, "[gm_dbg] vote phases (mean cycles per sampled read x strand, %llu samples): desc %.0f, loads+window %.0f, pass1 %.0f, pass2a %.0f, scan %.0f, "
                    "filter2 %.0f, table %.0f, emit %.0f\n", ctr[GMK_DBG8], ctr[GMK_DBG0] / ns, ctr[GMK_DBG1] / ns, ctr[GMK_DBG2] / ns, ctr[GMK_DBG3] / ns, ctr[GMK_DBG4] / ns,
            ctr[GMK_DBG5] / ns, ctr[GMK_DBG6] / ns, ctr[GMK_DBG7] / ns);
}

// the n_retry read x strands whose hits did not fit their vote kernel, through hash tables in HBM: all at once, or when the tables of all
// of them exceed GM_RETRY_BUDGET (table slots per launch: 2 GB of keys + counts; the switch is for tests) in groups.  Ends with the shards' new status
static int map_retry(gm_index* ix, gm_batch* b, MapState& s, uint32_t n_retry, hipStream_t st) {
    const size_t slots = (size_t)s.ctr[GMK_HEAVY_SLOTS];
    const size_t budget = (size_t)gm_opt_ll("GM_RETRY_BUDGET", 1ll << 28);
    if (slots <= budget) {
        if (int rc = map_retry_tables(b->gtab_keys, b->gtab_vals, slots, st)) return rc;
        map_fill_dev(b, s);
        { KTimer t(b, GM_K_VOTE_RETRY, st); KCHK(gmk_vote_retry(ix->dev, s.dp, b->dev, s.form.use_full, 0, n_retry, st)); }
    } else {
        // many read x strands at once (a kernel choice that did not fit the data): the tables are handed out again per
        // launch instead of all at once
        std::vector<uint32_t> list(n_retry), nent((size_t)2 * b->n);
        HIPCHK(hipMemcpyAsync(list.data(), b->retry_list.p, (size_t)n_retry * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(nent.data(), b->n_entries.p, nent.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (b->gtab_keys.ensure(budget * 4) || b->gtab_vals.ensure(budget * 4)) return GM_E_NOMEM;
        map_fill_dev(b, s);
        std::vector<unsigned long long> off(n_retry);
        KTimer t(b, GM_K_VOTE_RETRY, st);
        for (uint32_t j = 0; j < n_retry;) {
            const uint32_t j0 = j;
            size_t acc = 0;
            while (j < n_retry) {
                size_t need = 2 * (size_t)nent[list[j]], sz = 1024;
                while (sz < need && sz < 0x80000000u) sz <<= 1;
                if (sz > budget) { gm_set_error("a read x strand with more SA hits than the retry table budget; use -h"); return GM_E_BATCH_TOO_LARGE; }
                if (acc + sz > budget) break;
                off[j] = acc; acc += sz; ++j;
            }
            HIPCHK(hipMemcpyAsync(b->retry_off.as<unsigned long long>() + j0, off.data() + j0, (size_t)(j - j0) * 8, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(b->gtab_keys.p, 0xFF, acc * 4, st));
            HIPCHK(hipMemsetAsync(b->gtab_vals.p, 0, acc * 4, st));
            KCHK(gmk_vote_retry(ix->dev, s.dp, b->dev, s.form.use_full, j0, j - j0, st));
            HIPCHK(hipStreamSynchronize(st));        // off[] is reused by the next group
        }
    }
    return map_read_status(b, s, st);
}

// the heavy list: expand + sort + run-length vote, chunk by chunk under the key budget.  Ends with the shards' new status
static int map_heavy_chunks(gm_index* ix, gm_batch* b, MapState& s, hipStream_t st) {
    KTimer t(b, GM_K_VOTE_RETRY, st);
    const std::vector<uint32_t>& heavy = s.heavy;
    const uint64_t heavy_budget = s.form.heavy_budget;
    const uint32_t nh = (uint32_t)(heavy.size() / 3);
    std::vector<unsigned long long> off;
    for (uint32_t j = 0; j < nh;) {
        const uint32_t j0 = j;
        unsigned long long acc = 0;
        off.clear();
        while (j < nh && j - j0 < 65536u) {
            const unsigned long long e = heavy[3 * (size_t)j + 2];
            if (e == 0xFFFFFFFFull || e > heavy_budget) { gm_set_error("a read x strand with more SA hits than one heavy-path chunk holds; use -h"); return GM_E_BATCH_TOO_LARGE; }
            if (acc + e > heavy_budget) break;
            off.push_back(acc); acc += e; ++j;
        }
        const uint32_t nj = j - j0;
        unsigned item_bits = 1; while ((1u << item_bits) < nj) ++item_bits;
        const size_t tmp_bytes = gmk_heavy_sort_temp_bytes((size_t)acc);
        if (b->heavy_k0.ensure((size_t)acc * 8 + 64) || b->heavy_k1.ensure((size_t)acc * 8 + 64) || b->heavy_tmp.ensure(tmp_bytes + 64) ||
            b->heavy_off.ensure((size_t)nj * 8 + 64)) return GM_E_NOMEM;
        HIPCHK(hipMemcpyAsync(b->heavy_off.p, off.data(), (size_t)nj * 8, hipMemcpyHostToDevice, st));
        KCHK(gmk_heavy_chunk(ix->dev, s.dp, b->dev, s.form.use_full, b->heavy_list.as<uint32_t>(), j0, nj, b->heavy_off.as<unsigned long long>(),
                             b->heavy_k0.as<unsigned long long>(), b->heavy_k1.as<unsigned long long>(), acc, b->heavy_tmp.p, tmp_bytes, item_bits, st));
        HIPCHK(hipStreamSynchronize(st));        // off[] and the key buffers are reused by the next chunk
        GM_TRACE("heavy chunk: items %u..%u of %u, %llu keys sorted", j0, j, nh, acc);
    }
    return map_read_status(b, s, st);
}

// a candidate shard overflowed: grow the list for the next attempt, or give up after the ninth
static int map_grow_cands(gm_batch* b, const MapState& s, int attempt) {
    if (attempt > 8) { gm_set_error("candidate list keeps overflowing"); return GM_E_NOMEM; }
    const size_t want = ((size_t)s.mx + s.mx / 4 + 64) * GM_NSHARD;
    if (want > 0x7FFFFFFFu) { gm_set_error("more than 2^31 candidates in one batch; map the block in smaller pieces (or use -h)"); return GM_E_BATCH_TOO_LARGE; }
    b->cand_cap = (uint32_t)want;
    return b->cands.ensure((size_t)b->cand_cap * sizeof(GmCand)) ? GM_E_NOMEM : GM_OK;      // (map_vote_attempt fills b->dev)
}

static int map_nw_compact(gm_index* ix, gm_batch* b, const MapState& s, hipStream_t st) {
    if (b->raw_cap < b->n_cands + 16ull) b->raw_cap = b->n_cands + 16ull;
    if (b->raw_hits.ensure(b->raw_cap * sizeof(GmRawHit))) return GM_E_NOMEM;
    map_fill_dev(b, s);
    const uint32_t rows_len = map_nw_rows_len(b, s.ctr), lo = gm_qual_lo(s.ctr), hi = gm_qual_hi(s.ctr);
    b->path += std::string(" nw=") + gmk_nw_form(s.dp, b->dev, b->n_cands, rows_len, lo, hi);
    { KTimer t(b, GM_K_NW, st); KCHK(gmk_nw(ix->dev, s.dp, b->dev, b->n_cands, rows_len, lo, hi, s.any_superseded, st)); }
    { KTimer t(b, GM_K_COMPACT, st); KCHK(gmk_compact(b->dev, st)); }
    if (gm_trace_on()) { HIPCHK(hipStreamSynchronize(st)); GM_TRACE("NW + compaction done"); }
    b->mapped = true;
    return GM_OK;
}

// The form is this call's.  Outside gm_map_batch_device b->dev carries none: fill_dev_batch leaves pack, fixed_cands and fixed_cnt null
// and fixed_epoch 0, which is what every other caller of it gets (the two uploads, out_enqueue_traceback, the gm_dev_* probes) and what
// map_pipelined cuts its views from; none of their kernels reads those fields (k_prep, the vote kernels and k_cand_gather alone do).
// Inside, map_fill_dev puts the form on top and MapFormScope takes it off.
extern "C" int gm_map_batch_device(gm_index* ix, const gm_params* p, gm_batch* b, void* stream) {
    if (!ix || !p || !b || !p->finalized || b->ix != ix) return GM_E_ARG;
    HIPCHK(hipSetDevice(ix->device));
    hipStream_t st = S_(stream);
    MapState s;
    int rc = sync_params(ix, p, s.dp, st, true);
    if (rc) return rc;
    b->mapped = false;
    b->pair_flagged = 0;
    if ((rc = fasta_forced_form(b)) != GM_OK) return rc;
    if (b->n == 0) return map_empty_block(b);
    if ((rc = map_check_binding(p, b)) != GM_OK) return rc;
    const MapForm& f = s.form = map_choose_form(ix, p, b, s.dp);
    b->counters_on_host = false;
    if (f.pipeline) {
        b->path.clear();                             // the single-pass dispatch records its choice; a block the sub-batches map to the end has none (not the last call's)
        if ((rc = map_pipelined(ix, s.dp, b, f, st)) <= 0) return rc;      // done, or a real error; 1: a shard overflowed, the single pass can grow the list
    }
    MapFormScope scope{ b };
    if ((rc = map_form_buffers(b, f, st)) != GM_OK) return rc;
    s.dp.heavy_min = f.heavy_min; s.dp.fused = f.fused;
    if (!f.use_bucket) s.dp.bucket = nullptr;
    const std::string name = map_form_name(f, b, s.dp);
    b->path = std::string("reads=") + (b->fasta ? "fasta " : "fastq ") + name;
    GM_TRACE("path: %s", name.c_str());
    if ((rc = map_prep_seed(ix, b, s, st)) != GM_OK) return rc;
    if (!f.fused && (rc = map_heavy_after_seed(b, s, st)) != GM_OK) return rc;
    for (int attempt = 0;; ++attempt) {
        if ((rc = map_vote_attempt(ix, b, s, st)) != GM_OK) return rc;
        if (s.dp.dbg & 64) map_print_vote_phases(s);
        if ((rc = map_check_quals(b, s.ctr)) != GM_OK) return rc;
        const uint32_t n_retry = s.hs_small[1], region = b->dev.cand_region;
        s.any_superseded = n_retry != 0 || !s.heavy.empty();
        if (n_retry && s.mx <= region && (rc = map_retry(ix, b, s, n_retry, st)) != GM_OK) return rc;
        if (!s.heavy.empty() && s.mx <= region && (rc = map_heavy_chunks(ix, b, s, st)) != GM_OK) return rc;
        if (s.mx <= region) {
            b->n_cands = (uint32_t)s.total;
            GM_TRACE("vote done: %llu candidates (attempt %d)", (unsigned long long)s.total, attempt);
            break;
        }
        if ((rc = map_grow_cands(b, s, attempt)) != GM_OK) return rc;      // a candidate shard overflowed: vote again
    }
    return map_nw_compact(ix, b, s, st);
}

extern "C" int gm_batch_counters(gm_batch* b, gm_counters* o) {
    if (!b || !o) return GM_E_ARG;
    HIPCHK(hipSetDevice(b->ix->device));
    unsigned long long c[GMK_N];
    if (b->counters_on_host) memcpy(c, b->counters_host, sizeof c);
    else HIPCHK(hipMemcpy(c, b->counters.p, sizeof c, hipMemcpyDeviceToHost));
    memset(o, 0, sizeof *o);
    o->reads = b->n; o->kmers_searched = c[GMK_KMERS]; o->occ_calls = c[GMK_OCC]; o->occ_blocks = c[GMK_OCC_BLOCKS];
    o->seeds_used = c[GMK_SEEDS]; o->sa_hits = c[GMK_SA_HITS];
    o->lf_steps = c[GMK_LF_STEPS]; o->candidates = b->n_cands; o->nw_cells = c[GMK_NW_CELLS]; o->accepted = c[GMK_ACCEPTED];
    o->vote_retries = c[GMK_OVERFLOW_RS]; o->table_lookups = c[GMK_TAB_LOOKUPS];
    return GM_OK;
}

extern "C" const char* gm_batch_path(gm_batch* b) { return b ? b->path.c_str() : ""; }

extern "C" int gm_batch_pair_flagged(gm_batch* b, uint32_t* flagged) {
    if (!b || !flagged) return GM_E_ARG;
    *flagged = b->pair_flagged;
    return GM_OK;
}

extern "C" const char* gm_kernel_name(int which) {
    static const char* names[GM_K_COUNT] = { "k_prep", "k_seed", "k_locate_sampled", "k_vote", "k_vote_retry", "k_nw", "k_compact(scan+scatter)", "k_md_sizes", "k_mate_*" };
    return which >= 0 && which < GM_K_COUNT ? names[which] : "?";
}

extern "C" int gm_batch_set_profiling(gm_batch* b, int on) {
    if (!b) return GM_E_ARG;
    b->profiling = on != 0;
    return GM_OK;
}

extern "C" int gm_batch_kernel_times(gm_batch* b, double* ms, uint64_t* launches) {
    if (!b || !ms || !launches) return GM_E_ARG;
    HIPCHK(hipSetDevice(b->ix->device));
    for (auto& ev : b->pending) {
        HIPCHK(hipEventSynchronize(ev.b));
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, ev.a, ev.b));
        b->k_ms[ev.which] += t; b->k_launches[ev.which] += 1;
        b->pool.push_back(ev.a); b->pool.push_back(ev.b);
    }
    b->pending.clear();
    for (int i = 0; i < GM_K_COUNT; ++i) { ms[i] = b->k_ms[i]; launches[i] = b->k_launches[i]; b->k_ms[i] = 0; b->k_launches[i] = 0; }
    return GM_OK;
}

static bool raw_less(const GmRawHit& a, const GmRawHit& b) {
    if (a.strand != b.strand) return a.strand < b.strand;       // POS pass first (Driver.cpp:506-556)
    if (a.step != b.step) return a.step < b.step;               // seed order (align_sequence loop)
    return a.pos < b.pos;                                       // std::map<unsigned long,int> order (process_hits)
}

struct RawDownload {
    std::vector<GmRawHit> hits;
    std::vector<uint64_t> begin;
    std::vector<int8_t> status;
    std::vector<float> self_score, top;
};

static int download_raw(gm_batch* b, RawDownload& r, hipStream_t st, bool no_nw) {
    if (!b->mapped) { gm_set_error("batch has not been mapped"); return GM_E_ARG; }
    const uint32_t n = b->n;
    r.begin.assign(n + 1, 0); r.status.assign(n, 0); r.self_score.assign(n, 0); r.top.assign(n, 0);
    if (n == 0) return GM_OK;
    HIPCHK(hipMemcpyAsync(r.begin.data(), b->hit_begin.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.status.data(), b->status.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.self_score.data(), b->self_score.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.top.data(), b->top_score.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t total = r.begin[n];
    if (total > b->raw_cap) { gm_set_error("internal: raw hit buffer too small"); return GM_E_CAPACITY; }
    r.hits.resize(total);
    if (total) HIPCHK(hipMemcpy(r.hits.data(), b->raw_hits.p, total * sizeof(GmRawHit), hipMemcpyDeviceToHost));
    b->n_raw = total;
    for (uint32_t i = 0; i < n; ++i) {
        auto first = r.hits.begin() + (ptrdiff_t)r.begin[i], last = r.hits.begin() + (ptrdiff_t)r.begin[i + 1];
        if (no_nw) std::sort(first, last, [](const GmRawHit& a, const GmRawHit& c) { return a.strand != c.strand ? a.strand < c.strand : a.pos < c.pos; });
        else std::sort(first, last, raw_less);
    }
    return GM_OK;
}

extern "C" int gm_batch_raw_hits(gm_batch* b, gm_raw_hit* out, uint64_t cap, uint64_t* n_out, int8_t* status, float* self_score, float* top_score) {
    if (!b || !n_out) return GM_E_ARG;
    HIPCHK(hipSetDevice(b->ix->device));
    RawDownload r;
    int rc = download_raw(b, r, nullptr, false);
    if (rc) return rc;
    *n_out = r.hits.size();
    if (status) memcpy(status, r.status.data(), b->n);
    if (self_score) memcpy(self_score, r.self_score.data(), (size_t)b->n * 4);
    if (top_score) memcpy(top_score, r.top.data(), (size_t)b->n * 4);
    if (r.hits.size() > cap) return GM_E_CAPACITY;
    static_assert(sizeof(gm_raw_hit) == sizeof(GmRawHit), "layout");
    if (out && !r.hits.empty()) memcpy(out, r.hits.data(), r.hits.size() * sizeof(GmRawHit));
    return GM_OK;
}

// host-side bookkeeping that is independent per item: cut into contiguous chunks, one host thread each (GM_HOST_THREADS; used by
// the track writers: threads made per call) ...
unsigned host_threads() {
    static const unsigned n = [] {
        const char* e = getenv("GM_HOST_THREADS");               // sizes thread pools once per process
        unsigned v = e ? (unsigned)atoi(e) : std::min(16u, std::thread::hardware_concurrency());
        return std::max(1u, v);
    }();
    return n;
}
template <class F> static unsigned parallel_chunks(uint32_t n, uint32_t grain, unsigned want, F&& fn) {   // fn(chunk, lo, hi); returns #chunks
    unsigned T = (unsigned)std::min<uint64_t>(want, std::max<uint32_t>(1, n / std::max<uint32_t>(1, grain)));
    if (T <= 1) { fn(0u, 0u, n); return 1; }
    std::vector<std::thread> th;
    const uint64_t per = (n + T - 1) / T;
    for (unsigned c = 1; c < T; ++c)
        th.emplace_back([&, c] { uint32_t lo = (uint32_t)std::min<uint64_t>(n, c * per), hi = (uint32_t)std::min<uint64_t>(n, (c + 1) * per); fn(c, lo, hi); });
    fn(0u, 0u, (uint32_t)std::min<uint64_t>(n, per));
    for (auto& x : th) x.join();
    return T;
}

// ... and the two fp64 passes of the batch calls (denominator += exp(score); posterior / winner / MAPQ): every read's sum is its own,
// in its own order, so the READS of a block are cut into slices that helper threads of a process-wide pool take beside the calling
// thread (GM_PASS_THREADS helpers, default 3 per process; 0 = the calling thread alone).  The pool is shared by every batch of the
// process: a slice is a queue entry, callers of different batches interleave.
namespace {
struct PassPool {
    std::mutex mu; std::condition_variable cv;
    std::deque<std::function<void()>> q;
    std::vector<std::thread> th;
    bool stop = false;
    unsigned n = 0;
    void start(unsigned helpers) {
        n = helpers;
        for (unsigned i = 0; i < helpers; ++i)
            th.emplace_back([this] {
                for (;;) {
                    std::function<void()> job;
                    { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return stop || !q.empty(); }); if (q.empty()) return; job = std::move(q.front()); q.pop_front(); }
                    job();
                }
            });
    }
    ~PassPool() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); for (auto& t : th) t.join(); }
};
PassPool& pass_pool() {
    static PassPool* pool = [] { auto* p = new PassPool(); const char* e = getenv("GM_PASS_THREADS"); p->start(e ? (unsigned)std::max(0, atoi(e)) : 3u); return p; }();
    return *pool;
}
// fn(lo, hi) over [0, n) in slices of at least `grain` items: the helpers take slices from the queue, the caller takes the rest
template <class F> void pass_parallel(uint32_t n, uint32_t grain, F&& fn) {
    PassPool& pool = pass_pool();
    const unsigned parts = (unsigned)std::min<uint64_t>(pool.n + 1, std::max<uint32_t>(1, n / std::max<uint32_t>(1, grain)));
    if (parts <= 1) { fn(0u, n); return; }
    const uint64_t per = (n + parts - 1) / parts;
    // completion state lives on the heap and is shared with every job: the last helper touches the mutex / condition variable AFTER the
    // count reaches zero, so they must outlive the caller's frame (the caller may already have seen zero and returned)
    struct Done { std::mutex mu; std::condition_variable cv; unsigned left; };
    auto done = std::make_shared<Done>();
    done->left = parts - 1;
    {
        std::lock_guard<std::mutex> lk(pool.mu);
        for (unsigned c = 1; c < parts; ++c)
            pool.q.emplace_back([&fn, done, n, per, c] {
                fn((uint32_t)std::min<uint64_t>(n, c * per), (uint32_t)std::min<uint64_t>(n, (c + 1) * per));
                std::lock_guard<std::mutex> lk2(done->mu);          // decrement UNDER the mutex: the waiter cannot leave before the notify
                if (--done->left == 0) done->cv.notify_one();
            });
    }
    pool.cv.notify_all();
    fn(0u, (uint32_t)std::min<uint64_t>(n, per));
    // a slice nobody has taken yet is run here rather than waited for
    for (;;) {
        std::function<void()> job;
        { std::lock_guard<std::mutex> lk(pool.mu); if (pool.q.empty()) break; job = std::move(pool.q.front()); pool.q.pop_front(); }
        job();
    }
    std::unique_lock<std::mutex> lk(done->mu);
    done->cv.wait(lk, [&] { return done->left == 0; });
}
}  // namespace

// host-only self test of the slice pool (no device): `callers` threads each run `iters` passes over [0, n) at once and check that
// every item was visited exactly once per pass.  Returns 0, or the number of passes that came out wrong.
extern "C" int gm_selftest_pass_parallel(uint32_t n, uint32_t grain, uint32_t callers, uint32_t iters) {
    std::atomic<int> bad{ 0 };
    auto run = [&] {
        std::vector<uint8_t> seen(n);
        for (uint32_t it = 0; it < iters; ++it) {
            std::fill(seen.begin(), seen.end(), (uint8_t)0);
            std::atomic<uint64_t> sum{ 0 };
            pass_parallel(n, grain, [&](uint32_t lo, uint32_t hi) { uint64_t s2 = 0; for (uint32_t i = lo; i < hi; ++i) { ++seen[i]; s2 += i; } sum += s2; });
            bool ok = sum.load() == (uint64_t)n * (n ? n - 1 : 0) / 2;
            for (uint32_t i = 0; i < n && ok; ++i) ok = seen[i] == 1;
            if (!ok) ++bad;
        }
    };
    std::vector<std::thread> th;
    for (uint32_t c = 1; c < callers; ++c) th.emplace_back(run);
    run();
    for (auto& t : th) t.join();
    return bad.load();
}

struct PhaseClock {                         // GM_TIMING=1: host-side phase times of the two batch calls on stderr
    bool on; const char* what; std::chrono::steady_clock::time_point t0; std::string line;
    explicit PhaseClock(const char* w) : on(gm_opt_ll("GM_TIMING", 0) != 0), what(w), t0(std::chrono::steady_clock::now()) {}
    void lap(const char* name) {
        if (!on) return;
        auto t1 = std::chrono::steady_clock::now();
        char buf[64]; snprintf(buf, sizeof buf, " %s %.2f ms", name, std::chrono::duration<double, std::milli>(t1 - t0).count());
        line += buf; t0 = t1;
    }
    ~PhaseClock() { if (on) fprintf(stderr, "[gm_timing] %s:%s\n", what, line.c_str()); }
};

extern "C" int gm_stream_create(gm_index* ix, void** out) {
    if (!ix || !out || ix->host_only) return GM_E_ARG;
    HIPCHK(hipSetDevice(ix->device));
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = s;
    return GM_OK;
}
extern "C" void gm_stream_destroy(gm_index* ix, void* s) {
    if (!ix || !s) return;
    (void)hipSetDevice(ix->device);
    (void)hipStreamDestroy(S_(s));
}

extern "C" void* gm_host_alloc(size_t bytes) {
    void* q = nullptr;
    if (hipHostMalloc(&q, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { gm_set_error("hipHostMalloc failed"); return nullptr; }
    return q;
}
extern "C" void gm_host_free(void* q) { if (q) (void)hipHostFree(q); }

static_assert(sizeof(gm_match) == sizeof(GmDevMatch) && offsetof(gm_match, first_pos) == offsetof(GmDevMatch, first_pos) &&
              offsetof(gm_match, first_strand) == offsetof(GmDevMatch, first_strand) && offsetof(gm_match, pos_begin) == offsetof(GmDevMatch, pos_begin) &&
              offsetof(gm_match, pos_end) == offsetof(GmDevMatch, pos_end), "gm_match layout");
static_assert(sizeof(gm_pos) == sizeof(GmDevPos) && offsetof(gm_pos, strand) == offsetof(GmDevPos, strand), "gm_pos layout");
static_assert(sizeof(gm_sam_rec) == sizeof(GmDevSamRec) && offsetof(gm_sam_rec, pos) == offsetof(GmDevSamRec, pos) &&
              offsetof(gm_sam_rec, contig) == offsetof(GmDevSamRec, contig) && offsetof(gm_sam_rec, chr_pos) == offsetof(GmDevSamRec, chr_pos) &&
              offsetof(gm_sam_rec, strand) == offsetof(GmDevSamRec, strand) && offsetof(gm_sam_rec, mapq) == offsetof(GmDevSamRec, mapq) &&
              offsetof(gm_sam_rec, a_score) == offsetof(GmDevSamRec, a_score) && offsetof(gm_sam_rec, post_prob) == offsetof(GmDevSamRec, post_prob) &&
              offsetof(gm_sam_rec, sim_matches) == offsetof(GmDevSamRec, sim_matches) && offsetof(gm_sam_rec, cigar_off) == offsetof(GmDevSamRec, cigar_off),
              "gm_sam_rec layout");

// ------------------------------------------------------------------------------------------------
// gm_map_batch = the block loop over set_top_matches (src/Driver.cpp:2344-2356).
// Device: prep -> seed -> locate+vote -> NW -> compaction (gm_map_batch_device), then process_hits' unique map as kernels
// (gm_output.hip: processing order, key grouping on the 2-bit reference, std::map order, -T / -u exits) writing gm_match /
// gm_pos records in HBM.  Host: ONE flat fp64 pass, denominator += exp(score) in the reference's order (glibc exp, the
// order-dependent part that has to stay bit-identical to the CPU program).
// ------------------------------------------------------------------------------------------------
static int map_batch_rest(gm_index* ix, const gm_params* p, gm_batch* b, gm_hits* out, hipStream_t st, bool resume, const void* resume_key, PhaseClock& pc);

extern "C" int gm_map_batch(gm_index* ix, const gm_params* p, gm_batch* b, const gm_reads* reads, gm_hits* out, void* stream) {
    if (!ix || !p || !b || !reads || !out) return GM_E_ARG;
    out->stamp = 0;                                            // every return path that does not leave a resident result leaves "none"
    PhaseClock pc("gm_map_batch");
    hipStream_t st = S_(stream);
    int rc;
    {   // test switch: behave as if blocks above this size outgrew a launch (exercises the callers' halving)
        const uint32_t test_max = (uint32_t)gm_opt_ll("GM_TEST_MAX_BLOCK", 0);
        if (test_max && reads->n > test_max) { gm_set_error("GM_TEST_MAX_BLOCK: block treated as too large"); return GM_E_BATCH_TOO_LARGE; }
    }
    // a call repeated with larger output buffers after GM_E_CAPACITY picks up where the first one stopped: the block is still mapped
    // and grouped in HBM (same reads pointer, same count), only the copies to the host are left to do
    const bool resume = b->resume_ptr != nullptr && b->resume_ptr == (const void*)reads->bases && b->n == reads->n;
    b->resume_ptr = nullptr;
    if (!resume) {
        rc = gm_batch_upload(b, p, reads, stream);
        if (rc) return rc;
        pc.lap("upload");
        rc = gm_map_batch_device(ix, p, b, stream);
        if (rc) return rc;
    } else HIPCHK(hipSetDevice(ix->device));
    return map_batch_rest(ix, p, b, out, st, resume, (const void*)reads->bases, pc);
}

// gm_map_batch for the block gm_batch_upload_text left resident.  The resume after GM_E_CAPACITY is keyed on the batch holding that text
// block (there is no gm_reads whose pointer could name it): the key is the address of the batch's own flag, which no caller's
// gm_reads.bases can be
extern "C" int gm_map_batch_text(gm_index* ix, const gm_params* p, gm_batch* b, gm_hits* out, void* stream) {
    if (!ix) return GM_E_ARG;
    if (ix->host_only) { gm_set_error("gm_map_batch_text: no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (!p || !b || !out) return GM_E_ARG;
    out->stamp = 0;
    if (!b->text_block) { gm_set_error("gm_map_batch_text: the batch holds no block from gm_batch_upload_text"); return GM_E_ARG; }
    PhaseClock pc("gm_map_batch_text");
    {
        const uint32_t test_max = (uint32_t)gm_opt_ll("GM_TEST_MAX_BLOCK", 0);
        if (test_max && b->n > test_max) { gm_set_error("GM_TEST_MAX_BLOCK: block treated as too large"); return GM_E_BATCH_TOO_LARGE; }
    }
    const void* const key = (const void*)&b->text_block;
    const bool resume = b->resume_ptr == key;
    b->resume_ptr = nullptr;
    if (!resume) {
        const int rc = gm_map_batch_device(ix, p, b, stream);
        if (rc) return rc;
    } else HIPCHK(hipSetDevice(ix->device));
    return map_batch_rest(ix, p, b, out, S_(stream), resume, key, pc);
}

// everything of gm_map_batch behind the upload and the mapping kernels: grouping, the copies to the host, the fp64 pass
static int map_batch_rest(gm_index* ix, const gm_params* p, gm_batch* b, gm_hits* out, hipStream_t st, bool resume, const void* resume_key, PhaseClock& pc) {
    const uint32_t n = b->n;
    out->n = n;
    if (n == 0) { out->match_begin[0] = 0; return GM_OK; }
    // the number of accepted hits stays on the device until the grouping kernels are done (no wait here): the workspace is sized by
    // its upper bound, the candidates of the block (resume: the count the first call read)
    const uint64_t hits_bound = resume ? b->n_raw : (uint64_t)b->n_cands;
    if (hits_bound > 0xFFFFFFF0ull) { gm_set_error("more than 2^32 accepted hits in one batch; map the block in smaller pieces"); return GM_E_BATCH_TOO_LARGE; }
    const size_t nh = (size_t)hits_bound + 16;
    if (b->g_sorted.ensure(nh * sizeof(GmRawHit)) || b->g_ord.ensure(nh * 4) || b->g_lead.ensure(nh * 4) || b->g_krank.ensure(nh * 4) ||
        b->g_khash.ensure(nh * 8) || b->g_positions.ensure(nh * sizeof(GmDevPos)) || b->g_matches.ensure(nh * sizeof(GmDevMatch)) || b->g_mhit.ensure(nh * 4) ||
        b->g_nmatch.ensure((size_t)n * 4) || b->g_mbegin.ensure(((size_t)n + 1) * 8) || b->g_multi.ensure((size_t)n * 4 + 64) ||
        b->g_big.ensure((size_t)n * 4 + 64) || b->g_bigdone.ensure((size_t)n + 64) || b->g_sk0.ensure(nh * 8) || b->g_sk1.ensure(nh * 8) || b->g_si0.ensure(nh * 4) || b->g_si1.ensure(nh * 4) ||
        b->scan_tmp.ensure(((size_t)n / 1024 + 8) * 8) || b->o_small.ensure(64)) return GM_E_NOMEM;
    GmDevGroup g;
    g.sorted = b->g_sorted.as<GmRawHit>(); g.ord_score = b->g_ord.as<float>(); g.lead = b->g_lead.as<uint32_t>(); g.krank = b->g_krank.as<uint32_t>();
    g.khash = b->g_khash.as<unsigned long long>(); g.n_match = b->g_nmatch.as<uint32_t>(); g.match_begin = b->g_mbegin.as<uint64_t>();
    g.multi_list = b->g_multi.as<uint32_t>(); g.n_multi = b->o_small.as<uint32_t>();
    g.big_list = b->g_big.as<uint32_t>(); g.n_big = b->o_small.as<uint32_t>() + 1; g.big_done = b->g_bigdone.as<uint8_t>();
    g.sk0 = b->g_sk0.as<unsigned long long>(); g.sk1 = b->g_sk1.as<unsigned long long>(); g.si0 = b->g_si0.as<uint32_t>(); g.si1 = b->g_si1.as<uint32_t>();
    g.matches = b->g_matches.as<GmDevMatch>(); g.match_hit = b->g_mhit.as<uint32_t>(); g.positions = b->g_positions.as<GmDevPos>();
    b->cache_hits = b->cache_matches = 0; b->stamp = 0; out->stamp = 0;
    if (!resume) {
        HIPCHK(hipMemsetAsync(b->o_small.p, 0, 64, st));
        // hits that end up in no match leave holes in the positions: those -u --no_nw drops, and every hit of a read whose matches are
        // dropped as a whole (GM_READ_TOO_MANY).  gm_hits.positions is copied out whole, so a hole must not hold the last block's entries
        HIPCHK(hipMemsetAsync(b->g_positions.p, 0, nh * sizeof(GmDevPos), st));
        KCHK(gmk_group_count(ix->dev, b->dev, g, p->nw, p->unique_only, p->max_matches, st));
        KCHK(gmk_scan_u32(g.n_match, n, g.match_begin, b->scan_tmp.as<unsigned long long>(), st));
        KCHK(gmk_group_write(b->dev, g, st));
    }
    // what the host pass needs: per-read status / top score, the CSR of the hits and their scores in processing order
    if (b->h_top.ensure((size_t)n * 4) || b->h_hbegin.ensure(((size_t)n + 1) * 8) || b->h_ord.ensure(nh * 4)) return GM_E_NOMEM;
    if (b->h_stat.ensure(64 + GMK_N * 8 + 64)) return GM_E_NOMEM;
    uint64_t* const hs64 = b->h_stat.as<uint64_t>();        // [0] matches, [1] accepted hits: page-locked, with the rest of the phase's copies
    HIPCHK(hipMemcpyAsync(&hs64[0], g.match_begin + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hs64[1], b->hit_begin.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out->status, b->status.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out->self_score, b->self_score.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b->h_top.p, b->top_score.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b->h_hbegin.p, b->hit_begin.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (hits_bound) HIPCHK(hipMemcpyAsync(b->h_ord.p, g.ord_score, (size_t)hits_bound * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out->match_begin, g.match_begin, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t n_m = hs64[0], n_hits = hs64[1];
    if (n_hits > hits_bound) { gm_set_error("internal: more accepted hits than candidates"); return GM_E_HIP; }
    b->n_raw = n_hits;
    pc.lap("group");
    if (gm_trace_on()) {
        uint32_t cnt[16] = { 0 };
        HIPCHK(hipMemcpy(cnt, b->o_small.p, sizeof cnt, hipMemcpyDeviceToHost));
        GM_TRACE("grouping done: %llu accepted hits -> %llu matches; reads: %u all-pairs list (incl. handed back), %u big path; handed back: %u (-u --no_nw), %u (> set limit), %u (hash collision)",
                 (unsigned long long)n_hits, (unsigned long long)n_m, cnt[0], cnt[1], cnt[2], cnt[3], cnt[4]);
    }
    if (n_m > out->matches_cap || n_hits > out->positions_cap) {
        out->matches_cap = n_m; out->positions_cap = n_hits;
        gm_set_error("output buffers too small");
        b->resume_ptr = resume_key;                              // the repeated call only copies
        return GM_E_CAPACITY;
    }
    if (n_m) HIPCHK(hipMemcpyAsync(out->matches, g.matches, (size_t)n_m * sizeof(gm_match), hipMemcpyDeviceToHost, st));
    if (n_hits) HIPCHK(hipMemcpyAsync(out->positions, g.positions, (size_t)n_hits * sizeof(gm_pos), hipMemcpyDeviceToHost, st));
    if (b->h_mhit.ensure((size_t)n_m * 4 + 16)) return GM_E_NOMEM;
    if (n_m) HIPCHK(hipMemcpyAsync(b->h_mhit.p, g.match_hit, (size_t)n_m * 4, hipMemcpyDeviceToHost, st));
    // the fp64 pass (process_hits :134-165: denominator += exp(align_score) for every new key and every new place of an old key, in
    // processing order) runs while the records are still in flight
    const float* top = b->h_top.as<float>(); const uint64_t* hb = b->h_hbegin.as<uint64_t>(); const float* ord = b->h_ord.as<float>();
    b->h_exp.resize((size_t)n_hits + 1);
    double* hexp = b->h_exp.data();
    pass_parallel(n, 16384, [&](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i) {
            const int8_t s = out->status[i];
            double den = 0.0, tp = 0.0;
            if (s == GM_READ_OK) {
                for (uint64_t h = hb[i]; h < hb[i + 1]; ++h) {
                    const float sc = ord[h];
                    const double e = sc != -INFINITY ? exp((double)sc) : 0.0;
                    hexp[h] = e;
                    if (sc != -INFINITY) den += e;
                }
                tp = (double)top[i];
            } else if (s == GM_READ_TOO_SHORT) tp = -2.0;
            else if (s == GM_READ_TOO_POOR) tp = -3.0;
            else if (s == GM_READ_TOO_MANY) tp = 999999.0;
            out->denominator[i] = den; out->top_score[i] = tp;
        }
    });
    pc.lap("exp");
    HIPCHK(hipStreamSynchronize(st));
    b->cache_hits = n_hits; b->cache_matches = n_m;          // h_exp / h_ord / h_mhit describe this result
    {
        // a stamp a caller's uninitialised memory does not hit by accident: per-process random base (clock + address entropy through
        // the 64-bit mixer) + counter, with the batch's address mixed in; never 0
        static const uint64_t stamp_base = [] {
            uint64_t x = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() ^ ((uint64_t)(uintptr_t)&gm_set_option << 17) ^ ((uint64_t)getpid() << 48);
            x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x | (1ull << 63);
        }();
        static std::atomic<uint64_t> next_stamp{ 1 };
        b->stamp = (stamp_base + next_stamp.fetch_add(1) * 0x9e3779b97f4a7c15ull) ^ ((uint64_t)(uintptr_t)b >> 4);
        if (b->stamp == 0) b->stamp = stamp_base;
        out->stamp = b->stamp;
    }
    pc.lap("records");
    return GM_OK;
}

// ------------------------------------------------------------------------------------------------
// gm_output_batch = the block loop over create_match_output (src/Driver.cpp:2360-2373).
// Host: ONE flat fp64 pass over the matches (posterior = exp(score) / denominator, winner = first strict maximum in key order,
// MAPQ = round(-10 log10(1 - p)): glibc exp / log / round).  Device: traceback of every kept sequence, run-length CIGAR text, SAM
// rows, coverage deposit (+ the per-nucleotide track of -b / -d).  Nothing per read is done on the host beyond that pass.
// ------------------------------------------------------------------------------------------------
// One call of the output step, as its entry point describes it.  The sink says where the records go, and names the one destination
// that is set: records + CIGAR pool to the host (gm_output_batch), finished SAM text (gm_output_batch_text), rows kept in the sorter's
// arena under sequence number seq (gm_output_batch_sorted), BAM records inside BGZF blocks (gm_output_batch_bam).
// What a form needs besides the pointers every form takes: a caller's gm_read_text, or the names gm_batch_upload_text left in the batch
// (such a form takes no gm_reads).  OUT_PLAIN_NO_DEVICE: the host-only message carries no name (gm_output_batch_text's never has).
enum { OUT_NEEDS_RT = 1, OUT_NEEDS_POOLS = 2, OUT_PLAIN_NO_DEVICE = 4 };
struct OutCall {
    const char* who;                           // the entry point, for its messages
    enum Sink { records, text, sorted, bam } sink;
    int needs;
    const gm_reads* reads; const gm_hits* hits;
    const gm_read_text* rt;                    // the rows' names and tails; null: the pools gm_batch_upload_text left in t_names / t_qtail
    uint64_t seq;                              // sorted: the block's sequence number
    void* dest;                                // the sink's one destination, as what the sink makes of it:
    gm_sam_out* recs_out() const { return static_cast<gm_sam_out*>(dest); }       gm_sam_text* text_out() const { return static_cast<gm_sam_text*>(dest); }
    gm_sam_sorter* sorter() const { return static_cast<gm_sam_sorter*>(dest); }   gm_bam_out* bam_out() const { return static_cast<gm_bam_out*>(dest); }
    bool rows() const { return sink != records; }                              // the records leave as rows; they and the CIGAR pool stay in HBM
    bool bam_rows() const { return sink == bam || (sink == sorted && gm_samsort_rows(sorter()) == GM_ROWS_BAM); }   // BAM records, not text (gm_bam.hip)
};

// what the steps of one call hand on to each other, by the step that sets it
struct OutState {
    GmDevParams dp;                            // sync_params, in output_batch
    uint32_t n, n_m; uint64_t n_p;             // out_check_hits: reads, kept sequences (matches), position slots in use,
    bool resident, snp, nuc; uint32_t ops_words, codes_stride;                 // and what the mode and the stride make of them
    uint64_t n_recs, cig_len; uint32_t max_span;                               // out_count_records
    bool unmapped;                             // output_batch: a rows sink on a batch with gm_batch_set_unmapped_rows on
    uint64_t n_rows, n_unmapped;               // out_row_inputs: the rows (the records, + the reads without one when `unmapped`), and those reads
    GmDevText t;                               // out_row_inputs (t.text: out_write_rows)
    uint64_t text_len; unsigned long long bad_row;                             // out_count_rows
};

// The destination first, as the entry points always have; then that reads and hits are the batch's; then the caller's names
static int out_check_call(const gm_batch* b, const OutCall& c) {
    const gm_hits* hits = c.hits; const gm_read_text* rt = c.rt;
    if (c.sink == OutCall::text && !c.text_out()->text && c.text_out()->text_cap) { gm_set_error("gm_sam_text: text is NULL"); return GM_E_ARG; }
    if (c.sink == OutCall::bam) {
        gm_bam_out* out = c.bam_out();
        out->len = 0; out->raw_len = 0; out->n_recs = 0;
        if (!gm_bgzf_level_ok(out->level)) { gm_set_error(std::string(c.who) + ": gm_bam_out.level: " + gm_bgzf_level_text(out->level)); return GM_E_ARG; }
        if (!out->data && out->cap) { gm_set_error(std::string(c.who) + ": gm_bam_out.data is NULL"); return GM_E_ARG; }
    }
    if (hits->n != b->n || c.reads->n != b->n) { gm_set_error("hits / reads do not belong to the batch"); return GM_E_ARG; }
    if (b->mates && (hits->n & 1u)) {
        gm_set_error(std::string(c.who) + ": gm_batch_set_mates is on and the block has an odd number of reads (" + std::to_string(hits->n) + "): reads 2i and 2i + 1 are the mates of pair i");
        return GM_E_ARG;
    }
    if (b->mates && b->mate_min > b->mate_max) {
        gm_set_error(std::string(c.who) + ": gm_batch_set_mates: min_insert " + std::to_string(b->mate_min) + " is above max_insert " + std::to_string(b->mate_max));
        return GM_E_ARG;
    }
    if (c.sink == OutCall::text) {
        c.text_out()->text_len = 0; c.text_out()->n_recs = 0;
        if (c.text_out()->row_off && c.text_out()->row_cap) c.text_out()->row_off[0] = 0;
    }
    if (!rt) return GM_OK;
    bool asc = rt->names && rt->name_off && (rt->qual_tail != nullptr) == (rt->qual_tail_off != nullptr);
    for (uint32_t i = 0; asc && i < hits->n; ++i) asc = rt->name_off[i] <= rt->name_off[i + 1] && (!rt->qual_tail_off || rt->qual_tail_off[i] <= rt->qual_tail_off[i + 1]);
    if (!asc) { gm_set_error("gm_read_text: names / name_off missing, qual_tail without qual_tail_off (or the reverse), or offsets that do not ascend"); return GM_E_ARG; }
    // a FASTA record has no quality line: QUAL is str2qual's string, one character per base, and nothing can follow it
    if (b->fasta && rt->qual_tail_off) { gm_set_error("gm_read_text: qual_tail / qual_tail_off must be NULL for a FASTA block (its QUAL is synthesised, one character per base)"); return GM_E_ARG; }
    return GM_OK;
}

// The block's limits, then the hits.  hits->stamp names this batch's resident result: its matches / positions are used where they are.
// Otherwise `hits` may have been edited by the caller: everything the kernels index with is checked HERE, before the first enqueue (a
// match of another read would make k_traceback read rows that do not exist, a position range beyond the buffer would make k_out_items
// write past o_posmatch), and the records are uploaded again.  Last, --snp's two preconditions (they stay behind the empty block's GM_OK
// in output_batch, so that answer is the one it always was) and the sizes the mode and the stride give: ops_words, codes_stride, nuc.
static int out_check_hits(const gm_index* ix, const gm_params* p, const gm_batch* b, const gm_hits* hits, OutState& s) {
    const uint32_t n = s.n = hits->n;
    const uint64_t n_m64 = hits->match_begin[n];
    if (n_m64 > 0x7FFFFFFFull) { gm_set_error("too many matches in one batch; map the block in smaller pieces"); return GM_E_BATCH_TOO_LARGE; }
    {   // test switch: the output stage treats a block of more reads as too large, as the two limits of the output step would
        const uint32_t test_max = (uint32_t)gm_opt_ll("GM_TEST_MAX_OUT_BLOCK", 0);
        if (test_max && n > test_max) { gm_set_error("GM_TEST_MAX_OUT_BLOCK: block treated as too large"); return GM_E_BATCH_TOO_LARGE; }
    }
    s.n_m = (uint32_t)n_m64;
    s.resident = hits->stamp != 0 && hits->stamp == b->stamp && b->cache_matches == n_m64 && b->cache_hits <= hits->positions_cap;
    uint64_t n_p = 0;
    if (s.resident) n_p = b->cache_hits;
    else {
        if (hits->match_begin[0] != 0) { gm_set_error("gm_hits: match_begin[0] must be 0"); return GM_E_ARG; }
        bool bad = false;
        for (uint32_t i = 0; i < n && !bad; ++i) {
            const uint64_t m0 = hits->match_begin[i], m1 = hits->match_begin[i + 1];
            if (m1 < m0 || m1 > n_m64) { bad = true; break; }
            for (uint64_t m = m0; m < m1; ++m) {
                const gm_match& mm = hits->matches[m];
                if (mm.read != i || mm.pos_end < mm.pos_begin || mm.pos_end > hits->positions_cap || mm.first_strand > 1 || mm.first_pos >= ix->h.l_pac) { bad = true; break; }
                for (uint32_t q = mm.pos_begin; q < mm.pos_end; ++q) if (hits->positions[q].strand > 1 || hits->positions[q].pos >= ix->h.l_pac) bad = true;   // the places of THIS match (slots no match points at are never read)
                n_p = std::max<uint64_t>(n_p, mm.pos_end);
            }
        }
        if (bad) { gm_set_error("gm_hits: a match does not belong to its read, or its positions / first position are out of range"); return GM_E_ARG; }
        if (b->cache_matches == n_m64 && b->cache_hits <= hits->positions_cap && b->cache_hits >= n_p) n_p = b->cache_hits;     // positions share the hit CSR
    }
    s.n_p = n_p;
    s.ops_words = gm_ops_words(b->stride); s.codes_stride = 32u * s.ops_words;
    s.snp = p->mode == GM_MODE_SNP;
    if (s.snp && b->fasta) { gm_set_error("GM_MODE_SNP with a FASTA block: the pair HMM of --snp takes FASTQ blocks only"); return GM_E_UNSUPPORTED; }
    if (s.snp && !ix->nuc_on) { gm_set_error("GM_MODE_SNP deposits into the per-nucleotide tracks: call gm_coverage_enable_nuc first"); return GM_E_ARG; }
    s.nuc = p->mode != GM_MODE_NORMAL && !s.snp && ix->nuc_on;
    return GM_OK;
}

// Device, part 1: everything that does not depend on the posteriors is enqueued BEFORE the host pass and runs under it
static int out_enqueue_traceback(gm_index* ix, const gm_params* p, gm_batch* b, const gm_hits* hits, const OutState& s, hipStream_t st) {
    const uint32_t n = s.n, n_m = s.n_m; const uint64_t n_p = s.n_p;
    if (b->g_matches.ensure((size_t)n_m * sizeof(GmDevMatch)) || b->g_positions.ensure((size_t)(n_p + 1) * sizeof(GmDevPos)) ||
        b->o_posmatch.ensure((size_t)(n_p + 1) * 4) || b->o_post.ensure((size_t)n_m * 4) || b->o_mapq.ensure((size_t)n_m * 4) || b->o_emit.ensure(n_m) ||
        b->tb_items.ensure((size_t)n_m * sizeof(GmCand)) || b->tb_ops.ensure((size_t)n_m * s.ops_words * 8) || b->tb_len.ensure((size_t)n_m * 2) ||
        b->o_reccnt.ensure((size_t)n_m * 4) || b->o_cigcnt.ensure((size_t)n_m * 4) || b->o_cigall.ensure((size_t)n_m * 4) || b->o_recoff.ensure(((size_t)n_m + 1) * 8) ||
        b->o_cigoff.ensure(((size_t)n_m + 1) * 8) || b->scan_tmp.ensure(((size_t)std::max<uint32_t>(n_m, n) / 1024 + 8) * 8) || b->o_small.ensure(64) ||
        (s.nuc && b->o_codes.ensure((size_t)n_m * s.codes_stride))) return GM_E_NOMEM;
    if (!s.resident) {
        HIPCHK(hipMemcpyAsync(b->g_matches.p, hits->matches, (size_t)n_m * sizeof(gm_match), hipMemcpyHostToDevice, st));
        if (n_p) HIPCHK(hipMemcpyAsync(b->g_positions.p, hits->positions, (size_t)n_p * sizeof(gm_pos), hipMemcpyHostToDevice, st));
        b->stamp = 0;                                          // what is resident now is the caller's version
    }
    HIPCHK(hipMemsetAsync(b->o_posmatch.p, 0xFF, (size_t)(n_p + 1) * 4, st));
    HIPCHK(hipMemsetAsync(b->o_small.p, 0, 64, st));
    if (p->max_gap != 3 && b->band_moves.ensure(gm_band_moves_words(n_m, b->stride) * 8)) return GM_E_NOMEM;
    fill_dev_batch(b);
    const GmDevMatch* d_m = b->g_matches.as<GmDevMatch>();
    KCHK(gmk_out_items(d_m, n_m, 0, b->tb_items.as<GmCand>(), b->o_posmatch.as<uint32_t>(), st));
    // one traceback per ScoredSeq, oriented by its first strand (NormalScoredSeq::score, ScoredSeq::get_SAM); the kernel also leaves the
    // length of every sequence's CIGAR text and finds the longest aligned length
    KCHK(gmk_traceback(ix->dev, s.dp, b->dev, b->tb_items.as<GmCand>(), n_m, b->tb_ops.as<unsigned long long>(), s.ops_words, b->tb_len.as<uint16_t>(),
                       nullptr, b->o_cigall.as<uint32_t>(), b->o_small.as<uint32_t>(), st));
    if (!p->nw && !b->adaptor.empty()) KCHK(gmk_adaptor_cigar_room(d_m, n_m, b->full_len.as<uint16_t>(), std::min<uint32_t>(n, b->n), b->o_cigall.as<uint32_t>(), st));
    return GM_OK;
}

// Host pass: posterior, winner and MAPQ of every match (ScoredSeq::get_SAM :300-309, is_greater :223-228, Driver.cpp:672-701) into the
// batch's page-locked h_post / h_mapq / h_emit.  Nothing is enqueued here: the pass runs while part 1 does.
static int out_host_posteriors(const gm_params* p, gm_batch* b, const gm_hits* hits, const OutState& s) {
    const uint32_t n = s.n, n_m = s.n_m;
    if (b->h_post.ensure((size_t)n_m * 4) || b->h_mapq.ensure((size_t)n_m * 4) || b->h_emit.ensure(n_m)) return GM_E_NOMEM;
    float* post = b->h_post.as<float>(); int32_t* mapq = b->h_mapq.as<int32_t>(); uint8_t* emit = b->h_emit.as<uint8_t>();
    const double log10v = log(10), e_m1 = exp(-1.0);                   // e_m1: the empty NormalScoredSeq a winner has to beat, ScoredSeq.h:117-120
    auto mapq_of = [&](double total) {
        int q;
        if (total == 1) q = 30; else q = (int)round(-10 * log(1 - total) / log10v);
        return q > 30 ? 30 : q;
    };
    const int all = p->print_all_sam;
    const uint64_t cached_m = b->cache_matches, cached_h = b->cache_hits;
    const uint32_t* mhit = b->h_mhit.as<uint32_t>(); const float* ord = b->h_ord.as<float>(); const double* hexp = b->h_exp.data();
    pass_parallel(n, 16384, [&](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i) {
            const uint64_t m0 = hits->match_begin[i], m1 = hits->match_begin[i + 1];
            if (m0 == m1) continue;
            if (hits->status[i] != GM_READ_OK) { for (uint64_t m = m0; m < m1; ++m) { post[m] = 0; mapq[m] = 0; emit[m] = 0; } continue; }
            const double den = hits->denominator[i], top = hits->top_score[i];
            int64_t best = -1;
            double best_log = e_m1, best_total = 0;
            for (uint64_t m = m0; m < m1; ++m) {
                const gm_match& mm = hits->matches[m];
                // exp(align_score): the value gm_map_batch already computed for the hit that gave this match its score, when the caller has
                // left the match as it was (exp is a function of the score alone, so equal score bits are all that has to hold)
                double lg;
                if (m < cached_m && mhit[m] < cached_h && memcmp(&ord[mhit[m]], &mm.score, 4) == 0) lg = hexp[mhit[m]];
                else lg = exp((double)mm.score);
                const double total = lg / den;                             // ScoredSeq.h:300
                post[m] = (float)total;                                    // AddScore(const float& amt), NormalScoredSeq.cpp:70
                emit[m] = (uint8_t)all;
                mapq[m] = all ? mapq_of(total) : 0;
                if (lg > best_log) { best = (int64_t)m; best_log = lg; best_total = total; }   // is_greater: strict, first in key order wins
            }
            if (!all && best >= 0 && (double)hits->matches[best].score > top - 0.00001) {      // Driver.cpp:695
                emit[best] = 1;
                mapq[best] = mapq_of(best_total);
            }
        }
    });
    return GM_OK;
}

// Device, part 2: the posteriors go up; how many records and CIGAR bytes they make, and the longest aligned length, come back
static int out_count_records(gm_batch* b, OutState& s, hipStream_t st) {
    const uint32_t n_m = s.n_m;
    HIPCHK(hipMemcpyAsync(b->o_post.p, b->h_post.p, (size_t)n_m * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->o_mapq.p, b->h_mapq.p, (size_t)n_m * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->o_emit.p, b->h_emit.p, n_m, hipMemcpyHostToDevice, st));
    KCHK(gmk_out_sizes(b->g_matches.as<GmDevMatch>(), n_m, b->o_emit.as<uint8_t>(), b->o_cigall.as<uint32_t>(), b->o_reccnt.as<uint32_t>(), b->o_cigcnt.as<uint32_t>(), st));
    KCHK(gmk_scan_u32(b->o_reccnt.as<uint32_t>(), n_m, b->o_recoff.as<uint64_t>(), b->scan_tmp.as<unsigned long long>(), st));
    KCHK(gmk_scan_u32(b->o_cigcnt.as<uint32_t>(), n_m, b->o_cigoff.as<uint64_t>(), b->scan_tmp.as<unsigned long long>(), st));
    HIPCHK(hipMemcpyAsync(&s.n_recs, b->o_recoff.as<uint64_t>() + n_m, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&s.cig_len, b->o_cigoff.as<uint64_t>() + n_m, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&s.max_span, b->o_small.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GM_OK;
}

// The records sink's capacity answer, then the records and the CIGAR pool: written in HBM for every sink, copied out for the records sink
static int out_write_records(gm_index* ix, const gm_params* p, gm_batch* b, const OutCall& c, const OutState& s, hipStream_t st) {
    const uint64_t n_recs = s.n_recs, cig_len = s.cig_len;
    if (c.sink == OutCall::records) {
        gm_sam_out* out = c.recs_out();
        out->n_recs = n_recs; out->cigar_len = cig_len;
        if (n_recs > out->recs_cap || cig_len > out->cigar_cap) {
            out->recs_cap = n_recs; out->cigar_cap = cig_len;
            gm_set_error("output buffers too small");
            return GM_E_CAPACITY;
        }
    }
    if (cig_len > 0xFFFFFFFFull) { gm_set_error("CIGAR pool beyond 4 GB in one batch; map the block in smaller pieces"); return GM_E_BATCH_TOO_LARGE; }
    if (b->o_recs.ensure((size_t)(n_recs + 1) * sizeof(GmDevSamRec)) || b->o_pool.ensure((size_t)cig_len + 16)) return GM_E_NOMEM;
    if (n_recs) {
        GmDevBatch wb = b->dev;                      // (k_out_write reads the lengths for --no_nw's "<L>M" only: consensus.size(), the whole line with -A, ScoredSeq.h:365)
        if (!b->adaptor.empty()) wb.len = b->full_len.as<uint16_t>();
        KCHK(gmk_out_write(ix->dev, wb, b->g_matches.as<GmDevMatch>(), b->g_positions.as<GmDevPos>(), s.n_m, b->o_emit.as<uint8_t>(), b->o_mapq.as<int32_t>(),
                           b->o_post.as<float>(), b->tb_ops.as<unsigned long long>(), s.ops_words, b->tb_len.as<uint16_t>(), p->nw, b->o_recoff.as<uint64_t>(),
                           b->o_cigoff.as<uint64_t>(), b->o_recs.as<GmDevSamRec>(), b->o_pool.as<char>(), st));
    }
    if (n_recs && c.sink == OutCall::records) {
        HIPCHK(hipMemcpyAsync(c.recs_out()->recs, b->o_recs.p, (size_t)n_recs * sizeof(gm_sam_rec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(c.recs_out()->cigar_pool, b->o_pool.p, (size_t)cig_len, hipMemcpyDeviceToHost, st));
    }
    if (c.sink == OutCall::text) c.text_out()->n_recs = n_recs;
    return GM_OK;
}

// Rows, their inputs: the names and quality tails of the block in HBM (a caller's are uploaded, the pools of a text block are in
// place), room for the row lengths and offsets, and the GmDevText the row kernels read
static int out_row_inputs(gm_index* ix, const gm_params* p, gm_batch* b, const OutCall& c, OutState& s, hipStream_t st) {
    const gm_read_text* rt = c.rt;
    const bool pools = !rt, bam = c.bam_rows();
    const uint32_t n = s.n;
    s.n_rows = s.n_recs; s.n_unmapped = 0;
    if (s.unmapped) {
        // the row source: the status bytes go up, the records are counted per read, and the one number the sizes below need comes back
        if (b->t_status.ensure((size_t)n + 16) || b->t_rowcnt.ensure((size_t)n * 4) || b->t_rowflag.ensure((size_t)n * 4) || b->t_rowfirst.ensure(((size_t)n + 1) * 8) ||
            b->t_rowucum.ensure(((size_t)n + 1) * 8) || b->t_rowsrc.ensure((size_t)(s.n_recs + n) * 8) || b->scan_tmp.ensure(((size_t)n / 1024 + 8) * 8)) return GM_E_NOMEM;
        HIPCHK(hipMemcpyAsync(b->t_status.p, c.hits->status, n, hipMemcpyHostToDevice, st));
        KCHK(gmk_row_source(s.n_recs ? b->o_recs.as<GmDevSamRec>() : nullptr, s.n_recs, n, b->t_rowcnt.as<uint32_t>(), b->t_rowflag.as<uint32_t>(), b->t_rowfirst.as<uint64_t>(),
                            b->t_rowucum.as<uint64_t>(), b->scan_tmp.as<unsigned long long>(), b->t_rowsrc.as<unsigned long long>(), st));
        HIPCHK(hipMemcpyAsync(&s.n_unmapped, b->t_rowucum.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (s.n_unmapped > n) { gm_set_error(std::string(c.who) + ": the row source counts more reads without a record than the block has reads"); return GM_E_HIP; }
        s.n_rows = s.n_recs + s.n_unmapped;
    }
    const uint64_t n_recs = s.n_rows;                              // (what is sized below is per row)
    if (const int rc = index_cnames(ix)) return rc;                // contig names, once per index
    // the pools of a text block start at offset 0 and are in place; a block without a quality tail passes none, as a caller would
    const bool tails = pools ? b->text_tail_bytes != 0 : rt->qual_tail_off != nullptr;
    const uint64_t name0 = pools ? 0 : rt->name_off[0], tail0 = pools || !tails ? 0 : rt->qual_tail_off[0];
    const uint64_t name_bytes = pools ? 0 : rt->name_off[n] - name0, tail_bytes = pools || !tails ? 0 : rt->qual_tail_off[n] - tail0;
    if ((!pools && (b->t_names.ensure((size_t)name_bytes + 16) || b->t_nameoff.ensure(((size_t)n + 1) * 8))) || b->t_slots.ensure((size_t)n_recs * 64) ||
        b->t_rowlen.ensure((size_t)n_recs * 4) || b->t_rowoff.ensure(((size_t)n_recs + 1) * 8) || b->t_bad.ensure(8) || (bam && b->t_bammeta.ensure((size_t)n_recs * 8)) ||
        b->scan_tmp.ensure(((size_t)n_recs / 1024 + 8) * 8) ||
        (!pools && tails && (b->t_qtail.ensure((size_t)tail_bytes + 16) || b->t_qtailoff.ensure(((size_t)n + 1) * 8)))) return GM_E_NOMEM;
    if (!pools) {
        b->text_pools = false;                                     // the caller's names take the place of the parse's
        // the offsets are used as they are: the kernels index names - name_off[0] so that a caller may pass a window of a larger pool
        if (name_bytes) HIPCHK(hipMemcpyAsync(b->t_names.p, rt->names + rt->name_off[0], (size_t)name_bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b->t_nameoff.p, rt->name_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    }
    if (!pools && tails) {
        if (tail_bytes) HIPCHK(hipMemcpyAsync(b->t_qtail.p, rt->qual_tail + rt->qual_tail_off[0], (size_t)tail_bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b->t_qtailoff.p, rt->qual_tail_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    }
    GmDevText& t = s.t;
    t.recs = b->o_recs.as<GmDevSamRec>(); t.n_recs = s.n_recs; t.pool = b->o_pool.as<char>();
    t.n_rows = s.n_rows; t.n_reads = n;
    t.row_src = s.unmapped ? b->t_rowsrc.as<unsigned long long>() : nullptr; t.status = s.unmapped ? b->t_status.as<int8_t>() : nullptr;
    t.names = b->t_names.as<char>() - name0; t.name_off = b->t_nameoff.as<uint64_t>();
    t.qtail = tails ? b->t_qtail.as<char>() - tail0 : nullptr; t.qtail_off = tails ? b->t_qtailoff.as<uint64_t>() : nullptr;
    t.cnames = ix->d_cnames.as<char>(); t.cname_off = ix->d_cname_off.as<uint32_t>();
    t.slots = b->t_slots.as<uint8_t>(); t.row_len = b->t_rowlen.as<uint32_t>(); t.row_off = b->t_rowoff.as<uint64_t>();
    t.inv_adjust = 1.0 / p->adjust; t.bad = b->t_bad.as<unsigned long long>();
    t.seq_len = b->adaptor.empty() ? b->dev.len : b->full_len.as<uint16_t>();
    t.fa_qual = fasta_qual_word();
    t.cigar_forward = b->cigar_order == GM_CIGAR_FORWARD ? 1u : 0u;
    t.mate = nullptr;                                          // (out_mates sets it)
    t.md = nullptr; t.pac = nullptr; t.contig_off = nullptr; t.l_pac = t.n_seqs = 0; t.holes = nullptr; t.n_holes = 0;
    if (b->row_tags & GM_ROW_TAG_MD) {
        // {NM, MD bytes} per row, the reference and its holes: allocated, uploaded and read only with the setting on
        if (const int rc = index_holes(ix)) return rc;
        if (b->t_md.ensure((size_t)n_recs * 8 + 16)) return GM_E_NOMEM;
        t.md = b->t_md.as<uint32_t>();
        t.pac = ix->dev.pac; t.contig_off = ix->dev.contig_off; t.l_pac = ix->dev.l_pac; t.n_seqs = ix->dev.n_seqs;
        t.holes = ix->d_holes.as<uint32_t>(); t.n_holes = (uint32_t)(ix->h.holes.size() / 3);
    }
    return GM_OK;
}

// gm_batch_set_mates: the pairs are resolved on the records where out_write_records left them, and every row gets its fields.  A rows
// sink comes here with the GmDevText of out_row_inputs (the row source, the names in HBM): the names are cut by the QNAME rule into a
// pool of their own, which the row kernels then read, and a pair whose printed names differ ends the call - before a row is
// written, a capacity is answered or anything is deposited.  The records sink has no rows and no names: its rows are its records.
// One read-back: the five counters and the first such pair
static int out_mates(gm_batch* b, const OutCall& c, OutState& s, hipStream_t st) {
    const uint32_t n = s.n;
    GmDevText& t = s.t;
    if (!c.rows() || !(s.n_recs || s.unmapped)) {              // no row step: the records are the rows
        t = GmDevText{};
        t.recs = s.n_recs ? b->o_recs.as<GmDevSamRec>() : nullptr; t.n_recs = s.n_recs; t.n_rows = s.n_recs; t.n_reads = n;
    }
    const bool names = c.rows() && t.names != nullptr;
    const uint64_t name_room = !names ? 0 : c.rt ? c.rt->name_off[n] - c.rt->name_off[0] : b->text_name_bytes;
    if (b->m_span.ensure((size_t)s.n_recs * 4 + 16) || b->m_first.ensure((size_t)n * 8 + 16) || b->m_end.ensure((size_t)n * 8 + 16) || b->m_prim.ensure((size_t)n * 8 + 16) ||
        b->m_proper.ensure((size_t)n / 2 + 16) || b->m_meta.ensure(MT_META_N * 8) || b->m_fields.ensure((size_t)t.n_rows * sizeof(GmDevMateRow) + 16) ||
        b->scan_tmp.ensure(((size_t)n / 1024 + 8) * 8) ||
        (names && (b->m_namelen.ensure((size_t)n * 4 + 16) || b->m_nameoff.ensure(((size_t)n + 1) * 8) || b->m_names.ensure((size_t)name_room + 16)))) return GM_E_NOMEM;
    GmDevMates m{};
    m.recs = t.recs; m.n_recs = s.n_recs; m.pool = b->o_pool.as<char>(); m.n_reads = n; m.min_insert = b->mate_min; m.max_insert = b->mate_max;
    m.span = b->m_span.as<uint32_t>(); m.first = b->m_first.as<unsigned long long>(); m.end = b->m_end.as<unsigned long long>();
    m.prim = b->m_prim.as<unsigned long long>(); m.proper = b->m_proper.as<uint8_t>(); m.meta = b->m_meta.as<unsigned long long>();
    unsigned long long meta[MT_META_N] = { 0 };
    {
        KTimer kt(b, GM_K_MATES, st);
        KCHK(gmk_mate_resolve(m, st));
        if (names) {
            KCHK(gmk_mate_names(t.names, t.name_off, n, b->m_namelen.as<uint32_t>(), b->m_nameoff.as<uint64_t>(), b->scan_tmp.as<unsigned long long>(), b->m_names.as<char>(),
                                name_room, c.bam_rows() ? 254u : 1023u, m.meta, st));
            t.names = b->m_names.as<char>(); t.name_off = b->m_nameoff.as<uint64_t>();
        }
        KCHK(gmk_mate_fields(m, t, b->m_fields.as<GmDevMateRow>(), st));
    }
    HIPCHK(hipMemcpyAsync(meta, m.meta, sizeof meta, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (names && meta[MT_META_BAD_PAIR] != ~0ull) {
        gm_set_error(std::string(c.who) + ": gm_batch_set_mates: the names of pair " + std::to_string(meta[MT_META_BAD_PAIR]) + " (reads " + std::to_string(2 * meta[MT_META_BAD_PAIR]) +
                     " and " + std::to_string(2 * meta[MT_META_BAD_PAIR] + 1) + " of the block) differ as printed: the two files are not in step");
        return GM_E_ARG;
    }
    t.mate = b->m_fields.as<GmDevMateRow>();
    b->mate_n_rows = t.n_rows;
    b->mate_stats = { meta[MT_META_PAIRS], meta[MT_META_BOTH], meta[MT_META_PROPER], meta[MT_META_ONE], meta[MT_META_NONE] };
    return GM_OK;
}

// Rows, their sizes: tails + row lengths (the records' sizes take their place when the rows are BAM), their scan, and what comes back:
// the length of all rows and the first record the device cannot print
static int out_count_rows(gm_batch* b, const OutCall& c, OutState& s, hipStream_t st) {
    const bool bam = c.bam_rows(), bam_timed = bam && b->profiling;
    HIPCHK(hipMemsetAsync(b->t_bad.p, 0xFF, 8, st));
    KCHK(gmk_out_text_sizes(b->dev, s.t, st));
    if (bam_timed) { for (auto& e : b->bam_ev) if (!e) HIPCHK(hipEventCreate(&e)); HIPCHK(hipEventRecord(b->bam_ev[0], st)); }
    if (bam) KCHK(gmk_bam_sizes(s.t, b->t_bammeta.as<uint32_t>(), st));
    if (bam_timed) HIPCHK(hipEventRecord(b->bam_ev[1], st));
    if (s.t.mate && !bam) { KTimer kt(b, GM_K_MATES, st); KCHK(gmk_mate_row_len(s.t, st)); }               // gm_batch_set_mates: the flag and the mate columns onto row_len (a BAM record's size does not move)
    if (s.t.md) { KTimer kt(b, GM_K_MD_SIZES, st); KCHK(gmk_md_sizes(b->dev, s.t, bam ? 1 : 0, st)); }      // gm_batch_set_row_tags: the two tags' bytes onto row_len
    KCHK(gmk_scan_u32(s.t.row_len, s.n_rows, b->t_rowoff.as<uint64_t>(), b->scan_tmp.as<unsigned long long>(), st));
    s.bad_row = ~0ull;
    HIPCHK(hipMemcpyAsync(&s.text_len, b->t_rowoff.as<uint64_t>() + s.n_rows, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&s.bad_row, b->t_bad.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GM_OK;
}

// The text sink's capacity answer, then the rows: SAM text or BAM records, in the batch's t_text
static int out_write_rows(gm_batch* b, const OutCall& c, OutState& s, hipStream_t st) {
    const bool bam = c.bam_rows(), bam_timed = bam && b->profiling;
    const uint64_t n_recs = s.n_rows, text_len = s.text_len;       // (rows: the records, and with them the reads without one)
    if (s.bad_row != ~0ull) {
        gm_set_error("SAM record " + std::to_string(s.bad_row) + ": XA or XP is outside the range the device prints exactly (2^-200 <= |v| < 2^200)");
        return GM_E_UNSUPPORTED;
    }
    b->n_unmapped = s.n_unmapped;
    if (c.sink == OutCall::text) {
        gm_sam_text* tout = c.text_out();
        tout->text_len = text_len; tout->n_recs = n_recs;
        const bool rows_fit = !tout->row_off || tout->row_cap >= n_recs + 1;
        if (text_len > tout->text_cap || !rows_fit) {
            tout->text_cap = text_len;
            if (tout->row_off) tout->row_cap = n_recs + 1;
            gm_set_error("output buffers too small");
            return GM_E_CAPACITY;
        }
    }
    if (b->t_text.ensure((size_t)text_len + 16)) return GM_E_NOMEM;
    s.t.text = b->t_text.as<char>();
    if (bam_timed) HIPCHK(hipEventRecord(b->bam_ev[2], st));
    if (bam) KCHK(gmk_bam_rows(b->dev, s.t, b->t_bammeta.as<uint32_t>(), st));
    else KCHK(gmk_out_text_rows(b->dev, s.t, st));
    if (bam_timed) {
        float ms_a = 0, ms_b = 0;
        HIPCHK(hipEventRecord(b->bam_ev[3], st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventElapsedTime(&ms_a, b->bam_ev[0], b->bam_ev[1]));
        HIPCHK(hipEventElapsedTime(&ms_b, b->bam_ev[2], b->bam_ev[3]));
        b->bam_rows_ms += (double)ms_a + ms_b; b->bam_raw_bytes += text_len;
    }
    return GM_OK;
}

// The rows leave: to the caller's buffers; into the sorter's arena, where they stay in HBM (an arena that cannot grow: GM_E_NOMEM from
// gm_samsort_add); or compressed where they lie, the BGZF blocks to the caller's buffer once it is known to hold them
static int out_deliver_rows(gm_batch* b, const OutCall& c, const OutState& s, hipStream_t st) {
    const uint64_t n_recs = s.n_rows, text_len = s.text_len;
    switch (c.sink) {
    case OutCall::text:
        HIPCHK(hipMemcpyAsync(c.text_out()->text, b->t_text.p, (size_t)text_len, hipMemcpyDeviceToHost, st));
        if (c.text_out()->row_off) HIPCHK(hipMemcpyAsync(c.text_out()->row_off, b->t_rowoff.p, ((size_t)n_recs + 1) * 8, hipMemcpyDeviceToHost, st));
        return GM_OK;
    case OutCall::sorted:
        return gm_samsort_add(c.sorter(), c.seq, s.t.recs, s.t.row_src, s.n_recs, n_recs, s.t.text, s.t.row_off, text_len, st);
    case OutCall::bam: {
        gm_bam_out* bout = c.bam_out();
        uint64_t z_len = 0;
        b->bz.timed = b->profiling;
        if (const int rc = gm_bgzf_device(b->t_text.p, text_len, bout->level, b->bz, &z_len, st)) return rc;
        bout->len = z_len; bout->raw_len = text_len; bout->n_recs = n_recs;
        if (z_len > bout->cap) { bout->cap = z_len; bout->len = 0; gm_set_error("output buffers too small"); return GM_E_CAPACITY; }
        HIPCHK(hipMemcpyAsync(bout->data, b->bz.out.p, (size_t)z_len, hipMemcpyDeviceToHost, st));
        return GM_OK;
    }
    case OutCall::records: break;                                  // (copied out where they were written)
    }
    return GM_OK;
}

// The coverage deposit (+ the per-nucleotide tracks of -b / -d / --snp): the one step that cannot be taken back
static int out_deposit(gm_index* ix, gm_batch* b, const OutState& s, hipStream_t st) {
    const uint32_t n_m = s.n_m;
    const GmDevMatch* d_m = b->g_matches.as<GmDevMatch>(); const GmDevPos* d_p = b->g_positions.as<GmDevPos>();
    if (!ix->cov_bins || !s.n_p) return GM_OK;
    if (s.snp) {
        // SNPScoredSeq::score: no traceback in the deposit - the pair HMM of every kept sequence against its window, chunk by chunk (a
        // lane's forward matrix is (L+1)^2 x 3 doubles of scratch), then coverage + the five tracks at every place of the sequence
        const uint32_t Lmax = b->stride;
        const uint32_t chunk = (uint32_t)std::min<long long>(std::max<long long>(64, gm_opt_ll("GM_SNP_CHUNK", 16384)), n_m) / 64u * 64u + 64u;
        const size_t cells = gmk_pair_hmm_cells(Lmax);
        if (b->snp_scratch.ensure((size_t)((chunk + 63) / 64) * cells * 8) || b->snp_hmm.ensure((size_t)chunk * Lmax * 5 * 4)) return GM_E_NOMEM;
        GM_TRACE("snp deposit: %u kept sequences, chunks of %u: %u chunk%s", n_m, chunk, (n_m + chunk - 1) / chunk, (n_m + chunk - 1) / chunk == 1 ? "" : "s");
        for (uint32_t m0 = 0; m0 < n_m; m0 += chunk) {
            const uint32_t cnt = std::min<uint32_t>(chunk, n_m - m0);
            KCHK(gmk_pair_hmm(ix->dev, s.dp, b->dev, b->tb_items.as<GmCand>() + m0, cnt, b->snp_scratch.as<double>(), Lmax, b->snp_hmm.as<float>(), st));
            KCHK(gmk_snp_deposit(ix->d_cov.as<float>(), ix->d_nuc.as<float>(), ix->cov_bins, ix->cov_bin_size, b->dev, d_m, d_p, m0, cnt, b->o_post.as<float>(),
                                 b->snp_hmm.as<float>(), Lmax, st));
        }
    } else if (s.max_span) {
        const bool nuc = s.nuc;
        if (nuc) KCHK(gmk_out_codes(b->dev, s.dp, d_m, n_m, b->tb_ops.as<unsigned long long>(), s.ops_words, b->tb_len.as<uint16_t>(), b->o_codes.as<uint8_t>(), s.codes_stride, st));
        KCHK(gmk_out_deposit(ix->d_cov.as<float>(), ix->cov_bins, ix->cov_bin_size, d_m, d_p, b->o_posmatch.as<uint32_t>(), s.n_p, b->tb_len.as<uint16_t>(),
                             b->o_post.as<float>(), s.max_span, nuc ? ix->d_nuc.as<float>() : nullptr, nuc ? b->o_codes.as<uint8_t>() : nullptr, s.codes_stride, st));
    }
    return GM_OK;
}

// The steps of one call, in the order things happen.  ONE RULE orders them: nothing is deposited before every capacity answer has been
// given.  A call that answers GM_E_CAPACITY is repeated with larger buffers, and the repeated call must deposit once, not twice: so the
// deposit is the last step, and the three capacity answers (records, text, BGZF blocks) come from steps before it; so does every other
// refusal, the sorter's among them (GM_E_NOMEM when its arena cannot grow).  What an earlier step does leave behind says so: the
// batch's stamp is cleared once a caller's matches have taken the place of the resident ones, its text_pools once a caller's names have.
// gm_batch_set_unmapped_rows (read by the rows sinks alone; the records sink ignores it): the four row steps size everything by ROWS -
// the records plus one row for every read without a record - and a block in which nothing matched gives n rows with no traceback,
// posterior pass or deposit instead of the early GM_OK.
static int output_batch(gm_index* ix, const gm_params* p, gm_batch* b, const OutCall& c, void* stream) {
    if (const int rc = out_check_call(b, c)) return rc;
    PhaseClock pc(c.rows() ? "gm_output_batch_text" : "gm_output_batch");
    HIPCHK(hipSetDevice(ix->device));
    hipStream_t st = S_(stream);
    OutState s{};
    if (const int rc = sync_params(ix, p, s.dp, st)) return rc;
    if (c.sink == OutCall::records) { c.recs_out()->n_recs = 0; c.recs_out()->cigar_len = 0; }
    s.unmapped = c.rows() && b->unmapped_rows;
    if (c.rows()) b->n_unmapped = 0;
    b->mate_n_rows = 0; b->mate_stats = gm_mate_stats{};
    const bool matched = c.hits->n && c.hits->match_begin[c.hits->n];
    if (!matched && !(s.unmapped && c.hits->n)) {                              // nothing matched: no record, no row, no deposit
        if (b->mates) b->mate_stats.pairs = b->mate_stats.none_mapped = c.hits->n / 2;
        return GM_OK;
    }
    if (matched) {
        if (const int rc = out_check_hits(ix, p, b, c.hits, s)) return rc;
        if (const int rc = out_enqueue_traceback(ix, p, b, c.hits, s, st)) return rc;
        pc.lap("enqueue");
        if (const int rc = out_host_posteriors(p, b, c.hits, s)) return rc;
        pc.lap("fp64");
        if (const int rc = out_count_records(b, s, st)) return rc;
        pc.lap("traceback+count");
        if (const int rc = out_write_records(ix, p, b, c, s, st)) return rc;
    } else s.n = c.hits->n;                                                    // n rows and no traceback, posterior pass or deposit
    if (c.rows() && (s.n_recs || s.unmapped)) {
        if (const int rc = out_row_inputs(ix, p, b, c, s, st)) return rc;
        if (b->mates) if (const int rc = out_mates(b, c, s, st)) return rc;
        if (const int rc = out_count_rows(b, c, s, st)) return rc;
        pc.lap("text sizes");
        if (const int rc = out_write_rows(b, c, s, st)) return rc;
        if (const int rc = out_deliver_rows(b, c, s, st)) return rc;
    }
    else if (b->mates) { if (const int rc = out_mates(b, c, s, st)) return rc; }      // (the records sink, and rows sinks with nothing to print)
    if (matched) if (const int rc = out_deposit(ix, b, s, st)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    pc.lap("records+coverage");
    return GM_OK;
}

// ---- the seven entry points: fill the call, run it ----
// The check they share, in the order every one of them answers: ix, a host-only index, the other pointers, then what the form needs
static int out_entry_check(const gm_index* ix, const gm_params* p, const gm_batch* b, const OutCall& c) {
    auto named = [&c](const char* why) { return std::string(c.who) + ": " + why; };
    if (!ix) return GM_E_ARG;
    if (ix->host_only) {
        const char* why = "no usable HIP device (host-only index)";
        gm_set_error(c.needs & OUT_PLAIN_NO_DEVICE ? std::string(why) : named(why));
        return GM_E_NO_DEVICE;
    }
    if (!p || !b || (!c.reads && !(c.needs & OUT_NEEDS_POOLS)) || !c.hits || !c.dest) return GM_E_ARG;
    if ((c.needs & OUT_NEEDS_RT) && !c.rt) { gm_set_error(named("gm_read_text is NULL")); return GM_E_ARG; }
    if ((c.needs & OUT_NEEDS_POOLS) && (!b->text_block || !b->text_pools)) { gm_set_error(named("the batch holds no names from gm_batch_upload_text")); return GM_E_ARG; }
    return GM_OK;
}

// The check, then the steps.  A resident form takes no gm_reads (the steps ask it for n only).  The sorted sink claims its sequence
// number before the steps and gives it back when they fail (a no-op once rows of the block are in the arena).
static int output_call(gm_index* ix, const gm_params* p, gm_batch* b, OutCall c, void* stream) {
    if (const int rc = out_entry_check(ix, p, b, c)) return rc;
    gm_reads resident{};
    if (c.needs & OUT_NEEDS_POOLS) { resident.n = b->n; resident.stride = b->stride; c.reads = &resident; }
    if (c.sink != OutCall::sorted) return output_batch(ix, p, b, c, stream);
    if (const int rc = gm_samsort_claim(c.sorter(), ix, c.seq)) return rc;
    const int rc = output_batch(ix, p, b, c, stream);
    if (rc != GM_OK) gm_samsort_release(c.sorter(), c.seq);
    return rc;
}

extern "C" int gm_output_batch(gm_index* ix, const gm_params* p, gm_batch* b, const gm_reads* reads, const gm_hits* hits, gm_sam_out* out, void* stream) {
    return output_call(ix, p, b, { "gm_output_batch", OutCall::records, 0, reads, hits, nullptr, 0, out }, stream);
}

// gm_output_batch with a different ending: the SAM rows leave as finished text (src/Driver.cpp:2146-2217, ScoredSeq::get_SAM
// inc/ScoredSeq.h:293-404, reverse_comp / reverse_CIGAR inc/SequenceOperations.h:56-123), written by k_out_text_sizes / k_out_text_rows
// (gm_output.hip) from the records and the CIGAR pool where k_out_write left them
extern "C" int gm_output_batch_text(gm_index* ix, const gm_params* p, gm_batch* b, const gm_reads* reads, const gm_read_text* rt, const gm_hits* hits, gm_sam_text* out,
                                    void* stream) {
    return output_call(ix, p, b, { "gm_output_batch_text", OutCall::text, OUT_NEEDS_RT | OUT_PLAIN_NO_DEVICE, reads, hits, rt, 0, out }, stream);
}

extern "C" int gm_output_batch_text_resident(gm_index* ix, const gm_params* p, gm_batch* b, const gm_hits* hits, gm_sam_text* out, void* stream) {
    return output_call(ix, p, b, { "gm_output_batch_text_resident", OutCall::text, OUT_NEEDS_POOLS, nullptr, hits, nullptr, 0, out }, stream);
}

// the rows as BAM records inside BGZF blocks (k_bam_sizes / k_bam_rows / k_bgzf_*, gm_bam.hip)
extern "C" int gm_output_batch_bam(gm_index* ix, const gm_params* p, gm_batch* b, const gm_reads* reads, const gm_read_text* rt, const gm_hits* hits, gm_bam_out* out,
                                   void* stream) {
    return output_call(ix, p, b, { "gm_output_batch_bam", OutCall::bam, OUT_NEEDS_RT, reads, hits, rt, 0, out }, stream);
}

extern "C" int gm_output_batch_bam_resident(gm_index* ix, const gm_params* p, gm_batch* b, const gm_hits* hits, gm_bam_out* out, void* stream) {
    return output_call(ix, p, b, { "gm_output_batch_bam_resident", OutCall::bam, OUT_NEEDS_POOLS, nullptr, hits, nullptr, 0, out }, stream);
}

extern "C" int gm_batch_bam_times(gm_batch* b, double* ms, uint64_t* bytes) {
    if (!b || !ms || !bytes) return GM_E_ARG;
    ms[0] = b->bam_rows_ms; ms[1] = b->bz.ms;
    bytes[0] = b->bam_raw_bytes; bytes[1] = b->bz.in_bytes; bytes[2] = b->bz.out_bytes;
    b->bam_rows_ms = 0; b->bam_raw_bytes = 0; b->bz.ms = 0; b->bz.in_bytes = 0; b->bz.out_bytes = 0;
    return GM_OK;
}

// the rows kept in HBM: appended to the sorter's arena under `seq` (gm_samsort.hip)
extern "C" int gm_output_batch_sorted(gm_index* ix, const gm_params* p, gm_batch* b, const gm_reads* reads, const gm_read_text* rt, const gm_hits* hits, gm_sam_sorter* sorter,
                                      uint64_t seq, void* stream) {
    return output_call(ix, p, b, { "gm_output_batch_sorted", OutCall::sorted, OUT_NEEDS_RT, reads, hits, rt, seq, sorter }, stream);
}

extern "C" int gm_output_batch_sorted_resident(gm_index* ix, const gm_params* p, gm_batch* b, const gm_hits* hits, gm_sam_sorter* sorter, uint64_t seq, void* stream) {
    return output_call(ix, p, b, { "gm_output_batch_sorted_resident", OutCall::sorted, OUT_NEEDS_POOLS, nullptr, hits, nullptr, seq, sorter }, stream);
}

// gm_batch_upload_text on a batch of its own, the rows brought back (unit level, parity tests)
extern "C" int gm_dev_fastq_rows(gm_index* ix, const char* text, uint64_t bytes, gm_text_info* info, gm_text_rec* recs, uint8_t* bases, uint8_t* quals, uint16_t* len,
                                 uint64_t rows_cap) {
    if (!ix) return GM_E_ARG;
    if (ix->host_only) { gm_set_error("gm_dev_fastq_rows: no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (!info || (bytes && !text)) return GM_E_ARG;
    gm_params p;
    gm_params_default(&p);
    int rc = gm_params_finalize(&p);
    if (rc) return rc;
    gm_batch* b = nullptr;
    rc = gm_batch_create(ix, 16000000u, 2048, &b);
    if (rc) return rc;
    auto run = [&]() -> int {
        int r = gm_batch_upload_text(b, &p, text, bytes, info, nullptr, 0, nullptr);
        if (r) return r;
        const uint32_t n = b->n;
        if (n > rows_cap) { gm_set_error("gm_dev_fastq_rows: room for fewer reads than the text holds"); return GM_E_CAPACITY; }
        if (n == 0) return GM_OK;
        const size_t row_bytes = (size_t)n * b->stride;
        if (recs) HIPCHK(hipMemcpy(recs, b->rt_recs.p, (size_t)n * sizeof(gm_text_rec), hipMemcpyDeviceToHost));
        if (bases) HIPCHK(hipMemcpy(bases, b->bases.p, row_bytes, hipMemcpyDeviceToHost));
        if (quals) HIPCHK(hipMemcpy(quals, b->quals.p, row_bytes, hipMemcpyDeviceToHost));
        if (len) memcpy(len, b->len_host.data(), (size_t)n * 2);
        return GM_OK;
    };
    rc = run();
    const std::string err = gm_last_error();
    gm_batch_destroy(b);
    if (rc) gm_set_error(err);
    return rc;
}

extern "C" uint32_t gm_dev_fastq_tile_bytes(void) { return gmk_readtext_tile_bytes(); }

// gm_put_g6_hd (gm_fmt_dev.h) on the device, one lane per value: out[i * 16 ..] holds len[i] characters (0 = outside its domain)
static int dev_fmt_probe(gm_index* ix, const double* v, uint32_t n, char* out, uint8_t* len, int (*kernel)(const double*, uint32_t, char*, uint8_t*, void*)) {
    if (!ix || (n && (!v || !out || !len))) return GM_E_ARG;
    if (ix->host_only) { gm_set_error("no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (n == 0) return GM_OK;
    HIPCHK(hipSetDevice(ix->device));
    DevBuf dv, dout, dlen;
    int rc = GM_OK;
    if (dv.ensure((size_t)n * 8) || dout.ensure((size_t)n * 16) || dlen.ensure(n)) rc = GM_E_NOMEM;
    auto run = [&]() -> int {
        HIPCHK(hipMemcpy(dv.p, v, (size_t)n * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dout.p, 0, (size_t)n * 16));
        KCHK(kernel(dv.as<double>(), n, dout.as<char>(), dlen.as<uint8_t>(), nullptr));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(len, dlen.p, n, hipMemcpyDeviceToHost));
        return GM_OK;
    };
    if (rc == GM_OK) rc = run();
    dv.release(); dout.release(); dlen.release();
    return rc;
}
extern "C" int gm_dev_fmt_g6(gm_index* ix, const double* v, uint32_t n, char* out, uint8_t* len) { return dev_fmt_probe(ix, v, n, out, len, gmk_fmt_g6); }
// gm_put_e2_hd the same way: "%.2e" as k_track_rows prints the p-value of --snp's ninth column
extern "C" int gm_dev_fmt_e2(gm_index* ix, const double* v, uint32_t n, char* out, uint8_t* len) { return dev_fmt_probe(ix, v, n, out, len, gmk_fmt_e2); }

// gmk_scan_u32 on values of the caller's: out[i] = in[0] + .. + in[i - 1] in 64 bits, out[n] the total (the scan behind every offset
// array of the map and output steps).  The scratch is sized as those steps size theirs
extern "C" int gm_dev_scan_u32(gm_index* ix, const uint32_t* in, uint64_t n, uint64_t* out) {
    if (!ix || !out || (n && !in)) return GM_E_ARG;
    if (ix->host_only) { gm_set_error("no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    if (n > (1ull << 32)) { gm_set_error("gm_dev_scan_u32: more than 2^32 values"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(ix->device));
    DevBuf din, dout, dtmp;
    int rc = GM_OK;
    if (din.ensure((size_t)n * 4 + 16) || dout.ensure(((size_t)n + 1) * 8) || dtmp.ensure(((size_t)n / 1024 + 8) * 8)) rc = GM_E_NOMEM;
    auto run = [&]() -> int {
        if (n) HIPCHK(hipMemcpy(din.p, in, (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dout.p, 0xFF, ((size_t)n + 1) * 8));                  // (a value the scan does not write shows)
        KCHK(gmk_scan_u32(din.as<uint32_t>(), n, dout.as<uint64_t>(), dtmp.as<unsigned long long>(), nullptr));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out, dout.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
        return GM_OK;
    };
    if (rc == GM_OK) rc = run();
    din.release(); dout.release(); dtmp.release();
    return rc;
}

// gmk_mate_resolve and gmk_mate_fields on records, a CIGAR pool and a row source of the caller's: the GmDevMates / GmDevText that
// out_mates fills for a block, with nothing of a mapped batch behind them.  Everything a kernel would index with is checked here, on
// the host, before anything is uploaded: a refused call launches nothing
extern "C" int gm_dev_mate_resolve(gm_index* ix, const gm_sam_rec* recs, uint64_t n_recs, const char* cigar_pool, uint64_t cigar_bytes, uint32_t n_reads,
                                   uint32_t min_insert, uint32_t max_insert, const uint64_t* row_src, uint64_t n_rows,
                                   uint32_t* span, uint64_t* prim, uint8_t* proper, gm_mate_stats* stats, gm_mate_row* rows) {
    if (!ix || !stats || (n_recs && (!recs || !cigar_pool || !span)) || (n_reads && (!prim || !proper))) { gm_set_error("gm_dev_mate_resolve: a NULL argument"); return GM_E_ARG; }
    if (!row_src) n_rows = n_recs;
    if (n_rows && !rows) { gm_set_error("gm_dev_mate_resolve: rows is NULL"); return GM_E_ARG; }
    if (n_reads & 1u) { gm_set_error("gm_dev_mate_resolve: an odd number of reads (" + std::to_string(n_reads) + ")"); return GM_E_ARG; }
    if (min_insert > max_insert) { gm_set_error("gm_dev_mate_resolve: min_insert " + std::to_string(min_insert) + " is above max_insert " + std::to_string(max_insert)); return GM_E_ARG; }
    if (n_recs >= (1ull << 32) || n_rows >= (1ull << 32)) { gm_set_error("gm_dev_mate_resolve: fewer than 2^32 records and rows"); return GM_E_ARG; }
    // k_mate_spans walks a CIGAR from cigar_off to its NUL: the pool ends in one, and every offset lies inside it
    if (n_recs && (cigar_bytes == 0 || cigar_pool[cigar_bytes - 1] != 0)) { gm_set_error("gm_dev_mate_resolve: the CIGAR pool does not end in a NUL"); return GM_E_ARG; }
    for (uint64_t k = 0; k < n_recs; ++k) {
        if (recs[k].cigar_off >= cigar_bytes) { gm_set_error("gm_dev_mate_resolve: cigar_off of record " + std::to_string(k) + " lies outside the pool"); return GM_E_ARG; }
        if (recs[k].read >= n_reads || (k && recs[k].read < recs[k - 1].read)) {
            gm_set_error("gm_dev_mate_resolve: record " + std::to_string(k) + " is not in read order, or names no read of the block"); return GM_E_ARG;
        }
    }
    if (ix->host_only) { gm_set_error("no usable HIP device (host-only index)"); return GM_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(ix->device));
    DevBuf d_recs, d_pool, d_span, d_first, d_end, d_prim, d_proper, d_meta, d_src, d_rows;
    int rc = GM_OK;
    if (d_recs.ensure((size_t)n_recs * sizeof(GmDevSamRec) + 16) || d_pool.ensure((size_t)cigar_bytes + 16) || d_span.ensure((size_t)n_recs * 4 + 16) ||
        d_first.ensure((size_t)n_reads * 8 + 16) || d_end.ensure((size_t)n_reads * 8 + 16) || d_prim.ensure((size_t)n_reads * 8 + 16) ||
        d_proper.ensure((size_t)n_reads / 2 + 16) || d_meta.ensure(MT_META_N * 8) || d_src.ensure((size_t)n_rows * 8 + 16) ||
        d_rows.ensure((size_t)n_rows * sizeof(GmDevMateRow) + 16)) rc = GM_E_NOMEM;
    auto run = [&]() -> int {
        if (n_recs) {
            HIPCHK(hipMemcpy(d_recs.p, recs, (size_t)n_recs * sizeof(GmDevSamRec), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_pool.p, cigar_pool, (size_t)cigar_bytes, hipMemcpyHostToDevice));
        }
        if (row_src && n_rows) HIPCHK(hipMemcpy(d_src.p, row_src, (size_t)n_rows * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d_span.p, 0xFF, (size_t)n_recs * 4 + 16));                // (a value the kernels do not write shows)
        HIPCHK(hipMemset(d_prim.p, 0xEE, (size_t)n_reads * 8 + 16));
        HIPCHK(hipMemset(d_proper.p, 0xEE, (size_t)n_reads / 2 + 16));
        HIPCHK(hipMemset(d_rows.p, 0xEE, (size_t)n_rows * sizeof(GmDevMateRow) + 16));
        GmDevMates m{};
        m.recs = n_recs ? d_recs.as<GmDevSamRec>() : nullptr; m.n_recs = n_recs; m.pool = d_pool.as<char>(); m.n_reads = n_reads; m.min_insert = min_insert; m.max_insert = max_insert;
        m.span = d_span.as<uint32_t>(); m.first = d_first.as<unsigned long long>(); m.end = d_end.as<unsigned long long>();
        m.prim = d_prim.as<unsigned long long>(); m.proper = d_proper.as<uint8_t>(); m.meta = d_meta.as<unsigned long long>();
        GmDevText t{};
        t.recs = m.recs; t.n_recs = n_recs; t.n_rows = n_rows; t.n_reads = n_reads;
        t.row_src = row_src ? d_src.as<unsigned long long>() : nullptr;
        KCHK(gmk_mate_resolve(m, nullptr));
        KCHK(gmk_mate_fields(m, t, d_rows.as<GmDevMateRow>(), nullptr));
        HIPCHK(hipDeviceSynchronize());
        unsigned long long meta[MT_META_N] = { 0 };
        HIPCHK(hipMemcpy(meta, d_meta.p, sizeof meta, hipMemcpyDeviceToHost));
        *stats = { meta[MT_META_PAIRS], meta[MT_META_BOTH], meta[MT_META_PROPER], meta[MT_META_ONE], meta[MT_META_NONE] };
        if (n_recs) HIPCHK(hipMemcpy(span, d_span.p, (size_t)n_recs * 4, hipMemcpyDeviceToHost));
        if (n_reads) {
            HIPCHK(hipMemcpy(prim, d_prim.p, (size_t)n_reads * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(proper, d_proper.p, (size_t)n_reads / 2, hipMemcpyDeviceToHost));
        }
        if (n_rows) HIPCHK(hipMemcpy(rows, d_rows.p, (size_t)n_rows * sizeof(gm_mate_row), hipMemcpyDeviceToHost));
        return GM_OK;
    };
    if (rc == GM_OK) rc = run();
    for (DevBuf* d : { &d_recs, &d_pool, &d_span, &d_first, &d_end, &d_prim, &d_proper, &d_meta, &d_src, &d_rows }) d->release();
    return rc;
}

// ------------------------------------------------------------------------------------------------
// enqueue / wait forms of the two batch calls: a caller thread hands a block to the batch's service thread and goes on with the next
// block on another batch; uploads, device work and the fp64 passes of different batches overlap without one caller thread per batch.
// Calls queued on one batch run in the order they were queued; after a failing call the rest of that batch's queue is skipped.
// ------------------------------------------------------------------------------------------------
static void svc_post(gm_batch* b, std::function<int()> job) {
    gm_batch::Service& sv = b->svc;
    std::lock_guard<std::mutex> lk(sv.mu);
    if (!sv.th.joinable())
        sv.th = std::thread([b] {
            gm_batch::Service& v = b->svc;
            for (;;) {
                std::function<int()> j;
                {
                    std::unique_lock<std::mutex> lk2(v.mu);
                    v.cv.wait(lk2, [&] { return v.quit || !v.q.empty(); });
                    if (v.q.empty()) return;
                    j = std::move(v.q.front()); v.q.pop_front();
                    v.busy = true;
                }
                int rc = GM_OK; std::string err;
                bool skip;
                { std::lock_guard<std::mutex> lk2(v.mu); skip = v.rc != GM_OK; }
                if (!skip) { rc = j(); if (rc != GM_OK) err = gm_last_error(); }
                {
                    std::lock_guard<std::mutex> lk2(v.mu);
                    if (rc != GM_OK && v.rc == GM_OK) { v.rc = rc; v.err = err; }
                    v.busy = false;
                }
                v.cv.notify_all();
            }
        });
    sv.q.push_back(std::move(job));
    sv.cv.notify_all();
}

extern "C" int gm_map_batch_enqueue(gm_index* ix, const gm_params* p, gm_batch* b, const gm_reads* reads, gm_hits* out, void* stream) {
    if (!ix || !p || !b || !reads || !out) return GM_E_ARG;
    const gm_params pc = *p; const gm_reads rc = *reads;           // the structs are copied; the arrays they point to stay the caller's until gm_batch_wait
    svc_post(b, [=]() { return gm_map_batch(ix, &pc, b, &rc, out, stream); });
    return GM_OK;
}

extern "C" int gm_output_batch_enqueue(gm_index* ix, const gm_params* p, gm_batch* b, const gm_reads* reads, const gm_hits* hits, gm_sam_out* out, void* stream) {
    if (!ix || !p || !b || !reads || !hits || !out) return GM_E_ARG;
    const gm_params pc = *p; const gm_reads rc = *reads;
    svc_post(b, [=]() { return gm_output_batch(ix, &pc, b, &rc, hits, out, stream); });     // `hits` is read when the call runs: the gm_hits a queued gm_map_batch fills
    return GM_OK;
}

extern "C" int gm_batch_wait(gm_batch* b) {
    if (!b) return GM_E_ARG;
    gm_batch::Service& sv = b->svc;
    std::unique_lock<std::mutex> lk(sv.mu);
    sv.cv.wait(lk, [&] { return sv.q.empty() && !sv.busy; });
    const int rc = sv.rc;
    if (rc != GM_OK) gm_set_error(sv.err);
    sv.rc = GM_OK; sv.err.clear();
    return rc;
}

// ------------------------------------------------------------------------------------------------
// unit-level device entry points
// ------------------------------------------------------------------------------------------------
extern "C" int gm_dev_sa_interval(gm_index* ix, const char* kmers, uint32_t n, uint32_t m, uint64_t* start, uint64_t* end) {
    if (!ix || !kmers || !start || !end || m == 0) return GM_E_ARG;
    if (ix->host_only) return GM_E_NO_DEVICE;
    HIPCHK(hipSetDevice(ix->device));
    DevBuf dk, ds, de;
    if (dk.ensure((size_t)n * m) || ds.ensure((size_t)n * 4) || de.ensure((size_t)n * 4)) return GM_E_NOMEM;
    int rc = GM_OK;
    std::vector<uint32_t> s(n), e(n);
    do {
        if (hipMemcpy(dk.p, kmers, (size_t)n * m, hipMemcpyHostToDevice) != hipSuccess) { rc = GM_E_HIP; break; }
        if (gmk_sa_interval(ix->dev, dk.as<uint8_t>(), n, m, ds.as<uint32_t>(), de.as<uint32_t>(), nullptr)) { rc = GM_E_HIP; break; }
        if (hipMemcpy(s.data(), ds.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = GM_E_HIP; break; }
        if (hipMemcpy(e.data(), de.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = GM_E_HIP; break; }
    } while (0);
    dk.release(); ds.release(); de.release();
    if (rc) { gm_set_error("gm_dev_sa_interval: HIP failure"); return rc; }
    for (uint32_t i = 0; i < n; ++i) { start[i] = s[i]; end[i] = e[i]; }
    return GM_OK;
}

extern "C" int gm_dev_locate(gm_index* ix, const uint64_t* ranks, uint32_t n, int use_full_sa, uint64_t* out) {
    if (!ix || !ranks || !out) return GM_E_ARG;
    if (ix->host_only) return GM_E_NO_DEVICE;
    if (use_full_sa && !ix->full_sa) { gm_set_error("index was opened without GM_INDEX_FULL_SA"); return GM_E_ARG; }
    HIPCHK(hipSetDevice(ix->device));
    std::vector<uint32_t> r32(n), o32(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (ranks[i] == 0 || ranks[i] > ix->h.seq_len) { gm_set_error("rank out of range"); return GM_E_ARG; }
        r32[i] = (uint32_t)ranks[i];
    }
    DevBuf dr, dout;
    if (dr.ensure((size_t)n * 4) || dout.ensure((size_t)n * 4)) return GM_E_NOMEM;
    int rc = GM_OK;
    do {
        if (hipMemcpy(dr.p, r32.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = GM_E_HIP; break; }
        if (gmk_locate(ix->dev, dr.as<uint32_t>(), n, use_full_sa, dout.as<uint32_t>(), nullptr)) { rc = GM_E_HIP; break; }
        if (hipMemcpy(o32.data(), dout.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = GM_E_HIP; break; }
    } while (0);
    dr.release(); dout.release();
    if (rc) { gm_set_error("gm_dev_locate: HIP failure"); return rc; }
    for (uint32_t i = 0; i < n; ++i) out[i] = o32[i];
    return GM_OK;
}

static int unit_batch(gm_index* ix, const gm_params* p, const gm_reads* reads, gm_batch** bo, GmDevParams& dp, bool nw_probe = false) {
    gm_batch* b = nullptr;
    int rc = gm_batch_create(ix, reads->n ? reads->n : 1, reads->stride ? reads->stride : 1, &b);
    if (rc) return rc;
    b->read_format = ix->probe_format;                   // gm_index_set_probe_format
    rc = gm_batch_upload(b, p, reads, nullptr);
    if (!rc && nw_probe) rc = fasta_forced_form(b);            // (the DP score kernel runs for gm_dev_nw_score only)
    if (!rc) rc = sync_params(ix, p, dp, nullptr);
    if (!rc) {
        if (hipMemsetAsync(b->counters.p, 0, GMK_N * 8, nullptr) != hipSuccess || hipMemsetAsync(b->small.p, 0, 64, nullptr) != hipSuccess ||
            hipMemsetAsync(b->rs_overflow.p, 0, 2 * (size_t)b->n, nullptr) != hipSuccess || gmk_prep(ix->dev, dp, b->dev, nullptr)) rc = GM_E_HIP;
    }
    if (rc) { gm_batch_destroy(b); return rc; }
    *bo = b;
    return GM_OK;
}

extern "C" int gm_dev_prep(gm_index* ix, const gm_params* p, const gm_reads* reads, uint32_t first_row, int exact, int8_t* status, float* self_score,
                           double* min_score, uint32_t* pack, uint32_t* pack_words, uint64_t* work) {
    if (!ix || !p || !reads || !status || !self_score || !min_score || !pack_words || !work || !p->finalized) return GM_E_ARG;
    if (first_row > reads->n || (exact && first_row)) return GM_E_ARG;
    if (ix->host_only) return GM_E_NO_DEVICE;
    HIPCHK(hipSetDevice(ix->device));
    gm_batch* b; GmDevParams dp;
    int rc = unit_batch(ix, p, reads, &b, dp);           // (uploads, and runs the prep kernel once over the whole block without 2-bit rows)
    if (rc) return rc;
    const uint32_t n = b->n, lo = first_row, pw = gm_pack_words(b->stride);
    *pack_words = pw;
    DevBuf xb, xq;
    unsigned long long ctr[GMK_N];
    do {
        if (b->pack.ensure((size_t)n * pw * 4 + 64)) { rc = GM_E_NOMEM; break; }
        if (hipMemset(b->pack.p, 0, (size_t)n * pw * 4) != hipSuccess || hipMemset(b->counters.p, 0, GMK_N * 8) != hipSuccess) { rc = GM_E_HIP; break; }
        GmDevBatch v = b->dev;
        v.n = n - lo; v.read_base = lo;
        v.illumina_until = b->illumina_until > lo ? b->illumina_until - lo : 0;
        v.bases += (size_t)lo * b->stride; v.quals += (size_t)lo * b->stride; v.len += lo;
        v.status += lo; v.self_score += lo; v.min_score += lo; v.top_score += lo; v.hit_count += lo; v.hit_cursor += lo;
        v.pack = b->pack.as<uint32_t>() + (size_t)lo * pw;
        const size_t row_bytes = (size_t)n * b->stride;
        if (exact && row_bytes) {                             // rows in allocations that end with the last row
            if (hipMalloc(&xb.p, row_bytes) != hipSuccess) { rc = GM_E_NOMEM; break; }
            xb.cap = row_bytes;
            if (hipMemcpy(xb.p, b->bases.p, row_bytes, hipMemcpyDeviceToDevice) != hipSuccess) { rc = GM_E_HIP; break; }
            v.bases = xb.as<uint8_t>();
            if (!b->fasta) {
                if (hipMalloc(&xq.p, row_bytes) != hipSuccess) { rc = GM_E_NOMEM; break; }
                xq.cap = row_bytes;
                if (hipMemcpy(xq.p, b->quals.p, row_bytes, hipMemcpyDeviceToDevice) != hipSuccess) { rc = GM_E_HIP; break; }
                v.quals = xq.as<uint8_t>();
            }
        }
        if (gmk_prep(ix->dev, dp, v, nullptr)) { rc = GM_E_HIP; break; }
        if (hipMemcpy(ctr, b->counters.p, sizeof ctr, hipMemcpyDeviceToHost) != hipSuccess) { rc = GM_E_HIP; break; }
        if (n && (hipMemcpy(status, b->status.p, n, hipMemcpyDeviceToHost) != hipSuccess ||
                  hipMemcpy(self_score, b->self_score.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                  hipMemcpy(min_score, b->min_score.p, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess ||
                  (pack && hipMemcpy(pack, b->pack.p, (size_t)n * pw * 4, hipMemcpyDeviceToHost) != hipSuccess))) { rc = GM_E_HIP; break; }
    } while (0);
    xb.release(); xq.release();
    gm_batch_destroy(b);
    if (rc) { gm_set_error("gm_dev_prep: HIP failure"); return rc; }
    work[0] = ctr[GMK_BAD_QUAL]; work[1] = ctr[GMK_HIGH_QUAL]; work[2] = gm_qual_lo(ctr); work[3] = gm_qual_hi(ctr);
    return GM_OK;
}

extern "C" int gm_dev_nw_score(gm_index* ix, const gm_params* p, const gm_reads* reads, const uint32_t* read_idx, const uint8_t* strand,
                               const uint64_t* pos, uint32_t n, float* score, uint8_t* valid) {
    if (!ix || !p || !reads || !read_idx || !strand || !pos || !score || !p->finalized) return GM_E_ARG;
    if (ix->host_only) return GM_E_NO_DEVICE;
    HIPCHK(hipSetDevice(ix->device));
    gm_batch* b; GmDevParams dp;
    int rc = unit_batch(ix, p, reads, &b, dp, true);
    if (rc) return rc;
    std::vector<GmCand> c(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (read_idx[i] >= reads->n || pos[i] > 0xFFFFFFFFull) { gm_batch_destroy(b); return GM_E_ARG; }
        c[i].rs = read_idx[i] * 2 + (strand[i] ? 1 : 0); c[i].b = (uint32_t)pos[i]; c[i].step = 0; c[i].flags = 0; c[i].pad = 0; c[i].score = 0;
    }
    do {
        b->cand_cap = std::max<uint32_t>(b->cand_cap, n + 16);
        if (b->cands.ensure((size_t)b->cand_cap * sizeof(GmCand))) { rc = GM_E_NOMEM; break; }
        fill_dev_batch(b);
        b->dev.cand_region = b->cand_cap;               // everything sits in shard 0
        if (n && hipMemcpy(b->cands.p, c.data(), (size_t)n * sizeof(GmCand), hipMemcpyHostToDevice) != hipSuccess) { rc = GM_E_HIP; break; }
        if (hipMemset(b->shards.p, 0, (size_t)GM_NSHARD * GM_SHARD_STRIDE * 4) != hipSuccess) { rc = GM_E_HIP; break; }
        if (hipMemcpy(b->shards.p, &n, 4, hipMemcpyHostToDevice) != hipSuccess) { rc = GM_E_HIP; break; }
        uint32_t rows_len = (b->len_min == b->len_max) ? b->len_max : 0u;          // (no k_prep here: the quality characters are looked at on the host)
        uint32_t qlo = 255, qhi = 0;                                                // (of the reads' own characters, as k_prep counts them: a row's padding is not data)
        for (uint32_t r = 0; r < reads->n && !b->fasta; ++r)
            for (uint32_t i = 0; i < reads->len[r] && i < reads->stride; ++i) { const uint32_t qc = reads->quals[(size_t)r * reads->stride + i]; qlo = std::min(qlo, qc); qhi = std::max(qhi, qc); }
        if (qhi >= 128) rows_len = 0;
        GM_TRACE("dev_nw_score: %u probes, nw=%s", n, gmk_nw_form(dp, b->dev, n, rows_len, qlo, qhi));
        if (gmk_nw(ix->dev, dp, b->dev, n, rows_len, qlo, qhi, false, nullptr)) { rc = GM_E_HIP; break; }
        if (n && hipMemcpy(c.data(), b->cands.p, (size_t)n * sizeof(GmCand), hipMemcpyDeviceToHost) != hipSuccess) { rc = GM_E_HIP; break; }
    } while (0);
    gm_batch_destroy(b);
    if (rc) { gm_set_error("gm_dev_nw_score: HIP failure"); return rc; }
    for (uint32_t i = 0; i < n; ++i) { score[i] = c[i].score; if (valid) valid[i] = (c[i].flags & GMC_VALID) ? 1 : 0; }
    return GM_OK;
}

extern "C" int gm_dev_traceback(gm_index* ix, const gm_params* p, const gm_reads* reads, const uint32_t* read_idx, const uint8_t* strand,
                                const uint64_t* pos, uint32_t n, char* ops, uint32_t ops_stride, uint16_t* ops_len) {
    if (!ix || !p || !reads || !read_idx || !strand || !pos || !ops || !ops_len || !p->finalized) return GM_E_ARG;
    if (ix->host_only) return GM_E_NO_DEVICE;
    HIPCHK(hipSetDevice(ix->device));
    gm_batch* b; GmDevParams dp;
    int rc = unit_batch(ix, p, reads, &b, dp);
    if (rc) return rc;
    std::vector<GmCand> c(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (read_idx[i] >= reads->n || pos[i] > 0xFFFFFFFFull) { gm_batch_destroy(b); return GM_E_ARG; }
        c[i].rs = read_idx[i] * 2 + (strand[i] ? 1 : 0); c[i].b = (uint32_t)pos[i]; c[i].step = 0; c[i].flags = 0; c[i].pad = 0; c[i].score = 0;
    }
    const uint32_t ow = gm_ops_words(b->stride);
    std::vector<unsigned long long> packed((size_t)n * ow);
    do {
        if (b->tb_items.ensure((size_t)n * sizeof(GmCand) + 16) || b->tb_ops.ensure((size_t)n * ow * 8 + 16) || b->tb_len.ensure((size_t)n * 2 + 16)) { rc = GM_E_NOMEM; break; }
        if (n && hipMemcpy(b->tb_items.p, c.data(), (size_t)n * sizeof(GmCand), hipMemcpyHostToDevice) != hipSuccess) { rc = GM_E_HIP; break; }
        if (n && hipMemset(b->tb_ops.p, 0, (size_t)n * ow * 8) != hipSuccess) { rc = GM_E_HIP; break; }
        if (p->max_gap != 3) { if (b->band_moves.ensure(gm_band_moves_words(n, b->stride) * 8)) { rc = GM_E_NOMEM; break; } fill_dev_batch(b); }
        GM_TRACE("dev_traceback: %u probes, traceback=%s", n, gmk_traceback_form(dp, b->dev));
        if (gmk_traceback(ix->dev, dp, b->dev, b->tb_items.as<GmCand>(), n, b->tb_ops.as<unsigned long long>(), ow, b->tb_len.as<uint16_t>(), nullptr, nullptr, nullptr, nullptr)) { rc = GM_E_HIP; break; }
        if (n && hipMemcpy(packed.data(), b->tb_ops.p, (size_t)n * ow * 8, hipMemcpyDeviceToHost) != hipSuccess) { rc = GM_E_HIP; break; }
        if (n && hipMemcpy(ops_len, b->tb_len.p, (size_t)n * 2, hipMemcpyDeviceToHost) != hipSuccess) { rc = GM_E_HIP; break; }
        for (uint32_t i = 0; i < n; ++i) {                                // the public form: one character per operation
            char* o = ops + (size_t)i * ops_stride;
            memset(o, 0, ops_stride);
            for (uint32_t k = 0; k < ops_len[i] && k < ops_stride; ++k) o[k] = "MID?"[(packed[(size_t)i * ow + (k >> 5)] >> (2 * (k & 31))) & 3];
        }
    } while (0);
    gm_batch_destroy(b);
    if (rc) { gm_set_error("gm_dev_traceback: HIP failure"); return rc; }
    return GM_OK;
}

extern "C" int gm_dev_pair_hmm(gm_index* ix, const gm_params* p, const gm_reads* reads, const uint32_t* read_idx, const uint8_t* strand, const uint64_t* pos,
                               uint32_t n, float* out) {
    if (!ix || !p || !reads || !read_idx || !strand || !pos || !out || !p->finalized) return GM_E_ARG;
    if (ix->host_only) return GM_E_NO_DEVICE;
    HIPCHK(hipSetDevice(ix->device));
    gm_batch* b; GmDevParams dp;
    if (ix->probe_format == GM_READS_FASTA) { gm_set_error("gm_dev_pair_hmm: the pair HMM of --snp takes FASTQ reads only"); return GM_E_UNSUPPORTED; }
    int rc = unit_batch(ix, p, reads, &b, dp);
    if (rc) return rc;
    std::vector<GmCand> c(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (read_idx[i] >= reads->n || pos[i] + reads->len[read_idx[i]] > ix->h.l_pac) { gm_batch_destroy(b); return GM_E_ARG; }
        c[i].rs = read_idx[i] * 2 + (strand[i] ? 1 : 0); c[i].b = (uint32_t)pos[i]; c[i].step = 0; c[i].flags = 0; c[i].pad = 0; c[i].score = 0;
    }
    const uint32_t Lmax = b->stride;
    do {
        if (b->tb_items.ensure((size_t)n * sizeof(GmCand) + 16) || b->snp_scratch.ensure((size_t)((n + 63) / 64) * gmk_pair_hmm_cells(Lmax) * 8 + 16) ||
            b->snp_hmm.ensure((size_t)n * Lmax * 5 * 4 + 16)) { rc = GM_E_NOMEM; break; }
        if (n && hipMemcpy(b->tb_items.p, c.data(), (size_t)n * sizeof(GmCand), hipMemcpyHostToDevice) != hipSuccess) { rc = GM_E_HIP; break; }
        if (n && hipMemset(b->snp_hmm.p, 0, (size_t)n * Lmax * 5 * 4) != hipSuccess) { rc = GM_E_HIP; break; }
        if (gmk_pair_hmm(ix->dev, dp, b->dev, b->tb_items.as<GmCand>(), n, b->snp_scratch.as<double>(), Lmax, b->snp_hmm.as<float>(), nullptr)) { rc = GM_E_HIP; break; }
        if (n && hipMemcpy(out, b->snp_hmm.p, (size_t)n * Lmax * 5 * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = GM_E_HIP; break; }
    } while (0);
    gm_batch_destroy(b);
    if (rc) { gm_set_error("gm_dev_pair_hmm: HIP failure"); return rc; }
    return GM_OK;
}
