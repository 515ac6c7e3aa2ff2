// gm_internal.h — structures shared by the HIP kernels (gm_kernels.hip) and the host side of libgnumap_hip.
// Nothing here is part of the public ABI (include/gnumap_hip.h).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

// ---- HBM-resident index, passed to kernels by value -------------------------------------------------
// bwt      : the occ-interleaved BWT exactly as <fa>.gnumap.bwt stores it: one 64-byte block per 128 bases
//            = 4 x u64 cumulative counts (A,C,G,T before the block) + 8 x u32 of 16 bases, MSB first
//            (reference: bwt_bwtupdate_core src/bwtindex.c:128-150, bwt_occ_intv inc/bwt.h:73)
// sa_samples: rank-sampled suffix array (every 32nd rank), narrowed to u32; [0] = 0xFFFFFFFF (= (u64)-1 mod 2^32)
// full_sa  : optional full suffix array SA[0..seq_len], u32, expanded on device from the samples
// pac      : 2 bit/base, 4 per byte MSB first (reference: _get_pac src/bntseq.c:225)
// occ_planes: the MI355X-native rank structure derived from bwt once per index: for each base c a bit plane over the
//            $-removed BWT, cut into 16-byte granules {u32 count of c before the granule, 96 membership bits}, so that
//            one rank query (bwt_occ) is ONE 16-byte load + three popcounts.  planes[c * occ_nblk + x / 96].
struct GmDevIndex {
    const uint32_t* bwt;
    const uint4* occ_planes;
    uint32_t occ_nblk;
    const uint32_t* sa_samples;
    const uint32_t* full_sa;
    const uint8_t* pac;
    const uint32_t* contig_off;     // n_seqs + 1 offsets, last = l_pac
    uint32_t seq_len, primary, l_pac, n_seqs;
    uint32_t sa_mask, sa_shift;     // sa_intv - 1, log2(sa_intv)
    uint32_t L2[5];
};

struct GmDevParams {
    int mer, jump, kmin, nw, fast, pos_strand, neg_strand, align_is_fraction;
    int max_gap;                    // -M: band half-width of the DP (3 = the register-band kernels, anything else = gm_band.hip)
    int fused;                      // 1 = the one-wave vote kernels look their seeds up themselves (no k_seed launch, no seed rows in HBM)
    uint32_t heavy_min;             // read x strands with more SA hits than this go to the sorted-key path (gm_heavy.hip)
    uint32_t hcap;
    int dbg;                        // GM_DBG bits for kernel timing experiments (0 in production)
    float gap, align_score, cutoff;
    const float* S256;              // gALIGN_SCORES, 256 x 4, in HBM: the self score indexes it with the FASTQ characters,
                                    // the DP with rows 'a','c','g','t' (genome windows are lowercase acgt)
    const uint2* kmer_tab;          // SA interval of every kmer_T-mer (suffix of the seed k-mer), or null: {k,l}; empty = {0xFFFFFFFF, depth}
    int kmer_T;
    const uint4* kmer_ctab;         // compact form of kmer_tab, 16 B per 8 consecutive codes: {first SA rank, 8 x u8 hit counts (2 words), escape flag}; null = not built
    const float2* lut;              // [0..255] Phred+33, [256..511] Phred+64: (p, (1-p)/3) as fp32; p = NaN when negative;
                                    // [512..527] FASTA blocks: (in-mask, out-of-mask) probability of a row by its 4-bit base mask (GM_LUT_FASTA)
    const uint4* bucket;            // direct-addressed k-mer -> positions table (gm_bucket.hip): 128 bytes per mer-mer code, or null
    uint32_t bucket_ecap, bucket_ovcap;   // k_vote_bucket votes itself on a strand with at most this many SA hits / seeds beyond 28 hits; more -> list kernel
    int bucket_T, bucket_ctx;       // the table's k-mer length; 1 = context records: seeds of bucket_T + 1 .. bucket_T + 5 characters (k_build_bucket_ctx)
};

#define GM_LUT_FASTA 512u         // GmDevParams::lut: where the 16 (p, q) pairs of the FASTA rows start
#define GM_LUT_ENTRIES 528u

struct GmSeed { uint32_t k, l, pos; };

#if defined(__HIPCC__)
// base masks of PWM rows (bit 0 = A .. bit 3 = T), for every kernel translation unit; see gm_get_val_mask (gm_device.h)
__device__ __forceinline__ uint32_t gm_mask_rc(uint32_t m) { return ((m & 1u) << 3) | ((m & 2u) << 1) | ((m & 4u) >> 1) | ((m & 8u) >> 3); }
__device__ __forceinline__ uint32_t gm_code_mask(uint32_t code) { return code < 4u ? 1u << code : 0u; }
// letters a .. z (either case) -> mask, 4 bits each: a 1, b 14, c 2, d 13, g 4, h 11, k 12, m 3, n 15, r 5, s 6, t 8, v 7, w 9, y 10;
// every other byte 0 (the host refuses such a file; here it is a row of four q)
__device__ __forceinline__ uint32_t gm_iupac_mask(uint32_t ch) {
    const uint32_t l = (ch | 0x20u) - 'a';                          // 0 .. 25 for a letter
    const unsigned long long lo = 0x00F30C00B400D2E1ull;            // a .. p (a = bits 0..3)
    const unsigned long long hi = 0x0000000A09708650ull;            // q .. z (q = bits 0..3)
    const uint32_t m = l < 16u ? (uint32_t)(lo >> (4u * l)) : (uint32_t)(hi >> (4u * (l & 15u)));
    return (l < 26u && (ch & 0xC0u) == 0x40u) ? (m & 15u) : 0u;
}
#endif

#define GM_FIXED_C 4
// own candidate slots of read x strand rs, in blocks of 64 read x strands: the 64 slots 0 side by side (what k_cand_gather reads of
// EVERY read x strand: one 1 KB stretch per wavefront instead of 16 bytes out of every 64), slots 1 .. 3 behind them
#define GM_FIXED_AT(b, rs, idx) (((size_t)(rs) >> 6) * (64 * GM_FIXED_C) + ((idx) == 0 ? ((size_t)(rs) & 63) : 64 + ((size_t)(rs) & 63) * (GM_FIXED_C - 1) + (size_t)(idx) - 1))
#define GM_GROUP_BIG 64          // accepted hits per read above which grouping takes the hash-set + sort path
#define GM_ADAPTOR_MAX 256       // longest -A / --adaptor sequence gm_batch_set_adaptor takes (k_adaptor_trim keeps it in LDS)
#define GM_NSHARD 1024
#define GM_SHARD_STRIDE 32

// flags of GmCand
enum { GMC_VALID = 1, GMC_ACCEPT = 2 };
struct GmCand {
    uint32_t rs;                    // read * 2 + strand
    uint32_t b;                     // candidate window start on the concatenated reference
    uint16_t step;                  // seed index at which the vote count reached kmin (NW order of the reference)
    uint8_t flags, pad;
    float score;                    // NW score, or the vote count with --no_nw
};

struct GmRawHit { uint32_t read; uint32_t pos; float score; uint16_t step; uint8_t strand; uint8_t pad; };

// device-side counters, one u64 each (see gm_counters in the public header)
enum {
    GMK_KMERS = 0, GMK_OCC, GMK_SEEDS, GMK_SA_HITS, GMK_LF_STEPS, GMK_CANDS, GMK_NW_CELLS, GMK_ACCEPTED,
    GMK_OVERFLOW_RS, GMK_BAD_QUAL, GMK_HEAVY_SLOTS, GMK_OCC_BLOCKS, GMK_TAB_LOOKUPS,
    GMK_HIGH_QUAL,                  // k_prep: reads with a quality character above 127 (k_nw_rows' value table stops there)
    GMK_QUAL_MIN, GMK_QUAL_MAX,     // k_prep: 255 - the smallest, and the largest, quality character of the block (a zeroed pair = no read):
                                    // the range k_nw_rows' pair table covers
    GMK_DBG0, GMK_DBG1, GMK_DBG2, GMK_DBG3, GMK_DBG4, GMK_DBG5, GMK_DBG6, GMK_DBG7, GMK_DBG8,      // GM_DBG & 64: sampled phase clocks of the vote kernel
    GMK_N
};

struct GmDevBatch {
    uint32_t n, stride, max_seeds, illumina_until;
    uint32_t read_base;             // index of read 0 of this (sub-)batch in the caller's batch (raw hits carry absolute indices)
    uint32_t fasta;                 // 1 = a FASTA block (gm_batch_set_read_format): `bases` holds the file's letters, a position's PWM row is its
                                    // IUPAC letter's (get_more_fasta, SeqReader.cpp:875-979: base mask + lut[GM_LUT_FASTA + mask]); `quals` is not read
    const uint8_t* bases;
    const uint8_t* quals;
    const uint16_t* len;
    int8_t* status;                 // n
    float* self_score;              // n
    double* min_score;              // n
    float* top_score;               // n
    GmSeed* seeds;                  // 2n x max_seeds
    uint16_t* n_seeds;              // 2n
    uint32_t* n_entries;            // 2n   number of SA hits of the seeds used
    uint64_t* entry_off;            // 2n+1 exclusive scan of n_entries (sampled-SA mode only)
    uint32_t* coords;               // located coordinates, entry_off order (sampled-SA mode only)
    uint8_t* rs_overflow;           // 2n   1 = LDS vote table overflowed, handled by the global-table kernel
    uint32_t* retry_list;           // list of overflowed rs
    uint64_t* retry_off;            // table offsets for the retry list
    uint32_t* gtab_keys;            // global vote tables (retry path)
    uint32_t* gtab_vals;
    // candidates are appended through GM_NSHARD bump counters (one 128-byte line each) instead of one global counter:
    // shard s owns cands[s * cand_region, (s+1) * cand_region)
    GmCand* cands;  uint32_t cand_cap, cand_region;
    uint32_t* shard_cnt;            // GM_NSHARD counters, GM_SHARD_STRIDE words apart
    // the one-wave vote kernels (k_vote_tiny*) do not wait for a bump counter: a read x strand with at most GM_FIXED_C candidates
    // stores them into its own slots (plain stores, the wave retires) and k_cand_gather moves them into the shards afterwards with
    // ONE atomic per 64 read x strands; null = not in use
    GmCand* fixed_cands;            // 2n x GM_FIXED_C
    uint8_t* fixed_cnt;             // 2n, zeroed before the vote kernel
    uint32_t fixed_epoch;           // != 0: no fixed_cnt - slot 0 of a read x strand says how many of its slots are in use (pad) and for which launch (score bits = this value)
    uint32_t* hit_count;            // n
    uint64_t* hit_begin;            // n+1
    uint32_t* hit_cursor;           // n
    GmRawHit* raw_hits;  uint64_t raw_cap;
    unsigned long long* counters;   // GMK_N
    uint32_t* n_retry;              // device counter
    uint32_t* n_big;                // device counter: read x strands handed from k_vote_sparse to k_vote_fast_list
    uint32_t* big_list;             // 2n
    // 2-bit forms of the reads for the fused seed lookup (written by k_prep when non-null), pack_words words per read:
    //   [0]                  length | (some base is not ACGT) << 16 | (status != 0) << 17
    //   F  [1, w2+2)         base p of the read at bit 2 (16 w2 - 1 - p): 2 mer bits from bit 2 (16 w2 - i - mer) are the table code of
    //                        the k-mer [i, i+mer) (last character lowest)
    //   F' [w2+2, 2 w2+3)    the same for the reverse complement of the read (its base p' at bit 2 (16 w2 - 1 - p'))
    // so that a k-mer's words sit at an address that does not depend on the read's length: one round trip for both.
    uint32_t* pack; uint32_t pack_w2, pack_words;
    unsigned long long* band_moves; // -M other than 3: move words of k_traceback_band, [row][item]; band_moves_words of them
    uint64_t band_moves_words;
};

// device mirrors of the public records (include/gnumap_hip.h: gm_match, gm_pos, gm_sam_rec; layouts asserted in gm_api.cpp), so that
// the kernels of gm_output.hip write them in HBM in their final form
struct GmDevMatch { uint32_t read; float score; unsigned long long first_pos; uint8_t first_strand; uint8_t pad[3]; uint32_t pos_begin, pos_end; uint32_t tail; };
struct GmDevPos { unsigned long long pos; uint8_t strand; uint8_t pad[7]; };
struct GmDevSamRec { uint32_t read, pad0; unsigned long long pos; uint32_t contig, pad1; unsigned long long chr_pos; uint8_t strand; uint8_t pad2[3];
                     int32_t mapq; float a_score, post_prob; int32_t sim_matches; uint32_t cigar_off; };

// gm_mate_row (layout asserted in gm_api.cpp): what a row prints of its mate - flag, contig of the mate's primary (-1: none), its POS
// (0: none), TLEN
struct GmDevMateRow { uint32_t flag; int32_t rnext; uint32_t pnext; int32_t tlen; };

// what the SAM text kernels (k_out_text_*, gm_output.hip) read and write besides the block itself
struct GmDevText {
    const GmDevSamRec* recs; unsigned long long n_recs;
    const char* pool;                               // CIGAR pool of k_out_write (NUL-terminated, forward orientation)
    const char* names; const uint64_t* name_off;    // gm_read_text::names / name_off of the block, in HBM
    const char* qtail; const uint64_t* qtail_off;   // gm_read_text::qual_tail / qual_tail_off, or null
    const char* cnames; const uint32_t* cname_off;  // contig names back to back, n_seqs + 1 offsets (uploaded once per index)
    // 64 bytes per record: [0, 56) the numeric tail "XA:f:..\tXP:f:..\tX0:i:..\n", [56] u16 CIGAR length in the pool, [58] u16 CIGAR
    // length in the row (a reversed CIGAR drops trailing digits without an operation), [60] u8 length of the tail
    uint8_t* slots;
    uint32_t* row_len; const uint64_t* row_off;     // bytes of every row; their exclusive scan (n_recs + 1)
    char* text;
    double inv_adjust;                              // 1.0 / gADJUST: XA is printed rescaled
    unsigned long long* bad;                        // smallest record whose XA / XP lies outside gm_put_g6_hd's domain (~0: none)
    const uint16_t* seq_len;                        // characters of SEQ / QUAL a row prints: the block's lengths as uploaded (with -A the whole line, not the kept part)
    uint32_t fa_qual;                               // FASTA blocks: str2qual's character of a row with 1, 2, 3, 4 bases in its mask, in bytes 0 .. 3
    // The row source.  n_rows rows are written: slots, row_len and row_off are per ROW.  row_src null (the default): row k is record k
    // and n_rows == n_recs.  gm_batch_set_unmapped_rows: row k is record row_src[k], or - GM_ROW_UNMAPPED set - read
    // row_src[k] & ~GM_ROW_UNMAPPED of the block, which has no record and gets a flag-4 row with YU:i:status[read] (gmk_row_source)
    unsigned long long n_rows; const unsigned long long* row_src; const int8_t* status; uint32_t n_reads;
    // gm_batch_set_cigar_order: 1 = a minus-strand row prints its CIGAR in pool order, as a plus-strand row does (0: token by token reversed)
    uint32_t cigar_forward;
    // gm_batch_set_row_tags (null / 0 with the setting off: nothing below is read).  md: {NM, bytes of the MD string} per row, left by
    // k_md_sizes; 0 bytes = the row gets no tags (no record, or CIGAR "*").  The walk (gm_mdtag_dev.h) reads the reference as pac
    // letters, or inside a hole of <fa>.gnumap.amb that hole's character: holes = {offset, length, upper-cased character} per hole,
    // ascending offsets, uploaded once per index
    uint32_t* md;
    const uint8_t* pac; const uint32_t* contig_off; uint32_t l_pac, n_seqs;
    const uint32_t* holes; uint32_t n_holes;
    // gm_batch_set_mates (null with the setting off: the instances of the row kernels that read it are not launched).  One entry per
    // row, in row order, left by k_mate_fields (gm_mates.hip).  names / name_off are then the names after the QNAME rule's cuts
    const GmDevMateRow* mate;
};
#define GM_ROW_UNMAPPED (1ull << 63)
#if defined(__HIPCC__)
// row k: true = it prints record `rec`; false = it stands for read `read`, which has no record.  An entry that names neither a record
// nor a read of the block (gmk_row_source leaves none) comes back as read ~0: the row kernels write nothing for it
__device__ __forceinline__ bool gm_row_is_record(const GmDevText& t, unsigned long long k, unsigned long long& rec, uint32_t& read) {
    rec = k; read = 0xFFFFFFFFu;
    if (!t.row_src) return true;
    const unsigned long long e = t.row_src[k];
    if (!(e & GM_ROW_UNMAPPED)) { rec = e; return e < t.n_recs; }
    const unsigned long long r = e & ~GM_ROW_UNMAPPED;
    if (r < t.n_reads) read = (uint32_t)r;
    return false;
}
#endif

// what the mate kernels (k_mate_*, gm_mates.hip) read and write: the block's records in read order and their CIGAR pool in; per record
// its span, per read its record range [first, end) and its primary (a record index, ~0: none), per pair whether it is proper
enum { MT_META_PAIRS = 0, MT_META_BOTH, MT_META_PROPER, MT_META_ONE, MT_META_NONE,     // gm_mate_stats, in its order
       MT_META_BAD_PAIR,            // the first pair whose printed names differ (~0: none)
       MT_META_N = 8 };
struct GmDevMates {
    const GmDevSamRec* recs; unsigned long long n_recs; const char* pool;
    uint32_t n_reads, min_insert, max_insert;
    uint32_t* span; unsigned long long* first; unsigned long long* end; unsigned long long* prim; uint8_t* proper;
    unsigned long long* meta;
};

// gm_snp_rec (layout asserted in gm_tracks.cpp): a row of --snp's .gmp that carries a 'Y' call, written by k_snp_gather (gm_snpcall.hip)
struct GmDevSnpRec { unsigned long long pos; uint32_t contig, pad0; unsigned long long chr_pos; float total, nuc[5]; double p_val; uint8_t ref, alt1, alt2, diploid;
                     uint8_t pad1[4]; };

// what the track text kernels (k_track_sizes / k_track_rows, gm_tracktext.hip) read and write: bins [lo, lo + n) of the coverage track
enum { GM_TRACK_SGR = 0, GM_TRACK_SNP = 1, GM_TRACK_BASE = 2,       // .sgr; --snp's .gmp; the .gmp of -b / --b2 / -d (rows of one reference base)
       GM_TRACK_CALLS = 3 };                                        // --snp's .gmp with PrintSNPCall's ninth column (bin size 1)
enum { TT_META_BYTES = 0, TT_META_ROWS = 1, TT_META_HOST = 2, TT_META_N = 4 };
struct GmDevTrack {
    const float* cov; const float* nuc; uint64_t nuc_stride;         // nuc: a c g t n tracks nuc_stride floats apart, or null (.sgr)
    const uint8_t* pac; const uint32_t* contig_off; uint32_t n_seqs;
    const char* cnames; const uint32_t* cname_off;                   // contig names back to back, n_seqs + 1 offsets
    uint64_t lo, n;
    uint32_t bin_size, kind, want;                                   // GM_TRACK_*; want: 2-bit code of the reference base of GM_TRACK_BASE
    uint32_t* tile_len; unsigned long long* tile_off;                // bytes of text per tile of 256 bins; their exclusive scan (tiles + 1)
    unsigned long long* meta;                                        // TT_META_*: bytes and rows of the slab, 1 = a value only the host can print (zeroed by the caller)
    char* text;                                                      // 16-byte aligned
    const uint8_t* code; const double* pval;                         // GM_TRACK_CALLS: k_snp_call's code byte and p-value of bin lo + i at [i]
};

// gm_text_rec (layout asserted in gm_api.cpp): where the name (behind '@'), the sequence line and the quality line of a read lie in the text
struct GmDevTextRec { uint32_t name_off, seq_off, qual_off, name_len, seq_len, qual_len; };
// what the FASTQ text kernels (k_rt_*, gm_readtext.hip) read and write
enum { RT_META_LINES = 0,           // lines of the text
       RT_META_END,                 // where the last line ends
       RT_META_RECS,                // records the text starts, good or not
       RT_META_BAD,                 // (index << 2 | RT_BAD_*) of the first record that ends the block; ~0: none (set by the caller)
       RT_META_N, RT_META_BAD_AT,   // records of the block; offset of the name line of the record that ended it
       RT_META_MAXLEN, RT_META_MINLEN,      // over the block's reads (MINLEN set to ~0 by the caller)
       RT_META_NAME_BYTES, RT_META_TAIL_BYTES,
       RT_META_N_WORDS = 16 };
enum { RT_BAD_FORM = 0, RT_BAD_LONG = 1 };
struct GmDevReadText {
    const uint8_t* text; uint64_t bytes;                             // 16-byte aligned, at least 16 readable bytes behind `bytes`; bytes < 2^32
    uint32_t* tile_cnt; uint32_t* tile_off; uint32_t n_tiles;        // newlines that start a line, per tile of text; their exclusive scan (n_tiles + 1)
    uint32_t* line_at; uint32_t n_lines;                             // line starts (known to the host after k_rt_scan)
    uint32_t* ltile_sum; uint32_t* ltile_in; uint32_t n_ltiles;      // per tile of lines: {map, records started when entered in phase 0 .. 3, -, -, -}; {phase entered in, records in front}
    GmDevTextRec* recs; uint32_t rec_cap;                            // n_lines / 4 + 1: every record but the last takes four lines
    uint16_t* len; uint32_t* name_len; uint32_t* tail_len;           // of the block's reads: sequence length, name bytes a row prints, quality bytes behind the sequence's length
    unsigned long long* meta;                                        // RT_META_*
};

// workspace of the grouping kernels (process_hits' unique map on the device); per-hit arrays share the CSR of hit_begin
struct GmDevGroup {
    GmRawHit* sorted;               // accepted hits of a read in the reference's processing order
    float* ord_score;               // their scores in that order (-inf: dropped by -u with --no_nw): the host sums exp() over these
    uint32_t* lead;                 // index (within the read) of the first hit with the same key; 0xFFFFFFFF = dropped
    uint32_t* krank;                // leaders: rank of the key among the read's keys (std::map<string> order)
    unsigned long long* khash;
    uint32_t* n_match;              // n: matches of a read (0 unless its status stays OK)
    uint64_t* match_begin;          // n+1: exclusive scan of n_match
    uint32_t* multi_list;           // reads with 2 .. GM_GROUP_BIG accepted hits (and the ones the big path hands back)
    uint32_t* n_multi;
    uint32_t* big_list;             // reads with more accepted hits: hash-set + sort path (k_group_big), linear in the hits
    uint32_t* n_big;
    uint8_t* big_done;              // per big_list entry: 1 = grouped by the big path (k_group_write_big finishes it)
    unsigned long long* sk0; unsigned long long* sk1; uint32_t* si0; uint32_t* si1;     // sort scratch, per hit
    GmDevMatch* matches;
    uint32_t* match_hit;            // per match: index (in the hit CSR, processing order) of the hit that gave the match its score
    GmDevPos* positions;            // same CSR as the hits (a read's positions live in [hit_begin[r], hit_begin[r+1]))
};

// Launchers (gm_kernels.hip, gm_output.hip).  All asynchronous on `stream`; they return a hipError_t cast to int.
#ifdef __cplusplus
extern "C++" {
// run-time switches (GM_*): the value set with gm_set_option(), else the environment variable, else null.  Read on EVERY call:
// a long-lived host (and one test process) can change a choice between two batches.  Defined in gm_api.cpp.
const char* gm_opt(const char* name);
inline long long gm_opt_ll(const char* name, long long dflt) { const char* e = gm_opt(name); return e && *e ? atoll(e) : dflt; }
inline bool gm_opt_is(const char* name, const char* value) { const char* e = gm_opt(name); return e && !strcmp(e, value); }
// TEST switch GM_TEST_GRID_CAP=N: at most N workgroups for a kernel that strides over its items with gridDim.x, so that a block of a few
// hundred reads gives every workgroup several trips (what a 10 M-read block does at the launcher's own cap).  Unset or 0: `grid` as it is.
// Only for launchers whose kernel loops: a kernel that takes one item per workgroup would drop items.
inline uint32_t gm_test_grid(uint32_t grid) {
    const long long cap = gm_opt_ll("GM_TEST_GRID_CAP", 0);
    return cap > 0 && (long long)grid > cap ? (uint32_t)cap : grid;
}
int gmk_expand_full_sa(const GmDevIndex& ix, uint32_t* full_sa, void* stream);
int gmk_build_occ_planes(const GmDevIndex& ix, uint4* planes, uint32_t nblk, void* stream);
int gmk_build_kmer_table(const GmDevIndex& ix, uint2* tab, int T, void* stream);
int gmk_build_kmer_compact(const uint2* tab, uint4* ctab, int T, void* stream);
int gmk_extend_kmer_table(const GmDevIndex& ix, const uint2* prev, uint2* next, int T, void* stream);
int gmk_prep(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, void* stream);
int gmk_prep_rows(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, void* stream);      // gm_prep.hip (stride <= 152)
// full_len != null (-A): the lengths as uploaded, b.len being what the adaptor trim kept: the minus strand's k-mers come from the END of the line
int gmk_seed(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, void* stream, const uint16_t* full_len = nullptr);
int gmk_scan_entries(const GmDevBatch& b, void* stream);
int gmk_locate_sampled(const GmDevIndex& ix, const GmDevBatch& b, unsigned long long n_entries /* SA hits of the block = entries of coords[] */, void* stream);
int gmk_vote(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, int use_full_sa, int dense, int slots_hint, void* stream);
int gmk_cand_gather(const GmDevBatch& b, void* stream);
int gmk_shard_stats(const GmDevBatch& b, uint32_t* out /* {total, max, *pair_n (0 without)} in device memory */, const uint32_t* pair_n, void* stream);
// gm_bucket.hip: the bucket table and the one-wave-per-read vote kernel that looks its seeds up in it
int gmk_build_bucket(const uint2* tab, const uint32_t* full_sa, const uint8_t* pac, uint4* bucket, int T, int ctx, void* stream);
// rlist / n_rlist (device memory) != null: only the reads of that list
int gmk_vote_bucket(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, uint32_t max_reg, const uint32_t* rlist, const uint32_t* n_rlist, void* stream);
// gm_pair.hip: two reads per wavefront for the common case; the reads it flags (fallback[r] = 1) are listed for gmk_vote_bucket
int gmk_vote_pair(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, uint32_t max_reg, uint8_t* fallback, uint32_t* list, uint32_t* n_list, void* stream);
int gmk_vote_list(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, int use_full_sa, void* stream);     // k_vote_fast_list over b.big_list
// gm_heavy.hip: read x strands with more than heavy_min SA hits (sorted-key vote path)
int gmk_heavy_collect(const GmDevBatch& b, uint32_t heavy_min, uint32_t* n_heavy, uint32_t* heavy_list /* {rs, n_seeds, SA hits} triples */, int sum_counters,
                      const uint32_t* rlist /* nullptr: all 2n read x strands; else only the reads listed here (device count n_rlist) */, const uint32_t* n_rlist, void* stream);
inline uint32_t gm_pack_w2(uint32_t stride) { return (stride + 15u) / 16u; }
inline uint32_t gm_pack_words(uint32_t stride) { const uint32_t w2 = gm_pack_w2(stride); return (1u + 2u * (w2 + 1u) + 3u) & ~3u; }
size_t gmk_heavy_sort_temp_bytes(size_t n_keys);
int gmk_heavy_chunk(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, int use_full_sa, const uint32_t* heavy_list, uint32_t j0, uint32_t nj,
                    const unsigned long long* key_off, unsigned long long* keys0, unsigned long long* keys1, unsigned long long n_keys, void* tmp,
                    size_t tmp_bytes, unsigned item_bits, void* stream);
int gmk_vote_retry(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, int use_full_sa, uint32_t j0, uint32_t n_retry, void* stream);
// rows_len != 0: every read of the block has this length and no quality character is above 127 -> k_nw_rows (gm_nw.hip) may take it
// [qual_lo, qual_hi] = the range of the block's quality characters (k_prep's GMK_QUAL_MIN / GMK_QUAL_MAX): the size of k_nw_rows' pair table
int gmk_nw(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, uint32_t n_cands, uint32_t rows_len, uint32_t qual_lo, uint32_t qual_hi, bool any_superseded, void* stream);
// which DP kernel gmk_nw launches for these arguments (k_nw_rows/pairs or k_nw_rows/cells for the two forms of k_nw_rows)
const char* gmk_nw_form(const GmDevParams& p, const GmDevBatch& b, uint32_t n_cands, uint32_t rows_len, uint32_t qual_lo, uint32_t qual_hi);
int gmk_nw_rows(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, uint32_t n_cands, uint32_t L, uint32_t qual_lo, uint32_t qual_hi, bool any_superseded, void* stream);
bool gmk_nw_rows_pairs(const GmDevBatch& b, uint32_t L, uint32_t qual_lo, uint32_t qual_hi);     // k_nw_rows takes its pair table (gm_nw.hip)
inline uint32_t gm_qual_lo(const unsigned long long* ctr) { return 255u - (uint32_t)ctr[GMK_QUAL_MIN]; }
inline uint32_t gm_qual_hi(const unsigned long long* ctr) { return (uint32_t)ctr[GMK_QUAL_MAX]; }
// gm_band.hip: the DP kernels for a band half-width other than 3 (-M)
int gmk_nw_band(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, uint32_t n_cands, int G, void* stream);
int gmk_traceback_band(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, const GmCand* items, uint32_t n, unsigned long long* ops,
                       uint32_t ops_words, uint16_t* ops_len, const uint8_t* emit, uint32_t* cig_cnt, uint32_t* max_span, int G, void* stream);
inline uint64_t gm_band_moves_words(uint32_t n, uint32_t stride) {          // at most 512 MB, at least one workgroup's worth of items
    const uint64_t rows = (uint64_t)stride + 1, cap = (512ull << 20) / 8, all = (uint64_t)n * rows;
    return all < cap ? all : (cap > 128 * rows ? cap : 128 * rows);
}
// gm_snp.hip: --snp (SNPScoredSeq): pair HMM per kept sequence + the deposit of its posteriors
size_t gmk_pair_hmm_cells(uint32_t Lmax);            // doubles of scratch per wavefront (64 kept sequences)
int gmk_pair_hmm(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, const GmCand* items, uint32_t n, double* scratch, uint32_t Lmax, float* hmm, void* stream);
int gmk_snp_deposit(float* cov, float* nuc, uint64_t bins, uint32_t bin_size, const GmDevBatch& b, const GmDevMatch* matches, const GmDevPos* positions,
                    uint32_t m0, uint32_t count, const float* post, const float* hmm, uint32_t Lmax, void* stream);
// gm_snpcall.hip: --snp's likelihood-ratio column (PrintSNPCall): code byte + p-value per position of [lo, lo + n), 'Y' rows per workgroup;
// then the 'Y' rows in position order (off: workgroups + 1 words of scratch; off[workgroups] = their number, to be read back by the caller)
uint32_t gmk_snp_call_groups(uint64_t n);
int gmk_snp_call(const float* cov, const float* nuc, uint64_t bins, const GmDevIndex& ix, uint64_t lo, uint64_t n, float snp_pval, int monop, uint8_t* code, double* pval,
                 uint32_t* ycnt, void* stream);
int gmk_snp_gather(const float* cov, const float* nuc, uint64_t bins, const GmDevIndex& ix, uint64_t lo, uint64_t n, const uint8_t* code, const double* pval,
                   const uint32_t* ycnt, unsigned long long* off, unsigned long long base, unsigned long long cap, GmDevSnpRec* out, void* stream);
int gmk_snp_stat(const float* counts, uint32_t n, int monop, double* pval, int8_t* pos1, int8_t* pos2, uint8_t* dip, void* stream);
// gm_tracktext.hip: .sgr / .gmp rows as text (GM_TRACK_CALLS: t.code / t.pval filled by gmk_snp_call for the same bins first).  Sizes + their scan (meta is read back by the caller), then the rows into text[0, meta[TT_META_BYTES])
uint32_t gmk_track_tiles(uint64_t n);
int gmk_track_sizes(const GmDevTrack& t, void* stream);
int gmk_track_rows(const GmDevTrack& t, void* stream);
int gmk_fmt_e2(const double* v, uint32_t n, char* out /* n x 16 */, uint8_t* len, void* stream);      // gm_put_e2_hd per value
int gmk_compact(const GmDevBatch& b, void* stream);
int gmk_scan_hits(const GmDevBatch& b, void* stream);
int gmk_scatter(const GmDevBatch& b, uint32_t grid, void* stream);
int gmk_sa_interval(const GmDevIndex& ix, const uint8_t* kmers, uint32_t n, uint32_t m, uint32_t* start, uint32_t* end, void* stream);
int gmk_locate(const GmDevIndex& ix, const uint32_t* ranks, uint32_t n, int use_full_sa, uint32_t* out, void* stream);
// traceback operations: 2 bits each (0 M, 1 I, 2 D), operation k in 64-bit word k / 32 at bits 2 (k % 32); ops_words words per item
inline uint32_t gm_ops_words(uint32_t stride) { return (2u * ((stride + 7u) & ~7u) + 8u + 31u) / 32u; }
const char* gmk_traceback_form(const GmDevParams& p, const GmDevBatch& b);      // the kernel gmk_traceback launches for this block
int gmk_traceback(const GmDevIndex& ix, const GmDevParams& p, const GmDevBatch& b, const GmCand* items, uint32_t n,
                  unsigned long long* ops, uint32_t ops_words, uint16_t* ops_len, const uint8_t* emit, uint32_t* cig_cnt, uint32_t* max_span, void* stream);
int gmk_scan_u32(const uint32_t* in, uint64_t n, uint64_t* out, unsigned long long* tmp, void* stream);
int gmk_group_count(const GmDevIndex& ix, const GmDevBatch& b, const GmDevGroup& g, int nw, int unique_only, uint32_t max_matches, void* stream);
int gmk_group_write(const GmDevBatch& b, const GmDevGroup& g, void* stream);
int gmk_out_items(const GmDevMatch* matches, uint32_t n_m, uint32_t read_base, GmCand* items, uint32_t* pos_match, void* stream);
int gmk_out_sizes(const GmDevMatch* matches, uint32_t n_m, const uint8_t* emit, const uint32_t* cig_all, uint32_t* rec_cnt, uint32_t* cig_cnt, void* stream);
int gmk_out_write(const GmDevIndex& ix, const GmDevBatch& b, const GmDevMatch* matches, const GmDevPos* positions, uint32_t n_m, const uint8_t* emit,
                  const int32_t* mapq, const float* post, const unsigned long long* ops, uint32_t ops_words, const uint16_t* ops_len, int nw,
                  const uint64_t* rec_off, const uint64_t* cig_off, GmDevSamRec* recs, char* pool, void* stream);
int gmk_out_codes(const GmDevBatch& b, const GmDevParams& p, const GmDevMatch* matches, uint32_t n_m, const unsigned long long* ops, uint32_t ops_words,
                  const uint16_t* ops_len, uint8_t* codes, uint32_t codes_stride, void* stream);
int gmk_out_deposit(float* cov, uint64_t bins, uint32_t bin_size, const GmDevMatch* matches, const GmDevPos* positions, const uint32_t* pos_match,
                    uint64_t n_p, const uint16_t* ops_len, const float* post, uint32_t max_span, float* nuc, const uint8_t* codes, uint32_t codes_stride,
                    void* stream);
// SAM rows as text (gm_output_batch_text): tails + row lengths, then - after the scan of the lengths - the rows themselves
// the row source of a block whose reads without a record get a row too: n reads, n_recs records in read order.  cnt / flag (n words
// each), first / ucum (n + 1 scans: records, and reads without a record, in front of a read), row_src (n_recs + n entries of room).
// ucum[n] = the rows of reads without a record (to be read back by the caller); the rows are n_recs + ucum[n]
int gmk_row_source(const GmDevSamRec* recs, uint64_t n_recs, uint32_t n, uint32_t* cnt, uint32_t* flag, uint64_t* first, uint64_t* ucum, unsigned long long* tmp,
                   unsigned long long* row_src, void* stream);
int gmk_out_text_sizes(const GmDevBatch& b, const GmDevText& t, void* stream);
int gmk_out_text_rows(const GmDevBatch& b, const GmDevText& t, void* stream);
// gm_batch_set_row_tags: behind gmk_out_text_sizes / gmk_bam_sizes and before the scan of row_len.  {NM, MD bytes} of every row into
// t.md, and the bytes the two tags take (SAM text, or bam != 0 BAM) added to row_len
int gmk_md_sizes(const GmDevBatch& b, const GmDevText& t, int bam, void* stream);
int gmk_fmt_g6(const double* v, uint32_t n, char* out /* n x 16 */, uint8_t* len, void* stream);
// gm_mates.hip: gm_batch_set_mates.  resolve: spans, record ranges, primaries and the pair counters (m.meta, zeroed here).  names: the
// QNAME rule - len (n_reads words) and new_off (n_reads + 1) are scratch, `out` takes the cut names (room: the block's own name bytes
// always hold them), cut = the bytes of a name the sink prints; m.meta[MT_META_BAD_PAIR] = the first pair whose printed names differ.
// fields: one GmDevMateRow per row of t (t.recs, t.n_recs, t.n_rows, t.row_src, t.n_reads are read).  row_len: SAM text only, behind
// gmk_out_text_sizes and before the scan - the bytes the flag and the mate columns add to every row
int gmk_mate_resolve(const GmDevMates& m, void* stream);
int gmk_mate_names(const char* names, const uint64_t* name_off, uint32_t n_reads, uint32_t* len, uint64_t* new_off, unsigned long long* tmp, char* out, uint64_t room,
                   uint32_t cut, unsigned long long* meta, void* stream);
int gmk_mate_fields(const GmDevMates& m, const GmDevText& t, GmDevMateRow* out, void* stream);
int gmk_mate_row_len(const GmDevText& t, void* stream);
// gm_adaptor.hip: -A / --adaptor (SeqReader::FixReads2): out_len[r] = the length read r keeps; len = the lengths as uploaded, stride a multiple of 8
int gmk_adaptor_cigar_room(const GmDevMatch* matches, uint32_t n_m, const uint16_t* full_len, uint32_t n, uint32_t* cig_all, void* stream);      // --no_nw with -A: room for "<whole length>M"
int gmk_adaptor_trim(const uint8_t* bases, uint32_t stride, const uint16_t* len, uint32_t n, const uint8_t* adaptor, uint32_t a_len, uint16_t* out_len, void* stream);
// gm_readtext.hip: FASTQ text -> rows.  count: newlines per tile + their scan (meta[RT_META_LINES] is read back by the caller); records: line
// starts, phases, the record table, the block's n / lengths / byte sums (t.n_lines, t.n_ltiles, t.rec_cap set from that read-back)
uint32_t gmk_readtext_tile_bytes();
uint32_t gmk_readtext_tiles(uint64_t bytes);
uint32_t gmk_readtext_line_tiles(uint64_t lines);
int gmk_readtext_count(const GmDevReadText& t, void* stream);
int gmk_readtext_records(const GmDevReadText& t, void* stream);
int gmk_readtext_rows(const GmDevReadText& t, uint32_t n, uint32_t stride, uint8_t* bases, uint8_t* quals, void* stream);
int gmk_readtext_names(const GmDevReadText& t, uint32_t n, char* names, const uint64_t* name_off, char* tails, const uint64_t* tail_off, void* stream);
int gmk_readtext_illumina(const uint8_t* quals, uint32_t stride, const uint16_t* len, uint32_t n, uint32_t* until /* set to n by the caller */, void* stream);
int gmk_coverage_add(float* cov, uint64_t bins, uint32_t bin_size, const uint64_t* pos, const uint32_t* span, const float* w,
                     uint32_t n, uint32_t max_span, float* nuc, const uint8_t* codes, const uint64_t* code_off, void* stream);
}
#endif
