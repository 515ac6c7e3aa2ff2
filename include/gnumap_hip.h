/* gnumap_hip.h — C ABI of libgnumap_hip.so: the MI355X (gfx950) implementation of GNUMAP's per-read
 * seed-and-extend hot path.  Plain C types only; no exceptions cross the boundary; every function
 * returns GM_OK (0) or a negative gm_status.
 *
 * What each entry point replaces in the reference (paths relative to the reference tree):
 *
 *   gm_index_open / gm_index_close   GenomeBwt::LoadGenome            src/GenomeBwt.cpp:282-328
 *                                    bwa_idx_load_from_disk           src/GenomeBwt.cpp:112-140
 *                                    (bwt_restore_bwt/_sa src/bwt.c:421-461, bns_restore src/bntseq.c:169)
 *   gm_index_build                   GenomeBwt::index_and_store       src/GenomeBwt.cpp:330-339 -> bwa_index src/bwtindex.c:187
 *   gm_params_default/_finalize      globals inc/const_define.h:29-131, setup_alignment_matrices inc/a_matrices.c:25,
 *                                    -b/-d table edits src/Driver.cpp:1260-1313, jump default src/Driver.cpp:1206
 *   gm_map_batch                     the per-thread block loop over set_top_matches   src/Driver.cpp:2344-2356
 *                                    = set_top_matches src/Driver.cpp:432-612, align_sequence/process_hits
 *                                    inc/align_seq2_raw.cpp:22-328, Genome::get_sa_int/get_sa_coord/GetString
 *                                    inc/Genome.h:88,98,99, bin_seq::get_align_score inc/bin_seq.h:133
 *   gm_output_batch                  the block loop over create_match_output          src/Driver.cpp:2360-2373
 *                                    = create_match_output src/Driver.cpp:614-753, NormalScoredSeq::score
 *                                    src/NormalScoredSeq.cpp:24-76, ScoredSeq::get_SAM inc/ScoredSeq.h:293-404,
 *                                    bin_seq::get_align_score_w_traceback inc/bin_seq.h:175, GenomeBwt::AddScore
 *                                    src/GenomeBwt.cpp:483-490
 *   gm_output_batch_text             the same block loop, ending in the SAM rows as text: the print loop of
 *                                    parallel_thread_run src/Driver.cpp:2146-2217, ScoredSeq::get_SAM inc/ScoredSeq.h:293-404,
 *                                    reverse_comp / reverse_CIGAR inc/SequenceOperations.h:56-123
 *   gm_batch_upload_text             SeqReader::get_more_fastq src/SeqReader.cpp:1023-1292 for a byte range of well-formed records
 *                                    (gm_map_batch_text / gm_output_batch_text_resident: the two calls above for that block)
 *   gm_batch_set_adaptor             -A: SeqReader::FixReads2 / Compare           src/SeqReader.cpp:1146-1150, 1294-1305, 1356-1372
 *   gm_coverage_*                    amount_genome, PrintFinalSGR src/GenomeBwt.cpp:1212-1273; the MPI
 *                                    Allreduce of the track src/Driver.cpp:1660-1672 (-> RCCL)
 *
 * Threading: one gm_index per device; a gm_batch is used by one host thread at a time; different
 * batches of the same index may be driven concurrently from different host threads / HIP streams
 * (the index is read-only; coverage deposits are float atomics, like the reference's mutex-ordered adds).
 */
#ifndef GNUMAP_HIP_H
#define GNUMAP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GM_OK = 0,
    GM_E_ARG = -1,          /* bad argument */
    GM_E_IO = -2,           /* index / file problem (reference: throw new Exception / err_fatal) */
    GM_E_NO_DEVICE = -3,    /* no usable HIP device or the gfx950 code object cannot be loaded */
    GM_E_HIP = -4,          /* a HIP call failed: gm_last_error() has the text */
    GM_E_CAPACITY = -5,     /* caller-provided output buffers too small: required sizes are written back */
    GM_E_UNSUPPORTED = -6,  /* e.g. reference longer than 2^32-2 bases (the reference's own `unsigned int vit`
                               loop, inc/align_seq2_raw.cpp:262, has the same limit) */
    GM_E_NOMEM = -7,
    GM_E_BAD_QUAL = -8,     /* negative base probability: reference throws "Invalid Fastq Character", SeqReader.cpp:1181-1189 */
    GM_E_BATCH_TOO_LARGE = -9   /* the block's intermediate lists (candidates, SA hits of one read) exceed what one launch addresses:
                                   map the block in smaller pieces (a repeat-rich reference without -h can yield > 2^31 candidates) */
} gm_status;

/* per-read status, the reference's sentinel values (inc/const_include.h:183-186) */
enum { GM_READ_OK = 0, GM_READ_TOO_MANY = 1, GM_READ_NONE = 2, GM_READ_TOO_SHORT = -2, GM_READ_TOO_POOR = -3 };
enum { GM_MODE_NORMAL = 0, GM_MODE_BS = 1, GM_MODE_BS2 = 2, GM_MODE_ATOG = 3, GM_MODE_ATOG2 = 4,
       GM_MODE_SNP = 5 /* --snp: SNPScoredSeq (src/SNPScoredSeq.cpp:25-109) - mapping as GM_MODE_NORMAL; gm_output_batch deposits the pair-HMM
                          posteriors of every kept sequence into the five per-nucleotide tracks (bin size 1, gm_coverage_enable_nuc first) */ };
enum { GM_POS_STRAND = 0, GM_NEG_STRAND = 1 };

/* gm_index_open flags */
enum {
    GM_INDEX_FULL_SA = 1,       /* expand the rank-sampled SA to a full 32-bit SA in HBM once (locate = one 4-byte read) */
    GM_INDEX_BUILD = 2,         /* build <fa>.gnumap.* when missing, like GenomeBwt::LoadGenome */
    GM_INDEX_HOST_ONLY = 4      /* no device: header/contig queries and gm_index_build only (CPU-side tests) */
};

typedef struct gm_index gm_index;
typedef struct gm_batch gm_batch;

typedef struct {
    uint64_t l_pac, seq_len, primary, bwt_words, n_sa;
    uint32_t sa_intv, n_seqs;
    int device_id, full_sa;
    uint64_t hbm_bytes;         /* device bytes held by the index */
} gm_index_info;

/* mirrors the globals of inc/const_define.h; fill with gm_params_default, edit, then gm_params_finalize */
typedef struct {
    int mer;                    /* -m  gMER_SIZE (10) */
    int jump;                   /* -j  gJUMP_SIZE (0 -> mer/2) */
    int min_seed_hits;          /* -k  gMIN_JUMP_MATCHES (2) */
    uint32_t max_kmer_hits;     /* -h  gMAX_KMER_SIZE (0 = unlimited) */
    uint32_t max_matches;       /* -T  gMAX_MATCHES (1000) */
    int max_gap;                /* -M  gMAX_GAP (3); 1 .. 7 (3 runs the register-band kernels, the rest the LDS-band kernels of gm_band.hip) */
    int nw;                     /* !--no_nw */
    int fast;                   /* --fast */
    int unique_only;            /* -u */
    int pos_strand, neg_strand; /* --up_strand / --down_strand */
    int mode;                   /* GM_MODE_* (-b, --b2, -d, --snp) */
    float align_score;          /* -a  gALIGN_SCORE (0.9) */
    int align_is_fraction;      /* perc (1); 0 with -r */
    float cutoff;               /* -q  gCUTOFF_SCORE (0) */
    float adjust, match, transition, transversion, gap;     /* gADJUST .25, 3, -2, -3, -4 (scaled by finalize) */
    float S[256][4];            /* gALIGN_SCORES, built by finalize */
    int bin_size;               /* --bin_size gGEN_SIZE (8; forced to 1 by -b/-d) */
    int print_all_sam;          /* --print_all_sam */
    int illumina;               /* --illumina (Phred+64 with automatic fallback, SeqReader.cpp:1171-1180) */
    int finalized;
} gm_params;

/* a block of reads exactly as they stand in the FASTQ (or, gm_batch_set_read_format, FASTA) file; caller-owned host memory */
typedef struct {
    uint32_t n;                 /* number of reads */
    uint32_t stride;            /* bytes between consecutive reads in bases[] / quals[] (>= longest read, multiple of 8) */
    const uint8_t* bases;       /* n x stride, FASTQ sequence characters verbatim (any case, N allowed); FASTA: the sequence lines of a
                                   record joined, the 15 IUPAC letters in either case */
    const uint8_t* quals;       /* n x stride, raw FASTQ quality characters; not read for a FASTA block (may be NULL) */
    const uint16_t* len;        /* n read lengths */
} gm_reads;

typedef struct { uint64_t pos; uint8_t strand; } gm_pos;

/* one ScoredSeq (inc/ScoredSeq.h:33): a unique genomic sequence the read matched, with all its places */
typedef struct {
    uint32_t read;              /* index of the read in the batch */
    float score;                /* align_score of the FIRST hit (fp32 NW score, or the vote count with --no_nw) */
    uint64_t first_pos;         /* position whose window is ScoredSeq::sequence */
    uint8_t first_strand;       /* ScoredSeq::firstStrand */
    uint32_t pos_begin, pos_end;/* [pos_begin,pos_end) in positions[]: the ordered set<(pos,strand)> */
} gm_match;

/* result of gm_map_batch: what set_top_matches leaves in gReadLocs / gReadDenominator / gTopReadScore.
 * All arrays are caller-owned; on GM_E_CAPACITY matches_cap / positions_cap hold the required sizes. */
typedef struct {
    uint32_t n;
    int8_t* status;             /* n: GM_READ_* */
    float* self_score;          /* n: max_align_score (Driver.cpp:466) */
    double* top_score;          /* n: gTopReadScore */
    double* denominator;        /* n: gReadDenominator */
    uint64_t* match_begin;      /* n+1: CSR into matches[], matches of a read in std::map (key) order */
    gm_match* matches;  uint64_t matches_cap;
    gm_pos* positions;  uint64_t positions_cap;
    uint64_t stamp;             /* set by gm_map_batch: names the result that is still resident in the batch's HBM.  gm_output_batch given the
                                   same stamp uses the resident matches / positions as they are (no upload, no re-validation); a caller
                                   that EDITS matches / positions / match_begin sets stamp = 0 (status, denominator and top_score are always
                                   taken from the host arrays).  A gm_hits the caller builds by hand must be ZERO-INITIALISED (stamp = 0 =
                                   "nothing resident"); gm_map_batch sets it to 0 first thing on every call (ABI 0.2) */
} gm_hits;

/* one SAM record (TopReadOutput, inc/const_include.h:193-206) */
typedef struct {
    uint32_t read;
    uint64_t pos;               /* 0-based position on the concatenated reference */
    uint32_t contig;            /* index into the contig table */
    uint64_t chr_pos;           /* 1-based position on the contig */
    uint8_t strand;
    int32_t mapq;
    float a_score;              /* XA before the 1/gADJUST rescale */
    float post_prob;            /* XP */
    int32_t sim_matches;        /* X0 */
    uint32_t cigar_off;         /* offset of the NUL-terminated CIGAR (forward orientation) in cigar_pool */
} gm_sam_rec;

typedef struct {
    gm_sam_rec* recs;  uint64_t recs_cap, n_recs;        /* caller-owned; in read order, then ScoredSeq position order */
    char* cigar_pool;  uint64_t cigar_cap, cigar_len;    /* caller-owned */
} gm_sam_out;

/* what a SAM row prints of a read besides its bases and qualities */
typedef struct {
    const char* names;              /* the names back to back, no terminators: exactly the bytes after '@' */
    const uint64_t* name_off;       /* n+1 offsets into names */
    const char* qual_tail;          /* NULL, or: bytes the row prints after the len[i] quality characters of read i (a quality
                                       line longer than its sequence line, SeqReader.cpp:1091) */
    const uint64_t* qual_tail_off;  /* n+1, NULL with qual_tail */
} gm_read_text;

/* finished SAM rows, one '\n'-terminated line per record, in gm_output_batch's record order */
typedef struct {
    char* text;  uint64_t text_cap, text_len;   /* caller-owned (page-locked for link rate) */
    uint64_t n_recs;
    uint64_t* row_off;  uint64_t row_cap;       /* optional (NULL / 0): n_recs+1 row offsets */
} gm_sam_text;

/* kernel-side work counters of the last gm_map_batch on a batch (algorithmic-bytes accounting) */
typedef struct {
    uint64_t reads, kmers_searched, occ_calls, occ_blocks, seeds_used, sa_hits, lf_steps, candidates, nw_cells, accepted, vote_retries,
        table_lookups;
} gm_counters;

/* kernels of gm_map_batch_device, for the HIP-event timing of gm_batch_kernel_times.  GM_K_SEED has no launches when the seed
 * lookup runs inside the vote kernel (full SA, k-mer table as long as the seed, k-mers expected >= 4 times in the reference, no -h;
 * env GM_SEED_FUSED=0|1 overrides): its time is then part of GM_K_VOTE; the work counters are the same either way.
 * GM_K_MD_SIZES belongs to the row-producing output calls: the sizes pass of gm_batch_set_row_tags (no launches with the setting off).
 * GM_K_MATES belongs to every output call: the k_mate_* kernels of gm_batch_set_mates (no launches with the setting off) */
enum { GM_K_PREP = 0, GM_K_SEED, GM_K_LOCATE, GM_K_VOTE, GM_K_VOTE_RETRY, GM_K_NW, GM_K_COMPACT, GM_K_MD_SIZES, GM_K_MATES, GM_K_COUNT };

const char* gm_last_error(void);
const char* gm_version(void);
/* run-time switches of the library (the GM_* names documented in DESIGN.md: kernel choices, test switches).  Every switch is read
 * on each call that uses it - from this table first, then from the environment - so a long-lived host can change a choice
 * between two batches.  value = NULL removes the override (back to the environment); "" hides an environment variable. */
int gm_set_option(const char* name, const char* value);

/* host-only self test of the library's slice pool (the fp64 passes of the two batch calls are cut over it): `callers` threads run
 * `iters` passes over [0, n) each, at once; returns the number of passes in which an item was not visited exactly once (0 = fine) */
int gm_selftest_pass_parallel(uint32_t n, uint32_t grain, uint32_t callers, uint32_t iters);

/* ---- index ---- */
int gm_index_build(const char* fasta_path);                      /* writes <fa>.gnumap.{pac,ann,amb,bwt,sa}; = gm_index_build_on(fa, GM_BUILD_AUTO, 0) */
/* where the suffix-array stage of the build runs (is_sa/is_bwt src/is.c:53-223): the files are byte-identical either way */
enum { GM_BUILD_AUTO = 0 /* device if there is one, else host; env GM_INDEX_BUILD=host|device */, GM_BUILD_HOST = 1 /* SA-IS */,
       GM_BUILD_DEVICE = 2 /* prefix doubling in HBM, gm_sa_build.hip */ };
int gm_index_build_on(const char* fasta_path, int where, int device_id);
int gm_index_open(const char* fasta_path, int device_id, int flags, gm_index** out);
void gm_index_close(gm_index*);
/* stage what the mapping kernels derive from the index for these parameters (k-mer tables, k-mer -> positions records: tens of GB of HBM
 * at human scale, built on the device in well under a second) now instead of inside the first gm_map_batch; optional */
int gm_index_prepare(gm_index*, const gm_params*);
int gm_index_get_info(const gm_index*, gm_index_info* out);
const char* gm_index_contig_name(const gm_index*, uint32_t i);
uint64_t gm_index_contig_offset(const gm_index*, uint32_t i);   /* i == n_seqs gives l_pac */
/* window fetch on the host copy of the packed reference (GenomeBwt::GetString); returns L or 0 at a boundary */
int gm_index_window(const gm_index*, uint64_t begin, uint32_t L, char* out);

/* ---- parameters ---- */
void gm_params_default(gm_params*);
int gm_params_finalize(gm_params*);
/* -S / --subst_file (readPWM, src/Driver.cpp:768-859; call AFTER gm_params_finalize): 5 rows (genome a, c, g, t, n) x 4 read bases,
 * with or without the label line / row labels; overwrites the LOWERCASE rows of S unscaled, sets adjust = 1 (XA is then printed
 * unscaled) and leaves the gap penalty as finalize scaled it - exactly what the reference does. */
int gm_params_load_subst(gm_params*, const char* path);

/* ---- batches: device-resident reads + workspace + raw results ---- */
int gm_batch_create(gm_index*, uint32_t max_reads /* <= 16 000 000 */, uint32_t max_len /* <= 2048 */, gm_batch** out);
void gm_batch_destroy(gm_batch*);
/* host -> HBM.  Of gm_params an upload (gm_batch_upload, gm_batch_upload_text) BINDS one field, `illumina`: the --illumina fallback
 * scan (the first read that shows a quality below '@') reads the quality rows while they are uploaded, and the block stays resident
 * with its outcome.  gm_map_batch_device / gm_map_batch_text with the other value of `illumina` on a FASTQ block return GM_E_ARG
 * (gm_last_error() names the field); a FASTA block ignores the field in both calls.  Every other field - mer, jump and the rest - is read
 * from the map call's own gm_params: the upload's values of them only pre-size workspace, which the map call sizes again where they differ. */
int gm_batch_upload(gm_batch*, const gm_params*, const gm_reads*, void* hip_stream);
/* -A / --adaptor: trim adaptor sequence from the 3' end of every read of the blocks uploaded from now on.  Replaces the
 * `if(g_adaptor) J=FixReads2(sequence)` of SeqReader::get_more_fastq (src/SeqReader.cpp:1146-1150) with FixReads2 (:1356-1372) and
 * Compare (:1294-1305), as one device kernel (k_adaptor_trim) behind the copies of gm_batch_upload / gm_map_batch: a read keeps its
 * first J characters, J = the smallest offset in [0, len - 4) where `(float)same / compared >= 0.85f` over min(|adaptor|, len - offset)
 * raw, case-sensitive characters, or len - 4 when there is none (a read without any adaptor loses four bases: FixReads2 has no
 * gMIN_CHOPPED_BASES guard).  Status, self score, -q, seeds, DP, CIGAR, coverage and the --illumina fallback scan see J characters;
 * SEQ and QUAL of a SAM row stay the whole lines (:1264-1265): gm_output_batch_text prints gm_reads.len characters.  The string is
 * used exactly as given (Driver.cpp:2793-2798), at most 256 characters (GM_E_ARG beyond); NULL or "" clears it.  Departure, where
 * the reference's unsigned bound wraps: a read of fewer than 4 bases keeps 0.  Cost: one launch and one small read-back per upload,
 * only while an adaptor is set. */
int gm_batch_set_adaptor(gm_batch*, const char* adaptor);
/* The read file's format, as SeqReader::find_type (src/SeqReader.cpp:175-244) tells it from the first byte: '@' FASTQ, '>' FASTA (the
 * reference's _prb.txt / _int.txt formats are not built).  Holds for the blocks uploaded from now on - gm_batch_upload, gm_map_batch(_device /
 * _enqueue) - and for what gm_output_batch(_text / _enqueue) does with them.  A FASTA block is its letters only: gm_reads.quals is not
 * read and not copied (half the upload).  A position's PWM row is get_more_fasta's (src/SeqReader.cpp:875-979, cast to float at :996):
 * a c g t one 1.0; r y k m s w two 0.5; b d h v three (float)(1.0 / 3.0); n four 0.25; everything else 0.0 - on the device a 4-bit base mask
 * with an in-mask and an out-of-mask probability, the mask's bits reversed for reverse_comp_cpy's row on the minus strand, every value
 * ((r0 s0 + r1 s1) + r2 s2) + r3 s3 in fp32 like bin_seq::get_val.  The self score takes S's row of the RAW character (Read::seq is the
 * file's text, GetConsensus Driver.cpp:352-364: 'K' and 'k' are different rows).  Every letter outside ACGTacgt ends a seed k-mer like
 * N.  SEQ of a row is the letters (reverse_comp on the minus strand: every letter outside ACGTacgt becomes 'n'), QUAL is str2qual's
 * string (inc/SequenceOperations.h:193-217), one character per position from the row's largest entry.  gm_params.illumina is ignored.
 * The caller checks the letters: a byte that is none of the 15 gives an all-zero row.  gm_output_batch_text: gm_read_text.qual_tail must be
 * NULL for a FASTA block (GM_E_ARG otherwise): there is no quality line a tail could come from.
 * GM_E_UNSUPPORTED for a FASTA block with an adaptor set (the reference's FixReads for FASTA is a different, PWM-based trim), with
 * GM_MODE_SNP, or with the switch that forces the one kernel form which takes FASTQ only (GM_NW=wave, the DP score kernel k_nw):
 * gm_last_error() names it. */
enum { GM_READS_FASTQ = 0, GM_READS_FASTA = 1 };
int gm_batch_set_read_format(gm_batch*, int format);
/* the lengths the kernels used for the block uploaded last (Read::length = J, SeqReader.cpp:1260): n values; gm_reads.len without an adaptor */
int gm_batch_trimmed_len(gm_batch*, uint16_t* out);
/* device time of k_adaptor_trim since the last call, measured with HIP events while gm_batch_set_profiling is on (it is not one of
 * the GM_K_* kernels of gm_map_batch_device: it runs inside the upload) */
int gm_batch_adaptor_time(gm_batch*, double* ms, uint64_t* launches);
/* the hot path proper, everything resident in HBM: prep -> seed -> locate+vote -> NW -> hit compaction.
 * Asynchronous on hip_stream except for one 16-byte size read-back used to size the workspace. */
int gm_map_batch_device(gm_index*, const gm_params*, gm_batch*, void* hip_stream);
int gm_batch_counters(gm_batch*, gm_counters* out);
/* per-kernel device time: HIP events recorded on the launch stream around every kernel of gm_map_batch_device while
 * profiling is on; gm_batch_kernel_times adds up what has completed since the last call (ms and launch counts) */
int gm_batch_set_profiling(gm_batch*, int on);
int gm_batch_kernel_times(gm_batch*, double* ms /* GM_K_COUNT */, uint64_t* launches /* GM_K_COUNT */);
const char* gm_kernel_name(int which);
/* the block's read format and which seed lookup / vote kernel / locate form / DP kernel the last gm_map_batch_device on this batch chose,
 * e.g. "reads=fastq seeds=bucket-table (in the vote kernel) vote=k_vote_bucket<4> locate=full-SA nw=k_nw_rows/pairs" (valid until the
 * next call on the batch).  "" after a call that the sub-batch pipeline (GM_PIPELINE) mapped to the end; an empty block names no kernel */
const char* gm_batch_path(gm_batch*);
/* reads that k_vote_pair left to k_vote_bucket in the last gm_map_batch_device on this batch (a k-mer that does not occur or has more
 * than 28 hits, an early position, a base that is not ACGT, too many hits or second arrivals in a strand); 0 when k_vote_pair did not run */
int gm_batch_pair_flagged(gm_batch*, uint32_t* flagged);
/* raw device results (accepted candidates), for tests and for callers that post-process themselves */
typedef struct { uint32_t read; uint32_t pos; float score; uint16_t step; uint8_t strand; uint8_t pad; } gm_raw_hit;
int gm_batch_raw_hits(gm_batch*, gm_raw_hit* out, uint64_t cap, uint64_t* n_out,
                      int8_t* status, float* self_score, float* top_score);

/* ---- the drop-in pair for the two block loops of parallel_thread_run ----
 * gm_map_batch   = upload + gm_map_batch_device + the unique-sequence map of process_hits as device kernels (processing order, key
 *                  grouping on the 2-bit reference, std::map order, -T / -u exits); the host does one flat fp64 pass
 *                  (denominator += exp(score) in the reference's order) on the calling thread.
 * gm_output_batch= one flat fp64 pass on the calling thread (posterior, winner, MAPQ), then traceback, run-length CIGAR text,
 *                  SAM rows and the coverage deposit as device kernels.  `reads` must be the block the batch was mapped with (it
 *                  is still resident in HBM); `hits` may have been edited by the caller (it is uploaded again).
 * Both are synchronous on hip_stream and use only the calling thread: a driver overlaps blocks by calling them from two or more
 * threads with one gm_batch and one stream each.  Host buffers from gm_host_alloc are page-locked (DMA at link rate). */
int gm_stream_create(gm_index*, void** hip_stream_out);          /* a non-blocking HIP stream on the index's device (one per driver thread) */
void gm_stream_destroy(gm_index*, void* hip_stream);
void* gm_host_alloc(size_t bytes);                               /* page-locked host memory for gm_reads / gm_hits / gm_sam_out buffers */
void gm_host_free(void*);
int gm_map_batch(gm_index*, const gm_params*, gm_batch*, const gm_reads*, gm_hits* out, void* hip_stream);
int gm_output_batch(gm_index*, const gm_params*, gm_batch*, const gm_reads*, const gm_hits*, gm_sam_out* out, void* hip_stream);

/* gm_output_batch with a different ending: same host fp64 pass, same traceback, same coverage / per-nucleotide / SNP deposit - call
 * one or the other for a block, never both - then the rows are formatted on the device (name cut to 1023 bytes, flag 0 / 16, contig,
 * position, MAPQ, CIGAR - reversed token by token on the minus strand -, reverse-complemented sequence, reversed qualities, exact
 * "%g" of XA / XP, X0) and come back as ONE buffer a host can fwrite: byte for byte what the reference program prints for these
 * records.  GM_E_CAPACITY: text_cap (and row_cap) hold the required sizes and NOTHING has been deposited yet - repeat the call.
 * GM_E_ARG: gm_read_text NULL or its offsets do not ascend.  GM_E_UNSUPPORTED: an XA / XP outside 2^-200 <= |v| < 2^200 (not reachable
 * with finite fp32 scores and the reference's adjust values); gm_last_error() names the record.  There is no enqueue form. */
int gm_output_batch_text(gm_index*, const gm_params*, gm_batch*, const gm_reads*, const gm_read_text*, const gm_hits*, gm_sam_text* out,
                         void* hip_stream);

/* ---- rows for the reads that do not map (a defined extension: the reference prints none) ----
 * Off by default: a read without a record has no row.  gm_batch_set_unmapped_rows(b, 1): from the next call on, the six row-producing
 * output calls (gm_output_batch_text, _text_resident, _sorted, _sorted_resident, _bam, _bam_resident) give every read of the block for
 * which they write no record - status GM_READ_NONE, _TOO_MANY, _TOO_SHORT, _TOO_POOR, or GM_READ_OK with nothing printed - exactly
 * one row.  The block's rows ascend by read index: a read's records keep their order and their bytes, such a read's row stands where
 * its records would.  SAM text:
 *     name \t 4 \t * \t 0 \t 0 \t * \t * \t 0 \t 0 \t SEQ \t QUAL \t YU:i:<gm_hits.status of the read> \n
 * with the name cut to 1023 bytes and SEQ / QUAL as a plus-strand row prints them (the bases as uploaded, whole even with an adaptor
 * set; the quality line with its tail; str2qual's string for a FASTA block); a read of length 0 - gm_batch_upload takes one, its status
 * is GM_READ_TOO_SHORT - prints "*" for both.  BAM: refID -1, pos -1, bin 4680, MAPQ 0, flag 4, no CIGAR operation, next refID -1, next
 * pos -1, tlen 0, the name cut to 254 bytes, l_seq / SEQ / QUAL as for a plus-strand record, one tag YU of type i.  In the sorter such a
 * row has the key of a row without a contig: it sorts behind every contig, and among themselves these rows keep input order.
 * gm_sam_text.n_recs / row_off, gm_bam_out.n_recs and the sorter's row count then count ROWS; the capacity-first contract holds with
 * sizes that include these rows.  A block in which nothing matched gives n rows (and no traceback, posterior pass or deposit); such a
 * read deposits nothing anywhere.  gm_output_batch (the records form) does not read the setting: its records are the same either way.
 * gm_batch_unmapped_rows: how many such rows the last row-producing output call on the batch wrote (0 with the setting off). */
int gm_batch_set_unmapped_rows(gm_batch*, int on);
int gm_batch_unmapped_rows(gm_batch*, uint64_t* n);

/* ---- NM:i and MD:Z on the rows, and CIGARs in reference order (two defined extensions) ----
 * Both are per-batch settings, off by default, read by the six row-producing output calls from the next call on; gm_output_batch
 * (the records form) reads neither.  With both at their defaults no byte and no launch changes.
 *
 * gm_batch_set_cigar_order(b, GM_CIGAR_FORWARD): a minus-strand row writes its CIGAR field exactly as a plus-strand row writes the
 * same pool entry - all its bytes in pool order; in BAM operation k goes to slot k.  GM_CIGAR_GNUMAP (the default) prints the tokens
 * last to first, as the reference program does - beside a SEQ that is already reverse-complemented, at a POS in forward coordinates,
 * which is the wrong way round for every row with an indel (the traceback ran against the forward window).  Reference length and bin
 * do not depend on the order.  Any other value: GM_E_ARG.
 *
 * gm_batch_set_row_tags(b, GM_ROW_TAG_MD): every row that prints a record whose CIGAR field is not "*" gains, behind X0,
 *     SAM text  \t NM:i:<nm> \t MD:Z:<md>            BAM  NM i <int32>, MD Z <md> NUL   (block_size includes them)
 * A row with CIGAR "*" and the row of a read without a record keep their bytes.  The tags describe THE ROW AS PRINTED - what
 * `samtools calmd` derives from the row's POS, CIGAR field, SEQ and the reference - so they agree with whichever CIGAR order is set:
 *     x = POS-1; z = 0; u = 0; nm = 0; md = ""
 *     for every token (n, op) of the CIGAR field as printed (n = 0 contributes nothing):
 *       M: n times: if z >= len(SEQ) or x >= len(contig): the walk ends
 *                   if code(SEQ[z]) == code(T[x]) and that code != 15: u += 1     else: md += str(u) + T[x]; u = 0; nm += 1
 *                   x += 1; z += 1
 *       I: z += n; nm += n
 *       D: md += str(u) + "^"; u = 0; nm += n; then n times, while x < len(contig): md += T[x]; x += 1
 *     md += str(u)
 * T is the contig's text in upper case: the pac letter, or inside a hole of <fa>.gnumap.amb that hole's character; code() is the BAM
 * nibble of a character ("=ACMGRSVTWYHKDBN", either case, anything else 15) - so an N on either side is a mismatch and the IUPAC letters
 * of a FASTA block compare by nibble.  Any bit but GM_ROW_TAG_MD: GM_E_ARG.  GM_E_UNSUPPORTED: the batch has an adaptor set (SEQ is then
 * the whole read and the CIGAR covers the kept part; gm_batch_set_adaptor refuses likewise while the tags are on).  GM_E_IO: the index
 * was opened without a <fa>.gnumap.amb that can be read and parsed; gm_last_error() names the file. */
#define GM_ROW_TAG_MD 1u
enum { GM_CIGAR_GNUMAP = 0, GM_CIGAR_FORWARD = 1 };
int gm_batch_set_row_tags(gm_batch*, uint32_t tags);
int gm_batch_set_cigar_order(gm_batch*, int order);

/* ---- paired-end reads: mate choice and mate fields on the device (a defined extension: the reference has no paired mode; gm_mates.hip) ----
 * gm_batch_set_mates(b, 1, min_insert, max_insert): a per-batch setting, off by default, sticky, read by ALL SEVEN output calls from
 * the next call on (the records form runs the step too, so that gm_batch_mate_rows has something to return).  With it off no byte and
 * no launch changes.  The map step is not touched: each mate is mapped exactly as a single read.  With it on, reads 2i and 2i + 1 of
 * a block are the first and the second mate of pair i, and the rule below is a function of the block's records alone - gm_sam_rec in
 * record order, and the CIGAR pool.  GM_E_ARG at the output call for an odd n and for min_insert > max_insert.
 *
 * Span: the sum of the M and D runs of a record's CIGAR in the pool; 1 where that is 0 - "*" (the .bai's rule).  END = chr_pos + span - 1.
 * Concordant: a record a of one mate and a record b of the other lie on one contig, their strands differ, and with f the plus-strand
 *   record and r the minus-strand one  POS_f <= POS_r  and  min_insert <= END_r - POS_f + 1 <= max_insert  (forward/reverse layout
 *   only, both limits inclusive).
 * Primaries: if any concordant combination exists, the one with the largest a.post_prob * b.post_prob (ONE fp32 multiply), ties to
 *   the smallest record index of the first mate, then of the second: those two records are the primaries and the pair is PROPER.
 *   Otherwise each mate's primary is its record with the largest post_prob, the first one on ties.  A read without a record has none.
 *   NaN: a NaN post_prob, and a NaN product, ranks below every number (a zero or a negative one included), and two NaNs rank alike.
 *   So among records that are all NaN the first one is the primary, a NaN never displaces a number whichever comes first, and a
 *   pair whose concordant combinations all have NaN products is still PROPER, with the first of them in (first mate, second mate)
 *   order.  Being concordant does not look at post_prob at all.
 * Rows of a mapped read: flag = 0x1 | 0x40 (first mate) or 0x80 (second) | 0x10 (this row is on the minus strand) | 0x20 (the mate's
 *   primary is on the minus strand) | 0x8 (the mate has no primary) | 0x2 (on the two primaries of a proper pair, and only there) |
 *   0x100 (every row that is not its read's primary).  RNEXT "=" when the mate's primary is on this row's contig, else that contig's
 *   name, "*" without a mate primary; PNEXT the mate primary's POS, or 0.  TLEN on primary rows whose mate's primary is on the same
 *   contig: max(END) - min(POS) + 1, positive on the row with the smaller POS, negative on the other, on equal POS positive on the
 *   first mate; 0 in every other case (secondary rows, another contig, no mate primary, a value beyond 2^31 - 1).
 * Rows of a read without a record (only with gm_batch_set_unmapped_rows): RNAME "*" and POS 0 stay; flag 0x4 | 0x1 | 0x40 / 0x80,
 *   plus 0x20 / 0x8 as above; RNEXT the mate primary's contig name or "*", PNEXT its POS or 0, TLEN 0; YU stays.
 * QNAME: the name is cut at its first space or tab; then, if the first mate's name ends in "/1" and the second's in "/2", those two
 *   bytes are dropped from both; the cuts to 1023 (text) / 254 (BAM) bytes apply after that.  If the two printed names of a pair
 *   differ the output call fails with GM_E_ARG and gm_last_error() names the first such pair by index (nothing is deposited).  The
 *   records form has no names and checks none.
 * BAM: flag, next_refID (the contig index, this record's own for "=", -1 for "*"), next_pos = PNEXT - 1 and tlen from the same
 *   fields; bin, refID and pos stay as they are; NM / MD follow as without mates.
 *
 * gm_batch_mate_rows: the fields of the last output call on the batch, one entry per row that call produced, in row order (with
 * gm_batch_set_unmapped_rows that order includes the rows of reads without a record; for gm_output_batch: one per record).
 * *n = the number of rows; GM_E_CAPACITY when that exceeds cap (nothing is written).  0 rows with the setting off.
 * gm_batch_mate_stats: the pair counters of the last output call. */
typedef struct {
    uint32_t flag;
    int32_t rnext;              /* contig index of the mate's primary; -1: none ("*").  "=" is rnext == the row's own contig */
    uint32_t pnext;             /* 1-based POS of the mate's primary; 0: none (its low 32 bits: a contig is shorter than 2^32) */
    int32_t tlen;
} gm_mate_row;
typedef struct { uint64_t pairs, both_mapped, proper, one_mapped, none_mapped; } gm_mate_stats;
int gm_batch_set_mates(gm_batch*, int on, uint32_t min_insert, uint32_t max_insert);
int gm_batch_mate_rows(gm_batch*, gm_mate_row* out, uint64_t cap, uint64_t* n);
int gm_batch_mate_stats(gm_batch*, gm_mate_stats* out);

/* ---- FASTQ text in: the reads cut into rows on the device ----
 * gm_batch_upload_text takes a byte range of FASTQ text as it stands in the file, uploads it verbatim and leaves the batch resident
 * exactly as gm_batch_upload would have with the rows a host had cut from it (n, stride, lengths, adaptor trim, --illumina fallback
 * index).  The rule is the chunk mode of the driver's parser: a line starts at 0 and behind every '\n' that is not the last byte; blank
 * lines are skipped before a name line only; a record is well-formed when its four lines exist, the name starts with '@', the plus
 * line is non-empty and starts with '+' and the sequence is no longer than the quality line.  The first record that is not (status
 * GM_TEXT_MALFORMED), or is but has more than 2048 bases (GM_TEXT_TOO_LONG), ends the block: n counts the records before it and bad_at
 * is the offset of its name line.  stride = max(8, max_len rounded up to 8). */
enum { GM_TEXT_OK = 0, GM_TEXT_MALFORMED = 1, GM_TEXT_TOO_LONG = 2 };
typedef struct {
    uint32_t n, max_len, stride;
    int32_t status;             /* GM_TEXT_* */
    uint64_t bad_at;            /* with a status other than GM_TEXT_OK */
} gm_text_info;
/* one read: offsets from the start of the text, lengths in bytes; the name without its '@' and uncut */
typedef struct { uint32_t name_off, seq_off, qual_off, name_len, seq_len, qual_len; } gm_text_rec;
/* recs: NULL, or room for recs_cap records; GM_E_CAPACITY (info->n = the number needed, nothing left resident) when n exceeds it.
 * GM_E_UNSUPPORTED for a batch set to GM_READS_FASTA.  GM_E_ARG, nothing left resident, for bytes >= 2^32 and for more records than
 * gm_batch_create's max_reads: gm_last_error() says which.  bytes == 0: n = 0.  `text` is read until the call returns (page-locked
 * memory from gm_host_alloc is copied at link rate).  Synchronous on hip_stream; there is no enqueue form. */
int gm_batch_upload_text(gm_batch*, const gm_params*, const char* text, uint64_t bytes, gm_text_info* info, gm_text_rec* recs, uint64_t recs_cap,
                         void* hip_stream);
/* gm_map_batch for the block gm_batch_upload_text left resident: everything behind the upload, GM_E_CAPACITY resume included (repeat
 * the call with larger buffers).  GM_E_ARG when the batch holds no such block. */
int gm_map_batch_text(gm_index*, const gm_params*, gm_batch*, gm_hits* out, void* hip_stream);
/* gm_output_batch_text for that block: names and quality tails are the ones the parse left in HBM.  Same capacity-first contract.
 * (gm_output_batch works on such a block too, with a gm_reads that carries its n and stride.) */
int gm_output_batch_text_resident(gm_index*, const gm_params*, gm_batch*, const gm_hits*, gm_sam_text* out, void* hip_stream);

/* ---- coordinate-sorted SAM: the rows stay in HBM until the input is exhausted (gm_samsort.hip) ----
 * A gm_sam_sorter belongs to one index and its device.  gm_output_batch_sorted / _sorted_resident do for a block exactly what
 * gm_output_batch_text / _text_resident do - fp64 pass, traceback, coverage / per-nucleotide / SNP deposit, the rows as text - but the
 * text is not downloaded: it is appended device to device, on hip_stream, to the sorter's arena (pieces of GM_SORT_PIECE bytes, default
 * 1 GiB, at least 64 KiB; a row never straddles two pieces) under the block's sequence number `seq`, with one key per row:
 *     key = (uint64_t)contig << 32 | chr_pos        (~0 for a record without a contig: sorts last)
 * gm_sam_sorter_finish orders the rows by key; equal keys keep input order: ascending seq, then gm_output_batch's record order within
 * the block.  Blocks may be added in any order and from several threads at once (different batches, one sorter).  One stable radix sort
 * of (key, 32-bit row ordinal) pairs over the key bits in use, a scan of the sorted rows' lengths, and gm_sam_sorter_read gathers the
 * rows of one slab at a time in HBM (k_ss_gather) and downloads them.
 * A call that fails before a row of its block is in the arena gives its seq back (GM_E_BATCH_TOO_LARGE: add the block in halves).
 * GM_E_ARG: a seq used before, or an add after finish (nothing is deposited).  GM_E_NOMEM: the arena cannot grow - nothing of the block
 * has been deposited; gm_last_error() gives the bytes the sorter holds and the bytes it asked for.  GM_E_UNSUPPORTED: more than
 * 2^32 - 1 rows.  GM_E_NO_DEVICE on a host-only index. */
typedef struct gm_sam_sorter gm_sam_sorter;
typedef struct {
    uint64_t rows, text_bytes, pieces, piece_bytes;     /* what the sorter holds */
    double add_s;                   /* host seconds inside the arena appends (all threads) */
    double sort_s;                  /* gm_sam_sorter_finish, host wall */
    double gather_ms;               /* device time of k_ss_spans + k_ss_gather over all reads (HIP events) */
    uint64_t gather_bytes;          /* bytes the gather kernel wrote */
    double download_s;              /* host seconds in the device-to-host copies of the reads */
    double bai_ms;                  /* device time of the .bai's kernels: k_bai_rows per slab, and the build (HIP events around it) */
    uint64_t bai_bytes, bai_chunks; /* the .bai: its bytes, the chunks of its bins (the pseudo-bins' aside); 0 before gm_sam_sorter_bai */
} gm_sam_sort_stats;
int gm_sam_sorter_create(gm_index*, gm_sam_sorter** out);
void gm_sam_sorter_destroy(gm_sam_sorter*);
int gm_output_batch_sorted(gm_index*, const gm_params*, gm_batch*, const gm_reads*, const gm_read_text*, const gm_hits*, gm_sam_sorter*, uint64_t seq,
                           void* hip_stream);
int gm_output_batch_sorted_resident(gm_index*, const gm_params*, gm_batch*, const gm_hits*, gm_sam_sorter*, uint64_t seq, void* hip_stream);
/* sorts; zero rows is GM_OK with *n_rows = *text_bytes = 0.  A second call returns the same numbers.  A finish that fails (GM_E_NOMEM
 * for the sort's buffers, GM_E_HIP) is remembered: every later finish and read returns its status, no block can be added */
int gm_sam_sorter_finish(gm_sam_sorter*, uint64_t* n_rows, uint64_t* text_bytes, void* hip_stream);
/* the next whole rows that fit in cap bytes, in sorted order; *n_out = 0: done.  GM_E_CAPACITY when the next row alone is longer than cap:
 * *n_out = that row's length, nothing is consumed.  GM_E_ARG before finish.  One reader at a time */
int gm_sam_sorter_read(gm_sam_sorter*, char* text, uint64_t cap, uint64_t* n_out, void* hip_stream);
int gm_sam_sorter_stats(gm_sam_sorter*, gm_sam_sort_stats* out);
/* unit level (parity tests, tools/sam_sort_bench.py): n_rows rows of the caller's - text[row_off[i], row_off[i + 1]) - under the caller's
 * keys (contig >= the number of contigs: the key ~0), added as block `seq` exactly as the rows of gm_output_batch_sorted are */
int gm_sam_sorter_add_rows(gm_sam_sorter*, uint64_t seq, const char* text, const uint64_t* row_off, const uint32_t* contig, const uint64_t* chr_pos,
                           uint64_t n_rows, void* hip_stream);

/* ---- BAM: binary records (SAMv1 section 4.2) inside BGZF, both written on the device (gm_bam.hip) ----
 * gm_bam_header: the uncompressed bytes that open a BAM file - "BAM\1", l_text, the n bytes of sam_header, n_ref, then per contig of
 * the index l_name, the name with its NUL and l_ref.  Host only: works on a host-only index.  *n_out = the size; GM_E_CAPACITY when
 * that exceeds cap (nothing is written). */
int gm_bam_header(gm_index*, const char* sam_header, uint64_t n, void* out, uint64_t cap, uint64_t* n_out);
/* any n bytes of the caller's -> whole BGZF blocks of at most 65280 input bytes each, compressed on the device: level 0 stored blocks,
 * level 1 one dynamic-Huffman block over literals only (no LZ77 matches), level 1 | GM_BGZF_LZ77 one dynamic-Huffman block over literals
 * and LZ77 matches (length 4 - 258, distance up to 32768, inside the block's own input; what the matcher finds: DESIGN.md section 4), each
 * written stored where that is not smaller.  The output is a function of the input bytes and the level word alone.  n = 0: *n_out = 0.
 * GM_E_ARG for any other level word (0 | GM_BGZF_LZ77, 2, another bit), GM_E_NO_DEVICE on a host-only index, GM_E_CAPACITY (*n_out = the
 * bytes needed, nothing is written) when the blocks exceed cap; n + 31 per started 65280 always holds them. */
enum { GM_BGZF_LZ77 = 0x100 };
int gm_bgzf_compress(gm_index*, const void* data, uint64_t n, int level, void* out, uint64_t cap, uint64_t* n_out, void* hip_stream);
/* the 28-byte empty block that ends a BGZF file */
int gm_bgzf_eof(void* out28);
/* gm_output_batch_text / _text_resident with a different ending: the same fp64 pass, traceback and deposits, and the block's records - one
 * per gm_sam_rec, in gm_output_batch's order - leave as BGZF blocks (records may span blocks).  A record is the SAM row of the text form
 * in binary: refID = contig, pos = chr_pos - 1, mapq clamped to 0 .. 255, bin = reg2bin(pos, pos + reference length of the CIGAR, 1 when
 * that is 0), flag 0 / 16, no mate; read_name = the first 254 bytes of the name (l_read_name is one byte; the SAM row keeps up to 1023);
 * the CIGAR operations, SEQ and the first l_seq characters of QUAL as the row prints them (len << 4 | op; nibbles of "=ACMGRSVTWYHKDBN",
 * anything else 15; minus 33, floored at 0); tags XA:f = (float)((double)a_score / adjust), XP:f = post_prob's bits, X0:i as int32.
 * level as in gm_bgzf_compress (0, 1 or 1 | GM_BGZF_LZ77).  len = bytes of the blocks, raw_len = bytes of the records.  GM_E_CAPACITY: cap holds the size needed and
 * NOTHING has been deposited - repeat the call.  GM_E_UNSUPPORTED exactly where gm_output_batch_text returns it (an XA / XP outside the
 * range the text form prints), so both forms accept the same blocks.  A block with no mapped read: len = 0.  No enqueue form. */
typedef struct {
    void* data;
    uint64_t cap, len, raw_len, n_recs;
    int level;
} gm_bam_out;
int gm_output_batch_bam(gm_index*, const gm_params*, gm_batch*, const gm_reads*, const gm_read_text*, const gm_hits*, gm_bam_out* out, void* hip_stream);
int gm_output_batch_bam_resident(gm_index*, const gm_params*, gm_batch*, const gm_hits*, gm_bam_out* out, void* hip_stream);
/* while gm_batch_set_profiling is on, the two calls above bracket their kernels with HIP events (two more waits per call).  Since the last
 * call of this function: ms[0] = k_bam_sizes + k_bam_rows, ms[1] = k_bgzf_deflate (k_bgzf_deflate_lz with GM_BGZF_LZ77) + the scan of the sizes + k_bgzf_compact; bytes[0] = bytes
 * of records written, bytes[1] = bytes into and bytes[2] = bytes out of the BGZF kernels (tools/bam_bench.py) */
int gm_batch_bam_times(gm_batch*, double* ms /* [2] */, uint64_t* bytes /* [3] */);
/* what gm_output_batch_sorted / _sorted_resident put into a sorter's arena: SAM rows as text (default) or BAM records.  Keys, stable
 * order and pieces are the same; gm_sam_sorter_read then returns whole records.  Before the first block: GM_E_ARG afterwards. */
enum { GM_ROWS_TEXT = 0, GM_ROWS_BAM = 1 };
int gm_sam_sorter_set_rows(gm_sam_sorter*, int rows);
/* gm_sam_sorter_read with the slab compressed on the device before the download: the next whole rows whose BGZF form is sure to fit in
 * cap (reserved for the worst case, stored: the rows' bytes + 31 per started 65280), as whole BGZF blocks.  *n_out = 0: done.
 * GM_E_CAPACITY when the next row alone needs more: *n_out = the cap it needs, nothing is consumed.  level as in gm_bgzf_compress
 * (0, 1 or 1 | GM_BGZF_LZ77); on an indexed sorter every read takes the same level word. */
int gm_sam_sorter_read_bgzf(gm_sam_sorter*, int level, void* out, uint64_t cap, uint64_t* n_out, void* hip_stream);
/* ---- the .bai (SAMv1 section 5.2) of a sorted BAM, built on the device from what the sorter holds (gm_bai.hip) ----
 * gm_sam_sorter_index_begin, after a successful finish and before the first read, on a sorter of GM_ROWS_BAM: from then on
 * gm_sam_sorter_read_bgzf notes, in HBM and 28 bytes per row, where the records of every slab it hands out lie in the file - it takes the
 * blocks it returns to be written back to back from file_offset (the bytes of the compressed header in front of them), at one level
 * (GM_E_ARG for another), and notes nothing on a read that fails; gm_sam_sorter_read is refused (GM_E_ARG).  GM_E_ARG: text rows, not
 * finished, a row already read, called twice.  GM_E_NOMEM as the sorter reports its own.
 * gm_sam_sorter_bai, once every row is read (GM_E_ARG before, and without index_begin): the finished file.  *n_out = its bytes;
 * GM_E_CAPACITY when that exceeds cap, nothing is written.  It may be called again.  The bytes are a function of the records, the
 * level and file_offset alone.  The rules where the specification leaves a choice:
 *   a record starts at the virtual offset (coffset << 16 | uoffset) of its block_size and ends at that of the byte behind it - (the next
 *   block, 0) when it ends on a payload's end, (whatever follows the last block, 0) for the last record; refID, pos, flag and the CIGAR
 *   are read from the record: beg = pos, end = pos + the CIGAR's reference length (1 when that is 0), bin = reg2bin(beg, end);
 *   a chunk = a maximal run of consecutive records of one (refID, bin); two chunks of a bin are merged when the later one starts in the
 *   compressed block in which the earlier one ends, or before; bins ascend; pseudo-bin 37450 last for every reference with records
 *   (first start / last end; records with flag 0x4 clear / set); linear index: n_intv = ((max end - 1) >> 14) + 1, entry w = the smallest
 *   start of the records that overlap window w, an empty window takes the entry before it, leading empty windows 0; n_no_coor = the
 *   records with refID < 0.
 * GM_E_UNSUPPORTED: a record ends beyond 2^29 (the message names reference, position and limit).  GM_E_ARG: the records do not ascend in
 * (refID as unsigned, pos) - keys of gm_sam_sorter_add_rows that disagree with the records -, a row is no whole record, or names a
 * reference the index does not have. */
int gm_sam_sorter_index_begin(gm_sam_sorter*, uint64_t file_offset);
int gm_sam_sorter_bai(gm_sam_sorter*, void* out, uint64_t cap, uint64_t* n_out, void* hip_stream);

/* enqueue / wait forms: the call is queued on the batch's own service thread and runs there exactly as the synchronous form would;
 * the caller goes on (with another batch).  Calls queued on one batch run in order - gm_output_batch_enqueue may be queued right
 * behind the gm_map_batch_enqueue whose gm_hits it reads - and after a failing call the rest of the batch's queue is skipped.
 * gm_batch_wait returns when the batch's queue is empty: GM_OK, or the status of the first call that failed (gm_last_error() has its
 * text).  gm_params / gm_reads are copied at enqueue time; the arrays behind gm_reads, gm_hits and gm_sam_out stay the caller's until
 * the wait.  One HIP stream per batch, as with the synchronous forms. */
int gm_map_batch_enqueue(gm_index*, const gm_params*, gm_batch*, const gm_reads*, gm_hits* out, void* hip_stream);
int gm_output_batch_enqueue(gm_index*, const gm_params*, gm_batch*, const gm_reads*, const gm_hits*, gm_sam_out* out, void* hip_stream);
int gm_batch_wait(gm_batch*);

/* ---- unit-level device entry points (parity tests) ---- */
int gm_dev_sa_interval(gm_index*, const char* kmers, uint32_t n, uint32_t m, uint64_t* start, uint64_t* end);
int gm_dev_locate(gm_index*, const uint64_t* ranks, uint32_t n, int use_full_sa, uint64_t* out);
int gm_dev_nw_score(gm_index*, const gm_params*, const gm_reads*, const uint32_t* read_idx, const uint8_t* strand,
                    const uint64_t* pos, uint32_t n, float* score, uint8_t* valid);
int gm_dev_traceback(gm_index*, const gm_params*, const gm_reads*, const uint32_t* read_idx, const uint8_t* strand,
                     const uint64_t* pos, uint32_t n, char* ops /* n x ops_stride, 'M','I','D', NUL padded */,
                     uint32_t ops_stride, uint16_t* ops_len);

/* the prep kernel alone (the form GM_PREP chooses) on rows first_row .. reads->n - 1 of the block, as a sub-batch view of a pipelined
 * call sees them, with the 2-bit rows.  status / self_score / min_score take reads->n entries (rows before first_row: those of a pass over
 * the whole block), pack reads->n x *pack_words words (zero before first_row; NULL: not wanted), work[4] = reads with a negative
 * probability, reads with a quality character above 127, the lowest and the highest quality character.  exact (first_row = 0 only): the
 * kernel reads the rows from allocations of exactly reads->n x stride bytes */
int gm_dev_prep(gm_index*, const gm_params*, const gm_reads*, uint32_t first_row, int exact, int8_t* status, float* self_score, double* min_score,
                uint32_t* pack, uint32_t* pack_words, uint64_t* work);

/* the format in which the unit probes above (and gm_dev_pair_hmm, which refuses FASTA) read their gm_reads from now on: GM_READS_FASTQ
 * (default) or GM_READS_FASTA - see gm_batch_set_read_format.  Per index, not thread-safe against probes running at the same time */
int gm_index_set_probe_format(gm_index*, int format);

/* SeqReader::FixReads2 / Compare (src/SeqReader.cpp:1356-1372, 1294-1305) of every read of the block against `adaptor`, on the device:
 * out_len[i] = the length read i keeps (see gm_batch_set_adaptor).  Only gm_reads.bases / len are read; NULL or "" copies len */
int gm_dev_adaptor_trim(gm_index*, const gm_reads*, const char* adaptor, uint16_t* out_len);

/* gm_batch_upload_text's parse on a text of the caller's, the rows brought back: bases / quals take info->n rows of info->stride bytes
 * (zero padded), len and recs info->n entries.  rows_cap = the reads the four buffers have room for (each row buffer rows_cap x
 * info->stride bytes; 2048 is the largest stride): GM_E_CAPACITY with info filled in when n exceeds it, so a first call with
 * rows_cap = 0 sizes the second.  Any of the four may be NULL. */
int gm_dev_fastq_rows(gm_index*, const char* text, uint64_t bytes, gm_text_info* info, gm_text_rec* recs, uint8_t* bases, uint8_t* quals, uint16_t* len,
                      uint64_t rows_cap);
/* text bytes one workgroup of the line pass covers (a tile): lets a test put a line start on either side of a tile edge */
uint32_t gm_dev_fastq_tile_bytes(void);

/* printf("%g") as the device prints XA / XP (gm_fmt_dev.h): out[16 i ..] holds len[i] characters, no terminator; len[i] = 0 for a
 * value outside the function's domain (0, -0, inf, nan, 2^-200 <= |v| < 2^200) */
int gm_dev_fmt_g6(gm_index*, const double* v, uint32_t n, char* out /* n x 16 */, uint8_t* len);
/* printf("%.2e") as the device prints the p-value of --snp's ninth .gmp column (gm_put_e2_hd), same contract: always 8 characters
 * on its domain (+0.0, 2^-200 <= v < 2^200), len[i] = 0 outside it (negative, -0.0, nan, inf, anything else) */
int gm_dev_fmt_e2(gm_index*, const double* v, uint32_t n, char* out /* n x 16 */, uint8_t* len);
/* the exclusive scan behind every offset array of the map and output steps, on values of the caller's: out[i] = in[0] + .. + in[i - 1]
 * in 64 bits, out[n] = the total.  n up to 2^32 */
int gm_dev_scan_u32(gm_index*, const uint32_t* in, uint64_t n, uint64_t* out /* n + 1 */);
/* the mate kernels of gm_batch_set_mates (k_mate_spans, k_mate_resolve, k_mate_fields) on inputs of the caller's, none from a mapped
 * batch: n_recs records in record order (ascending `read`, every one below n_reads), a CIGAR pool of cigar_bytes bytes that ends in a
 * NUL and that every cigar_off points into, and the limits.  row_src: n_rows 64-bit entries, a record index, or bit 63 set and a
 * read of the block that has no record (the rows of gm_batch_set_unmapped_rows); NULL = one row per record, n_rows is not read.
 * Out: span[n_recs], prim[n_reads] (a record index, ~0: none), proper[n_reads / 2], the counters, rows[n_rows] (a row that names
 * neither a record nor a read comes back with flag 0). GM_E_ARG, before anything is uploaded or launched, for an odd n_reads, for
 * min_insert > max_insert, for a cigar_off outside the pool or a pool without its last NUL, and for records out of read order */
int gm_dev_mate_resolve(gm_index*, const gm_sam_rec* recs, uint64_t n_recs, const char* cigar_pool, uint64_t cigar_bytes, uint32_t n_reads,
                        uint32_t min_insert, uint32_t max_insert, const uint64_t* row_src, uint64_t n_rows,
                        uint32_t* span, uint64_t* prim, uint8_t* proper, gm_mate_stats* stats, gm_mate_row* rows);

/* bin_seq::pairHMM (src/bin_seq.cpp:60-244) of read read_idx[k] in the orientation of strand[k] against the window at pos[k]:
 * out[k][max_len][5] floats (a, c, g, t, n per window position), max_len = gm_reads.stride */
int gm_dev_pair_hmm(gm_index*, const gm_params*, const gm_reads*, const uint32_t* read_idx, const uint8_t* strand, const uint64_t* pos, uint32_t n, float* out);

/* ---- coverage track (amount_genome) ---- */
int gm_coverage_reset(gm_index*, uint32_t bin_size);
uint64_t gm_coverage_bins(const gm_index*);
void* gm_coverage_device_ptr(gm_index*);                         /* float[bins] in HBM, for RCCL all-reduce by the caller */
int gm_coverage_add(gm_index*, const uint64_t* pos, const uint32_t* span, const float* w, uint32_t n, void* hip_stream);
int gm_coverage_download(gm_index*, float* host /* bins */);
int gm_coverage_allreduce(gm_index** per_gpu, int n_gpu);        /* single-process multi-GPU: ncclAllReduce(sum) over xGMI */
int gm_coverage_write_sgr(gm_index*, const float* host_bins, const char* path, int append);
/* -b / -d (bisulfite, A->G): the per-nucleotide track reads[A,C,G,T,N][loc] of BSScoredSeq::score (src/BSScoredSeq.cpp:24-88,
 * GenomeBwt::AddSeqScore src/GenomeBwt.cpp:556-603), 5 x bins floats in HBM, filled by gm_output_batch once enabled, and the
 * .gmp writer (GenomeBwt::PrintFinalBisulfite src/GenomeBwt.cpp:1092-1210; these modes write <out>.gmp INSTEAD of <out>.sgr) */
int gm_coverage_enable_nuc(gm_index*);
void* gm_coverage_nuc_device_ptr(gm_index*);
int gm_coverage_download_nuc(gm_index*, float* host /* 5 x bins */);
int gm_coverage_write_gmp(gm_index*, const gm_params*, const float* host_bins, const float* host_nuc, const char* path, int append);
/* (GM_MODE_SNP: PrintFinalSNP src/GenomeBwt.cpp:930-1009 - every position above 0.001: contig, position, %.5f total, five %.5f sums.  This
 * writer stops there, eight columns; gm_coverage_write_gmp_calls below writes the same rows with PrintSNPCall's ninth column.) */

/* ---- SNP calls (--snp): GenomeBwt::PrintSNPCall src/GenomeBwt.cpp:1011-1090 with is_snp :875-901, LRT :739-753, dipLRT :758-873 ----
 * One device pass (k_snp_call) over the total track and the five per-nucleotide tracks in HBM.  The reference's one GSL function,
 * gsl_cdf_chisq_P(x, 1 | 2), is evaluated in closed form - erf(sqrt(x/2)), 1 - exp(-x/2), 0 for x <= 0 - and the p-value as 1 - P in
 * fp64 like the reference's.  All three need bin size 1 and gm_coverage_enable_nuc (GM_E_ARG otherwise).  snp_pval is the reference's
 * --snp_pval (gSNP_PVAL, a float, default 0.001), monop its --snp_monop (LRT instead of dipLRT).
 * Two departures, where the reference has no defined answer: a forced-monoploid position (first / second sum above 3, or no second)
 * is never diploid and carries pval1 (the reference reads one float before its array there); and the likelihood ratios are kept as
 * logarithms, so totals above ~440, where the reference's pow() underflows to 0 / 0, still give a finite p-value. */
typedef struct {
    uint64_t pos;           /* 0-based on the concatenated reference */
    uint32_t contig;        /* contig index */
    uint64_t chr_pos;       /* 1-based within the contig, as the .gmp prints it */
    float total, nuc[5];    /* the row's six numbers: total, a c g t n */
    double p_val;
    uint8_t ref, alt1, alt2, diploid;   /* 0..4 = a c g t n; alt2 = 255 unless diploid */
} gm_snp_rec;
/* the rows PrintSNPCall marks 'Y', ascending position.  GM_E_CAPACITY when there are more than cap: *n_out has the number required */
int gm_snp_calls(gm_index*, float snp_pval, int monop, gm_snp_rec* out, uint64_t cap, uint64_t* n_out, void* hip_stream);
/* is_snp (src/GenomeBwt.cpp:875-901) on caller-supplied counts (unit level, parity tests): n x 5 floats -> p-value, first maximum,
 * second maximum (-1 where dipLRT drops it or with monop), diploid */
int gm_dev_snp_stat(gm_index*, const float* counts, uint32_t n, int monop, double* p_val, int8_t* pos1, int8_t* pos2, uint8_t* dip);
/* PrintFinalSNP (src/GenomeBwt.cpp:930-1009) with its ninth column: N, [YN]:r->x p_val=%.2e or [YN]:r->x/y p_val=%.2e.  The tracks are read
 * from HBM slab by slab (GM_TRACK_SLICE positions per host thread); no host copy of them is needed */
int gm_coverage_write_gmp_calls(gm_index*, float snp_pval, int monop, const char* path, int append);

/* ---- track files formatted on the device (k_track_sizes / k_track_rows, gm_tracktext.hip) ----
 * The same files as gm_coverage_write_sgr / gm_coverage_write_gmp, byte for byte, without a host copy of the tracks: the rows are
 * formatted where the tracks live, slab by slab (GM_TRACK_SLICE bins per slab, default 2^24), and only their text crosses the link,
 * into page-locked buffers that go to the file with pwrite at a running offset.  A slab in which a printed value lies outside
 * [0, 1e9) - negative, NaN, inf: what the host writers hand to snprintf - is formatted by the host emitters from that slab's tracks
 * (gm_track_text_stats.host_slabs counts them), so the file is the host writer's file whatever the tracks hold.
 * GM_E_NO_DEVICE on a host-only index; GM_E_ARG without a coverage track, for bin_lo > bin_hi or bin_hi > gm_coverage_bins, and for
 * gm_coverage_write_gmp_device in GM_MODE_NORMAL or without gm_coverage_enable_nuc; gm_last_error() names the call. */
typedef struct { uint64_t rows, bytes, slabs, host_slabs, launches; double kernel_ms; } gm_track_text_stats;
/* GenomeBwt::PrintFinalSGR src/GenomeBwt.cpp:1212-1273 */
int gm_coverage_write_sgr_device(gm_index*, const char* path, int append);
/* GenomeBwt::PrintFinalBisulfite src/GenomeBwt.cpp:1092-1210 (GM_MODE_BS, BS2, ATOG, ATOG2) and PrintFinalSNP :930-1009 without
 * PrintSNPCall's column (GM_MODE_SNP: eight columns) */
int gm_coverage_write_gmp_device(gm_index*, const gm_params*, const char* path, int append);
/* the rows of bins [bin_lo, bin_hi) as text in host memory: p NULL or GM_MODE_NORMAL = .sgr rows, else the .gmp rows of p->mode (bins
 * past the last one the files print have no row).  *n_out = the bytes needed; GM_E_CAPACITY when that exceeds cap, text[0, cap)
 * then holds the first cap bytes (the protocol of gm_snp_calls) */
int gm_coverage_text(gm_index*, const gm_params* p, uint64_t bin_lo, uint64_t bin_hi, char* text, uint64_t cap, uint64_t* n_out);
/* the file of gm_coverage_write_gmp_calls (nine columns), byte for byte, formatted on the device: per slab k_snp_call writes the code
 * byte and the p-value of every position into HBM, then the track text kernels' calls variant prints the rows with the ninth column,
 * the p-value with an exact "%.2e" (gm_put_e2_hd).  A slab with a printed count outside [0, 1e9) or a printed p-value outside that
 * function's domain is formatted by the host emitter.  gm_coverage_calls_text: the rows of the positions [bin_lo, bin_hi), protocol
 * and argument errors of gm_coverage_text.  Both need bin size 1 and gm_coverage_enable_nuc like gm_snp_calls (GM_E_ARG otherwise). */
int gm_coverage_write_gmp_calls_device(gm_index*, float snp_pval, int monop, const char* path, int append);
int gm_coverage_calls_text(gm_index*, float snp_pval, int monop, uint64_t bin_lo, uint64_t bin_hi, char* text, uint64_t cap, uint64_t* n_out);
/* of the last of the five calls above on this index: kernel_ms is the device time of the launches (hipEvent), launches their number
 * (four per slab with the ninth column: k_snp_call, sizes, scan, rows) */
int gm_coverage_text_stats(gm_index*, gm_track_text_stats*);

/* ---- <out>.vcf (--vcf): Genome::PrintFinalVCF src/Genome.cpp:1142-1245 over the records of gm_snp_calls ----
 * Header, unless appending: ##fileformat=VCFv4.0, ##fileDate=YYYYMMDD (local date), ##source=<gm_version()>, the #CHROM line.  One row
 * per record in ascending position, IDs snp0, snp1, ... counting the rows of this call, letters acgtn:
 *   contig \t pos \t snpN \t ref \t xy \t . \t . \t Diploid;pval=%.5f;coverage=%.5f;ratio=%.2f      ratio = nuc[y] / nuc[x] in float
 *   contig \t pos \t snpN \t ref \t x  \t . \t . \t Monoploid;pval=%.5f;coverage=%.5f
 * Formatted on the host (the rows are sparse): a count pass, then the records of one stretch of positions at a time.  Two departures:
 * the date is one well-formed line (the reference prints ctime()'s text with its newline), and a row needs a total above 0.001 like
 * the .gmp's 'Y' rows, not above 0, so both files name the same positions.  Needs bin size 1 and gm_coverage_enable_nuc. */
int gm_coverage_write_vcf(gm_index*, float snp_pval, int monop, const char* path, int append);

#ifdef __cplusplus
}
#endif
#endif
