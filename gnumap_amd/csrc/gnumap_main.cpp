// gnumap_main.cpp — the C++ host driver: keeps the reference's command line (src/Driver.cpp:172-250, 2658-3251),
// SAM format (src/Driver.cpp:2146-2217, 2317-2329) and .sgr output (src/GenomeBwt.cpp:1212-1273), and drives the hot
// path through the C ABI of libgnumap_hip.so only.  Per batch it mirrors parallel_thread_run (src/Driver.cpp:2303-2407):
//     parse FASTQ (or FASTA) block -> gm_map_batch (= loop over set_top_matches) -> gm_output_batch (= loop over create_match_output)
//     -> SAM text.
// I/O at rate: the FASTQ file is memory-mapped and cut into blocks by one scanner thread (memchr only, no
// copies); per GPU `--workers` host threads (default 3, each with its own gm_batch and HIP stream) pack a block, run the
// two batch calls and hand the records to formatter threads; SAM text is written in block order by one writer thread.
// --sam_text=device: the library formats the rows on the GPU (gm_output_batch_text) and the formatter stage is skipped.
// --read_text=device: a worker copies its block's byte range into a page-locked buffer and the library cuts it into reads on the GPU
// (gm_batch_upload_text); parse_range and pack_block do not run for that block.
// --sam_shards=K: the rows go to K files by input position, each with its own descriptor and writer; their concatenation in
// order is the single-file SAM.
// --sam_sort=coordinate: the rows never leave HBM unsorted - every block's text goes into a gm_sam_sorter (gm_output_batch_sorted) under its
// block index, and after the last block the rows come down in coordinate order, slab by slab, into the single <out>.sam.
// The number of blocks in flight is bounded by a fixed pool of Block objects.
// Multi-GPU (--gpus N): one index replica per GPU, blocks dealt to whichever worker is free, coverage tracks combined
// with one RCCL all-reduce (gm_coverage_allreduce).
// Layout: process_block = the two batch calls of one block; Run = what lives for the whole run, main() = its steps in order; Pass = one pass
// of the pipeline, its queues and the bodies of its scanner, worker, formatter and writer threads.
#include "gnumap_hip.h"
#include "gm_fmt.h"
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cctype>
#include <map>
#include <memory>
#include <set>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#define MAX_NAME_SZ 1024        // inc/const_include.h:46

struct Options {
    std::string genome, output = "gnumap_out", reads, subst;
    std::string adaptor;        // -A / --adaptor: trimmed from the 3' end of every read on the device (gm_batch_set_adaptor); empty = none
    gm_params p;
    int gpus = 1, locate_sampled = 0, verbose = 1;
    uint32_t batch = 262144;
    bool batch_set = false;     // --batch given: blocks of exactly that many reads (one sequential scanner); otherwise byte-range chunks parsed by the workers
    int workers = 3;            // host threads (and gm_batch objects) per GPU (measured: 2 -> 9.6, 3 -> 11.4, 4 -> 11.0 M reads/s)
    int fmt_threads = 0;        // SAM formatter threads per block (0 = min(8, cores))
    int threads = 1;            // -c: accepted for compatibility (the GPU replaces the pthread pool)
    float snp_pval = 0.001f;    // --snp_pval: gSNP_PVAL inc/const_define.h:33
    bool snp_monop = false, snp_calls = false;      // --snp_monop: gSNP_MONOP; --snp_calls: <out>.gmp with PrintSNPCall's ninth column
    bool sam_text_device = false;   // --sam_text=device: SAM rows formatted on the GPU (gm_output_batch_text); host = format_sam below
    bool vcf = false;               // --vcf: with --snp, <out>.vcf beside <out>.gmp (gm_coverage_write_vcf)
    bool track_text_device = false; // --track_text=device: <out>.sgr / <out>.gmp formatted on the GPU (gm_coverage_write_*_device); host = the whole tracks come down
    int sam_shards = 1;             // --sam_shards=K: <out>.0.sam .. <out>.<K-1>.sam by input position instead of one <out>.sam
    bool read_text_device = false;  // --read_text=device: chunk-mode blocks go up as FASTQ text and are cut into reads on the GPU (gm_batch_upload_text); host = parse_range + pack_block
    bool sam_sort = false;          // --sam_sort=coordinate: the rows stay in HBM, are sorted there once and written in coordinate order (implies --sam_text=device)
    bool sam_text_host_set = false; // an explicit --sam_text=host (refused with --sam_sort=coordinate)
    bool bam = false;               // --sam_format=bam: <out>.bam instead of <out>.sam, records and BGZF written on the GPU (gm_output_batch_bam; implies --sam_text=device)
    int bam_level = 1;              // --bam_level=0|1: stored blocks, or Huffman-coded ones
    bool bam_level_set = false;     // (refused without --sam_format=bam)
    bool bam_lz77 = false;          // --bam_lz77: LZ77 matches under the Huffman code of level 1; once the options are checked, GM_BGZF_LZ77 in bam_level
    bool sam_unmapped = false;      // --sam_unmapped: a read without a row gets a flag-4 row (gm_batch_set_unmapped_rows; implies --sam_text=device)
    bool sam_md = false;            // --sam_md: NM:i and MD:Z of every row as printed, behind X0 (gm_batch_set_row_tags; implies --sam_text=device)
    bool sam_cigar_set = false, sam_cigar_forward = false;      // --sam_cigar=gnumap|forward: a minus-strand row's CIGAR as the reference prints it, or in reference order (gm_batch_set_cigar_order; implies --sam_text=device)
    bool bam_index = false;       // --bam_index: <out>.bam.bai beside a sorted <out>.bam, built on the GPU from what the sorter holds (gm_sam_sorter_bai)
    bool fasta = false;             // the read file starts with '>' (SeqReader::find_type): FASTA records, gm_batch_set_read_format(GM_READS_FASTA)
    std::string mates;              // --mates=FILE2: the second mates' file; the positional file holds the first mates (gm_batch_set_mates; implies --sam_text=device)
    bool interleaved = false;       // --interleaved: the positional file holds the mates in alternation
    uint32_t min_insert = 0, max_insert = 500; const char* insert_opt = nullptr;      // --min_insert / --max_insert (insert_opt: the one that was given)
    bool paired() const { return interleaved || !mates.empty(); }
};

[[noreturn]] static void usage(int rc, const char* msg) {
    if (msg && *msg) fprintf(stderr, "%s\n", msg);
    fprintf(stderr,
            "Usage: gnumap [options] <file_to_parse>\n"
            "  <file_to_parse>              FASTQ (first byte '@') or FASTA (first byte '>': the 15 IUPAC letters in either case, sequence\n"
            "                               lines joined, the whole header line is the name); -A and --snp take FASTQ only\n"
            "  -g, --genome=STRING          Genome .fa file\n"
            "  -o, --output=STRING          Output file prefix (<out>.sam, <out>.sgr)\n"
            "  -a, --align_score=DOUBLE     Limit for sequence alignment (default: 0.9)\n"
            "  -r, --raw                    Use raw score when determining alignment cutoff\n"
            "  -q, --read_quality=DOUBLE    Read quality cutoff\n"
            "  -m, --mer_size=INT           Mer size (default: 10)\n"
            "  -j, --jump=INT               Number of bases to jump in the sequence indexing (default: mer_size/2)\n"
            "  -k, --num_seed=INT           Minimum number of seed matches per location (default: 2)\n"
            "  -h, --max_kmer=INT           Kmers occuring more often than this are skipped (default: no limit)\n"
            "  -T, --max_match=INT          Maximum number of matches per read (default: 1000)\n"
            "  -u X                         Only match sequences to one position (like the reference, -u swallows the next word)\n"
            "  -G, --gap_penalty=DOUBLE     Gap penalty (default: -4)\n"
            "  -S, --subst_file=STRING      5 x 4 substitution matrix file (rows a c g t n; scores are then used unscaled)\n"
            "  -A, --adaptor=STRING         Adaptor sequence to trim from the 3' end of every read (SeqReader::FixReads2, on the GPU):\n"
            "                               a read is cut at the first offset where 85%% of the compared characters equal the adaptor's,\n"
            "                               else loses its last 4 bases; SEQ and QUAL of a row stay whole.  At most 256 characters.\n"
            "                               -A takes the string as given and is pinned to the reference program's output;\n"
            "                               --adaptor=STRING is -A of the lower-cased string (the reference reads an unterminated buffer there)\n"
            "  -c, --num_proc=INT           accepted for compatibility (the GPU path ignores it)\n"
            "  -b, --bs_seq / --b2 / -d, --a_to_g   bisulfite / A-to-G scoring\n"
            "      --snp                    pair-HMM per-nucleotide deposit (SNPScoredSeq); <out>.gmp with eight columns (no SNP call)\n"
            "      --snp_calls              with --snp: append the reference's ninth column, the likelihood-ratio SNP call\n"
            "                               (N, [YN]:r->x p_val=.., [YN]:r->x/y p_val=..); not yet the default of --snp\n"
            "      --snp_pval=DOUBLE        P-Value cutoff for calling SNPs (default: 0.001); changes the ninth column only\n"
            "      --snp_monop              monoploid SNP calling; changes the ninth column only\n"
            "      --vcf                    with --snp: also write <out>.vcf (VCFv4.0), one row per position the ninth column marks 'Y',\n"
            "                               under --snp_pval / --snp_monop; <out>.gmp is written exactly as without the flag\n"
            "      --no_nw                  use k-mer hit counts instead of Needleman-Wunsch alignments\n"
            "      --fast, --print_all_sam, --illumina, --up_strand, --down_strand, --bin_size=INT\n"
            "  MI355X options: --gpus=N  --batch=N (blocks of exactly N reads)  --chunk_reads=N  --workers=N  --fmt_threads=N  --locate=sampled|full\n"
            "      --read_text=host|device  where a block of FASTQ text becomes read rows: host threads (default) or the GPU (the text is\n"
            "                               uploaded as it stands; same bytes out).  FASTQ only; blocks of --batch=N and --illumina runs and\n"
            "                               what follows a malformed record are cut by the host either way\n"
            "      --sam_text=host|device   where the SAM rows become text: host formatter threads (default) or the GPU\n"
            "                               (gm_output_batch_text; same bytes, no formatter stage)\n"
            "      --track_text=host|device where <out>.sgr / <out>.gmp (eight columns, or nine with --snp_calls) become text: host threads\n"
            "                               (default) or the GPU (same bytes; only the text crosses the link, no whole-genome host array)\n"
            "      --sam_shards=K           1 .. 64 (default 1 = <out>.sam): write <out>.0.sam .. <out>.<K-1>.sam, a block going to the\n"
            "                               shard of its position in the input, header lines in shard 0 only;\n"
            "                               cat <out>.0.sam .. <out>.<K-1>.sam is the single-file SAM\n"
            "      --sam_sort=none|coordinate   none (default): rows in input order.  coordinate: the rows stay on the GPU until the input is\n"
            "                               exhausted, are sorted there by (contig in @SQ order, position) - equal keys keep input order -\n"
            "                               and written once, behind a first header line @HD VN:1.0 SO:coordinate.  Implies --sam_text=device;\n"
            "                               one GPU, one <out>.sam (not with --sam_text=host, --sam_shards above 1 or --gpus above 1)\n"
            "      --sam_format=sam|bam     sam (default): <out>.sam.  bam: <out>.bam and no <out>.sam - the records and their BGZF blocks are\n"
            "                               written on the GPU; with --sam_sort=coordinate the file is a sorted BAM.  Implies --sam_text=device\n"
            "                               (not with --sam_text=host or --sam_shards above 1)\n"
            "      --bam_level=0|1          with --sam_format=bam: 0 = stored BGZF blocks, 1 (default) = Huffman-coded blocks (no LZ77 matches)\n"
            "      --bam_lz77               with --sam_format=bam at level 1: LZ77 matches (4 - 258 bytes, within the block) under the Huffman code,\n"
            "                               found on the GPU - a smaller <out>.bam with the same records (not with --bam_level=0)\n"
            "      --bam_index              with --sam_format=bam --sam_sort=coordinate: also write <out>.bam.bai (SAMv1 section 5.2), built on the\n"
            "                               GPU from the sorted records and their BGZF offsets; <out>.bam is written exactly as without the flag.\n"
            "                               Records must end at or below 2^29 (there is no .csi)\n"
            "      --sam_unmapped           keep the reads that do not map: each gets one row (flag 4, no contig, no position, SEQ and QUAL as in\n"
            "                               the read file, tag YU:i:<code>: 2 no match, 1 too many matches, -2 too short, -3 too poor, 0 nothing\n"
            "                               printed) where its rows would stand; with --sam_sort=coordinate behind every contig, in input order.\n"
            "                               Implies --sam_text=device (not with --sam_text=host).  Every other row is written as without the flag\n"
            "      --sam_md                 NM:i and MD:Z behind X0 on every row whose CIGAR is not *, computed on the GPU from the row as printed\n"
            "                               (POS, CIGAR, SEQ) and the reference - what samtools calmd would add.  Implies --sam_text=device\n"
            "                               (not with --sam_text=host or -A/--adaptor)\n"
            "      --sam_cigar=gnumap|forward  the CIGAR of a minus-strand row: gnumap (default) = its tokens last to first, as GNUMAP prints it;\n"
            "                               forward = in reference order, as the alignment was computed - the order POS and SEQ of the row are in.\n"
            "                               Implies --sam_text=device (not with --sam_text=host)\n"
            "      --mates=FILE2            paired-end reads: FILE2 holds the second mates, <file_to_parse> the first, in the same order and format.\n"
            "                               Each mate is mapped as a single read; the pair is resolved on the GPU: among the places of the two\n"
            "                               mates the forward/reverse combination on one contig with min_insert <= insert <= max_insert and the\n"
            "                               largest product of posteriors gives the primary rows (flag 0x2), the other rows are secondary (0x100);\n"
            "                               every row carries 0x1, 0x40 / 0x80, 0x20 / 0x8, RNEXT, PNEXT and TLEN.  Names are cut at the first blank,\n"
            "                               a trailing /1 and /2 is dropped, and two files that are not in step end the run.  The files are read in\n"
            "                               file order by one thread and a malformed record ends the run.  Implies --sam_text=device (not with\n"
            "                               --sam_text=host or --read_text=device); --batch=N must be even\n"
            "      --interleaved            the same for one file that holds first and second mates in alternation\n"
            "      --min_insert=N           smallest (default 0) and\n"
            "      --max_insert=N           largest (default 500) insert of a proper pair, both inclusive: from the plus-strand mate's POS to the\n"
            "                               last reference base of the minus-strand mate\n");
    exit(rc);
}

static bool starts(const char* s, const char* pre) { return strncmp(s, pre, strlen(pre)) == 0; }
static bool on_device(const char* flag, const char* v) {        // the value of --sam_text, --read_text, --track_text
    if (strcmp(v, "device") && strcmp(v, "host")) { fprintf(stderr, "Error: --%s takes host or device, not: %s\n", flag, v); exit(1); }
    return !strcmp(v, "device");
}

static void parse_args(int argc, char** argv, Options& o) {
    gm_params_default(&o.p);
    bool mer_set = false;
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        if (a[0] != '-') { if (!o.reads.empty()) usage(1, "Please specify only a single sequence file"); o.reads = a; continue; }
        if (a[1] == '-') {
            const char* s = a + 2;
            if (starts(s, "genome=")) o.genome = s + 7;
            else if (starts(s, "output=")) o.output = s + 7;
            else if (starts(s, "align_score=")) o.p.align_score = (float)atof(s + 12);
            else if (!strcmp(s, "percent")) o.p.align_is_fraction = 1;
            else if (!strcmp(s, "raw")) o.p.align_is_fraction = 0;
            else if (!strcmp(s, "no_nw")) o.p.nw = 0;
            else if (starts(s, "read_quality=")) o.p.cutoff = (float)atof(s + 13);
            else if (starts(s, "verbose=")) o.verbose = atoi(s + 8);
            else if (starts(s, "num_proc=")) o.threads = atoi(s + 9);
            else if (starts(s, "mer_size=")) { o.p.mer = atoi(s + 9); mer_set = true; }
            else if (starts(s, "max_match=")) o.p.max_matches = (uint32_t)atoi(s + 10);
            else if (starts(s, "max_kmer=")) o.p.max_kmer_hits = (uint32_t)atoi(s + 9);
            else if (starts(s, "gap_penalty=")) o.p.gap = (float)atof(s + 12);
            else if (starts(s, "subst_file=")) o.subst = s + 11;
            else if (starts(s, "adaptor=")) { o.adaptor = s + 8; for (char& ch : o.adaptor) ch = (char)tolower((unsigned char)ch); }     // Driver.cpp:3160-3163
            else if (starts(s, "max_gap=")) o.p.max_gap = atoi(s + 8);
            else if (!strcmp(s, "unique")) o.p.unique_only = 1;
            else if (!strcmp(s, "print_all_sam")) o.p.print_all_sam = 1;
            else if (!strcmp(s, "bs_seq")) o.p.mode = GM_MODE_BS;
            else if (!strcmp(s, "b2")) o.p.mode = GM_MODE_BS2;
            else if (!strcmp(s, "a_to_g")) o.p.mode = GM_MODE_ATOG;
            else if (!strcmp(s, "snp")) o.p.mode = GM_MODE_SNP;             // Driver.cpp:3207-3211: gSNP, bin size 1
            else if (starts(s, "snp_pval=")) {                                   // Driver.cpp:3030, 3200: "%f" into the float gSNP_PVAL
                if (sscanf(s + 9, "%f", &o.snp_pval) < 1) { fprintf(stderr, "Error: could not read --snp_pval in: %s\n", a); exit(1); }
            }
            else if (!strcmp(s, "snp_monop")) o.snp_monop = true;
            else if (!strcmp(s, "snp_calls")) o.snp_calls = true;
            else if (!strcmp(s, "vcf")) o.vcf = true;                            // Driver.cpp: gVCF
            else if (!strcmp(s, "fast")) o.p.fast = 1;
            else if (starts(s, "bin_size=")) o.p.bin_size = atoi(s + 9);
            else if (starts(s, "jump=")) o.p.jump = atoi(s + 5);
            else if (starts(s, "num_seed=")) o.p.min_seed_hits = atoi(s + 9);
            else if (!strcmp(s, "illumina")) o.p.illumina = 1;
            else if (!strcmp(s, "up_strand")) { o.p.pos_strand = 1; o.p.neg_strand = 0; }
            else if (!strcmp(s, "down_strand")) { o.p.pos_strand = 0; o.p.neg_strand = 1; }
            else if (starts(s, "gpus=")) o.gpus = atoi(s + 5);
            else if (starts(s, "batch=")) { o.batch = (uint32_t)atoi(s + 6); o.batch_set = true; }
            else if (starts(s, "chunk_reads=")) o.batch = (uint32_t)atoi(s + 12);       // byte-range chunks of about this many records (default 262144)
            else if (starts(s, "workers=")) o.workers = atoi(s + 8);
            else if (starts(s, "fmt_threads=")) o.fmt_threads = atoi(s + 12);
            else if (starts(s, "locate=")) o.locate_sampled = !strcmp(s + 7, "sampled");
            else if (starts(s, "sam_text=")) { o.sam_text_device = on_device("sam_text", s + 9); if (!o.sam_text_device) o.sam_text_host_set = true; }
            else if (starts(s, "read_text=")) o.read_text_device = on_device("read_text", s + 10);
            else if (starts(s, "track_text=")) o.track_text_device = on_device("track_text", s + 11);
            else if (starts(s, "sam_sort=")) {
                if (!strcmp(s + 9, "coordinate")) o.sam_sort = true;
                else if (!strcmp(s + 9, "none")) o.sam_sort = false;
                else { fprintf(stderr, "Error: --sam_sort takes none or coordinate, not: %s\n", s + 9); exit(1); }
            }
            else if (starts(s, "sam_format=")) {
                if (!strcmp(s + 11, "bam")) o.bam = true;
                else if (!strcmp(s + 11, "sam")) o.bam = false;
                else { fprintf(stderr, "Error: --sam_format takes sam or bam, not: %s\n", s + 11); exit(1); }
            }
            else if (starts(s, "bam_level=")) {
                if (strcmp(s + 10, "0") && strcmp(s + 10, "1")) { fprintf(stderr, "Error: --bam_level takes 0 or 1, not: %s\n", s + 10); exit(1); }
                o.bam_level = s[10] - '0'; o.bam_level_set = true;
            }
            else if (!strcmp(s, "bam_lz77")) o.bam_lz77 = true;
            else if (!strcmp(s, "bam_index")) o.bam_index = true;
            else if (!strcmp(s, "sam_unmapped")) o.sam_unmapped = true;
            else if (!strcmp(s, "sam_md")) o.sam_md = true;
            else if (starts(s, "sam_cigar=")) {
                if (strcmp(s + 10, "gnumap") && strcmp(s + 10, "forward")) { fprintf(stderr, "Error: --sam_cigar takes gnumap or forward, not \"%s\"\n", s + 10); exit(1); }
                o.sam_cigar_set = true; o.sam_cigar_forward = !strcmp(s + 10, "forward");
            }
            else if (starts(s, "sam_shards=")) {
                char* end = nullptr;
                const long k = strtol(s + 11, &end, 10);
                if (end == s + 11 || *end || k < 1 || k > 64) { fprintf(stderr, "Error: --sam_shards takes 1 .. 64, not: %s\n", s + 11); exit(1); }
                o.sam_shards = (int)k;
            }
            else if (starts(s, "mates=")) o.mates = s + 6;
            else if (!strcmp(s, "interleaved")) o.interleaved = true;
            else if (starts(s, "min_insert=") || starts(s, "max_insert=")) {
                char* end = nullptr;
                const unsigned long long v = strtoull(s + 11, &end, 10);
                if (end == s + 11 || *end || s[11] == '-' || v > 0xFFFFFFFFull) { fprintf(stderr, "Error: --%.10s takes a number of bases, not: %s\n", s, s + 11); exit(1); }
                (s[1] == 'i' ? o.min_insert : o.max_insert) = (uint32_t)v; o.insert_opt = s[1] == 'i' ? "--min_insert" : "--max_insert";
            }
            else if (!strcmp(s, "help")) usage(0, "");
            else { fprintf(stderr, "No matching arg in: %s\n", a); exit(1); }
            continue;
        }
        if (strlen(a) > 2) { fprintf(stderr, "Irregular Parameter in: %s\n", a); exit(1); }
        char c = a[1];
        // -u takes no value but the reference's parser consumes the next argv all the same (src/Driver.cpp:2768-2770 lacks the
        // count--): a command line written for the reference has a filler word there, so the same is done here
        bool flag = strchr("prbd0", c) != nullptr;
        const char* v = nullptr;
        if (!flag) { if (i + 1 >= argc) usage(1, "missing value"); v = argv[++i]; }
        switch (c) {
            case 'g': o.genome = v; break;
            case 'o': o.output = v; break;
            case 'a': o.p.align_score = (float)atof(v); break;
            case 'p': o.p.align_is_fraction = 1; break;
            case 'r': o.p.align_is_fraction = 0; break;
            case 'q': o.p.cutoff = (float)atof(v); break;
            case 'v': o.verbose = atoi(v); break;
            case 'c': o.threads = atoi(v); break;
            case 'm': o.p.mer = atoi(v); mer_set = true; break;
            case 'u': o.p.unique_only = 1; break;
            case 'T': o.p.max_matches = (uint32_t)atoi(v); break;
            case 'h': o.p.max_kmer_hits = (uint32_t)atoi(v); break;
            case 'G': o.p.gap = (float)atof(v); break;
            case 'M': o.p.max_gap = atoi(v); break;
            case 'b': o.p.mode = GM_MODE_BS; break;
            case 'd': o.p.mode = GM_MODE_ATOG; break;
            case '0': break;
            case 'j': o.p.jump = atoi(v); break;
            case 'k': o.p.min_seed_hits = atoi(v); break;
            case 'S': o.subst = v; break;
            case 'A': o.adaptor = v; break;                                     // Driver.cpp:2792-2798: exactly as given
            case 'l': case 'B': case 's': fprintf(stderr, "option -%c is outside the hot path of this build\n", c); exit(1);
            case '?': usage(0, "");
            default: fprintf(stderr, "Irregular Parameter in: %s\n", a); exit(1);
        }
    }
    if (o.reads.empty()) usage(1, "Specify a single file e.g., sequences.fa\n");
    if (o.genome.empty()) usage(1, "Specify a genome to map to with the -g flag\n");
    if (o.p.fast) { if (!mer_set) o.p.mer = 14; o.p.jump = o.p.mer; }      // Driver.cpp:1163-1171
    if ((o.p.mode == GM_MODE_BS || o.p.mode == GM_MODE_BS2) && !o.p.pos_strand) o.p.mode = GM_MODE_BS2;    // Driver.cpp:1260-1281
    if (o.p.mode == GM_MODE_ATOG && !o.p.pos_strand) o.p.mode = GM_MODE_ATOG2;
    if (gm_params_finalize(&o.p) != GM_OK) { fprintf(stderr, "%s\n", gm_last_error()); exit(1); }
    if (!o.subst.empty() && gm_params_load_subst(&o.p, o.subst.c_str()) != GM_OK) { fprintf(stderr, "ERROR: \n\t%s\n", gm_last_error()); exit(1); }
    if (o.vcf && o.p.mode != GM_MODE_SNP) { fprintf(stderr, "Error: --vcf writes the SNP calls of --snp: give --snp with --vcf\n"); exit(1); }
    if (o.adaptor.size() > 256) { fprintf(stderr, "Error: -A/--adaptor takes at most 256 characters\n"); exit(1); }
    if (o.gpus < 1) o.gpus = 1;
    if (o.sam_sort) {                                        // refused before a device is opened or a file is written
        if (o.sam_text_host_set) { fprintf(stderr, "Error: --sam_sort=coordinate sorts the rows the GPU formats: it cannot be combined with --sam_text=host\n"); exit(1); }
        if (o.sam_shards > 1) { fprintf(stderr, "Error: --sam_sort=coordinate writes one sorted <out>.sam: it cannot be combined with --sam_shards above 1\n"); exit(1); }
        if (o.gpus > 1) { fprintf(stderr, "Error: --sam_sort=coordinate sorts on one GPU: it cannot be combined with --gpus above 1 (there is no cross-device merge)\n"); exit(1); }
        o.sam_text_device = true;
    }
    if (o.bam_level_set && !o.bam) { fprintf(stderr, "Error: --bam_level sets the compression of --sam_format=bam: give --sam_format=bam with --bam_level\n"); exit(1); }
    if (o.bam_lz77 && !o.bam) { fprintf(stderr, "Error: --bam_lz77 sets the compression of --sam_format=bam: give --sam_format=bam with --bam_lz77\n"); exit(1); }
    if (o.bam_lz77 && o.bam_level == 0) { fprintf(stderr, "Error: --bam_lz77 adds matches to the Huffman-coded blocks of --bam_level=1: it cannot be combined with --bam_level=0\n"); exit(1); }
    if (o.bam_lz77) o.bam_level |= GM_BGZF_LZ77;
    if (o.bam_index && !o.bam) { fprintf(stderr, "Error: --bam_index writes the index of a sorted <out>.bam: give --sam_format=bam (and --sam_sort=coordinate) with --bam_index\n"); exit(1); }
    if (o.bam_index && !o.sam_sort) { fprintf(stderr, "Error: --bam_index indexes a coordinate-sorted file: give --sam_sort=coordinate with --bam_index\n"); exit(1); }
    if (o.bam) {                                             // refused before a device is opened or a file is written
        if (o.sam_text_host_set) { fprintf(stderr, "Error: --sam_format=bam writes the records on the GPU: it cannot be combined with --sam_text=host\n"); exit(1); }
        if (o.sam_shards > 1) { fprintf(stderr, "Error: --sam_format=bam writes one <out>.bam: it cannot be combined with --sam_shards above 1\n"); exit(1); }
        o.sam_text_device = true;
    }
    if (o.sam_md || o.sam_cigar_set) {                       // refused before a device is opened or a file is written
        const char* flag = o.sam_md ? "--sam_md" : "--sam_cigar";
        if (o.sam_text_host_set) { fprintf(stderr, "Error: %s is applied where the GPU writes the rows: it cannot be combined with --sam_text=host\n", flag); exit(1); }
        if (o.sam_md && !o.adaptor.empty()) {
            fprintf(stderr, "Error: --sam_md cannot be combined with -A/--adaptor: with an adaptor SEQ is the whole read and the CIGAR covers the kept part, "
                            "so NM / MD of the row as printed would describe nothing\n");
            exit(1);
        }
        o.sam_text_device = true;
    }
    if (o.sam_unmapped) {                                    // refused before a device is opened or a file is written
        if (o.sam_text_host_set) { fprintf(stderr, "Error: --sam_unmapped writes its rows on the GPU: it cannot be combined with --sam_text=host\n"); exit(1); }
        o.sam_text_device = true;
    }
    if (!o.mates.empty() && o.interleaved) { fprintf(stderr, "Error: --mates=FILE2 names a second file and --interleaved says there is none: give one of them\n"); exit(1); }
    if (o.insert_opt && !o.paired()) { fprintf(stderr, "Error: %s sets the insert limits of paired reads: give --mates=FILE2 or --interleaved with it\n", o.insert_opt); exit(1); }
    if (o.paired()) {                                        // refused before a device is opened or a file is written
        const char* flag = o.interleaved ? "--interleaved" : "--mates";
        if (o.min_insert > o.max_insert) { fprintf(stderr, "Error: --min_insert=%u is above --max_insert=%u\n", o.min_insert, o.max_insert); exit(1); }
        if (o.sam_text_host_set) { fprintf(stderr, "Error: %s resolves the pairs where the GPU writes the rows: it cannot be combined with --sam_text=host\n", flag); exit(1); }
        if (o.read_text_device) { fprintf(stderr, "Error: %s reads its files in file order on the host: it cannot be combined with --read_text=device\n", flag); exit(1); }
        if (o.batch_set && (o.batch & 1u)) { fprintf(stderr, "Error: %s needs blocks of whole pairs: --batch=%u is odd\n", flag, o.batch); exit(1); }
        o.sam_text_device = true;
    }
    if (o.batch < 1) o.batch = 1;
    if (o.paired() && (o.batch & 1u)) ++o.batch;            // (--chunk_reads: a block of whole pairs)
    if (o.workers < 1) o.workers = 1;
    if (o.fmt_threads < 1) o.fmt_threads = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
}

// page-locked host array (gm_host_alloc): the library's copies to and from it are DMA at link rate, no staging through the CPU
template <class T> struct PinVec {
    T* p = nullptr; size_t cap = 0;
    PinVec() = default;
    PinVec(const PinVec&) = delete; PinVec& operator=(const PinVec&) = delete;
    ~PinVec() { if (p) gm_host_free(p); }
    void ensure(size_t n) {                       // contents are NOT kept
        if (n <= cap) return;
        if (p) gm_host_free(p);
        cap = n + n / 8 + 64;
        p = (T*)gm_host_alloc(cap * sizeof(T));
        if (!p) { fprintf(stderr, "ERROR: out of page-locked host memory (%zu bytes)\n", cap * sizeof(T)); exit(1); }
    }
    T* data() { return p; } const T* data() const { return p; } size_t size() const { return cap; }
    T& operator[](size_t i) { return p[i]; } const T& operator[](size_t i) const { return p[i]; }
};

// SAM text of one formatter slice: plain bytes that are never value-initialised (std::string::resize would write every byte of the
// 8.7 GB of a 32 M-read run once before the formatter writes it again)
struct TextBuf {
    std::unique_ptr<char[]> p; size_t len = 0, cap = 0;
    void clear() { len = 0; }
    size_t size() const { return len; }
    const char* data() const { return p.get(); }
    char* room(size_t extra) {                        // at least `extra` writable bytes at the end
        if (len + extra > cap) {
            const size_t nc = std::max(len + extra, cap + cap / 2 + 4096);
            std::unique_ptr<char[]> q(new char[nc]);
            if (len) memcpy(q.get(), p.get(), len);
            p = std::move(q); cap = nc;
        }
        return p.get() + len;
    }
};

// --sam_text=device: the page-locked buffers gm_output_batch_text writes a block's rows into.  A worker takes one when its block reaches
// the output call, the writer gives it back once the rows are in the file: a handful are in use at a time, far fewer than there are
// Block objects (page-locking 80 MB costs tens of milliseconds, and a short run pays that for every buffer it ever touches).
struct TextPool {
    std::mutex mu; std::vector<std::unique_ptr<PinVec<char>>> idle;
    PinVec<char>* get() {
        { std::lock_guard<std::mutex> lk(mu); if (!idle.empty()) { PinVec<char>* p = idle.back().release(); idle.pop_back(); return p; } }
        return new PinVec<char>();
    }
    void put(PinVec<char>* p) { if (p) { std::lock_guard<std::mutex> lk(mu); idle.emplace_back(p); } }
};

// ---- blocks ------------------------------------------------------------------------------------------------------
struct Block {
    uint64_t index = 0;
    uint64_t sort_seq = 0;                  // --sam_sort: the block's sequence number in the sorter: (blocks before it in the run) << 21, the low bits order the halves of a split block
    uint32_t n = 0, maxlen = 0, stride = 8;
    // views into the memory-mapped FASTQ text (no per-read strings)
    std::vector<const char*> name, seq, qual;
    std::vector<uint32_t> name_len, qual_len;
    std::vector<uint16_t> len;
    std::vector<char> fa_text;              // FASTA: the joined sequence lines of the records that span several, and the QUAL strings the rows print (seq / qual point here)
    std::vector<uint16_t> kept;             // -A with --illumina: what the adaptor trim keeps of every read (the fallback scan sees only that); else empty
    // packed for gm_reads (page-locked)
    PinVec<uint8_t> bases, qbuf; PinVec<uint16_t> plen;
    // results of the two batch calls (page-locked)
    PinVec<gm_sam_rec> recs; PinVec<char> pool; uint64_t n_recs = 0;
    int gpu = 0;
    size_t text_lo = 0, text_hi = 0; bool lazy = false;   // chunk mode: the byte range of the FASTQ text a worker still has to cut into records
    int illumina = 0;                      // --illumina still in force when this block starts (the fallback is sticky, SeqReader.cpp:1171-1180)
    std::vector<TextBuf> text;              // SAM text, one piece per formatter thread
    // --sam_text=device: what gm_output_batch_text reads of the block besides bases and qualities, and the text it returns (page-locked)
    PinVec<char> names_pool, qtail_pool; PinVec<uint64_t> name_off, qtail_off; bool has_qtail = false;
    PinVec<char>* dtext = nullptr; uint64_t dtext_len = 0;      // from the TextPool, while the block holds rows that are not written yet
    size_t first_byte = 0;                  // where the block starts in the FASTQ text: decides its shard (--sam_shards)
    // --read_text=device: the block was cut on the GPU (gm_batch_upload_text) and is resident in its worker's batch; trecs = where its reads lie in
    // the text from text_lo on (page-locked; only filled for the host formatter)
    bool text_dev = false; PinVec<gm_text_rec> trecs;
    bool failed = false;
    std::unique_ptr<Block> mate_src[2];     // --mates=FILE2: the records of the two files this block's views alternate over (a FASTA record's joined lines live there)
    // what the three parsers share: no record, one more record (`head` = its name line with the '@' or '>'), the row stride behind the last
    void reset() { n = 0; maxlen = 0; name.clear(); seq.clear(); qual.clear(); name_len.clear(); qual_len.clear(); len.clear(); fa_text.clear(); }
    void append(const char* head, size_t head_len, const char* sq, size_t sl, const char* ql, size_t qll) {
        name.push_back(head + 1); name_len.push_back((uint32_t)(head_len - 1));
        seq.push_back(sq); len.push_back((uint16_t)sl); qual.push_back(ql); qual_len.push_back((uint32_t)qll);
        maxlen = std::max<uint32_t>(maxlen, (uint32_t)sl); ++n;
    }
    bool finish() { stride = std::max<uint32_t>(8, (maxlen + 7u) & ~7u); return n > 0; }
    // --illumina's fallback: a quality below '@' in what the adaptor trim keeps of the first `upto` reads (the reference's quality characters are signed chars)
    bool has_quality_below_64(uint32_t upto) const {
        for (uint32_t i = 0; i < upto; ++i)
            for (uint32_t t = 0; t < (kept.empty() ? len[i] : kept[i]); ++t) if ((signed char)qual[i][t] < 64) return true;
        return false;
    }
};

static void report_too_long(const char* head, size_t head_len) {      // the kernels' limit, not the reference's
    fprintf(stderr, "ERROR: read %.*s is longer than 2048 bases\n", (int)std::min<size_t>(head_len, 200), head);
}

template <class T> struct Queue {             // unbounded MPMC queue; the Block pool bounds what is in flight
    std::mutex mu; std::condition_variable cv; std::deque<T> q; bool closed = false;
    void push(T v) { { std::lock_guard<std::mutex> lk(mu); q.push_back(v); } cv.notify_one(); }
    bool pop(T& v) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !q.empty() || closed; });
        if (q.empty()) return false;
        v = q.front(); q.pop_front();
        return true;
    }
    void close() { { std::lock_guard<std::mutex> lk(mu); closed = true; } cv.notify_all(); }
};

// ---- FASTQ scanner (SeqReader::get_more_fastq src/SeqReader.cpp:1023-1292: 4-line records, blank lines before a name skipped)
struct FastqScanner {
    const char* base = nullptr; size_t size = 0, at = 0;
    int fd = -1; bool mapped = false; std::vector<char> heap;
    bool done = false;
    bool open(const std::string& fn) {
        fd = ::open(fn.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
            size = (size_t)st.st_size;
            if (size == 0) { base = ""; return true; }
            void* p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (p != MAP_FAILED) { base = (const char*)p; mapped = true; madvise(p, size, MADV_SEQUENTIAL); return true; }
        }
        char buf[1 << 16]; ssize_t k;                       // pipes and the like: slurp
        while ((k = ::read(fd, buf, sizeof buf)) > 0) heap.insert(heap.end(), buf, buf + k);
        base = heap.data(); size = heap.size();
        return true;
    }
    ~FastqScanner() { if (mapped) munmap((void*)base, size); if (fd >= 0) ::close(fd); }
    // Chunk mode: cut base[cur, limit) into records until max_reads (thread-safe: no scanner state).  Only well-formed records are
    // taken here; at the first one that is not, `stop` is set and `bad_at` is where its name line starts: the driver then reads the rest
    // of the input again from there in file order (parse_resync), because what the reference does with a malformed record depends on
    // the lines that follow it.  `too_long` = a read longer than the kernels take (this implementation's limit, not the reference's).
    static bool parse_range(const char* base, size_t& cur, size_t limit, Block& b, uint32_t max_reads, bool* stop, size_t* bad_at, bool* too_long) {
        b.reset();
        auto line = [&](const char*& p, size_t& len) -> bool {       // one line without its newline; false at the end of the range
            if (cur >= limit) return false;
            const char* s0 = base + cur;
            const char* e = (const char*)memchr(s0, '\n', limit - cur);
            if (!e) { p = s0; len = limit - cur; cur = limit; return true; }
            p = s0; len = (size_t)(e - s0); cur = (size_t)(e - base) + 1;
            return true;
        };
        while (b.n < max_reads) {
            const char *nm, *sq = nullptr, *pl = nullptr, *ql = nullptr; size_t nl, sl = 0, pll = 0, qll = 0;
            if (!line(nm, nl)) break;
            bool eof = false;
            while (nl == 0) { if (!line(nm, nl)) { eof = true; break; } }
            if (eof) break;
            const size_t rec_at = (size_t)(nm - base);
            const bool l2 = line(sq, sl), l3 = line(pl, pll), l4 = line(ql, qll);
            if (!l2 || !l3 || !l4 || nm[0] != '@' || pll == 0 || pl[0] != '+' || sl > qll) { *stop = true; *bad_at = rec_at; break; }
            if (sl > 2048) { report_too_long(nm, nl); *too_long = true; break; }
            b.append(nm, nl, sq, sl, ql, qll);
        }
        return b.finish();
    }
    // FASTA (SeqReader::get_more_fasta src/SeqReader.cpp:813-1018): a record runs from one '>' line to the next, the name is the whole
    // header line after '>', the sequence lines are joined.  base[cur, limit) starts at a '>' (the whole input was checked by
    // fasta_check before anything was mapped).  QUAL is str2qual's string (fasta_qual): the host formatter prints it from the block.
    static bool parse_range_fasta(const char* base, size_t& cur, size_t limit, Block& b, uint32_t max_reads, bool* too_long, const char* qual_of) {
        b.reset();
        std::vector<size_t> seq_at, qual_at;                // offsets into fa_text (npos: a one-line sequence, printed from the mapping)
        std::vector<const char*> one_line;
        const size_t npos = ~(size_t)0;
        while (b.n < max_reads && cur < limit) {
            const char* hd = base + cur;
            const char* e = (const char*)memchr(hd, '\n', limit - cur);
            const size_t hl = e ? (size_t)(e - hd) : limit - cur;
            cur = e ? (size_t)(e - base) + 1 : limit;
            // sequence lines up to the next header
            const char* first = nullptr; size_t first_len = 0, total = 0; int lines = 0; size_t joined_at = npos;
            while (cur < limit && base[cur] != '>') {
                const char* l = base + cur;
                const char* le = (const char*)memchr(l, '\n', limit - cur);
                const size_t ll = le ? (size_t)(le - l) : limit - cur;
                cur = le ? (size_t)(le - base) + 1 : limit;
                if (ll == 0) continue;
                if (lines == 0) { first = l; first_len = ll; }
                else {
                    if (lines == 1) { joined_at = b.fa_text.size(); b.fa_text.insert(b.fa_text.end(), first, first + first_len); }
                    b.fa_text.insert(b.fa_text.end(), l, l + ll);
                }
                total += ll; ++lines;
            }
            if (total > 2048) { report_too_long(hd, hl); *too_long = true; break; }
            b.append(hd, hl, nullptr, total, nullptr, total);      // (the views follow below)
            one_line.push_back(first ? first : hd); seq_at.push_back(joined_at);
        }
        // the QUAL strings behind the joined sequences, then the views (fa_text does not move any more)
        qual_at.resize(b.n);
        for (uint32_t i = 0; i < b.n; ++i) { qual_at[i] = b.fa_text.size(); b.fa_text.resize(b.fa_text.size() + b.len[i]); }
        for (uint32_t i = 0; i < b.n; ++i) {
            b.seq[i] = seq_at[i] == npos ? one_line[i] : b.fa_text.data() + seq_at[i];
            char* q = b.fa_text.data() + qual_at[i];
            for (uint32_t t = 0; t < b.len[i]; ++t) q[t] = qual_of[(unsigned char)b.seq[i][t]];
            b.qual[i] = q;
        }
        return b.finish();
    }
    bool fasta = false; const char* fasta_qual = nullptr;    // set by main() for a FASTA input
    // File order, with the recovery of SeqReader::get_more_fastq (src/SeqReader.cpp:1060-1150): four lines are read; while the first does
    // not start with '@' or the third not with '+', the lines are shifted up by one and one more is read; a quality line shorter than
    // its sequence makes the reader take the next four lines instead.  The lines come from std::getline on an ifstream, whose end-of-input
    // behaviour decides what happens to a record the input ends in: a stream that is no longer good fails WITHOUT touching the string,
    // the end of input empties the string and sets eofbit + failbit, a last line without a newline is delivered and sets eofbit; every
    // end-of-input test inside the recovery ends the input (a record completed by a line without a newline is lost there).
    struct Line { const char* p = ""; size_t n = 0; char first() const { return n ? p[0] : 0; } };
    bool rs_eof = false, rs_fail = false;
    void rs_getline(Line& s) {
        if (rs_eof || rs_fail) { rs_fail = true; return; }
        if (at >= size) { s = Line(); rs_eof = rs_fail = true; return; }
        const char* s0 = base + at;
        const char* e = (const char*)memchr(s0, '\n', size - at);
        s.p = s0;
        if (e) { s.n = (size_t)(e - s0); at = (size_t)(e - base) + 1; } else { s.n = size - at; at = size; rs_eof = true; }
    }
    bool parse_resync(Block& b, uint32_t max_reads, bool* too_long) {
        b.reset();
        Line name, seq, plus, qual;
        while (b.n < max_reads) {
            if (rs_eof) { done = true; break; }                                               // :1061
            rs_getline(name);
            while (name.n == 0 && !rs_eof) rs_getline(name);                                  // blank lines before a name :1076-1079
            if (rs_eof) { done = true; break; }                                               // :1082
            rs_getline(seq); rs_getline(plus); rs_getline(qual);
            while (name.first() != '@' || plus.first() != '+' || seq.n > qual.n) {            // :1095
                fprintf(stderr, "--Found error...atteming to resolve...\n");
                if (name.first() != '@' || plus.first() != '+') {
                    fprintf(stderr, "--ERROR at sequence %.*s (name[s] formatted incorrectly)\n\tTrying to recover...\n", (int)std::min<size_t>(name.n, 200), name.p);
                    while ((name.first() != '@' || plus.first() != '+') && !rs_eof) {         // :1101-1115
                        name = seq; seq = plus; plus = qual; rs_getline(qual);
                        if (rs_eof) { done = true; break; }
                    }
                    if (done || rs_eof) { done = true; break; }
                }
                if (seq.n > qual.n) {                                                         // :1128-1142
                    fprintf(stderr, "--ERROR at sequence %.*s (length of fastq and sequence not equal)\n\tTrying to recover...\n", (int)std::min<size_t>(name.n, 200), name.p);
                    rs_getline(name); rs_getline(seq); rs_getline(plus); rs_getline(qual);
                    if (rs_eof) { done = true; break; }
                }
            }
            if (done) break;
            if (seq.n > 2048) { report_too_long(name.p, name.n); *too_long = true; done = true; break; }
            b.append(name.p, name.n, seq.p, seq.n, qual.p, qual.n);
        }
        return b.finish();
    }
    bool next(Block& b, uint32_t max_reads, bool* too_long) {    // file-order mode: blocks of exactly max_reads reads
        if (done) return false;
        if (fasta) {
            const bool got = parse_range_fasta(base, at, size, b, max_reads, too_long, fasta_qual);
            if (at >= size || *too_long) done = true;
            return got;
        }
        return parse_resync(b, max_reads, too_long);
    }
    // chunk mode: the start of the first record at or after `off` (a line starting with '@' whose next-but-one line starts with
    // '+': a quality line may start with '@' too, but then the line two below is a sequence, never '+')
    size_t record_start(size_t off) const {
        if (off == 0) return 0;
        if (off >= size) return size;
        const char* e = (const char*)memchr(base + off - 1, '\n', size - off + 1);      // the line containing off-1 ends here
        size_t p = e ? (size_t)(e - base) + 1 : size;
        while (fasta && p < size) {                          // FASTA: the next line that starts with '>'
            if (base[p] == '>') return p;
            const char* l1 = (const char*)memchr(base + p, '\n', size - p);
            if (!l1) return size;
            p = (size_t)(l1 - base) + 1;
        }
        while (p < size) {
            const char* l1 = (const char*)memchr(base + p, '\n', size - p);
            if (!l1) return size;
            const char* l2 = (const char*)memchr(l1 + 1, '\n', size - (size_t)(l1 + 1 - base));
            if (!l2) return size;
            if (base[p] == '@' && (size_t)(l2 + 1 - base) < size && l2[1] == '+') return p;
            p = (size_t)(l1 - base) + 1;
        }
        return size;
    }
    size_t chunk_bytes = 0;
    bool next_chunk(Block& b, uint32_t target_reads) {       // a byte range of about target_reads records, cut at record starts
        if (done || at >= size) { done = true; return false; }
        if (!chunk_bytes) {                                  // record size from the first records of the file
            size_t p = 0; uint32_t recs = 0;
            while (recs < 4000 && p < size) { const char* e = (const char*)memchr(base + p, '\n', size - p); if (!e) break; p = (size_t)(e - base) + 1; ++recs; }
            if (fasta) { uint32_t hd = 0; for (size_t q = 0; q < p; ++q) hd += base[q] == '>' && (q == 0 || base[q - 1] == '\n'); recs = 4 * std::max<uint32_t>(hd, 1u); }
            const double per_rec = recs >= 4 ? (double)p / (recs / 4) : 256.0;
            chunk_bytes = (size_t)std::max(4096.0, per_rec * target_reads);
        }
        const size_t lo = at, hi = record_start(std::min(size, at + chunk_bytes));
        b.text_lo = lo; b.text_hi = hi > lo ? hi : size; b.lazy = true; b.n = 0;
        at = b.text_hi;
        if (at >= size) done = true;
        return true;
    }
};

template <class F> static void run_slices(uint32_t n, int threads, uint32_t grain, F&& fn) {          // fn(slice, lo, hi)
    int T = (int)std::min<uint64_t>((uint64_t)threads, std::max<uint32_t>(1, n / std::max<uint32_t>(1, grain)));
    if (T <= 1) { fn(0, 0u, n); return; }
    const uint64_t per = (n + (uint64_t)T - 1) / (uint64_t)T;
    std::vector<std::thread> th;
    for (int s = 1; s < T; ++s)
        th.emplace_back([&, s] { fn(s, (uint32_t)std::min<uint64_t>(n, s * per), (uint32_t)std::min<uint64_t>(n, (s + 1) * per)); });
    fn(0, 0u, (uint32_t)std::min<uint64_t>(n, per));
    for (auto& x : th) x.join();
}

// with_text: also the names (cut to what a row prints of them) and the rare quality tails, back to back, for gm_read_text
// fasta: the letters only (gm_reads.quals is not read for a FASTA block)
static void pack_block(Block& b, int threads, bool with_text, bool fasta) {          // rows of `stride` bytes, zero padded, as gm_reads wants them
    const size_t bytes = (size_t)b.n * b.stride;
    b.bases.ensure(bytes); if (!fasta) b.qbuf.ensure(bytes);
    b.plen.ensure(b.n);
    memcpy(b.plen.data(), b.len.data(), (size_t)b.n * 2);
    if (with_text) {
        b.name_off.ensure((size_t)b.n + 1); b.qtail_off.ensure((size_t)b.n + 1);
        uint64_t no = 0, qo = 0;
        for (uint32_t i = 0; i < b.n; ++i) {
            b.name_off[i] = no; b.qtail_off[i] = qo;
            no += std::min<uint32_t>(b.name_len[i], MAX_NAME_SZ - 1);
            qo += b.qual_len[i] > b.len[i] ? b.qual_len[i] - b.len[i] : 0u;
        }
        b.name_off[b.n] = no; b.qtail_off[b.n] = qo;
        b.has_qtail = qo != 0;
        b.names_pool.ensure((size_t)no + 1); b.qtail_pool.ensure((size_t)qo + 1);
        run_slices(b.n, threads, 8192, [&](int, uint32_t lo, uint32_t hi) {
            for (uint32_t i = lo; i < hi; ++i) {
                memcpy(&b.names_pool[(size_t)b.name_off[i]], b.name[i], (size_t)(b.name_off[i + 1] - b.name_off[i]));
                if (b.qtail_off[i + 1] > b.qtail_off[i]) memcpy(&b.qtail_pool[(size_t)b.qtail_off[i]], b.qual[i] + b.len[i], (size_t)(b.qtail_off[i + 1] - b.qtail_off[i]));
            }
        });
    }
    run_slices(b.n, threads, 8192, [&](int, uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i) {
            uint8_t* pb = &b.bases[(size_t)i * b.stride];
            const uint32_t L = b.len[i];
            memcpy(pb, b.seq[i], L); memset(pb + L, 0, b.stride - L);
            if (fasta) continue;
            uint8_t* pq = &b.qbuf[(size_t)i * b.stride];
            memcpy(pq, b.qual[i], L); memset(pq + L, 0, b.stride - L);
        }
    });
}

// ---- SAM text (src/Driver.cpp:2146-2217) ---------------------------------------------------------------------------
static inline char comp_char(char c) {                   // reverse_comp, SequenceOperations.h:56-96
    switch (c) {
        case 'a': return 't'; case 'A': return 'T'; case 't': return 'a'; case 'T': return 'A';
        case 'c': return 'g'; case 'C': return 'G'; case 'g': return 'c'; case 'G': return 'C';
        case '-': return '-'; default: return 'n';
    }
}

static size_t reverse_cigar(const char* s, char* out) {  // SequenceOperations.h:109-123 (':' counts as a digit there, 48..58)
    const size_t n = strlen(s);
    size_t w = n, tok = 0;
    for (size_t i = 0; i < n; ++i) {
        if (s[i] >= 48 && s[i] <= 58) continue;
        const size_t len = i + 1 - tok;                    // digits + the operation character
        w -= len;
        memcpy(out + w, s + tok, len);
        tok = i + 1;
    }
    // trailing digits without an operation are dropped by the reference
    const size_t used = n - w;
    memmove(out, out + w, used);
    return used;
}

static const struct CompLut { char t[256]; CompLut() { for (int c = 0; c < 256; ++c) t[c] = comp_char((char)c); } } g_comp;

// dst[0..n) = src[n-1..0], 8 bytes at a time
static inline void reverse_bytes(char* dst, const char* src, uint32_t n) {
    uint32_t k = 0;
    for (; k + 8 <= n; k += 8) { uint64_t x; memcpy(&x, src + n - 8 - k, 8); x = __builtin_bswap64(x); memcpy(dst + k, &x, 8); }
    for (; k < n; ++k) dst[k] = src[n - 1 - k];
}

static void format_sam(TextBuf& out, const gm_index* ix, const gm_params& p, const gm_sam_rec& r, const char* cigar, const Block& b) {
    const uint32_t i = r.read;
    const uint32_t L = b.len[i], QL = b.qual_len[i];
    const uint32_t nl = std::min<uint32_t>(b.name_len[i], MAX_NAME_SZ - 1);
    const char* cn = gm_index_contig_name(ix, r.contig);
    const size_t cl = strlen(cn), gl = strlen(cigar);
    char* const w0 = out.room(nl + cl + gl + L + QL + 160);
    char* w = w0;
    memcpy(w, b.name[i], nl); w += nl;
    if (r.strand == GM_POS_STRAND) { memcpy(w, "\t0\t", 3); w += 3; } else { memcpy(w, "\t16\t", 4); w += 4; }
    memcpy(w, cn, cl); w += cl;
    *w++ = '\t'; w = gm_put_u64(w, r.chr_pos); *w++ = '\t';
    if (r.mapq < 0) { *w++ = '-'; w = gm_put_u64(w, (uint64_t)(-(int64_t)r.mapq)); } else w = gm_put_u64(w, (uint64_t)r.mapq);
    *w++ = '\t';
    if (r.strand == GM_POS_STRAND) {
        memcpy(w, cigar, gl); w += gl;
        memcpy(w, "\t*\t0\t0\t", 7); w += 7;
        memcpy(w, b.seq[i], L); w += L; *w++ = '\t';
        memcpy(w, b.qual[i], QL); w += QL; *w++ = '\t';
    } else {
        w += reverse_cigar(cigar, w);
        memcpy(w, "\t*\t0\t0\t", 7); w += 7;
        reverse_bytes(w, b.seq[i], L);
        for (uint32_t k = 0; k < L; ++k) w[k] = g_comp.t[(unsigned char)w[k]];
        w += L; *w++ = '\t';
        reverse_bytes(w, b.qual[i], QL);
        w += QL; *w++ = '\t';
    }
    // "XA:f:%g\tXP:f:%g\tX0:i:%d\n" (gm_fmt.h: exactly printf's %g)
    memcpy(w, "XA:f:", 5); w += 5;
    w = gm_put_g6(w, (double)(float)r.a_score * (1.0 / p.adjust));
    memcpy(w, "\tXP:f:", 6); w += 6;
    if (r.post_prob == 1.0f) *w++ = '1'; else w = gm_put_g6(w, (double)(float)r.post_prob);
    memcpy(w, "\tX0:i:", 6); w += 6;
    if (r.sim_matches < 0) { *w++ = '-'; w = gm_put_u64(w, (uint64_t)(-(int64_t)r.sim_matches)); } else w = gm_put_u64(w, (uint64_t)r.sim_matches);
    *w++ = '\n';
    out.len += (size_t)(w - w0);
}

// ---- FASTA reads --------------------------------------------------------------------------------------------------
// bases in the row of a sequence character (get_more_fasta src/SeqReader.cpp:884-950), 0 = not one of the 15 letters
static int fasta_row_bases(unsigned char c) {
    switch (tolower(c)) {
        case 'a': case 'c': case 'g': case 't': return 1;
        case 'r': case 'y': case 'k': case 'm': case 's': case 'w': return 2;
        case 'b': case 'd': case 'h': case 'v': return 3;
        case 'n': return 4;
        default: return 0;
    }
}
// str2qual (inc/SequenceOperations.h:193-217): the QUAL character of every letter, from the largest entry of its row
static void fasta_qual_table(char* t /* 256 */) {
    static const double share[5] = { 0.0, 1.0, 0.5, 1.0 / 3.0, 0.25 };
    const double MAX_PRB = 0.9999;
    for (int c = 0; c < 256; ++c) {
        const float pmax = (float)share[fasta_row_bases((unsigned char)c)];
        t[c] = pmax > MAX_PRB ? (char)((-10 * log(1 - MAX_PRB) / log(10.)) + 33) : (char)((-10 * log(1 - pmax) / log(10)) + 33);
    }
}
// The whole input, once, before anything is mapped: every record has a sequence of the 15 letters.  The reference skips CR, space, VT and
// FF inside a sequence when it builds the rows but keeps them in the text it prints and seeds from, so rows and text fall out of step
// there; this driver refuses such a file instead.  Blank lines inside a record are skipped, here and in
// parse_range_fasta (the reference appends their nothing).  One serial pass at memory rate: a table look-up per byte.
static bool fasta_check(const char* base, size_t size, const char* fn) {
    size_t at = 0, rec = 0, hd_at = 0, seq_len = 0;
    bool letter[256];
    for (int c = 0; c < 256; ++c) letter[c] = fasta_row_bases((unsigned char)c) != 0;
    auto name = [&](size_t h) { const char* e = (const char*)memchr(base + h, '\n', size - h); return std::string(base + h, std::min<size_t>(e ? (size_t)(e - (base + h)) : size - h, 200)); };
    while (at < size) {
        const char* l = base + at;
        const char* e = (const char*)memchr(l, '\n', size - at);
        const size_t ll = e ? (size_t)(e - l) : size - at;
        if (ll && l[0] == '>') {
            if (rec && !seq_len) { fprintf(stderr, "ERROR: %s: FASTA record %s has no sequence\n", fn, name(hd_at).c_str()); return false; }
            ++rec; hd_at = at; seq_len = 0;
        } else {
            for (size_t k = 0; k < ll; ++k) {
                const unsigned char c = (unsigned char)l[k];
                if (letter[c]) continue;
                if (c == '\r' || c == ' ' || c == 11 || c == 12)
                    fprintf(stderr, "ERROR: %s: FASTA record %s: white space (CR, space, VT or FF) inside a sequence line is not supported\n", fn, name(hd_at).c_str());
                else
                    fprintf(stderr, "ERROR: %s: FASTA record %s: sequence character '%c' (%d) at position %zu is not one of the 15 letters acgtnrykmswbdhv\n", fn,
                            name(hd_at).c_str(), c >= 32 && c < 127 ? c : '?', (int)c, seq_len + k);
                return false;
            }
            seq_len += ll;
        }
        at = e ? (size_t)(e - base) + 1 : size;
    }
    if (rec && !seq_len) { fprintf(stderr, "ERROR: %s: FASTA record %s has no sequence\n", fn, name(hd_at).c_str()); return false; }
    return true;
}

// ---- per worker: the two batch calls ---------------------------------------------------------------------------------
using Clock = std::chrono::steady_clock;
static double secs_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
static double secs_since(Clock::time_point t0) { return secs_between(t0, Clock::now()); }

static int fail() { fprintf(stderr, "ERROR: %s\n", gm_last_error()); return 1; }

struct Worker {
    int gpu = 0;
    gm_index* ix = nullptr;
    gm_batch* batch = nullptr;
    void* stream = nullptr;                 // this worker's own HIP stream: its device work overlaps the other workers'
    TextPool* text_pool = nullptr;
    PinVec<int8_t> status; PinVec<float> self_score; PinVec<double> top, den; PinVec<uint64_t> mbegin;
    PinVec<gm_match> matches; PinVec<gm_pos> positions;
    uint64_t n_reads = 0, n_matched = 0, n_records = 0;
    uint64_t n_unmapped = 0;                // --sam_unmapped: rows of reads without a record, among n_records (or among the sorter's rows)
    gm_mate_stats mates{};                  // --mates / --interleaved: the pair counters of this worker's blocks
    double t_pack = 0, t_map = 0, t_out = 0, t_scan = 0;
    gm_sam_sorter* sorter = nullptr;       // --sam_sort=coordinate: where the blocks' rows go instead of a host buffer
    TextPool* stage_pool = nullptr;         // --read_text=device: page-locked buffers a block's FASTQ text is copied into for the upload
    // the result arrays of a block of n reads, and a gm_hits that points at them (filled again after a capacity retry has made them grow)
    void ensure_hits(uint32_t n) {
        status.ensure(n); self_score.ensure(n); top.ensure(n); den.ensure(n); mbegin.ensure((size_t)n + 1);
        matches.ensure(2 * (size_t)n + 64); positions.ensure(2 * (size_t)n + 64);
    }
    void fill(gm_hits& h, uint32_t n) {
        h.n = n; h.status = status.data(); h.self_score = self_score.data(); h.top_score = top.data();
        h.denominator = den.data(); h.match_begin = mbegin.data();
        h.matches = matches.data(); h.matches_cap = matches.size();
        h.positions = positions.data(); h.positions_cap = positions.size();
    }
};

// --read_text=device, before the gate: the block's byte range goes up as it stands and the GPU cuts it (gm_batch_upload_text).  What the host
// parser would have reported comes back: the records in front of the first malformed (or too long) one, and where that one starts
static int upload_text_block(Worker& w, const Options& o, const char* base, Block& b, bool* stop, size_t* bad_at, bool* too_long) {
    const size_t bytes = b.text_hi - b.text_lo;
    auto c0 = Clock::now();
    PinVec<char>* stage = w.stage_pool->get();
    stage->ensure(bytes + 1);
    memcpy(stage->data(), base + b.text_lo, bytes);
    auto c1 = Clock::now();
    const bool want_recs = !o.sam_text_device;          // the host formatter prints names, bases and qualities from the mapped file
    if (want_recs) b.trecs.ensure(bytes / 128 + 64);
    gm_text_info ti;
    int rc;
    for (;;) {
        rc = gm_batch_upload_text(w.batch, &o.p, stage->data(), bytes, &ti, want_recs ? b.trecs.data() : nullptr, want_recs ? b.trecs.size() : 0, w.stream);
        if (rc == GM_E_CAPACITY) { b.trecs.ensure((size_t)ti.n + 64); continue; }
        break;
    }
    w.stage_pool->put(stage);
    w.t_pack += secs_between(c0, c1); w.t_map += secs_since(c1);
    if (rc != GM_OK) { fprintf(stderr, "ERROR: gm_batch_upload_text: %s\n", gm_last_error()); return rc; }
    b.n = ti.n; b.maxlen = ti.max_len; b.stride = ti.stride; b.text_dev = true;
    if (ti.status == GM_TEXT_MALFORMED) { *stop = true; *bad_at = b.text_lo + (size_t)ti.bad_at; }
    if (ti.status == GM_TEXT_TOO_LONG) {
        const char* nm = base + b.text_lo + (size_t)ti.bad_at;
        const char* e = (const char*)memchr(nm, '\n', b.text_hi - (b.text_lo + (size_t)ti.bad_at));
        report_too_long(nm, e ? (size_t)(e - nm) : b.text_hi - (b.text_lo + (size_t)ti.bad_at));
        *too_long = true;
    }
    return GM_OK;
}

// a batch call that did not return GM_OK: a block too large for one launch is no error (process_block_split takes it in halves)
static int batch_call_failed(int rc, const char* call, bool output, uint32_t n) {
    if (rc == GM_E_BATCH_TOO_LARGE)
        fprintf(stderr, output ? "note: block of %u reads is written in halves (%s)\n" : "note: block of %u reads is mapped in halves (%s)\n", n, gm_last_error());
    else fprintf(stderr, "ERROR: %s: %s\n", call, gm_last_error());
    return rc;
}

// The two batch calls of one block.  A block the host cut (parse_range*, parse_resync) is packed into rows here; a block gm_batch_upload_text
// left resident in the worker's batch (b.text_dev) has its rows and names in HBM already, and every call takes its _text / _resident form.
// The rows go to the sorter, come back as text, or come back as records for the host formatter - which reads a resident block's names,
// bases and qualities in the mapped file through the gm_text_rec table.
static int process_block(Worker& w, const Options& o, const char* base, Block& b) {
    const uint32_t n = b.n;
    const bool resident = b.text_dev;
    gm_params bp = o.p; bp.illumina = b.illumina;
    auto c0 = Clock::now();
    gm_reads reads{}; reads.n = n; reads.stride = b.stride;      // (all a call reads of it for a resident block)
    gm_read_text rt{};
    if (!resident) {
        pack_block(b, 4, o.sam_text_device, o.fasta);
        reads.bases = b.bases.data(); reads.quals = o.fasta ? nullptr : b.qbuf.data(); reads.len = b.plen.data();
        if (o.sam_text_device) {
            rt.names = b.names_pool.data(); rt.name_off = b.name_off.data();
            rt.qual_tail = b.has_qtail ? b.qtail_pool.data() : nullptr; rt.qual_tail_off = b.has_qtail ? b.qtail_off.data() : nullptr;
        }
    }
    w.ensure_hits(n);
    gm_hits hits{};
    auto c1 = Clock::now();
    int rc;
    for (;;) {
        w.fill(hits, n);
        rc = resident ? gm_map_batch_text(w.ix, &bp, w.batch, &hits, w.stream) : gm_map_batch(w.ix, &bp, w.batch, &reads, &hits, w.stream);
        if (rc != GM_E_CAPACITY) break;
        w.matches.ensure(hits.matches_cap + 64); w.positions.ensure(hits.positions_cap + 64);
    }
    if (rc != GM_OK) return batch_call_failed(rc, resident ? "gm_map_batch_text" : "gm_map_batch", false, n);
    auto c2 = Clock::now();
    uint64_t n_recs = 0, text_len = 0;
    const char* call;
    if (o.sam_sort) {                                       // the rows stay in HBM; their number is known when the sorter finishes
        call = resident ? "gm_output_batch_sorted_resident" : "gm_output_batch_sorted";
        rc = resident ? gm_output_batch_sorted_resident(w.ix, &bp, w.batch, &hits, w.sorter, b.sort_seq, w.stream)
                      : gm_output_batch_sorted(w.ix, &bp, w.batch, &reads, &rt, &hits, w.sorter, b.sort_seq, w.stream);
    } else if (o.sam_text_device) {                         // the rows come back as text: no records, no CIGAR pool on the host
        call = o.bam ? (resident ? "gm_output_batch_bam_resident" : "gm_output_batch_bam") : resident ? "gm_output_batch_text_resident" : "gm_output_batch_text";
        if (!b.dtext) b.dtext = w.text_pool->get();
        const size_t name_bytes = resident ? b.text_hi - b.text_lo : (size_t)b.name_off[n];
        b.dtext->ensure(((size_t)n + (size_t)n / 16) * (2 * (size_t)b.maxlen + 64) + name_bytes + 4096);
        if (o.bam) {                                        // the block's records as BGZF blocks: its run of <out>.bam
            gm_bam_out bo{};
            for (;;) {
                bo.data = b.dtext->data(); bo.cap = b.dtext->size(); bo.level = o.bam_level;
                rc = resident ? gm_output_batch_bam_resident(w.ix, &bp, w.batch, &hits, &bo, w.stream)
                              : gm_output_batch_bam(w.ix, &bp, w.batch, &reads, &rt, &hits, &bo, w.stream);
                if (rc != GM_E_CAPACITY) break;
                b.dtext->ensure((size_t)bo.cap + 64);
            }
            n_recs = bo.n_recs; text_len = bo.len;
        } else {
            gm_sam_text st;
            for (;;) {
                st.text = b.dtext->data(); st.text_cap = b.dtext->size(); st.text_len = 0; st.n_recs = 0; st.row_off = nullptr; st.row_cap = 0;
                rc = resident ? gm_output_batch_text_resident(w.ix, &bp, w.batch, &hits, &st, w.stream)
                              : gm_output_batch_text(w.ix, &bp, w.batch, &reads, &rt, &hits, &st, w.stream);
                if (rc != GM_E_CAPACITY) break;
                b.dtext->ensure((size_t)st.text_cap + 64);
            }
            n_recs = st.n_recs; text_len = st.text_len;
        }
    } else {
        call = "gm_output_batch";
        if (resident) {
            const char* t0 = base + b.text_lo;
            b.name.resize(n); b.seq.resize(n); b.qual.resize(n); b.name_len.resize(n); b.qual_len.resize(n); b.len.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                const gm_text_rec& r = b.trecs[i];
                b.name[i] = t0 + r.name_off; b.seq[i] = t0 + r.seq_off; b.qual[i] = t0 + r.qual_off;
                b.name_len[i] = r.name_len; b.qual_len[i] = r.qual_len; b.len[i] = (uint16_t)r.seq_len;
            }
        }
        b.recs.ensure((size_t)n + (size_t)n / 4 + 64);
        b.pool.ensure(8 * (size_t)n + 1024);
        gm_sam_out so;
        for (;;) {
            so.recs = b.recs.data(); so.recs_cap = b.recs.size(); so.cigar_pool = b.pool.data(); so.cigar_cap = b.pool.size();
            rc = gm_output_batch(w.ix, &bp, w.batch, &reads, &hits, &so, w.stream);
            if (rc != GM_E_CAPACITY) break;
            b.recs.ensure(so.recs_cap + 64); b.pool.ensure(so.cigar_cap + 64);
        }
        n_recs = so.n_recs;
    }
    if (rc != GM_OK) return batch_call_failed(rc, call, true, n);        // (nothing is booked: the halves book themselves)
    b.n_recs = n_recs; b.dtext_len = text_len; b.gpu = w.gpu;
    w.t_pack += secs_between(c0, c1); w.t_map += secs_between(c1, c2); w.t_out += secs_since(c2);
    w.n_reads += n; w.n_records += n_recs;                  // (sorted: no records here, main takes their number from the sorter)
    if (o.sam_unmapped) { uint64_t u = 0; if (gm_batch_unmapped_rows(w.batch, &u) == GM_OK) w.n_unmapped += u; }
    if (o.paired()) {
        gm_mate_stats ms;
        if (gm_batch_mate_stats(w.batch, &ms) == GM_OK) {
            w.mates.pairs += ms.pairs; w.mates.both_mapped += ms.both_mapped; w.mates.proper += ms.proper; w.mates.one_mapped += ms.one_mapped; w.mates.none_mapped += ms.none_mapped;
        }
    }
    for (uint32_t i = 0; i < n; ++i) w.n_matched += (w.status[i] == GM_READ_OK || w.status[i] == GM_READ_TOO_MANY);
    return GM_OK;
}

// a block whose intermediate lists outgrow one launch (GM_E_BATCH_TOO_LARGE: e.g. > 2^31 candidates on a repeat-rich reference
// without -h) is mapped as two halves, recursively; the halves' records are put back together in read order
static int process_block_split(Worker& w, const Options& o, const char* base, Block& b, int depth) {
    int rc = process_block(w, o, base, b);
    if (rc != GM_E_BATCH_TOO_LARGE || b.n < (o.paired() ? 4u : 2u) || depth > 20) return rc;
    if (b.text_dev) {                                       // a text block that is too large: the host parser cuts the same records, and the halves go the host's way
        size_t cur = b.text_lo, bad_at = 0; bool stop = false, too_long = false;
        const uint32_t n_dev = b.n;
        FastqScanner::parse_range(base, cur, b.text_hi, b, n_dev, &stop, &bad_at, &too_long);
        b.text_dev = false;
        if (b.n != n_dev) { fprintf(stderr, "ERROR: the host parser finds %u reads where the device found %u\n", b.n, n_dev); return GM_E_ARG; }
    }
    const uint32_t half = o.paired() ? (b.n / 2) & ~1u : b.n / 2;      // (paired: a pair never straddles the halves)
    uint64_t total = 0; size_t pool_len = 0;
    std::vector<gm_sam_rec> recs; std::vector<char> pool, text;
    for (int part = 0; part < 2; ++part) {
        const uint32_t lo = part ? half : 0, hi = part ? b.n : half;
        Block c;
        c.index = b.index; c.sort_seq = b.sort_seq | (uint64_t)part << (20 - depth); c.n = hi - lo; c.maxlen = b.maxlen; c.stride = b.stride; c.illumina = b.illumina;
        c.name.assign(b.name.begin() + lo, b.name.begin() + hi); c.seq.assign(b.seq.begin() + lo, b.seq.begin() + hi);
        c.qual.assign(b.qual.begin() + lo, b.qual.begin() + hi); c.name_len.assign(b.name_len.begin() + lo, b.name_len.begin() + hi);
        c.qual_len.assign(b.qual_len.begin() + lo, b.qual_len.begin() + hi); c.len.assign(b.len.begin() + lo, b.len.begin() + hi);
        if (!b.kept.empty()) c.kept.assign(b.kept.begin() + lo, b.kept.begin() + hi);
        if (part && b.illumina && b.has_quality_below_64(half)) c.illumina = 0;      // the fallback may have happened inside the first half
        rc = process_block_split(w, o, base, c, depth + 1);
        if (rc != GM_OK) { w.text_pool->put(c.dtext); return rc; }
        if (o.sam_text_device) {                            // rows are text already: the halves' text, one behind the other
            if (c.dtext) { text.insert(text.end(), c.dtext->data(), c.dtext->data() + c.dtext_len); w.text_pool->put(c.dtext); c.dtext = nullptr; }
            total += c.n_recs;
            continue;
        }
        for (uint64_t k = 0; k < c.n_recs; ++k) { gm_sam_rec r = c.recs[k]; r.read += lo; r.cigar_off += (uint32_t)pool_len; recs.push_back(r); }
        size_t used = 0;
        for (uint64_t k = 0; k < c.n_recs; ++k) used = std::max<size_t>(used, c.recs[k].cigar_off + strlen(c.pool.data() + c.recs[k].cigar_off) + 1);
        pool.insert(pool.end(), c.pool.data(), c.pool.data() + used);
        pool_len += used; total += c.n_recs;
    }
    if (o.sam_sort) b.dtext_len = 0;                        // each half went into the sorter under its own sequence number
    else if (o.sam_text_device) {
        if (!b.dtext) b.dtext = w.text_pool->get();
        b.dtext->ensure(text.size() + 1);
        if (!text.empty()) memcpy(b.dtext->data(), text.data(), text.size());
        b.dtext_len = text.size();
    } else {
        b.recs.ensure(recs.size() + 1); b.pool.ensure(pool.size() + 1);
        if (!recs.empty()) memcpy(b.recs.data(), recs.data(), recs.size() * sizeof(gm_sam_rec));
        if (!pool.empty()) memcpy(b.pool.data(), pool.data(), pool.size());
    }
    b.n_recs = total; b.gpu = w.gpu;
    return GM_OK;
}

// ---- the run: what lives from the first step of main() to the last ---------------------------------------------------------------------
static const size_t NPOS = ~(size_t)0;

struct Run {
    Options o;
    std::string cl;                                 // the command line, for @PG (Driver.cpp:1032-1039)
    Clock::time_point t0, t_pipe0;
    FastqScanner fq; bool reads_open = false; char fasta_qual[256];
    FastqScanner fq2;                               // --mates=FILE2: the second mates' file, read in step with fq
    bool next_mates(Block& b, uint32_t max_reads, bool* too_long, bool* bad);
    std::vector<gm_index*> gpu_ix; gm_index_info info;
    std::vector<Worker> workers;
    gm_sam_sorter* sorter = nullptr; uint64_t sorted_rows = 0;
    TextPool text_pool, stage_pool;
    // one <out>.sam, or --sam_shards=K files <out>.<k>.sam: every shard has its own descriptor and offset counter (no two share an inode)
    std::vector<int> ofds; std::vector<uint64_t> file_offs;
    std::string bai;                // --bam_index: the finished <out>.bam.bai, as gm_sam_sorter_bai returned it
    std::atomic<int> failed{ 0 };
    double t_index = 0, t_scan = 0, t_fmt = 0, t_write = 0;     // t_scan: the scanner thread's; t_fmt, t_write: summed under their locks
    std::mutex fmt_mu, tw_mu;                       // (t_write is summed by several writers with --sam_shards)
    uint64_t seq_base = 0;                          // --sam_sort: blocks handed out by the passes before this one
    bool file_order() const { return o.batch_set || o.p.illumina || o.paired(); }       // (paired: byte ranges cannot keep two files, or an even count, in step)
};

static bool write_all(int fd, const char* p, size_t n) {
    while (n) { ssize_t k = ::write(fd, p, n); if (k <= 0) return false; p += k; n -= (size_t)k; }
    return true;
}
static bool pwrite_all(int fd, const char* p, size_t n, uint64_t off) {
    while (n) { ssize_t k = ::pwrite(fd, p, n, (off_t)off); if (k <= 0) return false; p += k; n -= (size_t)k; off += (uint64_t)k; }
    return true;
}

// Paired input, one block of whole pairs in file order.  The records are cut strictly: the reference's recovery from a malformed record
// skips lines and would lose the pairing, so such a record ends the run (*bad), and so do two files that end after different numbers
// of reads and an interleaved file with an odd number.  --mates=FILE2: half the block from either file, the views alternating
bool Run::next_mates(Block& b, uint32_t max_reads, bool* too_long, bool* bad) {
    auto cut = [&](FastqScanner& f, Block& dst, uint32_t want, const std::string& fn) {
        if (f.at >= f.size) { dst.reset(); dst.finish(); return; }
        if (o.fasta) { FastqScanner::parse_range_fasta(f.base, f.at, f.size, dst, want, too_long, fasta_qual); return; }
        bool stop = false; size_t bad_at = 0;
        FastqScanner::parse_range(f.base, f.at, f.size, dst, want, &stop, &bad_at, too_long);
        if (stop) {
            const char* nm = f.base + bad_at; const char* e = (const char*)memchr(nm, '\n', f.size - bad_at);
            fprintf(stderr, "ERROR: %s: malformed FASTQ record at byte %zu (%.*s): with paired reads there is no recovery, it would lose the pairing\n", fn.c_str(), bad_at,
                    (int)std::min<size_t>(e ? (size_t)(e - nm) : f.size - bad_at, 200), nm);
            *bad = true;
        }
    };
    if (o.interleaved) {
        cut(fq, b, max_reads, o.reads);
        if (*bad || *too_long) return false;
        if (b.n & 1u) { fprintf(stderr, "ERROR: %s: --interleaved and an odd number of reads: the last read has no mate\n", o.reads.c_str()); *bad = true; return false; }
        return b.n > 0;
    }
    for (auto& m : b.mate_src) if (!m) m.reset(new Block());
    Block& A = *b.mate_src[0]; Block& B = *b.mate_src[1];
    cut(fq, A, max_reads / 2, o.reads);
    if (!*bad && !*too_long) cut(fq2, B, max_reads / 2, o.mates);
    if (*bad || *too_long) return false;
    if (A.n != B.n) {
        fprintf(stderr, "ERROR: %s and %s end after different numbers of reads (%s has more): the files are not the two halves of one paired run\n", o.reads.c_str(), o.mates.c_str(),
                A.n > B.n ? o.reads.c_str() : o.mates.c_str());
        *bad = true;
        return false;
    }
    b.reset();
    for (uint32_t i = 0; i < A.n; ++i)
        for (Block* m : { &A, &B }) {
            b.name.push_back(m->name[i]); b.name_len.push_back(m->name_len[i]); b.seq.push_back(m->seq[i]); b.len.push_back(m->len[i]);
            b.qual.push_back(m->qual[i]); b.qual_len.push_back(m->qual_len[i]);
        }
    b.n = 2 * A.n; b.maxlen = std::max(A.maxlen, B.maxlen);
    return b.finish();
}

// the read file's format from its first byte, as SeqReader::find_type (src/SeqReader.cpp:175-244) - and what a FASTA input rules out -
// before the device is opened
static int detect_read_format(Run& R) {
    Options& o = R.o; FastqScanner& fq = R.fq;
    R.reads_open = fq.open(o.reads);
    if (!R.reads_open || !fq.size) return 0;
    if (fq.base[0] == '>') {
        o.fasta = true;
        if (!o.adaptor.empty()) {
            fprintf(stderr, "ERROR: -A/--adaptor with FASTA reads is not supported (the reference trims FASTA reads with the PWM-based FixReads, a different rule); use FASTQ reads\n");
            return 1;
        }
        if (o.p.mode == GM_MODE_SNP) { fprintf(stderr, "ERROR: --snp with FASTA reads is not supported; use FASTQ reads\n"); return 1; }
        if (o.read_text_device) { fprintf(stderr, "ERROR: --read_text=device cuts FASTQ only; FASTA reads are cut by the host (--read_text=host)\n"); return 1; }
        if (!fasta_check(fq.base, fq.size, o.reads.c_str())) return 1;
        o.p.illumina = 0;                                  // accepted and ignored, as in the reference
        fasta_qual_table(R.fasta_qual);
        fq.fasta = true; fq.fasta_qual = R.fasta_qual;
    } else if (fq.base[0] != '@') {
        fprintf(stderr, "ERROR: %s starts with neither '@' (FASTQ) nor '>' (FASTA): the _prb.txt and _int.txt read formats are not supported\n", o.reads.c_str());
        return 1;
    }
    if (!o.mates.empty()) {                                 // the second file: there, and in the first one's format
        if (!R.fq2.open(o.mates)) { fprintf(stderr, "ERROR: --mates: cannot open %s\n", o.mates.c_str()); return 1; }
        if (R.fq2.size && R.fq2.base[0] != (o.fasta ? '>' : '@')) {
            fprintf(stderr, "ERROR: --mates: %s is %s and %s is not: the two files of a paired run have one format\n", o.reads.c_str(), o.fasta ? "FASTA" : "FASTQ", o.mates.c_str());
            return 1;
        }
        if (o.fasta && R.fq2.size && !fasta_check(R.fq2.base, R.fq2.size, o.mates.c_str())) return 1;
    }
    return 0;
}

// the index (built once if missing, then one replica per GPU), the sorter, and per GPU `--workers` batches with a stream each
static int open_devices(Run& R) {
    const Options& o = R.o;
    const int flags = GM_INDEX_BUILD | (o.locate_sampled ? 0 : GM_INDEX_FULL_SA);
    R.gpu_ix.assign((size_t)o.gpus, nullptr);
    if (gm_index_open(o.genome.c_str(), 0, flags, &R.gpu_ix[0]) != GM_OK) return fail();
    for (int g = 1; g < o.gpus; ++g)
        if (gm_index_open(o.genome.c_str(), g, flags, &R.gpu_ix[(size_t)g]) != GM_OK) { fprintf(stderr, "ERROR: GPU %d: %s\n", g, gm_last_error()); return 1; }
    for (int g = 0; g < o.gpus; ++g)                                   // k-mer tables / records for these parameters: part of staging the index
        if (gm_index_prepare(R.gpu_ix[(size_t)g], &o.p) != GM_OK) { fprintf(stderr, "ERROR: GPU %d: %s\n", g, gm_last_error()); return 1; }
    if (o.sam_sort && (gm_sam_sorter_create(R.gpu_ix[0], &R.sorter) != GM_OK || gm_sam_sorter_set_rows(R.sorter, o.bam ? GM_ROWS_BAM : GM_ROWS_TEXT) != GM_OK)) return fail();
    R.workers = std::vector<Worker>((size_t)o.gpus * (size_t)o.workers);
    for (int g = 0; g < o.gpus; ++g) {
        gm_index* ix = R.gpu_ix[(size_t)g];
        if (gm_coverage_reset(ix, (uint32_t)o.p.bin_size) != GM_OK || (o.p.mode != GM_MODE_NORMAL && gm_coverage_enable_nuc(ix) != GM_OK)) return fail();
        for (int k = 0; k < o.workers; ++k) {
            Worker& w = R.workers[(size_t)g * (size_t)o.workers + (size_t)k];
            w.gpu = g; w.ix = ix; w.text_pool = &R.text_pool; w.stage_pool = &R.stage_pool; w.sorter = R.sorter;
            if (gm_batch_create(w.ix, R.file_order() ? o.batch : 16000000u, 2048, &w.batch) != GM_OK || gm_stream_create(w.ix, &w.stream) != GM_OK ||
                gm_batch_set_adaptor(w.batch, o.adaptor.c_str()) != GM_OK || gm_batch_set_unmapped_rows(w.batch, o.sam_unmapped ? 1 : 0) != GM_OK ||
                gm_batch_set_row_tags(w.batch, o.sam_md ? GM_ROW_TAG_MD : 0u) != GM_OK || gm_batch_set_cigar_order(w.batch, o.sam_cigar_forward ? GM_CIGAR_FORWARD : GM_CIGAR_GNUMAP) != GM_OK ||
                gm_batch_set_read_format(w.batch, o.fasta ? GM_READS_FASTA : GM_READS_FASTQ) != GM_OK ||
                gm_batch_set_mates(w.batch, o.paired() ? 1 : 0, o.min_insert, o.max_insert) != GM_OK) return fail();
        }
    }
    gm_index_get_info(R.gpu_ix[0], &R.info);
    R.t_index = secs_since(R.t0);
    if (o.verbose > 0)
        fprintf(stderr, "gnumap-mi355x: genome %s (%lu bp, %u contigs), %s locate, %d GPU(s), index %.1f MB in HBM\n", o.genome.c_str(),
                (unsigned long)R.info.l_pac, R.info.n_seqs, R.info.full_sa ? "full-SA" : "sampled-SA", o.gpus, R.info.hbm_bytes / 1e6);
    if (o.verbose > 0 && !o.adaptor.empty()) fprintf(stderr, "\tUsing Adaptor Sequence: %s\n", o.adaptor.c_str());      // Driver.cpp:1231-1233
    return 0;
}

// <out>.sam or the K shard files, and the header lines in the first (or only) one
static int open_outputs(Run& R) {
    const Options& o = R.o;
    const int K = o.sam_shards;
    R.ofds.assign((size_t)K, -1);
    R.file_offs.assign((size_t)K, 0);
    for (int k = 0; k < K; ++k) {
        const std::string fn = o.bam ? o.output + ".bam" : K == 1 ? o.output + ".sam" : o.output + "." + std::to_string(k) + ".sam";
        R.ofds[(size_t)k] = ::open(fn.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (R.ofds[(size_t)k] < 0) { fprintf(stderr, "ERROR: cannot write %s\n", fn.c_str()); return 1; }
    }
    std::ostringstream hd;
    if (o.sam_sort) hd << "@HD\tVN:1.0\tSO:coordinate\n";
    for (uint32_t i = 0; i < R.info.n_seqs; ++i)                       // Driver.cpp:2322-2327
        hd << "@SQ\tSN:" << gm_index_contig_name(R.gpu_ix[0], i) << "\tLN:"
           << (gm_index_contig_offset(R.gpu_ix[0], i + 1) - gm_index_contig_offset(R.gpu_ix[0], i)) << "\n";
    hd << "@PG\tID:gnumap\tPN:gnumap\tVN:4.0.0 BETA\tCL:" << R.cl << "\n";
    std::string s = hd.str();
    if (o.bam) {                                                       // the same lines inside the BAM header, as BGZF blocks
        uint64_t raw_len = 0, z_len = 0;
        (void)gm_bam_header(R.gpu_ix[0], s.data(), s.size(), nullptr, 0, &raw_len);
        std::string raw((size_t)raw_len, '\0'), z((size_t)(raw_len + 31 * (raw_len / 65280 + 1)), '\0');
        if (gm_bam_header(R.gpu_ix[0], s.data(), s.size(), &raw[0], raw.size(), &raw_len) != GM_OK ||
            gm_bgzf_compress(R.gpu_ix[0], raw.data(), raw.size(), o.bam_level, &z[0], z.size(), &z_len, nullptr) != GM_OK) return fail();
        s.assign(z.data(), (size_t)z_len);
    }
    if (!write_all(R.ofds[0], s.data(), s.size())) { fprintf(stderr, "ERROR: write failed\n"); return 1; }
    return 0;
}

// ---- one pass of the pipeline -----------------------------------------------------------------------------------------------------------
// The gate of chunk mode: nothing of a block reaches the GPU before every block below it is known to be well-formed.
struct ParseGate {
    std::mutex mu; std::condition_variable cv;
    uint64_t parsed = 0; std::set<uint64_t> done;          // `parsed` = every block below it has been cut into records
    std::atomic<uint64_t> stop{ ~0ull }; size_t bad_at = NPOS;      // the first block with a malformed record, and where that record starts
    bool stopped() const { return stop.load() != ~0ull; }  // (the scanner asks without the lock)
    // Block `index` has been cut into records (`malformed`: up to a malformed record at `at`).  Returns once the block may go on (true) or is
    // known to lie behind a malformed record (false: dropped, the next pass reads it again); a failed run lets everything through.
    bool pass(uint64_t index, bool malformed, size_t at, const std::atomic<int>& failed) {
        std::unique_lock<std::mutex> lk(mu);
        if (malformed && index < stop) { stop = index; bad_at = at; }
        done.insert(index);
        while (done.count(parsed)) { done.erase(parsed); ++parsed; }
        cv.notify_all();
        cv.wait(lk, [&] { return parsed >= index || stop < index || failed.load(); });
        return !(stop < index);
    }
};

// The writer only hands out file offsets in block order; the text pieces of a block (one per formatter slice, or cuts of the
// device's text) are written by pwrite() from a few threads at once (a single write() stream tops out at ~8 GB/s of page-cache
// copies).  --sam_shards=K: a block belongs to the shard of its first byte in the input, which only grows with the block index,
// so blocks keep their order inside a shard; the writer then only assigns (shard, offsets) and the shard's own writer thread does
// the writing, side by side with the other shards'.
// (Tried in round 4: the pieces copied in through shared mappings of the file's byte ranges instead - no inode write lock, which is
// what holds buffered pwrite()s to ONE file to the rate of one thread, 8.4-8.8 GB/s whatever the number of writers.  4 x SLOWER on the
// GPU box's file system: 2.1 M first-touch page faults of a growing file cost more than the copies.  The write calls stay.)
struct Piece { const char* p; size_t n; uint64_t off; };
struct WriteJob { Block* b; int shard; std::vector<Piece> pieces; };

// One pass over the FASTQ text from fq.at on.  chunks = byte ranges cut into records by the workers in parallel (well-formed records
// only); run() returns where a malformed record starts (NPOS: none) - everything before it has been mapped and written, nothing after it
// has touched the SAM file or the coverage track.  !chunks = file order with the reference's recovery from malformed records (--batch=N,
// --illumina - its fallback is a property of the reads in file order -, and the rest of an input in which a malformed record was found).
// Members are grouped by the two stages they link; of the Run, a stage uses what its body names.
struct Pass {
    static const int N_FMT = 2;
    Run& R; const Options& o; FastqScanner& fq; const bool chunks;
    // the pool of blocks in flight: scanner <- writers
    std::vector<Block> blocks; Queue<Block*> free_q;
    // scanner -> workers (the gate: among the workers, and its stop flag back to the scanner)
    Queue<Block*> map_q; ParseGate gate; uint64_t idx_end = 0;
    // workers -> formatters
    Queue<Block*> fmt_q; std::atomic<int> live_workers;
    // formatters -> writer: blocks by index
    std::mutex wr_mu; std::condition_variable wr_cv; std::map<uint64_t, Block*> ready; bool fmt_done = false; std::atomic<int> live_fmt{ N_FMT };
    // writer -> shard writers (--sam_shards above 1)
    std::vector<std::unique_ptr<Queue<WriteJob*>>> shard_q; std::vector<std::thread> shard_th;

    Pass(Run& run, bool chunk_mode) : R(run), o(run.o), fq(run.fq), chunks(chunk_mode), blocks(run.workers.size() * 2 + 4), live_workers((int)run.workers.size()) {
        for (auto& b : blocks) free_q.push(&b);
    }

    void scan() {
        uint64_t idx = 0;
        int ill_state = o.p.illumina;
        Block* b;
        while (!R.failed && !gate.stopped() && free_q.pop(b)) {
            auto s0 = Clock::now();
            b->lazy = false; b->text_dev = false;
            bool too_long = false;
            b->first_byte = fq.at;
            bool bad_pairs = false;
            const bool more = chunks ? fq.next_chunk(*b, o.batch) : o.paired() ? R.next_mates(*b, o.batch, &too_long, &bad_pairs) : fq.next(*b, o.batch, &too_long);
            R.t_scan += secs_since(s0);
            if (too_long || bad_pairs) R.failed = 1;
            if (!more || R.failed) { free_q.push(b); break; }
            b->index = idx++; b->failed = false;
            b->sort_seq = (R.seq_base + b->index) << 21;
            b->illumina = ill_state;
            b->kept.clear();
            if (ill_state && !o.adaptor.empty()) {      // -A: the fallback scan sees only the characters the trim keeps (SeqReader.cpp:1152)
                std::vector<uint8_t> rows((size_t)b->n * b->stride, 0);
                for (uint32_t i = 0; i < b->n; ++i) memcpy(&rows[(size_t)i * b->stride], b->seq[i], b->len[i]);
                gm_reads rr; rr.n = b->n; rr.stride = b->stride; rr.bases = rows.data(); rr.quals = nullptr; rr.len = b->len.data();
                b->kept.resize(b->n);
                const int rc = gm_dev_adaptor_trim(R.gpu_ix[0], &rr, o.adaptor.c_str(), b->kept.data());
                if (rc != GM_OK) { fprintf(stderr, "ERROR: gm_dev_adaptor_trim: %s\n", gm_last_error()); R.failed = 1; free_q.push(b); break; }
            }
            if (ill_state && b->has_quality_below_64(b->n)) ill_state = 0;      // gILLUMINA is cleared for the rest of the run by the first quality below '@'
            map_q.push(b);
        }
        idx_end = idx;
        map_q.close();
    }

    void work(Worker& w) {
        Block* b;
        while (map_q.pop(b)) {
            if (b->lazy) {                              // chunk mode: this worker cuts its byte range into records
                auto s0 = Clock::now();
                size_t cur = b->text_lo, bad_at = NPOS; bool stop = false, too_long = false;
                if (o.fasta) FastqScanner::parse_range_fasta(fq.base, cur, b->text_hi, *b, 16000000u, &too_long, fq.fasta_qual);
                else if (o.read_text_device && b->text_hi - b->text_lo < ((size_t)1 << 32)) {
                    if (upload_text_block(w, o, fq.base, *b, &stop, &bad_at, &too_long) != GM_OK) { R.failed = 1; b->n = 0; }
                }
                else FastqScanner::parse_range(fq.base, cur, b->text_hi, *b, 16000000u, &stop, &bad_at, &too_long);
                if (too_long) R.failed = 1;
                if (!b->text_dev) w.t_scan += secs_since(s0);      // (a text block's staging and upload are booked by upload_text_block)
                if (!gate.pass(b->index, stop, bad_at, R.failed)) b->n = 0;
            }
            if (b->n == 0) { b->n_recs = 0; fmt_q.push(b); continue; }
            if (!R.failed && process_block_split(w, o, fq.base, *b, 0) != GM_OK) { R.failed = 1; gate.cv.notify_all(); }
            if (R.failed) { b->failed = true; b->n_recs = 0; }
            fmt_q.push(b);
        }
        if (--live_workers == 0) fmt_q.close();
    }

    // formatters: a block is cut into slices of records, one string each; the writer emits blocks in index order
    void format() {
        Block* b;
        while (fmt_q.pop(b)) {
            auto f0 = Clock::now();
            const gm_index* ix = R.gpu_ix[(size_t)b->gpu];
            const uint32_t nr = (uint32_t)b->n_recs;
            const int T = o.fmt_threads;
            if ((int)b->text.size() < T) b->text.resize((size_t)T);
            for (auto& s : b->text) s.clear();
            if (!o.sam_text_device)                  // (device: the block's text is there already, b->dtext)
                run_slices(nr, T, 4096, [&](int s, uint32_t lo, uint32_t hi) {
                    TextBuf& out = b->text[(size_t)s];
                    out.room((size_t)(hi - lo) * 320);
                    for (uint32_t k = lo; k < hi; ++k) { const gm_sam_rec& r = b->recs[k]; format_sam(out, ix, o.p, r, b->pool.data() + r.cigar_off, *b); }
                });
            { std::lock_guard<std::mutex> lk(R.fmt_mu); R.t_fmt += secs_since(f0); }
            { std::lock_guard<std::mutex> lk(wr_mu); ready[b->index] = b; }
            wr_cv.notify_all();
        }
        if (--live_fmt == 0) { { std::lock_guard<std::mutex> lk(wr_mu); fmt_done = true; } wr_cv.notify_all(); }
    }

    void write_job(WriteJob& j) {
        auto w0 = Clock::now();
        const int fd = R.ofds[(size_t)j.shard];
        const int nt = (int)std::min<size_t>(8, j.pieces.size());
        std::atomic<size_t> nextp{ 0 }; std::atomic<int> bad{ 0 };
        auto job = [&] { for (size_t k; (k = nextp++) < j.pieces.size();) if (j.pieces[k].n && !pwrite_all(fd, j.pieces[k].p, j.pieces[k].n, j.pieces[k].off)) bad = 1; };
        std::vector<std::thread> ws;
        for (int t = 1; t < nt; ++t) ws.emplace_back(job);
        job();
        for (auto& x : ws) x.join();
        if (bad) { fprintf(stderr, "ERROR: write failed\n"); R.failed = 1; }
        { std::lock_guard<std::mutex> lk(R.tw_mu); R.t_write += secs_since(w0); }
    }
    void release(Block* b) { R.text_pool.put(b->dtext); b->dtext = nullptr; free_q.push(b); }       // the rows are written (or there are none)
    void shard_write(Queue<WriteJob*>* q) { WriteJob* j; while (q->pop(j)) { write_job(*j); release(j->b); delete j; } }

    void write() {
        const int K = o.sam_shards;
        const size_t in_size = fq.size;
        uint64_t next = 0;
        for (;;) {
            Block* b = nullptr;
            {
                std::unique_lock<std::mutex> lk(wr_mu);
                wr_cv.wait(lk, [&] { return (!ready.empty() && ready.begin()->first == next) || (fmt_done && ready.empty()) || (fmt_done && R.failed); });
                if (ready.empty() || ready.begin()->first != next) break;
                b = ready.begin()->second; ready.erase(ready.begin());
            }
            ++next;
            if (b->failed || !b->n_recs || o.sam_sort) { release(b); continue; }      // (sorted: the rows are in the sorter)
            WriteJob* j = new WriteJob();
            j->b = b;
            j->shard = K == 1 || in_size == 0 ? 0 : (int)std::min<unsigned __int128>((unsigned __int128)(K - 1), (unsigned __int128)b->first_byte * (unsigned)K / in_size);
            uint64_t& off = R.file_offs[(size_t)j->shard];
            if (o.sam_text_device) {
                const size_t cut = std::max<size_t>((size_t)1 << 22, ((size_t)b->dtext_len + 7) / 8);
                for (size_t at = 0; at < b->dtext_len; at += cut) {
                    const size_t n = std::min<size_t>(cut, (size_t)b->dtext_len - at);
                    j->pieces.push_back({ b->dtext->data() + at, n, off }); off += n;
                }
            } else
                for (size_t k = 0; k < b->text.size(); ++k) { j->pieces.push_back({ b->text[k].data(), b->text[k].size(), off }); off += b->text[k].size(); }
            if (K == 1) { write_job(*j); delete j; release(b); }
            else shard_q[(size_t)j->shard]->push(j);
        }
        for (auto& q : shard_q) q->close();
        for (auto& x : shard_th) x.join();
        free_q.close();
    }

    size_t run() {
        std::thread scanner(&Pass::scan, this);
        std::vector<std::thread> wth, fth;
        for (Worker& w : R.workers) wth.emplace_back(&Pass::work, this, std::ref(w));
        for (int f = 0; f < N_FMT; ++f) fth.emplace_back(&Pass::format, this);
        if (o.sam_shards > 1)
            for (int k = 0; k < o.sam_shards; ++k) {
                shard_q.emplace_back(new Queue<WriteJob*>());
                shard_th.emplace_back(&Pass::shard_write, this, shard_q.back().get());
            }
        std::thread writer(&Pass::write, this);
        scanner.join();
        for (auto& x : wth) x.join();
        for (auto& x : fth) x.join();
        writer.join();
        R.seq_base += idx_end;
        return gate.bad_at;
    }
};

static size_t run_pass(Run& R, bool chunks) { return Pass(R, chunks).run(); }

// --sam_sort=coordinate: sort once, then the rows come down slab by slab; a slab is written while the next one is gathered and downloaded
static int drain_sorter(Run& R) {
    uint64_t sorted_bytes = 0;
    void* const stream = R.workers[0].stream;
    if (gm_sam_sorter_finish(R.sorter, &R.sorted_rows, &sorted_bytes, stream) != GM_OK) { fprintf(stderr, "ERROR: gm_sam_sorter_finish: %s\n", gm_last_error()); return 1; }
    PinVec<char> slab[2];
    const size_t slab_cap = (size_t)std::min<uint64_t>((uint64_t)64 << 20, std::max<uint64_t>(sorted_bytes, 1 << 16));
    slab[0].ensure(slab_cap); slab[1].ensure(slab_cap);
    const int ofd = R.ofds[0];
    std::thread wr; std::atomic<int> wr_bad{ 0 };
    if (R.o.bam_index && gm_sam_sorter_index_begin(R.sorter, R.file_offs[0]) != GM_OK) { fprintf(stderr, "ERROR: gm_sam_sorter_index_begin: %s\n", gm_last_error()); return 1; }
    auto w0 = Clock::now();
    size_t cap = slab_cap;                                           // what gm_sam_sorter_read may fill of either buffer
    for (int k = 0;;) {                                              // k: the buffer the next slab goes into, while the other one is written
        uint64_t got = 0;
        int rc = R.o.bam ? gm_sam_sorter_read_bgzf(R.sorter, R.o.bam_level, slab[k].data(), cap, &got, stream)      // (compressed before it comes down)
                         : gm_sam_sorter_read(R.sorter, slab[k].data(), cap, &got, stream);
        if (rc == GM_E_CAPACITY) {                                   // a row longer than a slab: both buffers grow to it, the same read again
            if (wr.joinable()) wr.join();
            cap = (size_t)got;
            slab[0].ensure(cap); slab[1].ensure(cap);
            continue;
        }
        if (rc != GM_OK) { fprintf(stderr, "ERROR: %s: %s\n", R.o.bam ? "gm_sam_sorter_read_bgzf" : "gm_sam_sorter_read", gm_last_error()); R.failed = 1; break; }
        if (wr.joinable()) wr.join();
        if (!got || wr_bad) break;
        const uint64_t off = R.file_offs[0];
        R.file_offs[0] += got;
        const char* p = slab[k].data();
        wr = std::thread([ofd, p, got, off, &wr_bad] { if (!pwrite_all(ofd, p, (size_t)got, off)) wr_bad = 1; });
        k ^= 1;
    }
    if (wr.joinable()) wr.join();
    if (wr_bad) { fprintf(stderr, "ERROR: write failed\n"); R.failed = 1; }
    if (R.o.bam_index && !R.failed) {                                // every row has its place in the file: the index, grown once to its size
        R.bai.resize(1 << 16);
        for (;;) {
            uint64_t got = 0;
            const int rc = gm_sam_sorter_bai(R.sorter, &R.bai[0], R.bai.size(), &got, stream);
            if (rc == GM_E_CAPACITY && got > R.bai.size()) { R.bai.resize((size_t)got); continue; }
            if (rc != GM_OK) { fprintf(stderr, "ERROR: gm_sam_sorter_bai: %s\n", gm_last_error()); R.failed = 1; break; }
            R.bai.resize((size_t)got);
            break;
        }
    }
    R.t_write += secs_since(w0);
    return 0;
}

static void report_sorter(const Run& R) {
    gm_sam_sort_stats ss;
    if (gm_sam_sorter_stats(R.sorter, &ss) != GM_OK) return;
    fprintf(stderr, "sam sort on the device: %lu rows, %lu text bytes in %lu pieces of %lu bytes; seconds: arena appends %.3f, sort %.3f, gather %.3f, download %.3f\n",
            (unsigned long)ss.rows, (unsigned long)ss.text_bytes, (unsigned long)ss.pieces, (unsigned long)ss.piece_bytes, ss.add_s, ss.sort_s, ss.gather_ms / 1e3, ss.download_s);
    if (R.o.bam_index)
        fprintf(stderr, "bam index on the device: %lu bytes, %lu chunks, %.3f ms in kernels\n", (unsigned long)ss.bai_bytes, (unsigned long)ss.bai_chunks, ss.bai_ms);
}

// coverage: all-reduce over the GPUs, then PrintFinalSGR / PrintFinalBisulfite / PrintFinalSNP, and the .vcf beside a .gmp
static int write_tracks(Run& R) {
    const Options& o = R.o;
    gm_index* const ix = R.gpu_ix[0];
    const std::string sgr = o.output + ".sgr", gmp = o.output + ".gmp";
    if (gm_coverage_allreduce(R.gpu_ix.data(), o.gpus) != GM_OK) return fail();
    if (o.p.mode == GM_MODE_SNP && o.snp_calls && !o.track_text_device) {      // PrintFinalSNP with PrintSNPCall's column: the tracks are read where they are, slab by slab
        if (gm_coverage_write_gmp_calls(ix, o.snp_pval, o.snp_monop, gmp.c_str(), 0) != GM_OK) return fail();
    } else if (o.track_text_device) {                                  // GPU 0 formats the rows where the tracks are: no host copy of a track
        const int rc = o.p.mode == GM_MODE_NORMAL ? gm_coverage_write_sgr_device(ix, sgr.c_str(), 0)
                       : o.p.mode == GM_MODE_SNP && o.snp_calls ? gm_coverage_write_gmp_calls_device(ix, o.snp_pval, o.snp_monop, gmp.c_str(), 0)
                                                                : gm_coverage_write_gmp_device(ix, &o.p, gmp.c_str(), 0);
        if (rc != GM_OK) return fail();
        gm_track_text_stats ts;
        if (o.verbose > 0 && gm_coverage_text_stats(ix, &ts) == GM_OK)
            fprintf(stderr, "track text on the device: %lu rows, %lu bytes, %lu slabs (%lu formatted by the host), %lu launches, %.2f ms in kernels\n", (unsigned long)ts.rows,
                    (unsigned long)ts.bytes, (unsigned long)ts.slabs, (unsigned long)ts.host_slabs, (unsigned long)ts.launches, ts.kernel_ms);
    } else {
        PinVec<float> cov; cov.ensure(gm_coverage_bins(ix));                            // page-locked: the 1.5 GB of a human track come down at link rate
        if (gm_coverage_download(ix, cov.data()) != GM_OK) return fail();
        if (o.p.mode == GM_MODE_NORMAL) {                              // GenomeBwt::PrintFinal src/GenomeBwt.cpp:915-926
            if (gm_coverage_write_sgr(ix, cov.data(), sgr.c_str(), 0) != GM_OK) return fail();
        } else {
            std::vector<float> nuc(5 * (size_t)gm_coverage_bins(ix));
            if (gm_coverage_download_nuc(ix, nuc.data()) != GM_OK || gm_coverage_write_gmp(ix, &o.p, cov.data(), nuc.data(), gmp.c_str(), 0) != GM_OK) return fail();
        }
    }
    // Genome::PrintFinalVCF src/Genome.cpp:1142-1245 beside the .gmp (the reference's compiled GenomeBwt accepts --vcf and writes no file)
    if (o.vcf && gm_coverage_write_vcf(ix, o.snp_pval, o.snp_monop, (o.output + ".vcf").c_str(), 0) != GM_OK) return fail();
    return 0;
}

static void report(const Run& R, double t_pipe, double t_cov, double secs) {
    const Options& o = R.o;
    struct { uint64_t n_reads = 0, n_matched = 0, n_records = 0; double t_pack = 0, t_map = 0, t_out = 0, t_scan = 0; } t;      // summed over the workers
    for (const Worker& w : R.workers) {
        t.n_reads += w.n_reads; t.n_matched += w.n_matched; t.n_records += w.n_records;
        t.t_pack += w.t_pack; t.t_map += w.t_map; t.t_out += w.t_out; t.t_scan += w.t_scan;
    }
    if (o.sam_sort) t.n_records = R.sorted_rows;
    const bool text_blocks = o.read_text_device && !R.file_order();      // the chunk-mode blocks went up as text: name the path that ran
    const char* const pack = text_blocks ? "stage" : "pack";       // copying the text into a page-locked buffer takes the place of cutting and packing it
    const char* const map = text_blocks ? "gm_map_batch_text" : "gm_map_batch";      // (with the flag it includes gm_batch_upload_text, as gm_map_batch includes its upload)
    const double t_scan = R.t_scan + t.t_scan;
    if (o.sam_text_device)                               // no formatter stage: the rows were text when they left the library
        fprintf(stderr, "stage seconds (summed over threads): index %.2f, scan %.2f, %s %.2f, %s %.2f, %s %.2f, write %.2f\n",
                R.t_index, t_scan, pack, t.t_pack, map, t.t_map, o.bam ? (text_blocks ? "gm_output_batch_bam_resident" : "gm_output_batch_bam") : text_blocks ? "gm_output_batch_text_resident" : "gm_output_batch_text", t.t_out, R.t_write);
    else
        fprintf(stderr, "stage seconds (summed over threads): index %.2f, scan %.2f, %s %.2f, %s %.2f, gm_output_batch %.2f, SAM format %.2f, write %.2f\n",
                R.t_index, t_scan, pack, t.t_pack, map, t.t_map, t.t_out, R.t_fmt, R.t_write);
    fprintf(stderr, "wall seconds: index %.2f, FASTQ->SAM pipeline %.2f (%.3f M reads/s), coverage all-reduce + track file %.2f\n", R.t_index, t_pipe,
            t.n_reads / std::max(t_pipe, 1e-9) / 1e6, t_cov);
    fprintf(stderr, "Finished: %lu reads, %lu matched, %lu SAM records, %.2f s total (%.2f s after the index was resident)\n", (unsigned long)t.n_reads,
            (unsigned long)t.n_matched, (unsigned long)t.n_records, secs, secs - R.t_index);
    if (o.paired()) {
        gm_mate_stats m{};
        for (const Worker& w : R.workers) { m.pairs += w.mates.pairs; m.both_mapped += w.mates.both_mapped; m.proper += w.mates.proper; m.one_mapped += w.mates.one_mapped; m.none_mapped += w.mates.none_mapped; }
        fprintf(stderr, "%s: %lu pairs: %lu with both mates mapped (%lu of them proper: forward/reverse on one contig, insert %u .. %u), %lu with one mate mapped, %lu with none\n",
                o.interleaved ? "--interleaved" : "--mates", (unsigned long)m.pairs, (unsigned long)m.both_mapped, (unsigned long)m.proper, o.min_insert, o.max_insert,
                (unsigned long)m.one_mapped, (unsigned long)m.none_mapped);
    }
    if (o.sam_unmapped) {
        uint64_t n_unmapped = 0;
        for (const Worker& w : R.workers) n_unmapped += w.n_unmapped;
        fprintf(stderr, "--sam_unmapped: %lu of the %lu SAM records are rows of reads that did not map (flag 4, YU:i:<code>)\n", (unsigned long)n_unmapped, (unsigned long)t.n_records);
    }
}

int main(int argc, char** argv) {
    Run R;
    parse_args(argc, argv, R.o);
    // (--bam_index stays out of the @PG line: <out>.bam is byte for byte the file of the run without it)
    for (int i = 0; i < argc; ++i) if (strcmp(argv[i], "--bam_index")) { R.cl += argv[i]; R.cl += " "; }
    R.t0 = Clock::now();
    if (detect_read_format(R) || open_devices(R) || open_outputs(R)) return 1;
    R.t_pipe0 = Clock::now();
    if (!R.reads_open) { fprintf(stderr, "ERROR: cannot open %s\n", R.o.reads.c_str()); return 1; }
    { struct stat hs; if (fstat(R.ofds[0], &hs) == 0) R.file_offs[0] = (uint64_t)lseek(R.ofds[0], 0, SEEK_CUR); }
    const size_t bad_at = run_pass(R, !R.file_order());
    if (!R.failed && bad_at != NPOS) {                 // a malformed record: the reference's recovery needs the lines in file order from there on
        R.fq.at = bad_at; R.fq.done = false;
        run_pass(R, false);
    }
    if (R.o.sam_sort && !R.failed && drain_sorter(R)) return 1;
    if (R.o.bam && !R.failed) {                        // the empty block that ends a BGZF file
        char eof[28];
        (void)gm_bgzf_eof(eof);
        if (!pwrite_all(R.ofds[0], eof, sizeof eof, R.file_offs[0])) { fprintf(stderr, "ERROR: write failed\n"); return 1; }
        R.file_offs[0] += sizeof eof;
    }
    if (R.o.bam_index && !R.failed) {                  // <out>.bam.bai, behind the end marker of <out>.bam
        const std::string fn = R.o.output + ".bam.bai";
        const int fd = ::open(fn.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        const bool ok = fd >= 0 && write_all(fd, R.bai.data(), R.bai.size());
        if (fd >= 0) ::close(fd);
        if (!ok) { fprintf(stderr, "ERROR: cannot write %s\n", fn.c_str()); return 1; }
    }
    for (int fd : R.ofds) ::close(fd);
    if (R.failed) return 1;
    const double t_pipe = secs_since(R.t_pipe0);
    if (R.o.sam_sort && R.o.verbose > 0) report_sorter(R);
    gm_sam_sorter_destroy(R.sorter);
    auto t_cov0 = Clock::now();
    if (write_tracks(R)) return 1;
    for (Worker& w : R.workers) { gm_batch_destroy(w.batch); gm_stream_destroy(w.ix, w.stream); }
    const double t_cov = secs_since(t_cov0);
    for (auto ix : R.gpu_ix) gm_index_close(ix);
    if (R.o.verbose > 0) report(R, t_pipe, t_cov, secs_since(R.t0));
    return 0;
}

