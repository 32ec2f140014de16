/*
 * include/f2q.h -- C ABI of libf2q_hip.so, the MI355X-native read-counting path of 2FAST2Q.
 *
 * The reference (afombravo/2FAST2Q v2.8.1) is a pure-Python program with no FFI; the seam this
 * library sits behind is the Python call
 *     reads_counter(i, raw, features, param, reads_stats) -> (features, reads_stats, local_read_stats)
 * (fast2q/fast2q.py:514-582) made once per FASTQ file by aligner() (:762).  Everything below
 * that call -- fastq_parser (:306-409), sequence_tinder (:215-285), border_finder (:628-658),
 * binary_subtract (:601-626), features_all_vs_all (:660-690), mismatch_search_handler (:692-750),
 * the Features counters (:21-44) and the chunk pool single_file_reads_binner (:411-512) -- is
 * replaced by the entry points declared here.  2fast2q_amd/fast2q.py binds them with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * F2Q_E* code, with text from f2q_last_error(); the caller owns every buffer it passes; the
 * library owns the context and all device memory; a context is bound to one HIP device and is not
 * thread-safe; there is no global state, so several contexts may coexist.  There is NO CPU
 * fallback: without a usable HIP device f2q_create fails with F2Q_ENODEVICE.
 */
#ifndef F2Q_H
#define F2Q_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F2Q_ABI_VERSION 1
#define F2Q_MAX_ITER 16          /* --st values / --us,--ds pairs per run                     */

enum {
    F2Q_OK = 0,
    F2Q_EINVAL = -1,             /* bad argument                                              */
    F2Q_ENODEVICE = -2,          /* no HIP device / kernel image not loadable                 */
    F2Q_EHIP = -3,               /* a HIP runtime call failed                                 */
    F2Q_ENOMEM = -4,
    F2Q_EIO = -5,                /* file could not be opened / read                           */
    F2Q_ETRUNCATED = -6,         /* corrupted or truncated gzip stream (partial counts kept,
                                    as fast2q.py:405-407,580-582)                             */
    F2Q_ESTATE = -7,             /* call order (e.g. counting before f2q_set_features)        */
    F2Q_EUNSUPPORTED = -8,       /* input outside what the device path implements             */
    F2Q_EPAIRING = -9            /* paired files: one holds complete records beyond the other's
                                    last (the common pairs stay counted)                      */
};

/* index into the stats vector == the keys of local_read_stats (fast2q.py:310-316) */
enum { F2Q_READS = 0, F2Q_PERFECT = 1, F2Q_IMPERFECT = 2, F2Q_NON_ALIGNED = 3, F2Q_QUALITY_FAILED = 4 };

typedef struct f2q_ctx f2q_ctx;

/* The subset of the reference's `param` dict (fast2q.py:1226-1309) that the path reads. */
typedef struct {
    int32_t mode;                        /* 0 = "C" Counter, 1 = "EC" Extract+Count (:364,:382) */
    int32_t miss;                        /* --m   allowed mismatches per feature  (:1266)       */
    int32_t phred;                       /* --ph  raw CLI value; <=0 behaves as 1 (:1118)       */
    int32_t length;                      /* --l   feature length                  (:1250)       */
    int32_t n_start;                     /* number of --st values (fixed mode)    (:539)        */
    int32_t start[F2Q_MAX_ITER];         /* --st values                                         */
    int32_t n_upstream;                  /* number of --us sequences, 0 = None    (:546-548)    */
    int32_t n_downstream;                /* number of --ds sequences, 0 = None    (:549-551)    */
    const char *upstream[F2Q_MAX_ITER];  /* NUL-terminated, any case (upper-cased inside, :547) */
    const char *downstream[F2Q_MAX_ITER];
    int32_t miss_search_up;              /* --msu (:1278) */
    int32_t miss_search_down;            /* --msd (:1282) */
    int32_t qual_up;                     /* --qsu (:1286) */
    int32_t qual_down;                   /* --qsd (:1290) */
    int32_t device;                      /* HIP device ordinal this context drives              */
    int32_t reserved[7];
} f2q_params;

/* Device-side synthetic workload of SURVEY.md §8(d) (spec: tests/synth.py). Probabilities are
 * cumulative 32-bit thresholds (p * 2^32). */
typedef struct {
    uint64_t seed;
    uint64_t n_reads;
    uint64_t first_read;                 /* global index of read 0 of this block (sharding)     */
    int32_t read_len;
    int32_t start;                       /* window position when cassette == 0                  */
    int32_t cassette;                    /* 1: up+guide+down at a uniform offset in [0,max_offset] */
    int32_t max_offset;
    const char *up;                      /* cassette flanks (may be NULL when cassette == 0)    */
    const char *down;
    uint32_t t_sub, t_rand, t_n, t_lowq, t_q29, t_q28;
    int32_t reserved[4];
} f2q_synth;

typedef struct {
    double kernel_ms;                    /* HIP-event time of the counting kernels of the call  */
    double total_ms;                     /* HIP-event time of the whole call on its stream      */
    uint64_t reads;                      /* reads the call processed                            */
    uint64_t fast_reads;                 /* ... of which went through the packed fast path      */
    uint64_t general_reads;              /* ... of which went through the general path          */
    uint32_t launches;                   /* kernel launches in the call                         */
    uint32_t path;                       /* kernel family that counted the packed tiles of the call (F2Q_PATH_*, diagnostics) */
} f2q_timing;
/* f2q_timing.path */
enum {
    F2Q_PATH_NONE = 0,                   /* no packed tiles / not recorded                        */
    F2Q_PATH_FIXED_V1 = 1,               /* one read per lane, wide tables                        */
    F2Q_PATH_FIXED_PACKED = 2,           /* k_count_fixed4: packed tables in L2                   */
    F2Q_PATH_FIXED_LDS = 3,              /* k_count_fixed4_lds: the library in LDS                */
    F2Q_PATH_FIXED_PART = 4,             /* k_part_*: a large library dealt into LDS-sized partitions */
    F2Q_PATH_MULTI = 5,                  /* k_count_multi4                                        */
    F2Q_PATH_ANCHOR = 6,                 /* k_count_anchor                                        */
    F2Q_PATH_ANCHOR_LDS = 7,             /* k_count_anchor_lt                                     */
    F2Q_PATH_PAIRS = 8,                  /* k_count_anchor_pairs                                  */
    F2Q_PATH_EXTRACT = 9,                /* the Extract+Count kernels                             */
    F2Q_PATH_MULTI_LDS = 10              /* k_count_fixed4_lds<.., MW>: several windows, joined keys in the LDS tables */
};

typedef struct f2q_block f2q_block;      /* a device-resident block of reads (opaque)           */

/* ---- lifetime --------------------------------------------------------------------------- */
int f2q_version(void);
/* 16 hex digits identifying the sources this binary was compiled from (SHA-256 over csrc/ and this header, computed
 * by __graft_entry__.build() and passed as -DF2Q_BUILD_ID); "unknown" for a build made any other way.  smoke() and
 * the GPU tests compare it with the tree they run from, so a stale binary cannot pass for HEAD. */
const char *f2q_build_id(void);
/* Replaces the per-file set-up half of reads_counter (fast2q.py:536-558): resolves fixed vs
 * anchored mode and search_iterations, builds the Phred fail thresholds (initializer :1112-1129). */
int f2q_create(const f2q_params *p, f2q_ctx **out);
void f2q_destroy(f2q_ctx *ctx);
const char *f2q_last_error(const f2q_ctx *ctx);   /* ctx may be NULL: last f2q_create error   */

/* ---- library (Counter mode) ---------------------------------------------------------------
 * Replaces binary_converter (fast2q.py:188-213) and the `features` dict as a lookup structure.
 * seqs/offs: n sequences concatenated, offs has n+1 entries; already upper-cased and
 * de-duplicated in loader order by features_loader (:148-166), which stays in Python.
 * Feature i <-> row i of the count vector. */
int f2q_set_features(f2q_ctx *ctx, const char *seqs, const uint32_t *offs, uint32_t n);

/* ---- counting ------------------------------------------------------------------------------
 * All counting entry points ACCUMULATE into the context's device-resident count vector and
 * 5 stats (like Features.counts += 1, fast2q.py:366); read them with f2q_read_counts. */

/* fastq_parser over an in-memory FASTQ buffer (fast2q.py:324-393): 4-line framing with
 * rstrip(), trailing partial record ignored.  *consumed (optional) = bytes up to the end of the
 * last complete record so a caller can stream a file in blocks. */
int f2q_count_block(f2q_ctx *ctx, const uint8_t *fastq, size_t nbytes, size_t *consumed, f2q_timing *t);
/* The same for FASTQ text that is ALREADY in device memory: f2q_text_upload copies at most 1 GiB of text once;
 * f2q_count_text frames, packs and counts it on the device (the ingest kernels + the counting kernels, no host-to-device
 * copy in the call; accumulating like f2q_count_block, *consumed = bytes up to the end of the last complete record) and
 * may be called any number of times.  What the tile layout costs to produce, without PCIe in the way (bench.py:
 * end_to_end.device_text_to_counts); a producer that fills device memory itself would enter here.  The read-side half of
 * reads_counter, fast2q.py:560-578, once the bytes are on the device. */
typedef struct f2q_text f2q_text;
int f2q_text_upload(f2q_ctx *ctx, const uint8_t *fastq, size_t nbytes, f2q_text **out);
int f2q_count_text(f2q_ctx *ctx, f2q_text *text, size_t *consumed, f2q_timing *t);
void f2q_text_free(f2q_ctx *ctx, f2q_text *text);
/* An in-memory BGZF buffer (bgzip / BCL Convert output) inflated on the device into a device-resident text that
 * f2q_count_text counts: one workgroup per member (k_inflate_bgzf), CRC-32 and ISIZE checked as gzip does.  Replaces
 * the reference's gzip.open + line iteration (fast2q.py:566-578) for such a buffer.  F2Q_EUNSUPPORTED: the buffer is not
 * a run of whole BGZF members of at most 64 KiB of text each; F2Q_EINVAL: more than 1 GiB of text.  F2Q_ETRUNCATED: a
 * member is damaged; *out is still set and holds the text of the members before it. */
int f2q_text_from_bgzf(f2q_ctx *ctx, const uint8_t *bgzf, size_t nbytes, f2q_text **out);
/* A device text back to the host: *nbytes = its size; with dst != NULL (cap >= *nbytes) the bytes too. */
int f2q_text_read(f2q_ctx *ctx, const f2q_text *text, uint8_t *dst, size_t cap, size_t *nbytes);
/* reads_counter's file half (fast2q.py:560-578): plain or .gz FASTQ by path (gzip by content; blocked gzip --
 * BGZF -- is inflated member-parallel).  The file is streamed in pieces by a reader thread while the device
 * frames, packs and counts.  F2Q_ETRUNCATED: the archive is cut off or damaged; every complete line before the damage has
 * been counted, as the reference does (its parser keeps what it counted when readline raises, fast2q.py:405-407, and
 * reads_counter returns those partial counts with a warning; the cut-off last line is never seen).  The harness too.
 * F2Q_DEVICE_INFLATE=1 (off by default): a BGZF regular file whose members each hold at most 64 KiB of text is inflated
 * on the device (k_inflate_bgzf), only its compressed bytes cross PCIe; same counts, same verdict on damage. */
int f2q_count_file(f2q_ctx *ctx, const char *path, f2q_timing *t);
/* The same file counted by `world` processes, one per GPU (replaces the chunk pool of
 * single_file_reads_binner, fast2q.py:447-512): every rank streams the whole file -- the 4-line framing is
 * global -- counts the pieces k with k % world == rank on its device and only frames the others (a newline
 * census on the host); read indices stay global, so Extract+Count tables merge by key with min(first).
 * The sum over the ranks of counts and stats equals f2q_count_file's. */
int f2q_count_file_shard(f2q_ctx *ctx, const char *path, uint32_t rank, uint32_t world, f2q_timing *t);

/* The same job without any rank reading -- or inflating -- another rank's share (regular files, plain or BGZF): the
 * file is cut into pieces, piece k belongs to rank k % world.  Plain: byte ranges of piece_bytes (4096 ... 1 GiB - 2 MiB:
 * a piece and its look-ahead are framed with 32-bit offsets; F2Q_EINVAL outside that range).  BGZF: runs
 * of whole members whose text adds up to at most piece_bytes (every member carries its compressed size in the header
 * and its text size in the trailer, so the cut needs no inflating); a rank inflates only its own runs -- once for the
 * census, once to count -- plus the few members behind a run that finish its last record.  The 4-line framing is
 * global, so the ranks first exchange how many lines each piece holds:
 *   1. f2q_file_pieces   -- number of pieces; *shardable = 1 plain, 2 BGZF, 0 for ordinary gzip / pipes / BGZF with
 *                           other members inside (use f2q_count_file_shard there)
 *   2. f2q_census_pieces -- census[2k] = newlines of piece k, census[2k+1] = 1 if it ends with one, for THIS rank's pieces
 *                           (the other entries are left as they are: pass a zeroed vector)
 *   3. the caller sums the census vectors over the ranks (one all-reduce of 2 * n_pieces uint64)
 *   4. f2q_count_pieces  -- counts the records whose first line starts in this rank's pieces (global read indices)
 * F2Q_EUNSUPPORTED from step 4: a line longer than the 1 MiB look-ahead behind a piece; nothing usable was counted on
 * this rank -- reset and use f2q_count_file_shard.  Errors of the two context-free calls: f2q_last_error(NULL). */
int f2q_file_pieces(const char *path, uint64_t piece_bytes, uint64_t *n_pieces, int *shardable);
int f2q_census_pieces(const char *path, uint32_t rank, uint32_t world, uint64_t piece_bytes, uint64_t *census, uint64_t n_pieces);
int f2q_count_pieces(f2q_ctx *ctx, const char *path, uint32_t rank, uint32_t world, uint64_t piece_bytes,
                     const uint64_t *census, uint64_t n_pieces, f2q_timing *t);

/* ---- paired-end samples ---------------------------------------------------------------------
 * The reference reads one file per sample; a dual-guide or barcode-plus-guide screen sequenced paired-end has part A at
 * a fixed place in R1 and part B at a fixed place in R2.  A paired context counts such a sample as the reference counts
 * ONE read with n_start + n_start2 windows (fast2q.py:349-367,382-393): record i of the first text pairs with record i of
 * the second (header lines are not compared; the reference never looks at them, :324-328); the parts are the context's
 * --st windows of mate 1, then the start2 windows of mate 2, each upper(seq[s:s+l]) of its own mate with Python-slice
 * clipping at the end of THAT mate (:354), each tested against --ph on its own quality slice (:355-360), failed parts
 * left out, the rest joined with ':' (:362); Counter mode matches the key with --m (:364-367), Extract+Count takes it as
 * a key (:382-387); the five counters as for one read, F2Q_READS counting pairs (:389-393).  With revcomp != 0 mate 2 is
 * taken reverse-complemented: its sequence reversed and complemented byte by byte (A<->T, C<->G, a<->t, c<->g, any other
 * byte unchanged), its quality line reversed.
 *
 * f2q_set_mate2 makes a fixed-offset context (no --us/--ds) a paired context: after f2q_create and before
 * f2q_set_features, which builds the joined-key index (F2Q_ESTATE afterwards or when called twice); F2Q_EINVAL for an
 * anchored context, n_start2 < 1, a negative start or n_start + n_start2 > F2Q_MAX_ITER.  From then on f2q_count_block,
 * f2q_block_from_fastq, f2q_count_text, f2q_count_file*, f2q_count_pieces and f2q_synth_create return F2Q_ESTATE on the
 * context, and the *_paired calls return F2Q_ESTATE on any other context. */
int f2q_set_mate2(f2q_ctx *ctx, const int32_t *start2, int32_t n_start2, int32_t revcomp);
/* fastq_parser (fast2q.py:324-393) over two in-memory FASTQ buffers in lockstep: counts min(records1, records2) pairs;
 * *consumed1 / *consumed2 (optional) = per text, the bytes up to the end of the last record used, so a caller can stream
 * two files in blocks.  rstrip() framing per text, a trailing partial record ignored, as f2q_count_block. */
int f2q_count_block_paired(f2q_ctx *ctx, const uint8_t *fastq1, size_t n1, const uint8_t *fastq2, size_t n2,
                           size_t *consumed1, size_t *consumed2, f2q_timing *t);
/* The same pairs packed into a device-resident block for f2q_count_resident / f2q_count_resident_queued (below): a clean
 * pair takes the tile slot the merged read would take, so the counting kernels run as they are (fast2q.py:349-367 over
 * the pair).  Less than 1 GiB of text per mate. */
int f2q_block_from_fastq_paired(f2q_ctx *ctx, const uint8_t *fastq1, size_t n1, const uint8_t *fastq2, size_t n2, f2q_block **out);
/* reads_counter's file half (fast2q.py:560-578) for the two files of a paired sample: each path plain, gzip or BGZF by
 * content (the two need not be alike), streamed in lockstep in pieces of F2Q_FILE_CHUNK bytes of text.  F2Q_EPAIRING:
 * one file holds complete records beyond the other's last; the common pairs stay counted.  F2Q_ETRUNCATED: an archive
 * is cut off or damaged; the pairs completed before the damage stay counted (as :405-407,580-582 keep what was counted). */
int f2q_count_file_paired(f2q_ctx *ctx, const char *path1, const char *path2, f2q_timing *t);

/* Device-resident blocks: the roofline entry points.  f2q_synth_create generates the §8(d)
 * reads on the device straight into the packed tile layout; f2q_block_from_fastq packs a host
 * FASTQ buffer the same way f2q_count_block does but keeps it resident; f2q_count_resident runs
 * the hot path over a resident block (this is what bench.py times). */
int f2q_synth_create(f2q_ctx *ctx, const f2q_synth *spec, f2q_block **out);
int f2q_block_from_fastq(f2q_ctx *ctx, const uint8_t *fastq, size_t nbytes, f2q_block **out);
int f2q_count_resident(f2q_ctx *ctx, const f2q_block *blk, f2q_timing *t);
/* The same without waiting: the launches are queued on the context's stream and the step gets its own pair of HIP
 * events; f2q_queued_times waits for the stream, returns the kernel time of every step queued since the last call
 * (kernel_ms[0 .. min(*n, cap))) and forgets them.  For callers that queue block after block (bench.py's timed loop). */
int f2q_count_resident_queued(f2q_ctx *ctx, const f2q_block *blk);
int f2q_queued_times(f2q_ctx *ctx, float *kernel_ms, uint32_t cap, uint32_t *n);
int f2q_block_info(const f2q_block *blk, uint64_t *n_reads, uint64_t *n_general, uint64_t *device_bytes);
void f2q_block_free(f2q_ctx *ctx, f2q_block *blk);

/* The guide set the generator plants into reads: by default the library given to f2q_set_features;
 * Extract+Count contexts (which take no library) and tests set it explicitly. n*length ACGT bytes. */
int f2q_synth_guides(f2q_ctx *ctx, const char *seqs, uint32_t n, uint32_t length);
/* Host-side twin of the device generator: FASTQ text of reads [lo,hi) of `spec` against the
 * library given to f2q_set_features. Two-call pattern: buf == NULL returns the size in *nbytes. */
int f2q_synth_fastq(f2q_ctx *ctx, const f2q_synth *spec, uint64_t lo, uint64_t hi, uint8_t *buf, size_t *nbytes);
/* n unique uniform ACGT strings of `length` bases (tests/synth.py make_library); out = n*length bytes */
int f2q_synth_library(uint64_t seed, uint32_t n, uint32_t length, char *out);

/* Global index of the next block's first read (default: running count of reads seen).  Only the
 * first-occurrence order of Extract+Count keys depends on it; sharded callers set it per block. */
int f2q_set_read_base(f2q_ctx *ctx, uint64_t first_read_index);

/* ---- results -------------------------------------------------------------------------------- */
/* A new job: every result reads zero from here on.  No host synchronisation.  The clear of counts + stats is left to
 * whatever touches them next on the context's stream (the step's first slab reduce stores over them instead); once
 * f2q_counts_device_ptr has handed the raw pointer out, the clear is queued here and now. */
int f2q_reset_counts(f2q_ctx *ctx);
/* Counter mode: counts[n_features] + stats[5] (device -> host, synchronises the stream). */
int f2q_read_counts(f2q_ctx *ctx, int64_t *counts, int64_t stats[5]);
/* Device address of the int64[n_features + 5] accumulator (counts then stats), so a caller can
 * all-reduce it in place over RCCL (torch.distributed) before reading it back.  No synchronisation is done here:
 * work on the accumulator must be ordered after the context's stream (f2q_stream), e.g. by issuing it on that stream. */
int f2q_counts_device_ptr(f2q_ctx *ctx, void **dptr, uint64_t *n_int64);
/* The HIP stream (hipStream_t) all work of this context is launched on. */
void *f2q_stream(f2q_ctx *ctx);

/* Extract+Count results (the de-novo dict of fast2q.py:382-387). Two-call pattern: sizes first,
 * then the caller allocates keys[n_bytes], offs[n_keys+1], counts[n_keys], first_read[n_keys]
 * (index of the first read that produced the key, so the caller can restore dict order). */
int f2q_ec_size(f2q_ctx *ctx, uint64_t *n_keys, uint64_t *n_bytes);
int f2q_ec_fetch(f2q_ctx *ctx, char *keys, uint64_t *offs, int64_t *counts, uint64_t *first_read);

/* ---- Extract+Count with a library ------------------------------------------------------------
 * The reference makes a run either Counter or Extract+Count (fast2q.py:364,382).  Its Counter-mode outcome for a read is
 * a function of the read's joined key alone: `seq in features`, else mismatch_search_handler(seq, ...), else
 * non-aligned (fast2q.py:362-380).  So one Extract+Count pass plus one match per DISTINCT key gives the de-novo table,
 * the feature every key belongs to, and the exact Counter-mode count vector and stats of the same reads.
 *
 * f2q_set_assign_library gives an Extract+Count context the library to match its keys against; seqs/offs/n as for
 * f2q_set_features (binary_converter, fast2q.py:188-213; features_loader :148-166 stays in Python), the allowed
 * mismatches are the context's --m (f2q_params.miss, unused by Extract+Count counting itself).  Once per context, before
 * or after counting, also on a paired context (the keys are then the ':'-joined parts of both mates); counting is
 * unchanged by it.  F2Q_ESTATE on a Counter context or when called twice. */
int f2q_set_assign_library(f2q_ctx *ctx, const char *seqs, const uint32_t *offs, uint32_t n);
/* Matches every key the Extract+Count tables hold NOW (exact hit fast2q.py:365-367, else the unique-nearest search of
 * mismatch_search_handler :692-750, else non-aligned :379-380), each weighted by the reads that carried it:
 * counts[n] = what Counter mode would have counted per feature, stats[5] = its five counters (F2Q_READS and
 * F2Q_QUALITY_FAILED are the context's own, :389-393).  The result is computed afresh by every call -- it never adds
 * to an earlier one -- and only it crosses to the host.  t->kernel_ms: HIP-event time of the assign kernels.
 * F2Q_ESTATE when no assign library has been set. */
int f2q_ec_assign(f2q_ctx *ctx, int64_t *counts, int64_t stats[5], f2q_timing *t);
/* Per key, in exactly the order f2q_ec_fetch returns the keys: the feature index the last f2q_ec_assign gave it (-1:
 * none -- non-aligned, fast2q.py:379-380 / :734-750 with no unique nearest feature) and its mismatches (0 for an exact
 * hit :365-367, -1: none); arrays of n_keys (f2q_ec_size) entries, either may be NULL.  F2Q_ESTATE when the tables have
 * changed since that f2q_ec_assign (a counting call, f2q_reset_counts) or it was never called. */
int f2q_ec_fetch_assigned(f2q_ctx *ctx, int32_t *feature, int32_t *dist);

/* ---- Extract+Count without a library: extracted keys one base apart collapsed -----------------
 * Random-barcode pools, lineage barcodes, Tn-seq tags: most distinct keys of such a run are sequencing errors of a few
 * true ones.  The reference has no counterpart and no outside tool is reproduced; the rule below is the specification
 * (it is in the spirit of message passing between Hamming neighbours, with ONE best parent per key so that the outcome
 * is a function of the key -> reads table alone: not of read order, table size or growth history).
 *
 *     def eligible(key):                                   # plain keys of the single-word table
 *         return 1 <= len(key) <= 29 and set(key) <= set("ACGT")
 *
 *     def ec_collapse(table, ratio):                       # table: {key: reads}  ->  {key: (centroid, cluster_reads)}
 *         parent = {}
 *         for b, nb in table.items():
 *             if not eligible(b):
 *                 continue                                 # never a child, never a parent
 *             best = None
 *             for j in range(len(b)):                      # the earliest substituted position wins a tie ...
 *                 for x in "ACGT":                         # ... then the alphabetically smallest substituted base
 *                     if x == b[j]:
 *                         continue
 *                     a = b[:j] + x + b[j + 1:]            # same length, one substitution; `a` is eligible as `b` is
 *                     if a in table and table[a] >= ratio * nb and (best is None or table[a] > table[best]):
 *                         best = a
 *             if best is not None:
 *                 parent[b] = best                         # ratio >= 2: a parent has strictly more reads, a forest
 *         def centroid(k):
 *             while k in parent:
 *                 k = parent[k]
 *             return k
 *         cluster = dict.fromkeys(table, 0)
 *         for k, n in table.items():
 *             cluster[centroid(k)] += n
 *         return {k: (centroid(k), cluster[k]) for k in table}         # cluster_reads of a non-centroid is 0
 *
 * Keys with an 'N', keys longer than 29 bases, ':'-joined keys of several parts, the empty key and everything else the
 * byte-string table holds are their own centroids with their own reads.  The comparison is made in 64 bits.
 *
 * f2q_ec_collapse: dist 1 collapses the keys the tables hold NOW; dist 0 makes every key its own centroid (all four
 * counters zero, nothing launched); any other dist, or a ratio outside 2 .. 255, is F2Q_EINVAL.  extra = eligible keys,
 * absorbed keys (keys with a parent), the reads of the absorbed keys, the longest parent chain.  The call is ordered
 * after everything that still counts into the tables, as f2q_ec_assign is, and synchronises the stream; t->kernel_ms is
 * the HIP-event time of its two kernels.  The result is computed afresh by every call, the call may come any number of
 * times, also between counting calls, and changes nothing another call reads.  F2Q_ESTATE on a Counter context,
 * F2Q_ENOMEM when the scratch (16 bytes per slot of the single-word table) cannot be had: the tables stay intact.
 *
 * f2q_ec_fetch_collapsed: per key, in exactly the order f2q_ec_fetch returns the keys: centroid[i] = the index, in that
 * order, of key i's centroid (i itself for a centroid), cluster_reads[i] as in the rule; arrays of n_keys (f2q_ec_size)
 * entries, either may be NULL.  F2Q_ESTATE when the tables have changed since that f2q_ec_collapse (a counting call,
 * f2q_reset_counts, a growth) or it was never called.
 * Not implemented: two mismatches, insertions and deletions between keys, keys with 'N' or longer than 29 bases,
 * multi-part and paired keys, collapsing across samples or ranks, a child's reads split among several parents. */
int f2q_ec_collapse(f2q_ctx *ctx, int32_t dist, int32_t ratio, int64_t extra[4], f2q_timing *t);
int f2q_ec_fetch_collapsed(f2q_ctx *ctx, uint64_t *centroid, int64_t *cluster_reads);

/* ---- distinct UMIs per feature ---------------------------------------------------------------
 * Libraries with an inline UMI next to the feature: how many MOLECULES does a feature's read count stand for?  The
 * reference has no counterpart; the verdict of every read stays the reference's (fast2q.py:362-380), so counts, the
 * five counters and everything made from them are what the same context gives without the call.
 *
 * f2q_set_umi names the UMI window [start, start + length) of every read, a plain read position in fixed-offset and
 * anchored runs alike; after f2q_create and before counting.  F2Q_ESTATE on an Extract+Count or a paired context, when
 * called twice or after a counting call; F2Q_EINVAL unless start >= 0 and 1 <= length <= 16.  From then on every read
 * of the context takes the byte-exact raw-record road (k_count_umi) through every counting entry point; f2q_set_mate2,
 * and the sharded calls with world > 1, return F2Q_ESTATE (the sets of several ranks are not merged).
 *
 * The UMI of a read is upper(seq[start:start+length]); it is valid when the read holds all `length` bases, each of them
 * is A/C/G/T, and the quality slice of the same positions is complete and passes --ph by the rule of a feature window
 * (fast2q.py:355-360).  A read assigned to feature f, exactly or within --m, with a valid UMI u brings the pair (f, u);
 * the set compares UMIs by identity (f2q_umi_collapse joins near ones afterwards).  The set of pairs lives across the pieces of a file and across
 * counting calls until f2q_reset_counts; it grows through the context's device-memory cache (F2Q_ENOMEM: a larger set
 * could not be allocated, the old one is intact).
 *
 * f2q_read_umis (synchronises the stream, as f2q_read_counts): umis[n_features] = distinct UMIs seen per feature;
 * extra[0] = assigned reads with a valid UMI, extra[1] = assigned reads with an invalid one; extra[0] + extra[1] ==
 * F2Q_PERFECT + F2Q_IMPERFECT.  Either pointer may be NULL.  F2Q_ESTATE without f2q_set_umi. */
int f2q_set_umi(f2q_ctx *ctx, int32_t start, int32_t length);
int f2q_read_umis(f2q_ctx *ctx, int64_t *umis, int64_t extra[2]);

/* ---- UMIs at Hamming distance 1 collapsed per feature -----------------------------------------
 * One substitution inside a UMI turns one molecule into two, so the distinct UMIs of a feature are an upper bound that
 * grows with depth.  f2q_umi_collapse joins them by the "cluster" rule of UMI-tools: for one feature f take the distinct
 * valid UMIs the set holds for f (those f2q_read_umis counts); two of them are joined when they differ in exactly one of
 * their `length` bases (a substitution: same length, no indels); molecules[f] is the number of connected components of
 * that graph.  UMIs of different features are never joined.  extra[0] = pairs the set holds (the nodes), extra[1] =
 * joined unordered pairs, each once, over all features (the edges); with no edges molecules[f] == umis[f].  The result
 * depends on the set alone -- not on read order, the set's size or its growth -- so it is exact and reproducible.
 * The count-aware "directional" rule is f2q_umi_collapse_directional below; "adjacency" is not implemented.
 *
 * dist 1 collapses; dist 0 returns umis[] and 0 edges; anything else is F2Q_EINVAL.  F2Q_ESTATE without f2q_set_umi;
 * F2Q_ENOMEM when the scratch (4 bytes per slot of the set, 8 per feature) cannot be had: the set is intact.  Nothing
 * counted yet: all zero.  The call synchronises the stream, as f2q_read_umis; either pointer may be NULL.  It may come
 * any number of times, also between counting calls, and changes no state that another call reads.
 * F2Q_TRACE=1 prints one line per call: "[f2q trace] UMI collapse: P pairs, E edges, M molecules, T ms (...)". */
int f2q_umi_collapse(f2q_ctx *ctx, int32_t dist, int64_t *molecules, int64_t extra[2]);

/* ---- reads per (feature, UMI) pair; the directional rule ---------------------------------------
 * f2q_set_umi_reads(ctx, on != 0) makes the set keep, next to every pair, the number of reads that brought it: 32 bits
 * per pair, carried along when the set grows, cleared by f2q_reset_counts.  After f2q_set_umi and before counting:
 * F2Q_ESTATE without f2q_set_umi or once a counting call has been made.  Counts, the five counters, f2q_read_umis and
 * f2q_umi_collapse are what the same context gives without the call.
 *
 * A pair's count wraps at 2^32.  Every wrap is excluded on the host: f2q_umi_collapse_directional and f2q_umi_pairs
 * return F2Q_EUNSUPPORTED once the context has counted 2^32 or more reads with a valid UMI (f2q_read_umis' extra[0]);
 * below that no pair can have wrapped.
 *
 * f2q_umi_collapse_directional: the "directional" rule of UMI-tools (its default).  For one feature, with c(x) the reads
 * of UMI x: a absorbs b when they differ in exactly one base and c(a) >= 2 c(b) - 1; UMI-tools visits the UMIs by
 * descending count and every UMI not yet reached from an earlier one starts a molecule.  Which UMIs end up together
 * depends on the order among equal counts, the NUMBER of molecules does not, and molecules[f] is that number:
 *   #{ v : c(v) >= 2 and no neighbour u has c(u) >= 2 c(v) - 1 }
 * + #{ connected components of the UMIs with c == 1 in which no member has a neighbour u with c(u) >= 2 }
 * so that f2q_umi_collapse's molecules[f] <= molecules[f] <= umis[f].  extra[0] = pairs the set holds, extra[1] =
 * unordered pairs of them one base apart (f2q_umi_collapse's edges), extra[2] = pairs some neighbour absorbs directly,
 * extra[3] = the sum of the reads of all pairs (f2q_read_umis' extra[0]).  Group membership is not reported.
 * F2Q_ESTATE unless f2q_set_umi_reads(ctx, 1) came before counting; F2Q_ENOMEM when the scratch (8 bytes per slot of the
 * set, 8 per feature) cannot be had or the set has more than 2^31 slots: the set is intact.  Nothing counted yet: all
 * zero.  The call synchronises the stream; either pointer may be NULL; it may come any number of times, also between
 * counting calls, and changes no state that another call reads.  F2Q_TRACE=1 prints one line per call:
 * "[f2q trace] UMI collapse directional: P pairs, E edges, D dominated, M molecules, R reads, T ms (...)".
 *
 * f2q_umi_pairs: every pair with its reads, sorted by (feature, codes) -- a function of the set, not of read order.
 * codes holds the UMI's bases as 2-bit codes (A, C, G, T = 0 .. 3), base j in bits 2j .. 2j+1.  *n = pairs held; with
 * all three arrays NULL that is all (call once for n, then with arrays of cap >= n entries; any of them may be NULL).
 * F2Q_EINVAL when cap < n; F2Q_ESTATE without reads kept; F2Q_ENOMEM when the host copy of the set (12 bytes per slot)
 * cannot be had.  Synchronises the stream. */
int f2q_set_umi_reads(f2q_ctx *ctx, int32_t on);
int f2q_umi_collapse_directional(f2q_ctx *ctx, int64_t *molecules, int64_t extra[4]);
int f2q_umi_pairs(f2q_ctx *ctx, uint64_t cap, uint64_t *n, uint32_t *feature, uint32_t *codes, uint32_t *reads);

/* ---- UMIs on paired-end samples ----------------------------------------------------------------
 * Libraries with the feature at a fixed place in one mate and the UMI at the 5' end of the other, or split over both.
 * f2q_set_umi_paired makes a paired Counter context (f2q_set_mate2, fixed windows) keep the same (feature, UMI) set:
 * f2q_read_umis, f2q_umi_collapse, f2q_set_umi_reads, f2q_umi_collapse_directional, f2q_umi_pairs, the growth of the set
 * and f2q_reset_counts work on it unchanged, through f2q_count_block_paired, f2q_block_from_fastq_paired +
 * f2q_count_resident and f2q_count_file_paired (the set lives across the pieces of the files).
 *
 * The UMI of a pair has one or two parts.  Part 1 is [start1, start1 + length1) of mate 1, part 2 is
 * [start2, start2 + length2) of mate 2; a length of 0 means no part in that mate.  Positions in mate 2 are positions in
 * its own text AS SEQUENCED, whatever f2q_set_mate2's revcomp says: revcomp concerns the feature parts only, the UMI
 * text is never complemented or reversed.  At least one part is present, length1 + length2 <= 16, each present part
 * has a start >= 0 and a length >= 1.  The UMI is part 1 followed by part 2; in the set's 2-bit codes base j of that
 * concatenation sits in bits 2j .. 2j+1 (f2q_umi_pairs' layout with length1 + length2 bases).
 *
 * A part is valid by f2q_set_umi's rule applied to its own mate, the per-mate rule the feature parts follow: all its
 * bases lie inside that mate's rstrip()-ed sequence line, each is A/C/G/T (lower case counts), and the same positions
 * of that mate's rstrip()-ed quality line are complete and pass --ph.  The UMI is valid when every present part is.
 * A pair is decided exactly as without the call: an assigned pair with a valid UMI brings (feature, UMI), any other
 * assigned pair counts as one with an invalid UMI -- counts, the five counters and every other output are unchanged,
 * and f2q_read_umis' extra[0] + extra[1] == F2Q_PERFECT + F2Q_IMPERFECT.  The collapse rules see the concatenation as
 * one string of length1 + length2 bases: a substitution in either part is one edge.
 *
 * The call comes once, after f2q_set_mate2 and before counting.  F2Q_ESTATE on a context that is not paired, on an
 * Extract+Count context, on one that is a UMI context already, or after a counting call; F2Q_EINVAL when both lengths
 * are 0, a start or a length is negative, a start is above 0x3FFFFFFF, or length1 + length2 > 16.  F2Q_UMI_SLOTS is
 * honoured as by f2q_set_umi; f2q_set_umi_reads may follow.  f2q_set_umi on a paired context and f2q_set_mate2 on a UMI
 * context stay F2Q_ESTATE, and so do the sharded calls with world > 1.  Every pair of the context takes the merged-record
 * road (k_count_umi_pair); F2Q_UMI_PAIR_STAGE=0 / 1 picks that kernel's layout for A/B runs. */
int f2q_set_umi_paired(f2q_ctx *ctx, int32_t start1, int32_t length1, int32_t start2, int32_t length2);

/* ---- UMIs in read headers -----------------------------------------------------------------------
 * umi_tools extract and fastp --umi move the UMI out of the read and append it to the read id (@NAME_ACGTACGT);
 * bcl-convert / bcl2fastq write an index-read UMI as the last colon field of the id (@M0:7:FC:1:1101:100:200:ACGTACGT
 * 1:N:0:ATCACG), a dual UMI as ACGT+TTGA.  f2q_set_umi_header makes a Counter context keep the same (feature, UMI) set
 * from those: f2q_set_umi_reads, f2q_read_umis, f2q_umi_collapse, f2q_umi_collapse_directional, f2q_umi_pairs,
 * F2Q_UMI_SLOTS, the growth of the set and f2q_reset_counts work on it unchanged.
 *
 * The rule, for a record's line 0 (`header_line`, bytes), sep (one byte) and length L:
 *
 *     def header_umi(header_line, sep, L):           # -> bytes or None
 *         h = header_line.rstrip()                   # rstrip()-ed as the other three lines are
 *         for i, c in enumerate(h):
 *             if c in b" \t": h = h[:i]; break       # the read id: up to the first space or tab
 *         k = h.rfind(bytes([sep]))
 *         if k < 0: return None                      # no separator in the id
 *         tail = h[k + 1:]
 *         if tail.count(b"+") > 1: return None       # at most one '+' (dual UMI) is skipped, wherever it stands
 *         tail = tail.replace(b"+", b"")
 *         if len(tail) != L or set(tail.upper()) - set(b"ACGT"): return None
 *         return tail.upper()                        # lower case counts, as for f2q_set_umi; an N makes it invalid
 *
 * There is no Phred test (a header has no quality) and a leading '@' is not asked for.  In the set's 2-bit codes base j
 * of the returned string sits in bits 2j .. 2j+1, as everywhere else.  Every read is decided exactly as without the call:
 * an assigned read with a valid header UMI brings (feature, UMI), any other assigned read counts as one with an invalid
 * UMI (f2q_read_umis' extra[1]).  On a paired context the UMI of a pair is read from MATE 1's header by the same rule;
 * mate 2's header is neither looked at nor compared.
 *
 * On a single-end Counter context the call takes the place of f2q_set_umi, on a paired one (after f2q_set_mate2) that of
 * f2q_set_umi_paired; it comes once, before counting.  F2Q_EINVAL unless sep is one printable ASCII byte (33 .. 126)
 * that is not alphanumeric and not '+', and 1 <= length <= 16.  F2Q_ESTATE on an Extract+Count context, on a context that
 * is a UMI context already, after a counting call; afterwards for the sharded calls with world > 1, for f2q_synth_create
 * (its blocks have no headers) and for f2q_count_resident on a block made before the call.  Every entry point that takes
 * FASTQ text or files carries the UMI: f2q_count_block, f2q_block_from_fastq + f2q_count_resident, f2q_count_text,
 * f2q_count_file (plain, gzip, BGZF, F2Q_DEVICE_INFLATE=1) and the three paired calls.  The header is read at ingest
 * (k_header_umi on the framed text, one entry per record, owned by the block; the F2Q_HOST_PACK=1 road fills the same
 * array on the host) and the counting kernels take the UMI from there.  Not implemented: a header UMI combined with an
 * inline part, UMIs in the comment after the first space, comparing the two mates' headers. */
int f2q_set_umi_header(f2q_ctx *ctx, int32_t sep, int32_t length);

/* ---- pooled samples: inline sample barcodes -----------------------------------------------------
 * Pooled amplicon and CRISPR libraries are often multiplexed with a 6 .. 12 base tag at a fixed position of the same read
 * that carries the feature.  It is no i5/i7 index, so the sequencer's software does not split on it.
 * f2q_set_sample_barcodes makes a single-end Counter context decide, for EVERY read, which of n barcodes the read carries,
 * and keep a count matrix [sample][feature] next to everything it kept before.
 *
 * The rule, for the rstrip()-ed sequence and quality lines of a record, the barcode start S >= 0, the common length L
 * (1 .. 16) of the nb (1 .. 1024) barcodes -- A/C/G/T only, upper-cased on the way in, pairwise distinct -- and M in {0, 1}:
 *
 *     def barcode_of(seq, qual, S, L, phred, barcodes, M):       # -> (sample, verdict)
 *         nb = len(barcodes)
 *         if S + L > len(seq) or S + L > len(qual): return nb, UNREADABLE
 *         ph = max(phred, 1)
 *         if any(33 <= c <= min(ph + 31, 126) for c in qual[S:S + L]): return nb, UNREADABLE   # --ph, as a feature window
 *         w = seq[S:S + L].upper()
 *         d = [sum(x != y for x, y in zip(w, b)) for b in barcodes]   # bytes compared: an 'N' differs from every base
 *         if 0 in d: return d.index(0), EXACT                         # unique: the barcodes are distinct
 *         if M == 1 and d.count(1) == 1: return d.index(1), ONE_MISMATCH
 *         if M == 1 and d.count(1) > 1: return nb, AMBIGUOUS
 *         return nb, NO_MATCH
 *
 * The barcode verdict is independent of the feature verdict.  Counts, the five counters and every other output are what
 * the same context gives without the call.  A read whose verdict is UNREADABLE, AMBIGUOUS or NO_MATCH belongs to the
 * pseudo-sample nb, "unassigned".
 *
 * f2q_set_sample_barcodes: seqs holds n * length bytes, barcode b at seqs[b * length].  It comes once, after f2q_create
 * and before counting (before or after f2q_set_features; a new library starts a new matrix).  F2Q_ESTATE on an
 * Extract+Count context, a paired context (f2q_set_mate2), a UMI context of any kind, a context that has the barcodes
 * already, or after a counting call; afterwards f2q_set_umi, f2q_set_umi_paired, f2q_set_umi_header, f2q_set_mate2 and
 * the sharded calls with world > 1 are F2Q_ESTATE in turn.  F2Q_EINVAL for n outside 1 .. 1024, length outside 1 .. 16,
 * start < 0, miss not 0 / 1, a byte that is not A/C/G/T (either case) or two equal barcodes: the message names the
 * offending barcode.  F2Q_ENOMEM when the matrix ((n + 1) * n_features words of 8 bytes) cannot be had: nothing was
 * counted into it, and the call that failed (this one, f2q_set_features or the counting call) may be repeated.
 * From then on every read takes the raw-record road (k_count_demux), through f2q_count_block, f2q_block_from_fastq +
 * f2q_count_resident / f2q_count_resident_queued, f2q_count_text and f2q_count_file (plain, gzip, BGZF,
 * F2Q_DEVICE_INFLATE=1, F2Q_HOST_PACK=1); the state lives across the pieces of a file and across counting calls.
 * F2Q_DEMUX_TABLE=lds / global picks where the kernel reads the barcode table from (A/B runs).
 *
 * f2q_read_demux: matrix[b * n_features + f] = reads of sample b assigned to feature f (row n: unassigned);
 * sample_stats[b * 5 + k] = the five counters of f2q_read_counts restricted to sample b; verdicts = reads with verdict
 * EXACT, ONE_MISMATCH, AMBIGUOUS, NO_MATCH, UNREADABLE (F2Q_BC_*).  It synchronises as f2q_read_counts does; any pointer
 * may be NULL; F2Q_ESTATE without f2q_set_sample_barcodes.  f2q_reset_counts zeroes all three.  Invariants:
 *   sum over b of matrix[b][f] == counts[f];  sum over b of sample_stats[b][k] == stats[k];
 *   sum(verdicts) == stats[F2Q_READS];  verdicts[EXACT] + verdicts[ONE_MISMATCH] == sum over b < n of sample_stats[b][F2Q_READS].
 * Not implemented: barcodes in the header comment, in mate 2 or on paired samples, with UMIs, with Extract+Count, on
 * several ranks, indels or staggers in the barcode (one-base indels in the FEATURE are reported by f2q_set_indel, without
 * sample barcodes), distance 2, the packed-tile kernels. */
#define F2Q_BC_EXACT 0
#define F2Q_BC_ONE_MISMATCH 1
#define F2Q_BC_AMBIGUOUS 2
#define F2Q_BC_NO_MATCH 3
#define F2Q_BC_UNREADABLE 4
int f2q_set_sample_barcodes(f2q_ctx *ctx, const char *seqs, uint32_t n, int32_t length, int32_t start, int32_t miss);
int f2q_read_demux(f2q_ctx *ctx, int64_t *matrix /* (n+1) * n_features */, int64_t *sample_stats /* (n+1) * 5 */, int64_t verdicts[5]);

/* ---- read orientation: single reads counted on the reverse strand, or on either ------------------
 * Ligation-based amplicon libraries, PCR-free preps and pools with flipped amplicons come off the sequencer with the
 * feature on the reverse strand of some or all reads: reverse-complemented, at the other end of the read.
 * f2q_set_strand makes a single-end Counter context read every record as its mirror image (F2Q_STRAND_REV), or as
 * written first and as its mirror image when that assigned no feature (F2Q_STRAND_BOTH).
 *
 * The rule.  verdict(seq, qual) is the reference's decision for a record whose rstrip()-ed lines 2 and 4 are seq and
 * qual: the feature or none, and which of the five counters the read adds to.
 *
 *     COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")     # comp8: every other byte stays what it is, case is kept
 *
 *     def mirrored(seq, qual):
 *         # each line is mirrored by ITS OWN length; quality bytes are never translated.  The second rstrip() is
 *         # deliberate: the reverse strand of a record is exactly what the reference would read from the four lines
 *         # "@", revcomp(seq), "+", reversed(qual) -- leading blanks of a line become trailing ones and fall away
 *         return seq.translate(COMP)[::-1].rstrip(), qual[::-1].rstrip()
 *
 *     def strand_verdict(seq, qual, mode):                 # -> (verdict, strand)
 *         if mode == REV:
 *             return verdict(*mirrored(seq, qual)), REVERSE
 *         F = verdict(seq, qual)
 *         if mode == FWD or F.feature is not None:         # forward first: an assigned forward strand is never re-examined,
 *             return F, FORWARD                            # not even when it is imperfect and the reverse strand is perfect
 *         R = verdict(*mirrored(seq, qual))
 *         return (R, REVERSE) if R.feature is not None else (F, FORWARD)   # nobody assigns it: counted as the forward strand counts it
 *
 * It holds for every read shape of the single-end Counter road: fixed windows (one or several, ':'-joined), --us/--ds
 * anchors with --msu/--msd/--qsu/--qsd, any --m, any --ph.  Consequences: BOTH on a sample without reverse-strand reads
 * gives the plain run; counts under BOTH are >= counts under FWD for every feature; REV on a text equals a plain run on
 * the text with every record mirrored.
 *
 * f2q_set_strand comes after f2q_create and before counting (before or after f2q_set_features).  Mode 0 is accepted on
 * every context, at any time, and changes nothing.  F2Q_EINVAL for a mode outside the three.  With a non-zero mode:
 * F2Q_ESTATE on an Extract+Count context, a paired context (f2q_set_mate2), a UMI context of any kind, a demultiplexing
 * context (f2q_set_sample_barcodes), a context that has a non-zero mode already, or after a counting call; afterwards
 * f2q_set_mate2, f2q_set_umi, f2q_set_umi_paired, f2q_set_umi_header, f2q_set_sample_barcodes and the sharded calls with
 * world > 1 are F2Q_ESTATE in turn, with a message that names the strand mode.  From then on every read takes the
 * raw-record road (k_count_strand), through f2q_count_block, f2q_block_from_fastq + f2q_count_resident /
 * f2q_count_resident_queued, f2q_count_text and f2q_count_file (plain, gzip, BGZF, F2Q_DEVICE_INFLATE=1,
 * F2Q_HOST_PACK=1); the state lives across the pieces of a file and across counting calls.
 *
 * f2q_read_strands: rev_counts[f] = reads assigned to feature f on the reverse strand; extra[0] = reads assigned on the
 * forward strand, extra[1] / extra[2] = reads assigned perfectly / imperfectly on the reverse strand, extra[3] = reads
 * whose reverse strand was examined.  It synchronises as f2q_read_counts does; either pointer may be NULL; F2Q_ESTATE
 * without a non-zero mode.  f2q_reset_counts zeroes it; a new library starts it afresh.  Invariants:
 *   rev_counts[f] <= counts[f];  sum(rev_counts) == extra[1] + extra[2];
 *   extra[0] + extra[1] + extra[2] == stats[F2Q_PERFECT] + stats[F2Q_IMPERFECT];
 *   BOTH: extra[3] == stats[F2Q_READS] - extra[0];
 *   REV:  extra[0] == 0, extra[3] == stats[F2Q_READS], rev_counts == counts.
 * Not implemented: Extract+Count, paired samples, UMIs and sample barcodes with a strand mode, several ranks, the best
 * of both strands by distance, the packed-tile kernels. */
#define F2Q_STRAND_FWD 0
#define F2Q_STRAND_REV 1
#define F2Q_STRAND_BOTH 2
int f2q_set_strand(f2q_ctx *ctx, int32_t mode);
int f2q_read_strands(f2q_ctx *ctx, int64_t *rev_counts /* n_features */, int64_t extra[4]);

/* ---- pair libraries: each part matched alone, recombinants counted --------------------------------
 * Dual-guide and barcode x guide pools are A:B features over two windows.  The reference joins the two windows with ':'
 * and matches the JOINED key with --m mismatches in total (fast2q.py:362-380); a perfectly good A next to a perfectly good
 * B that the library does not pair -- a recombinant, from template switching in PCR or lentiviral packaging -- is then
 * "non-aligned", next to junk.  f2q_set_parts makes a Counter context with exactly two fixed windows give every read, next
 * to the reference's verdict, one verdict per part, and keep new tables from them.  Counts, the five counters and every
 * other output stay what the same context gives without the call.
 *
 * The rule.  features = the library of f2q_set_features, every one "A:B" with A and B non-empty.
 *
 *     def part_libraries(features):                    # ids in first-occurrence order; the two id spaces are separate
 *         lib1, lib2 = [], []                          # (a sequence may be a part 1 and a part 2)
 *         for f in features:
 *             a, b = f.split(":")
 *             if a not in lib1: lib1.append(a)
 *             if b not in lib2: lib2.append(b)
 *         return lib1, lib2
 *
 *     def part_verdicts(read, run):                    # -> ((kind1, i1), (kind2, i2))
 *         # verdict_i = what a Counter run with the single window --st s_i --l L, the run's --ph and --m, gives this read
 *         # against part library i: PERFECT (id), IMPERFECT (id: the unique nearest within --m), NON_ALIGNED or
 *         # QUALITY_FAILED (fast2q.py:349-380 with one window).  Single-end: both windows of the one read.  Paired: window 1
 *         # on mate 1, window 2 on mate 2 as the run takes it (reverse-complemented, its quality reversed, under revcomp).
 *         # A clipped window, lower case, 'N' and the unique-nearest rule all follow; --m counts mismatches PER PART here.
 *         return counter_verdict(lib1, read, s_1), counter_verdict(lib2, read, s_2)
 *
 *     def parts_class(v1, v2, features):               # -> (class, feature or None)
 *         a1, a2 = v1.kind in (PERFECT, IMPERFECT), v2.kind in (PERFECT, IMPERFECT)
 *         if not a1 and not a2: return NEITHER, None
 *         if not a2: return PART1_ONLY, None
 *         if not a1: return PART2_ONLY, None
 *         key = lib1[v1.id] + ":" + lib2[v2.id]
 *         if key not in features: return RECOMBINANT, None
 *         f = features.index(key)                      # a repeated feature: the first, the exact hit of the joined key
 *         return (PAIR_PERFECT if v1.kind == v2.kind == PERFECT else PAIR_IMPERFECT), f
 *
 * Per read: PAIR_* adds 1 to parts_counts[f]; RECOMBINANT adds 1 to the reads of (i1, i2) in a growing set; every assigned
 * part adds 1 to its marginal (part1_reads[i1], part2_reads[i2]) whatever the other part did.  At --m 0 parts_counts equals
 * counts.  Invariants: sum(classes) == stats[F2Q_READS]; sum(parts_counts) == classes[PAIR_PERFECT] + classes[PAIR_IMPERFECT];
 * the reads of the set add up to classes[RECOMBINANT]; sum(part1_reads) == pairs + recombinant + part1_only (part 2 alike).
 *
 * f2q_set_parts comes once, after f2q_create (and f2q_set_mate2) and before counting, before or after f2q_set_features; a
 * new library rebuilds the part libraries and the pair table and starts new tables.  F2Q_ESTATE, the message naming the
 * cause: an Extract+Count context, --us/--ds, a window count other than two (paired: other than one per mate), a UMI
 * context of any kind, a demultiplexing context, a non-zero strand mode, called twice or after a counting call; afterwards
 * f2q_set_umi, f2q_set_umi_paired, f2q_set_umi_header, f2q_set_sample_barcodes, f2q_set_strand with a non-zero mode,
 * f2q_set_mate2 and the sharded calls with world > 1 are F2Q_ESTATE in turn.  F2Q_EINVAL, from this call or from
 * f2q_set_features on such a context, naming the feature: a feature that is not two non-empty parts.  F2Q_ENOMEM leaves the
 * context as it was.  From then on every read takes the raw-record road (k_count_parts) through f2q_count_block,
 * f2q_block_from_fastq + f2q_count_resident / f2q_count_resident_queued, f2q_count_text, f2q_count_file (plain, gzip, BGZF,
 * F2Q_DEVICE_INFLATE=1, F2Q_HOST_PACK=1) and the three paired calls.  The recombinant set lives across the pieces of a file
 * and across counting calls and grows through the context's device-memory cache; F2Q_PARTS_SLOTS=n sets its first size;
 * F2Q_TRACE=1 names every rehash and prints n1, n2 and the pair table's slots once.
 *
 * f2q_parts_info: the sizes of the two part libraries.  f2q_read_parts (synchronises as f2q_read_counts does; any pointer
 * may be NULL): parts_counts[n_features], part1_reads[n1], part2_reads[n2], classes[6] in the order of F2Q_PARTS_*.
 * f2q_parts_recombinants: every pair of the set with its reads, sorted by (i1, i2) -- a function of the set, not of read
 * order.  *n = pairs held; with all three arrays NULL that is all; F2Q_EINVAL when cap < n.  A pair's reads are 32 bits:
 * F2Q_EUNSUPPORTED once the context has counted 2^32 recombinant reads.  f2q_reset_counts clears all of it.
 * Not implemented: three or more parts, anchored runs, UMIs / sample barcodes / a strand mode on a parts context, several
 * ranks (everything is additive), the packed-tile kernels. */
#define F2Q_PARTS_PAIR_PERFECT 0
#define F2Q_PARTS_PAIR_IMPERFECT 1
#define F2Q_PARTS_RECOMBINANT 2
#define F2Q_PARTS_PART1_ONLY 3
#define F2Q_PARTS_PART2_ONLY 4
#define F2Q_PARTS_NEITHER 5
int f2q_set_parts(f2q_ctx *ctx);
int f2q_parts_info(f2q_ctx *ctx, uint32_t *n1, uint32_t *n2);
int f2q_read_parts(f2q_ctx *ctx, int64_t *parts_counts /* n_features */, int64_t *part1_reads /* n1 */, int64_t *part2_reads /* n2 */, int64_t classes[6]);
int f2q_parts_recombinants(f2q_ctx *ctx, uint64_t cap, uint64_t *n, uint32_t *part1, uint32_t *part2, uint32_t *reads);

/* ---- staggered libraries: one fixed window tried at a range of starts ------------------------------
 * Stagger primers put 0 .. 8 extra bases in front of the amplicon, a different number for each read, so the feature
 * starts at s + d with d unknown.  f2q_set_stagger(ctx, n) makes a single-end Counter context with exactly one fixed
 * window (--st s --l L) try that window at the starts s, s + 1, .. s + n.
 *
 * The rule.  V(d) is what the reference decides for the read (its rstrip()-ed lines 2 and 4) in a run with --st s+d --l L
 * and the run's --m and --ph: PERFECT (feature), IMPERFECT (feature), NON_ALIGNED or QUALITY_FAILED.  Clipped windows,
 * lower case, 'N', features of other lengths and the unique-nearest rule all follow from that.
 *
 *     def stagger_verdict(V, n):                           # -> (verdict, offset or None)
 *         for d in range(n + 1):
 *             if V(d).kind == PERFECT:                     # the earliest exact start; it outranks a window with
 *                 return V(d), d                           # mismatches at an earlier start
 *         for d in range(n + 1):
 *             if V(d).kind == IMPERFECT:                   # else the earliest start within --m; a start whose window is
 *                 return V(d), d                           # ambiguous is NON_ALIGNED there and is passed over
 *         return V(0), None                                # nobody assigns it: counted as start s counts it
 *
 * counts and the five counters hold the reads by that rule.  Consequences: a read that the plain run (start s) assigns
 * perfectly keeps that verdict; n on a sample whose features all sit at s gives the plain run's perfect reads at offset 0.
 *
 * f2q_set_stagger comes after f2q_create and before the first counting call, before or after f2q_set_features; it may be
 * repeated with another n.  n = 0 makes the context a plain one again (on a plain context it is accepted at any time
 * and changes nothing): it then launches the kernels it launched before.  F2Q_EINVAL for n outside 0 .. 32.  With
 * n > 0, F2Q_ESTATE with a message that names the cause: an Extract+Count context, a paired context (f2q_set_mate2),
 * --us/--ds, several windows, a window that starts before the first base, a UMI context of any kind, a demultiplexing
 * context, a non-zero strand mode, a parts context, or after a counting call; afterwards f2q_set_mate2, f2q_set_umi,
 * f2q_set_umi_paired, f2q_set_umi_header, f2q_set_sample_barcodes, f2q_set_strand with a non-zero mode, f2q_set_parts
 * and the sharded calls with world > 1 are F2Q_ESTATE in turn.  From then on every read takes the raw-record road
 * (k_count_stagger) through f2q_count_block, f2q_block_from_fastq + f2q_count_resident / f2q_count_resident_queued,
 * f2q_count_text and f2q_count_file (plain, gzip, BGZF, F2Q_DEVICE_INFLATE=1, F2Q_HOST_PACK=1).  F2Q_STAGGER_WALK=1
 * (read by f2q_set_stagger) decides every start by the byte-exact routine instead of from registers: same results.
 *
 * f2q_read_stagger: perfect[d] / imperfect[d] = reads assigned without / with mismatches at offset d, d = 0 .. n;
 * n_offsets must be n + 1 (F2Q_EINVAL otherwise); either pointer may be NULL; F2Q_ESTATE on a plain context.  It
 * synchronises as f2q_read_counts does.  f2q_reset_counts zeroes it; a new library starts it afresh.  Invariants:
 *   sum(perfect) == stats[F2Q_PERFECT];  sum(imperfect) == stats[F2Q_IMPERFECT].
 * Not implemented: Extract+Count, paired samples, anchored runs, several windows, UMIs / sample barcodes / a strand mode /
 * part verdicts with a stagger, several ranks, the packed-tile kernels. */
#define F2Q_STAGGER_MAX_N 32
int f2q_set_stagger(f2q_ctx *ctx, int32_t n);
int f2q_read_stagger(f2q_ctx *ctx, int64_t *perfect /* n + 1 */, int64_t *imperfect /* n + 1 */, int32_t n_offsets);

/* ---- reads whose feature carries one inserted or deleted base ---------------------------------------
 * Single-base deletions are the dominant error of oligo-pool synthesis, insertions follow.  Such a read compares badly
 * at every fixed window, so the plain rule calls it non-aligned.  f2q_set_indel(ctx, 1) makes a single-end Counter context
 * with exactly one fixed window (--st s --l L, 2 <= L <= 31) REPORT these reads next to everything it counts: counts and
 * the five counters stay what they are without the call.
 *
 * The rule.  seq / qual are the rstrip()-ed lines 2 and 4 of the record.  V0 is what the reference decides for the read
 * with the run's --st s --l L --m --ph.  The candidates are the library's features of exactly L bases, all A/C/G/T (a
 * sequence the library holds twice takes part once, under its first index); features of other lengths or with other
 * symbols take part in V0 only.  passes(q) is the Phred test of a feature window: no byte c of q with
 * 33 <= c <= min(max(ph, 1) + 31, 126) when ph > 1, and always true when ph <= 1.
 *
 *     def indel_verdict(V0, seq, qual, s, L, candidates, passes):   # -> (kind, feature, position) or "ambiguous" or None
 *         if V0.kind in (PERFECT, IMPERFECT):              # a substitution match is never re-examined, even where an
 *             return None                                  # indel would explain the read better
 *         D, I = {}, {}                                    # feature -> smallest position
 *         Wd, Qd = seq[s:s + L - 1].upper(), qual[s:s + L - 1]          # the deletion window: L - 1 bases
 *         if len(Wd) == L - 1 and len(Qd) == L - 1 and passes(Qd):
 *             for f in candidates:
 *                 for p in range(L):
 *                     variant = f[:p] + f[p + 1:]
 *                     if variant == f[:L - 1]:             # only says that the window's last base is unknown: it cannot
 *                         continue                         # be told from a substitution of the last base
 *                     if variant == Wd:
 *                         D.setdefault(f, p)
 *         Wi, Qi = seq[s:s + L + 1].upper(), qual[s:s + L + 1]          # the insertion window: L + 1 bases
 *         if len(Wi) == L + 1 and len(Qi) == L + 1 and passes(Qi):
 *             for p in range(L):                           # bytes are compared: one 'N' can be the inserted base and
 *                 f = Wi[:p] + Wi[p + 1:]                  # nothing else; p == L would make the plain window exact
 *                 if f in candidates:
 *                     I.setdefault(f, p)
 *         both = set(D) | set(I)
 *         if len(both) >= 2:
 *             return "ambiguous"                           # counted as such, assigned nothing
 *         for f in both:
 *             return ("ins", f, I[f]) if f in I else ("del", f, D[f])      # L + 1 bases of evidence outrank L - 1
 *         return None
 *
 * --m plays no part in the trial: an indel read has exactly one indel and no substitution.  A read is "tried" when V0
 * assigned it nothing (non-aligned or quality failed), whether or not a window was usable.
 *
 * f2q_set_indel comes after f2q_create and before the first counting call, before or after f2q_set_features (the
 * deletion-variant table is built when both the flag and a library are known).  0 makes the context a plain one again (on a
 * plain context it is accepted at any time and changes nothing): it then launches the kernels it launched before.  With a
 * non-zero value, F2Q_ESTATE with a message that names the cause: an Extract+Count context, a paired context
 * (f2q_set_mate2), --us/--ds, several windows, a window that starts before the first base, L outside 2 .. 31, a UMI context
 * of any kind, a demultiplexing context, a non-zero strand mode, a parts context, a stagger context, or after a counting
 * call; afterwards f2q_set_mate2, f2q_set_umi, f2q_set_umi_paired, f2q_set_umi_header, f2q_set_sample_barcodes,
 * f2q_set_strand with a non-zero mode, f2q_set_parts, f2q_set_stagger with n > 0 and the sharded calls with world > 1 are
 * F2Q_ESTATE in turn.  From then on every read takes the raw-record road (k_count_indel) through f2q_count_block,
 * f2q_block_from_fastq + f2q_count_resident / f2q_count_resident_queued, f2q_count_text and f2q_count_file (plain, gzip,
 * BGZF, F2Q_DEVICE_INFLATE=1, F2Q_HOST_PACK=1).
 *
 * f2q_read_indels: del_counts[f] / ins_counts[f] = deletion / insertion reads of feature f; del_pos[p] / ins_pos[p] =
 * those reads by position p = 0 .. L - 1; totals = reads tried, deletion reads, insertion reads, ambiguous reads.  n_pos
 * must be L (F2Q_EINVAL otherwise); any pointer may be NULL; F2Q_ESTATE on a plain context.  It synchronises as
 * f2q_read_counts does.  f2q_reset_counts zeroes it; a new library starts it afresh.  Invariants:
 *   sum(del_counts) == sum(del_pos) == totals[1];  sum(ins_counts) == sum(ins_pos) == totals[2];
 *   totals[0] == stats[F2Q_NON_ALIGNED] + stats[F2Q_QUALITY_FAILED];  totals[1] + totals[2] + totals[3] <= totals[0].
 * Not implemented: Extract+Count, paired samples, anchored runs, several windows, UMIs / sample barcodes / a strand mode /
 * part verdicts / a stagger with indel reads, several ranks, two edits, an indel next to a substitution, adding indel
 * reads to the counts, the packed-tile kernels. */
int f2q_set_indel(f2q_ctx *ctx, int32_t on);
int f2q_read_indels(f2q_ctx *ctx, int64_t *del_counts /* n_features */, int64_t *ins_counts /* n_features */, int64_t *del_pos /* L */,
                    int64_t *ins_pos /* L */, int32_t n_pos, int64_t totals[4]);

#ifdef __cplusplus
}
#endif
#endif /* F2Q_H */
