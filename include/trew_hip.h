/*
 * trew_hip.h -- C ABI of the MI355X-native TREW scan (libtrew_hip.so).
 *
 * Drop-in boundary for the hot path of Chemical118/TREW (reference @ 2025-02-18):
 * the per-read tandem-repeat detector of src/kmer.cpp.  The reference has no
 * FFI; its de-facto seam is the kmer.h function set between trew.cpp and
 * kmer.cpp.  Each entry point below names the
 * reference interface it replaces.  Plain pointers and sizes only; no C++ or
 * torch types.  All functions return 0 on success, non-zero on error
 * (trew_hip_last_error() gives the text); the CLI layer turns a non-zero status
 * into the reference's "message on stderr + exit(EXIT_FAILURE)" convention
 * (kmer.cpp:84-87, 1007-1008).
 *
 * Packed read format ("bit planes", produced by trew_pack_reads or by the
 * device-side generator): a read of n bases occupies 3*ceil(n/32) 32-bit words,
 * one {lo, hi, nmask} triple per 32 bases; bit i of a triple's words describes
 * base 32*j+i.  code = 2*hi+lo with T=0 G=1 C=2 A=3 (codes[], kmer.cpp:14-31);
 * nmask bit = 1 for any other byte (N, lower/upper IUPAC, '\r', bytes >= 0x80).
 * Bits past the end of the read are zero in lo/hi and may be anything in nmask.
 */
#ifndef TREW_HIP_H
#define TREW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Still 4 with the annotation entry points (trew_motif_parse, trew_hip_annotate, trew_hip_annotate_results,
 * trew_annotate_host), the tract entry points (trew_hip_tracts, trew_hip_tracts_results, trew_tracts_host), the interval
 * entry points (trew_hip_intervals, trew_hip_intervals_results, trew_intervals_host), the variant entry points
 * (trew_hip_variants, trew_hip_variants_results, trew_variants_host), the period entry points (trew_hip_periods,
 * trew_hip_periods_results, trew_periods_host), the satellite entry points (trew_hip_satellites,
 * trew_hip_satellites_results, trew_satellites_host), the alignment entry points (trew_hip_align, trew_hip_align_results,
 * trew_align_host), the refinement entry points (trew_hip_refine, trew_hip_refine_results, trew_refine_host), the tandem
 * entry points (trew_hip_tandems, trew_hip_tandems_results, trew_tandems_host), the traceback entry points (trew_hip_trace,
 * trew_hip_trace_results, trew_trace_host), the decomposition entry points (trew_hip_decompose, trew_hip_decompose_results,
 * trew_decompose_host), the dissection entry points (trew_hip_dissect, trew_hip_dissect_results, trew_dissect_host), the
 * resolution entry points (trew_hip_resolve, trew_hip_resolve_results, trew_resolve_host), the resolved forms of three
 * of them (trew_hip_tandems_resolved, trew_hip_decompose_resolved, trew_hip_dissect_resolved and their _host functions) and
 * the monomer entry points (trew_monomer_parse, trew_hip_monomers, trew_hip_monomers_results, trew_monomers_host), the
 * copies entry points and the polish entry points (trew_hip_polish, trew_hip_polish_results, trew_polish_host): they
 * are purely additive -- no existing
 * structure, enumerator or function changed. */
#define TREW_HIP_ABI_VERSION 4

/* scan modes: which per-read driver of the reference is reproduced */
enum {
    TREW_MODE_SHORT = 0,   /* buffer_task       kmer.cpp:80-266  (trew short)              */
    TREW_MODE_PAIR = 1,    /* buffer_task_pair  kmer.cpp:268-745 (trew short --paired_end) */
    TREW_MODE_LONG = 2,    /* buffer_task_long  kmer.cpp:747-985 (trew long)               */
    TREW_MODE_SEGMENT = 3  /* k_mer_check on every read as one segment, kmer.h:232-236     */
};

/* result tables: ResultMapData = {forward, backward, both} x {high(first), low(second)}, kmer.h:79-81 */
enum {
    TREW_TABLE_FORWARD_HIGH = 0,
    TREW_TABLE_FORWARD_LOW = 1,
    TREW_TABLE_BACKWARD_HIGH = 2,
    TREW_TABLE_BACKWARD_LOW = 3,
    TREW_TABLE_BOTH_HIGH = 4,
    TREW_TABLE_BOTH_LOW = 5,
    TREW_NUM_TABLES = 6
};

/* debug / test flags for trew_hip_params.flags */
enum {
    TREW_FLAG_NO_FILTER = 1, /* skip the bucket-bound prefilter: every k is a candidate (exact path only) */
    TREW_FLAG_DEBUG_NO_EMIT = 2, /* timing experiments only: drop every table update (results are empty) */
    TREW_FLAG_DEBUG_NO_KLOOP = 4, /* timing experiments only: prefilter without its k loop (nothing is flagged) */
    TREW_FLAG_DEBUG_POISON_LDS = 32, /* tests: the exact kernel starts from garbage-filled LDS */
    TREW_FLAG_DEBUG_WIDE_NO_WAIT = 128, /* tests: the wide table (k > 32) never waits for a claimed slot's ready bit -- every such
                                  wait counts as timed out (trew_hip_debug_counters), duplicates are left for collect to merge */
    TREW_FLAG_NO_TIMING = 64, /* no HIP events around the kernels (trew_hip_last_timing is unavailable): for hosts that
                                submit ~10^4 small batches a second and are bound by API calls */
    TREW_FLAG_COMPAT_G1 = 512, /* pair mode, MAX_MER <= 32, n_slots = 1 only: follow the reference's 64-bit pair branch as written --
                                temp_result_left is not cleared after the whole-read block (kmer.cpp:467-505; the 128-bit twin
                                clears it, 722-723), so what that block recorded is added once more by the next pair: to `both`
                                if that pair's four segments chain, else to `forward` (kmer.cpp:378-399, 438-455).  Batches must
                                be submitted in file order; this reproduces the reference run with ONE consumer thread (with
                                more its output depends on scheduling).  Default: the cleared semantics. */
    TREW_FLAG_DEBUG_NO_JOINT = 2048, /* tests: the prefilter's uniform path judges every segment in a k loop of its own instead of both
                                halves of a read in one (filter_halves_uni); the flagged reads may differ by a few (odd lengths use a
                                joint threshold), the tables never */
    TREW_FLAG_DEBUG_NO_UNI_DRAIN = 4096, /* tests and A/B runs: the prefilter judges the reads its uniform path set aside with the
                                general per-segment path (filter_segment) instead of the joint loop of filter_deferred_uni; the
                                flagged reads may differ only where a segment's [kmin, kmax] is narrower than the k loop, the tables never */
    TREW_FLAG_DEBUG_NO_GROUP = 1024, /* tests and A/B runs: the exact kernel gives every segment a wave of its own (decide()) instead
                                of deciding four segments in lock step, 16 lanes each (decide_group); results are identical */
    TREW_FLAG_DEBUG_ANNOT_GENERAL = 8192, /* tests: trew_hip_annotate gives every batch a wave per read, also where its reads are
                                short enough for the lane-per-read kernel; results are identical */
    TREW_FLAG_DEBUG_SMALL_BOUNDS = 16384, /* tests: the buffer in which the bounds pass hands the packed bounds of the flagged short reads
                                to the exact kernel holds 64 worklist entries instead of a share of max_batch_reads, so that a small
                                batch has reads on either side of it (stored bounds / bounds in row layout); results are identical */
    TREW_FLAG_DEBUG_NO_LIVE_LIST = 32768, /* tests and A/B runs: the bounds pass neither sharpens the bound of halves with an N on sixteen
                                buckets nor drops the worklist entries no k of which can still count; the exact kernel reads the
                                prefilter's worklist and the 8-bucket words (trew_hip_debug_live_list then returns the worklist,
                                and no entry is counted dead); results are identical */
    TREW_FLAG_DEBUG_ONE_CU = 65536, /* tests: the wave-per-read kernels of the per-read measures get the grid of a one-CU device, 8 blocks
                                and 32 waves, so a batch of a few thousand reads gives every wave many reads (the scan's kernels and
                                annotate's lane-per-read kernel keep their grids; trew_hip_debug_measure_grid tells the blocks);
                                results are identical */
    TREW_FLAG_TRACK_PRESSURE = 256 /* every batch ends with a copy of the table's fill counters into pinned host memory, and
                                trew_hip_table_pressure answers from those copies (and from what collect / add_rows /
                                reset read since) instead of asking the device: for hosts that ask before every batch.
                                Like the device query, the answer does not include batches still in flight. */
};

/* Replaces the eight configuration globals MIN_MER ... HIGH_BASELINE
 * (kmer.h:55-63, set in trew.cpp:165-172, 246-253). */
typedef struct {
    int32_t min_mer;          /* MIN_MER, >= 3 (ABS_MIN_MER)                                  */
    int32_t max_mer;          /* MAX_MER, <= 64; > 32 selects the 128-bit-word kernels         */
    double low_baseline;      /* LOW_BASELINE  (-L)                                           */
    double high_baseline;     /* HIGH_BASELINE (-H)                                           */
    int32_t slice_length;     /* SLICE_LENGTH (-s), long mode only                            */
    int32_t mode;             /* TREW_MODE_*                                                  */
    int32_t device;           /* HIP device ordinal                                           */
    int32_t n_slots;          /* batch slots (one HIP stream each), 1 .. 512                  */
    uint64_t max_batch_words; /* capacity of one slot's packed-read buffer, 32-bit words      */
    uint64_t max_batch_reads; /* capacity of one slot, reads (pairs count as two)             */
    uint32_t table_log2_slots;/* device count table: 2^table_log2_slots entries (>= 12)       */
    uint32_t flags;           /* TREW_FLAG_*                                                  */
    uint64_t max_batch_ascii_bytes; /* ABI 3: capacity of one slot for trew_hip_submit_ascii (sequence bytes + 12 B per
                                 read of index arrays); 0 = text batches are not used            */
} trew_hip_params;

/* Replaces QueueData / PairQueueData + LocationVector (kmer.h:73, 93-103): one
 * chunk of reads handed to the consumer.  The caller keeps ownership of every
 * pointer until trew_hip_wait(slot) returns.  With on_device != 0 the pointers
 * are device pointers and nothing is copied.
 * Host batches: when the three arrays lie back to back in one (pinned) buffer, laid out [offsets][lengths][words]
 * (lengths == offsets + n_reads, words == lengths + n_reads) or [words][offsets][lengths] (offsets == words +
 * n_words, lengths == offsets + n_reads), the batch is shipped with a single asynchronous copy; any other layout
 * works too and costs three. */
typedef struct {
    const uint32_t *words;    /* packed triples                                               */
    uint64_t n_words;
    const uint32_t *offsets;  /* word offset of each read, or NULL: read r starts at r*uniform_stride */
    const uint32_t *lengths;  /* bases of each read, or NULL: every read has uniform_length   */
    uint32_t uniform_length;
    uint32_t uniform_stride;
    uint64_t n_reads;         /* number of reads; in pair mode reads 2i and 2i+1 are mates (R1, R2) */
    int32_t on_device;
    int32_t max_length;       /* on_device + lengths only: longest read of the batch (0 = unknown) */
} trew_hip_batch;

/* The same chunk as TEXT, closest to what the reference's consumers pop (QueueData: a char buffer plus the [st, nd]
 * locations of the sequence lines, kmer.h:93-96): the bytes of the sequence lines only, in one pinned host buffer, and the
 * DEVICE applies codes[] (kmer.cpp:14-31) -- a pack kernel in front of the prefilter -- so that host threads only locate
 * lines and copy bytes.  Two shapes:
 *   uniform  byte_offsets == lengths == word_offsets == NULL: read r is bases[r * uniform_length .. + uniform_length)
 *   ragged   read r is bases[byte_offsets[r] .. + lengths[r]); word_offsets[r] = 3 * sum_{q<r} ceil(lengths[q] / 32), the
 *            place of its first packed triple (a running sum the host has anyway)
 * When the arrays lie back to back as [word_offsets][byte_offsets][lengths][bases] the batch is shipped with one copy.
 * The caller keeps ownership until trew_hip_wait(slot).  n_bytes + 12 * n_reads <= max_batch_ascii_bytes. */
typedef struct {
    const char *bases;
    uint64_t n_bytes;
    const uint32_t *byte_offsets;
    const uint32_t *lengths;
    const uint32_t *word_offsets;
    uint32_t uniform_length;
    uint32_t reserved;
    uint64_t n_reads;         /* pair mode: reads 2i and 2i+1 are mates                       */
} trew_hip_ascii_batch;

/* one (k, word) -> count row; word = the 2k-bit k-mer, first base most
 * significant (KmerSeq, kmer.h:77); word_hi is 0 for k <= 32. */
typedef struct {
    int32_t k;
    int32_t table;
    uint64_t word_lo;
    uint64_t word_hi;
    uint64_t count;
} trew_hip_row;

typedef struct trew_hip_ctx trew_hip_ctx;

/* Replaces set_extract_k_mer / set_rotation_table / ThreadData set-up,
 * trew.cpp:382-406: allocates streams, device buffers, the count table. */
int trew_hip_init(const trew_hip_params *params, trew_hip_ctx **out);
void trew_hip_destroy(trew_hip_ctx *ctx);
/* Text of the calling thread's last failing call (several host threads may share a context, one slot each);
 * ctx may be NULL: last trew_hip_init error. */
const char *trew_hip_last_error(const trew_hip_ctx *ctx);

/* Replaces one pop+process iteration of buffer_task* (kmer.cpp:106-177):
 * asynchronously copies the batch (unless on_device), runs the prefilter and
 * the exact kernel on the slot's stream, accumulating into the device tables. */
int trew_hip_submit(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot);
/* trew_hip_submit for a chunk of text: copies the batch, packs it on the device (bit planes identical to
 * trew_pack_reads, word for word) and runs the two kernels on the packed reads. */
int trew_hip_submit_ascii(trew_hip_ctx *ctx, const trew_hip_ascii_batch *batch, int slot);
/* Diagnostic: packs `batch` on the device exactly as trew_hip_submit_ascii does and copies the packed words back
 * (words_cap words available; *n_words = words the batch packs to).  Tests compare them with trew_pack_reads. */
int trew_hip_pack_ascii(trew_hip_ctx *ctx, const trew_hip_ascii_batch *batch, uint32_t *words, uint64_t words_cap, uint64_t *n_words);
/* Blocks until the slot's work is done (tasks.wait, kmer.cpp:1323-1325). */
int trew_hip_wait(trew_hip_ctx *ctx, int slot);

/* Replaces the thread merge of process_output (kmer.cpp:1486-1515): waits for
 * every slot and returns the rows of one table (any order).  *n_rows receives
 * the number of rows in the table even when it exceeds cap. */
int trew_hip_collect(trew_hip_ctx *ctx, int table, trew_hip_row *rows, uint64_t cap, uint64_t *n_rows);
/* Clears the six tables (start of a new file, kmer.cpp:89). */
int trew_hip_reset_tables(trew_hip_ctx *ctx);
/* Adds rows (e.g. another rank's tables) into the device tables. */
int trew_hip_add_rows(trew_hip_ctx *ctx, const trew_hip_row *rows, uint64_t n_rows);

/* ---- cross-GPU reduction of the tables; the reference's only counterpart is the
 * single-threaded map merge of process_output, kmer.cpp:1486-1515, and the cross-file merge, trew.cpp:454-467 ----
 * Counts are sums, so a table is reduced by adding every other table's rows into it.
 *
 * trew_hip_collect_device: device-to-device form of trew_hip_collect(table = -1) for an exchange that never
 * leaves HBM (one process per GPU: the caller all_gathers d_rows with RCCL).  d_rows is a device buffer of cap
 * rows on the context's GPU; *n_rows receives the number of rows there are (nothing is written past cap, call
 * again with a larger buffer).  Rows may repeat a key (spilled rows); every consumer below merges by adding.
 * trew_hip_add_rows_device: trew_hip_add_rows for rows that already live on the context's GPU.
 * trew_hip_merge: one process driving several GPUs (`trew --devices 0,1,...`): adds every row of src's tables
 * into dst's tables with one peer copy (xGMI between two GPUs); src is left unchanged. */
int trew_hip_collect_device(trew_hip_ctx *ctx, trew_hip_row *d_rows, uint64_t cap, uint64_t *n_rows);
int trew_hip_add_rows_device(trew_hip_ctx *ctx, const trew_hip_row *d_rows, uint64_t n_rows);
int trew_hip_merge(trew_hip_ctx *dst, trew_hip_ctx *src);
/* The whole exchange behind ONE collective (ABI 3).  Every rank owns one slice of 1 + slice_rows rows of a gather
 * buffer: row 0 is the slice's header (count = number of rows the rank has, everything else 0), rows 1.. are what
 * trew_hip_collect_device wrote.  After a single all_gather of the slices, d_buf holds n_slices of them and this call
 * adds the rows of every slice but own_slice into the context's tables with one kernel over the whole buffer
 * (preceded by a validation pass on the same stream: a row out of range fails the call and NOTHING is added).
 * producer_stream: the HIP stream (hipStream_t) the collective ran on -- the kernels are ordered behind it on the
 * device, no host synchronisation in between; NULL = wait for the whole device first.
 * *max_rows receives the largest header count.  If it exceeds slice_rows some rank's rows did not fit: nothing was
 * added anywhere (every rank sees the same headers), the call returns 0 and the caller repeats the exchange with
 * larger slices.  Matches the thread merge of process_output, kmer.cpp:1486-1515 (sums over contributors). */
int trew_hip_add_gathered_device(trew_hip_ctx *ctx, const trew_hip_row *d_buf, uint32_t n_slices, uint32_t own_slice,
                                 uint64_t slice_rows, void *producer_stream, uint64_t *max_rows);
/* The producing side of that exchange with no host hop (ABI 4): compacts the context's tables straight into rows 1.. of
 * d_slice (1 + slice_rows rows of device memory) and writes the header row -- count = rows the rank has, which may
 * exceed slice_rows (then only slice_rows of them are there and trew_hip_add_gathered_device reports it on every rank) --
 * with a kernel of its own behind the compaction; the spill log is appended on the device as well.  consumer_stream:
 * the HIP stream the collective will be issued on; it is made to wait for the header on the device (and this call first
 * waits, on the device, for what that stream still has queued on the slice), so the host neither reads the count nor
 * writes the header.  NULL = synchronise the device before and after instead.  n_rows may be NULL; asking for the count
 * costs one host synchronisation.  Replaces the size exchange a merge of per-thread maps needs (kmer.cpp:1486-1515). */
int trew_hip_collect_slice_device(trew_hip_ctx *ctx, trew_hip_row *d_slice, uint64_t slice_rows, void *consumer_stream, uint64_t *n_rows);

/* Fill state of the device tables (a snapshot; does not wait for running batches).  The reference's hash maps
 * grow without bound (absl::flat_hash_map, kmer.h:79); the device table has a fixed number of slots, rows that
 * find their partition full go to a spill log of spill_capacity rows, and only a full log loses counts (then
 * trew_hip_collect fails).  A host that scans unbounded input calls this between batches and, when
 * used_slots nears total_slots or spilled_rows > 0, drains: trew_hip_collect, keep the rows, trew_hip_reset_tables.
 * Any pointer may be NULL.  With TREW_FLAG_TRACK_PRESSURE the call touches no device (see the flag). */
int trew_hip_table_pressure(trew_hip_ctx *ctx, uint64_t *used_slots, uint64_t *total_slots, uint64_t *spilled_rows,
                            uint64_t *spill_capacity);

/* How often the kernels took their rare fall-back paths since the last trew_hip_reset_tables (waits for every slot).
 * Diagnostic: tests assert that each path is live code and that results still equal the oracle when it runs.
 * (The three fall-back counters are kept per DEVICE: contexts that share a GPU share them.)
 * out[0] decide(): speculative skip refused, segment decided again with every k counted
 * out[1] eval_runs(): more than 64 runs of adjacent same-class windows, classes counted window by window
 * out[2] wide table (k > 32): gave up waiting for a slot's ready bit (collect merges the duplicate slot this can leave)
 * out[3] keys inserted into the narrow table, out[4] into the wide table
 * out[5] decide_group(): a 16-lane row gave its segment back to decide() (an N where a class count was needed, a k with
 *        more than 16 runs and no skip slot left, a failed skip check)
 * out[6] reads of the group pass routed and recorded by the wave-per-segment code, out[7] whose k_mer_target was counted by it.
 * out[8] prefilter, uniform batches of short or paired reads: units of which only one half had to be judged after the fast
 *        loop (an N in it, or a 4-bucket pass) and was, a lane per half; out[9] units judged whole by the same drain (two or
 *        more such halves).  Both count items drained, flagged or not.
 * out[10] worklist entries the bounds pass of the most recent submit found dead (both halves bounded, no k of either with a pass
 *        bit, no whole-read segment) and kept from the exact kernel; unlike the others a figure of ONE launch, and zero after
 *        trew_hip_reset_tables, without a bounds pass and with TREW_FLAG_DEBUG_NO_LIVE_LIST.
 * n <= TREW_DEBUG_COUNTERS entries are written. */
#define TREW_DEBUG_COUNTERS 11
int trew_hip_debug_counters(trew_hip_ctx *ctx, uint64_t *out, int n);

/* Diagnostic: the unit indices (reads, or pairs in pair mode) the prefilter of the last submit on `slot` handed to the exact
 * kernel, in worklist order (after trew_hip_wait).  *n receives their number even when it exceeds cap.  Tests use it to assert
 * that the prefilter is sound: every read with a (segment, k) that k_mer_check accepts (kmer.cpp:2221-2258) must be there. */
int trew_hip_debug_worklist(trew_hip_ctx *ctx, int slot, uint32_t *units, uint64_t cap, uint64_t *n);

/* Diagnostic: the unit indices the exact kernel of the last submit on `slot` walked, in its order (after trew_hip_wait): the live
 * entries the bounds pass kept of the worklist's leading ones, then the worklist's entries beyond the hand-over buffer, which that
 * pass does not look at.  A subset of trew_hip_debug_worklist as a multiset; equal to it where no bounds pass ran (other modes,
 * MAX_MER > 32, TREW_FLAG_DEBUG_NO_GROUP) and with TREW_FLAG_DEBUG_NO_LIVE_LIST.  Arguments as trew_hip_debug_worklist. */
int trew_hip_debug_live_list(trew_hip_ctx *ctx, int slot, uint32_t *units, uint64_t cap, uint64_t *n);

/* Diagnostic: the blocks (of four waves, a wave per read) the launcher of the per-read measures below would start for a batch of
 * n_reads reads on this context -- on the device's compute units, or on one with TREW_FLAG_DEBUG_ONE_CU.  A wave of that grid
 * works through reads wave, wave + 4 * blocks, ...; tests use it to assert that their batches give every wave a second read.
 * Touches no device.  Also additive: TREW_HIP_ABI_VERSION stays 4. */
int trew_hip_debug_measure_grid(trew_hip_ctx *ctx, uint64_t n_reads, uint32_t *blocks);

/* Per-read results of the last submit on `slot` (after trew_hip_wait): for
 * TREW_MODE_SEGMENT the (k_high, k_low, MAX_SEQ at k_high, MAX_SEQ at k_low)
 * that k_mer_check returns / reports through repeat_seq (kmer.cpp:2260-2262,
 * 2327).  Arrays of n_reads entries; any may be NULL.  seq_* hold the low 64 bits of
 * the word, seq_*_hi the high 64 bits (non-zero only for k > 32). */
int trew_hip_segment_results(trew_hip_ctx *ctx, int slot, int32_t *k_high, int32_t *k_low,
                             uint64_t *seq_high, uint64_t *seq_low, uint64_t *seq_high_hi, uint64_t *seq_low_hi,
                             uint64_t n_reads);
/* Candidate-k masks of the prefilter for the last submit on `slot`: bit (k-1)
 * of cand[r*slots_per_read + s] is set when k survived for segment s of read r.
 * Diagnostic: used to test that the prefilter never drops a passing k. */
int trew_hip_filter_masks(trew_hip_ctx *ctx, const trew_hip_batch *batch, uint64_t *cand, int slots_per_read);

/* Mean kernel timings of the submits on `slot` since the previous call (HIP events on the
 * slot's own stream, at most the last 128 submits), milliseconds; n_flagged (optional) = reads
 * the prefilter passed to the exact kernel in the last submit.  ms_exact covers everything queued
 * behind the prefilter: the bounds pass over the worklist, where a batch takes one, and the exact kernel. */
int trew_hip_last_timing(trew_hip_ctx *ctx, int slot, float *ms_filter, float *ms_exact, uint64_t *n_flagged);

/* ---- per-read annotation against given motifs (no counterpart in the reference, which only sums over reads) ----
 * For a read of n bases and a motif M of k bases (3 <= k <= 32): window i (0 <= i <= n - k) is valid when none of its k
 * bases has its nmask bit set; it matches strand fwd when it is valid and a rotation of M (its smallest rotation as a 2k-bit
 * word, get_rot_seq kmer.cpp:1815-1823, equals that of M), strand rev when it is a rotation of the reverse complement of M.
 *   windows_s      number of matching windows of strand s
 *   tract_start_s  first window of the longest run of consecutive matching windows (the earliest run on a tie)
 *   tract_len_s    that run's length in BASES: its number of windows + k - 1; no run: start = len = 0
 * A self-reverse-complementary class reports the same numbers on both strands; non-primitive motifs and homopolymers follow
 * the same definition; n < k gives zeros. */
typedef struct {
    int32_t k;        /* 3 .. 32 */
    int32_t reserved; /* 0 */
    uint64_t word;    /* any rotation of the motif, packed like trew_hip_row.word_lo: first base most significant, no bits above 2k */
} trew_hip_motif;
typedef struct {
    uint32_t windows_fwd, windows_rev, tract_start_fwd, tract_len_fwd, tract_start_rev, tract_len_rev;
} trew_hip_annot;
#define TREW_ANNOT_MAX_MOTIFS 8

/* "TTAGGG" (upper or lower case A, C, G, T only) -> motif; host only.  Non-zero for any other character or a k outside [3, 32]
 * (text through trew_hip_last_error with a NULL context). */
int trew_motif_parse(const char *text, trew_hip_motif *out);
/* Annotates every read of the batch against n_motifs (1 .. 8) motifs.  Behaves like trew_hip_submit: the same batch shapes,
 * copied the same way, queued on the slot's stream, asynchronous; the caller keeps the batch until trew_hip_wait(slot).  Works
 * on a context of any mode (in pair mode the mates are two reads) and is independent of the scan: it neither reads nor writes
 * the count tables and may be interleaved with submits on any slot.  max_batch_words / max_batch_reads apply, the scan's
 * read-length rules do not.  Batches whose longest read has at most 256 bases (uniform_length, the lengths of a host batch,
 * max_length of a device-resident one; 0 = unknown) run one lane per read, all others one wave per read. */
int trew_hip_annotate(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs);
/* Waits for the slot and copies the records of its last trew_hip_annotate: out[r * n_motifs + m], n_reads * n_motifs of them;
 * *n receives that number even when it exceeds cap (then cap records are copied).  ms_kernel (may be NULL): kernel time from
 * HIP events on the slot's stream. */
int trew_hip_annotate_results(trew_hip_ctx *ctx, int slot, trew_hip_annot *out, uint64_t cap, uint64_t *n, float *ms_kernel);
/* The same records computed on the host, window by window, over packed planes (words / offsets / lengths as trew_pack_reads
 * writes them): what tests compare the device with where the inputs are large. */
int trew_annotate_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                       const trew_hip_motif *motifs, int n_motifs, trew_hip_annot *out);

/* ---- error-tolerant terminal tracts per read (how long is the telomere at the end of this read?) ----
 * match_s[i] as above.  cov_s[p] (0 <= p < n) = 1 when some matching window of strand s contains base p, else 0: one
 * substitution inside a perfect repeat removes k windows but leaves only that base uncovered.  score(p) = +1 when covered,
 * else -penalty (1 <= penalty <= 64); S(e) = sum of score(p) over p < e, S(0) = 0.
 *   covered_s   number of covered bases
 *   head_len_s  the smallest e in [0, n] at which S(e) is largest (0 when the maximum is 0): the tract at the 5' end
 *   head_cov_s  covered bases among the first head_len_s
 *   tail_len_s  n - b, b the largest position in [0, n] at which S(b) is smallest: the best-scoring suffix, the 3' tract
 *   tail_cov_s  covered bases among the last tail_len_s
 * On ties the shorter tract wins at both ends; n < k gives zeros; a self-reverse-complementary class reports the same numbers
 * on both strands.  Also additive: TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t covered_fwd, head_len_fwd, head_cov_fwd, tail_len_fwd, tail_cov_fwd;
    uint32_t covered_rev, head_len_rev, head_cov_rev, tail_len_rev, tail_cov_rev;
} trew_hip_tract;
/* Like trew_hip_annotate (batch shapes, staging, asynchronous on the slot's stream, independent of the scan and of the
 * annotation), with a result buffer of its own that the slot's first call allocates.  One kernel, a wave per read, for every
 * read length. */
int trew_hip_tracts(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, int penalty);
/* Waits for the slot and copies the records of its last trew_hip_tracts; arguments as trew_hip_annotate_results. */
int trew_hip_tracts_results(trew_hip_ctx *ctx, int slot, trew_hip_tract *out, uint64_t cap, uint64_t *n, float *ms_kernel);
/* The same records on the host, base by base from the definition, over packed planes. */
int trew_tracts_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                     const trew_hip_motif *motifs, int n_motifs, int penalty, trew_hip_tract *out);

/* ---- gap-tolerant motif intervals anywhere in a read (where in this read does the repeat lie, and how many tracts are there?) ----
 * cov_s[p] as above.  Every motif m has a rule {max_gap, min_len}: max_gap is any u32, min_len >= 1.  With the covered
 * positions of strand s p_1 < p_2 < ..., an interval is a maximal group of consecutive covered positions in which every two
 * neighbours satisfy p_(j+1) - p_j - 1 <= max_gap.  Its record:
 *   start    its first covered position (0-based)
 *   end      its last covered position + 1
 *   covered  the number of covered bases in [start, end)
 * An interval is kept when end - start >= min_len.  n < k or no covered base gives no interval; start and end - 1 are always
 * covered; the intervals of one (read, motif, strand) are disjoint and more than max_gap uncovered bases apart; a
 * self-reverse-complementary class yields the same intervals on both strands, reported under both.  strand: 0 = the motif,
 * 1 = its reverse complement.  Also additive: TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t max_gap, min_len;
} trew_hip_interval_rule; /* one per motif */
typedef struct {
    uint32_t read, motif, strand, start, end, covered;
} trew_hip_interval;
/* Like trew_hip_tracts (batch shapes, staging, asynchronous on the slot's stream, a context of any mode, independent of the
 * scan, the annotation and the tracts), with buffers of its own that the slot's first call allocates: a log of max_intervals
 * records (>= 1; the log grows when a call asks for more) to which the kernel appends every kept interval, and one count per
 * (read, motif, strand).  A batch holds at most 2^32 - 1 reads.  One kernel, a wave per read, for every read length. */
int trew_hip_intervals(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, const trew_hip_interval_rule *rules,
                       int n_motifs, uint64_t max_intervals);
/* Waits for the slot.  *n = the number of kept intervals found, also when that exceeds max_intervals or cap.  Copies
 * min(cap, *n, max_intervals) records sorted by (read, motif, strand, start), so the output does not depend on device
 * scheduling.  counts (n_reads * n_motifs * 2 values, [read][motif][strand]; may be NULL) = the kept intervals of every key,
 * whether or not they fitted in the log.  When *n > max_intervals the records are an unspecified subset while counts and *n
 * are still exact: repeat trew_hip_intervals with max_intervals >= *n -- one retry always suffices.  That case is no error
 * (the call returns 0), like trew_hip_collect with too small a buffer. */
int trew_hip_intervals_results(trew_hip_ctx *ctx, int slot, trew_hip_interval *out, uint64_t cap, uint64_t *n, uint32_t *counts, float *ms_kernel);
/* The same on the host, base by base from the definition, over packed planes: *n = intervals found, min(cap, *n) records
 * (the first ones of the sorted order), counts as above (may be NULL). */
int trew_intervals_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                        const trew_hip_interval_rule *rules, int n_motifs, trew_hip_interval *out, uint64_t cap, uint64_t *n, uint32_t *counts);

/* ---- telomere variant repeats: in-phase variant units per read, batch histogram (what is the repeat made of?) ----
 * Base codes as in trew_motif_parse: T = 0, G = 1, C = 2, A = 3; the complement of code c is 3 - c.  The motif M of k bases is
 * taken AS TYPED (trew_hip_motif.word keeps the typed rotation) and variants are named relative to that rotation.  Target of
 * strand fwd: T_0 = M; of strand rev: T_1 = revcomp(M), T_1[j] = 3 - M[k-1-j].  Window i (0 <= i <= n - k) is valid when none
 * of its k bases has its nmask bit set.  Per strand s:
 *   exact_s[i]  window i is valid and equals T_s base for base (this rotation, not any rotation)
 *   var_s[i]    window i is valid and differs from T_s in exactly one position j, where the read has base c
 * A variant window is ANCHORED when its in-phase neighbour is exact: (i >= k and exact_s[i-k]) or (i + k <= n - k and
 * exact_s[i+k]).  Phase is local: an indel shifts it, nothing global is assumed.  The bin of an anchored variant window is in
 * motif coordinates on both strands: fwd 4 j + c, rev 4 (k-1-j) + (3-c), so TCAGGG on the forward strand and CCCTGA on the
 * reverse strand both land in bin (1, C) of TTAGGG.  A bin whose base equals M[j] is always 0.
 *   units_s      number of windows with exact_s, anchored or not
 *   variants_s   number of anchored variant windows
 *   distinct_s   number of non-zero bins of this read and strand
 *   top_s        the bin with the largest count, the smallest such bin on a tie; TREW_VARIANT_NONE when variants_s = 0
 *   top_count_s  the count of that bin, 0 when there is none
 * n < k: everything 0, top_s = TREW_VARIANT_NONE.  Per batch two arrays of u64, each [motif][strand][bin]:
 *   hist = sum over reads of the read's bin count;  reads_with = number of reads whose bin count is non-zero.
 * Consequences: the bins of a read's histogram sum to variants_s; units_s <= trew_hip_annot.windows_s; a read that is an exact
 * periodic repeat of M has variants = 0; the rev record of a read equals the fwd record of its reverse complement and vice
 * versa, the histograms likewise; for a self-reverse-complementary motif strand rev is strand fwd under (j, c) ->
 * (k-1-j, 3-c).  Only substitutions are variants: a unit with an inserted or deleted base is trew_hip_trace_item's, below, not this measure's (it shifts the
 * phase and is seen by no window).  Also additive: TREW_HIP_ABI_VERSION stays 4. */
#define TREW_VARIANT_BINS 128
#define TREW_VARIANT_NONE 0xffffffffu
typedef struct {
    uint32_t units_fwd, variants_fwd, distinct_fwd, top_fwd, top_count_fwd;
    uint32_t units_rev, variants_rev, distinct_rev, top_rev, top_count_rev;
} trew_hip_variant;
/* Like trew_hip_tracts (batch shapes, staging, asynchronous on the slot's stream, a context of any mode, independent of the
 * scan and of the other three kernels), with buffers of its own that the slot's first call allocates: the records and the
 * two batch histograms, which are zeroed on the slot's stream in front of every launch.  One kernel, a wave per read, for
 * every read length. */
int trew_hip_variants(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs);
/* Waits for the slot and copies the records of its last trew_hip_variants: out[r * n_motifs + m]; *n receives their number
 * even when it exceeds cap (then cap records are copied).  hist / reads_with: n_motifs * 2 * TREW_VARIANT_BINS values each,
 * [motif][strand][bin]; either may be NULL.  ms_kernel (may be NULL): kernel time from HIP events on the slot's stream. */
int trew_hip_variants_results(trew_hip_ctx *ctx, int slot, trew_hip_variant *out, uint64_t cap, uint64_t *n, uint64_t *hist, uint64_t *reads_with,
                              float *ms_kernel);
/* The same on the host, window by window from the definition, over packed planes; hist / reads_with may be NULL. */
int trew_variants_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                       int n_motifs, trew_hip_variant *out, uint64_t *hist, uint64_t *reads_with);

/* ---- de novo repeat period and unit per read: what repeats in this read, with which unit, and where (no motif given) ----
 * Integer-exact (tests/period_ref.py is the brute-force form).  Read of n bases, base p valid when its nmask bit
 * is 0.  Parameters: 1 <= min_period <= max_period <= 32, penalty P in [1, 64], min_score >= 1.
 * Per period k in [min_period, min(max_period, n - 1)]: eq_k[i] (0 <= i < n - k) = bases i and i + k are both valid and
 * equal; score(i) = +1 if eq_k[i], else -P; S_k(e) = sum of score(i) over i < e (e in [0, n - k]); score_k = the largest
 * S_k(e) - min over b <= e of S_k(b), e_k = the smallest e that attains it, b_k = the largest b <= e_k at which S_k is
 * smallest over [0, e_k]: the best-scoring segment of eq_k, the earliest end on a tie, then the shortest segment.
 * k* = the smallest k whose score_k is largest.  No k (n <= min_period) or score_k* < min_score: the record is all zero.
 *   scored_period  k*
 *   score          score_k*
 *   start, end     b and e + k* (end exclusive, in bases)
 *   matches        eq positions in [b, e) = (score + P (e - b)) / (1 + P)
 *   support        with cnt[j][c] = valid bases p in [start, end) with (p - start) mod k* = j and code c (T 0, G 1, C 2, A 3)
 *                  and u[j] = the code with the largest count (the smallest code on a tie, 0 without a valid base): the sum
 *                  of cnt[j][u[j]]
 *   period         the smallest divisor d of k* with u[j] = u[(j + d) mod k*] for all j (on a noisy tract the multiples of
 *                  the true period score within a percent of it; the majority unit's primitive root undoes that)
 *   unit           u[0 .. period - 1] packed like trew_hip_motif.word: first base most significant, no bits above 2 period
 * This is the one best tract of a read; trew_hip_repeats below reports every tract.  Periods above 32 are the business of
 * trew_hip_satellites (further below), not of this record.  Also additive: TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t period, scored_period, score, start, end, matches, support, reserved;
    uint64_t unit;
} trew_hip_period;
/* Like trew_hip_tracts (batch shapes, staging, asynchronous on the slot's stream, a context of any mode, independent of the
 * scan and of the other four kernels), without motifs; the records are a buffer of its own that the slot's first call
 * allocates.  One kernel, a wave per read, for every read length. */
int trew_hip_periods(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score);
/* Waits for the slot and copies the records of its last trew_hip_periods, one per read; arguments as trew_hip_annotate_results. */
int trew_hip_periods_results(trew_hip_ctx *ctx, int slot, trew_hip_period *out, uint64_t cap, uint64_t *n, float *ms_kernel);
/* The same on the host, position by position from the definition, over packed planes. */
int trew_periods_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                      int penalty, uint32_t min_score, trew_hip_period *out);

/* ---- ordered unit chain per read: exact runs and variant units in place (in which order do the units come?) ----
 * Integer-exact (tests/chain_ref.py is the brute-force form).  Base codes, the typed rotation, T_0 / T_1,
 * exact_s[i], var_s[i], "anchored" and the bin are those of the variant repeats above, unchanged.  Per (read, motif, strand s)
 * an ITEM is one of two kinds:
 *   exact run     a maximal sequence of windows i, i + k, ..., i + (r - 1) k that are all exact_s: it starts at a window i
 *                 with exact_s[i] and not (i >= k and exact_s[i - k]) and ends at a window e with exact_s[e] and not
 *                 (e + k <= n - k and exact_s[e + k]).  start = i, count = r >= 1, bin = TREW_VARIANT_NONE
 *   variant unit  an anchored var_s window i.  start = i, count = 1, bin = the variant's bin (below TREW_VARIANT_BINS)
 * No two items of a key share a start (a window is exact or variant, never both), so (read, motif, strand, start) is a
 * total order: the order every interface returns.  Items of different residue classes mod k may overlap (TGT in TGTGT:
 * windows 0 and 2 are both exact); that is part of the definition.  n < k gives no items.  Every key also has two counts,
 * {runs, variants}.  Consequences: the counts of a key's runs sum to trew_hip_variant.units_s; its variant items number
 * variants_s and their bins make the read's histogram; a read that is a primitive M repeated r times has the one forward
 * item {0, r, NONE}; the rev items of a read are the fwd items of its reverse complement with start -> n - k - start for a
 * variant and n - k - (start + (count - 1) k) for a run, the bin unchanged; an item does not depend on the rest of the
 * batch.  Units with an inserted or deleted base (they shift the phase) are left to trew_hip_trace, below.  Also additive:
 * TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t read, motif, strand, start, count, bin;
} trew_hip_chain_item;
/* Like trew_hip_intervals (batch shapes, staging, asynchronous on the slot's stream, a context of any mode, independent of
 * the scan and of the other five kernels), with buffers of its own that the slot's first call allocates: a log of max_events
 * entries (>= 1; the log grows when a call asks for more), whose counter is zeroed on the slot's stream in front of every
 * launch, and the two counts of every key.  The kernel appends EVENTS, not items: a run's start, its end (one event for
 * both when the run has one unit), a variant unit; an item takes one or two events.  The layout of an event is internal.
 * A batch holds at most 2^32 - 1 reads.  One kernel, a wave per read, for every read length. */
int trew_hip_chain(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, uint64_t max_events);
/* Waits for the slot.  *n_events = the events the kernel found, also when that exceeds max_events; counts (n_reads *
 * n_motifs * 2 * 2 values, [read][motif][strand]{runs, variants}; may be NULL) is always exact; *n_items = the sum of the
 * counts, so it is exact even on overflow.  n_items and n_events must not be NULL.  When *n_events <= max_events the host
 * pairs the events into items and copies min(cap, *n_items) of them sorted by (read, motif, strand, start), so the output
 * does not depend on device scheduling.  When *n_events > max_events the stored events are an unspecified subset that
 * cannot be paired: no item is copied, counts, *n_items and *n_events are still exact; repeat trew_hip_chain with
 * max_events >= *n_events -- one retry always suffices.  That case is no error (the call returns 0), like
 * trew_hip_intervals_results with too small a log. */
int trew_hip_chain_results(trew_hip_ctx *ctx, int slot, trew_hip_chain_item *out, uint64_t cap, uint64_t *n_items, uint64_t *n_events,
                           uint32_t *counts, float *ms_kernel);
/* The same on the host, window by window from the definition, over packed planes: *n_items = items found, min(cap,
 * *n_items) items (the first ones of the sorted order), counts as above (may be NULL). */
int trew_chain_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                    int n_motifs, trew_hip_chain_item *out, uint64_t cap, uint64_t *n_items, uint32_t *counts);

/* ---- de novo repeats: every tract of a read, not only the best one (no motif given) ----
 * Integer-exact (tests/repeat_ref.py is the brute-force form).  The parameters are those of trew_hip_periods, with
 * the same checks.  A PIECE is a half-open base range [lo, hi) of a read.  Its record is the trew_hip_periods record of the
 * bases lo .. hi - 1 taken as a read of their own -- nothing outside the piece is seen, valid or not -- with start and end
 * shifted back into read coordinates.
 *   repeats(piece)  a piece without a record (no admissible k, or score < min_score) yields nothing; otherwise it yields its
 *                   record R, then repeats([lo, R.start)) and repeats([R.end, hi))
 * The tracts of a read are repeats([0, n)).  depth is 0 for the read's own record and parent + 1 below it; the other fields
 * are those of trew_hip_period.  Consequences: the depth-0 record of a read equals its trew_hip_periods record field for
 * field, and a read without one has no tract; the tracts of a read are disjoint; none scores above the read's depth-0
 * tract; a read's records do not depend on the rest of the batch; a piece with hi - lo - min_period < min_score cannot
 * have a record (score_k <= length - k); a read has at most n / (min_score + 1) tracts.  The consensus keeps the fixed phase
 * of trew_hip_periods: under indels a long tract's unit can come out wrong, here as there.  Periods above 32:
 * trew_hip_satellites below.  Also additive: TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t read, depth, period, scored_period, score, start, end, matches, support, reserved;
    uint64_t unit;
} trew_hip_repeat; /* 48 bytes */
/* Like trew_hip_periods (batch shapes, staging, asynchronous on the slot's stream, a context of any mode, independent of the
 * scan and of the other six kernels, no motifs), with buffers of its own that the slot's first call allocates: a log of
 * max_records records (>= 1; the log grows when a call asks for more) to which the kernel appends every tract, and one count
 * per read; the log's counter and the counts are zeroed on the slot's stream in front of every launch.  A batch holds at most
 * 2^32 - 1 reads.  One kernel, a wave per read, for every read length; the recursion runs inside the wave. */
int trew_hip_repeats(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                     uint64_t max_records);
/* Waits for the slot.  *n = the number of tracts found, also when that exceeds max_records or cap; n must not be NULL.
 * counts (n_reads values; may be NULL) = the tracts of every read, always exact.  When *n <= max_records, min(cap, *n) records
 * are copied, sorted by (read, start), so the output does not depend on device scheduling.  When *n > max_records the log
 * holds an unspecified subset and nothing is copied; counts and *n are still exact: repeat trew_hip_repeats with max_records
 * >= *n -- one retry always suffices.  That case is no error (the call returns 0), like trew_hip_intervals_results with too
 * small a log. */
int trew_hip_repeats_results(trew_hip_ctx *ctx, int slot, trew_hip_repeat *out, uint64_t cap, uint64_t *n, uint32_t *counts, float *ms_kernel);
/* The same on the host, piece by piece from the definition, over packed planes: *n = tracts found, min(cap, *n) records (the
 * first ones of the sorted order), counts as above (may be NULL). */
int trew_repeats_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                      int penalty, uint32_t min_score, trew_hip_repeat *out, uint64_t cap, uint64_t *n, uint32_t *counts);

/* ---- de novo repeats with periods up to 256: minisatellites and satellite monomers (no motif given) ----
 * Integer-exact (tests/satellite_ref.py is the brute-force form).  trew_hip_repeats with
 * 1 <= min_period <= max_period <= TREW_SATELLITE_MAX_PERIOD and a unit wide enough for the result; penalty and min_score as
 * there.  The definition is unchanged: the record of a piece is that of trew_hip_periods with k over
 * [min_period, min(max_period, length - 1)] (tie rules, matches, support, the majority with the smallest code on a tie, code
 * 0 for a phase without a valid base, the primitive root), the recursion over pieces, depth, counts, the order (read, start)
 * and the overflow protocol are those of trew_hip_repeats.
 *   unit   base j of the unit (j < period) lies in bits [2 (j & 15), 2 (j & 15) + 2) of unit[j >> 4]; codes T 0, G 1, C 2,
 *          A 3; every bit at or above base `period` is zero
 * Consequences: with max_period <= 32 the records equal those of trew_hip_repeats on the same input record for record and
 * field for field, the two units decoding to the same string, and so do counts and *n; the depth-0 record then equals the
 * trew_hip_periods record.  Over the whole range, as for trew_hip_repeats: the tracts of a read are disjoint; none scores
 * above the read's depth-0 tract; a read's records do not depend on the rest of the batch; pruning the pieces with
 * hi - lo - min_period < min_score changes nothing; score and scored_period are invariant under reverse complement; period
 * divides scored_period.
 * Limits: periods are at most 256.  eq_k compares NEIGHBOURING copies, so an array whose monomers have diverged (human alpha
 * satellite monomers differ from each other by a fifth or more) does not score at the default penalty; higher-order repeat
 * units of kilobases are out of reach; the consensus keeps the fixed phase of trew_hip_periods, so under indels a long
 * tract's unit can come out wrong.  Also additive: TREW_HIP_ABI_VERSION stays 4. */
#define TREW_SATELLITE_MAX_PERIOD 256
typedef struct {
    uint32_t read, depth, period, scored_period, score, start, end, matches, support, reserved;
    uint32_t unit[16];
} trew_hip_satellite; /* 104 bytes */
/* Like trew_hip_repeats in every respect (batch shapes, staging, the log of max_records records >= 1 with its counter, one
 * count per read, at most 2^32 - 1 reads a batch), with buffers of its own and independent of the scan and of the other seven
 * kernels.  Argument error: "1 <= min_period <= max_period <= 256".  One kernel, a wave per read, for every read length. */
int trew_hip_satellites(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                        uint64_t max_records);
/* The contract of trew_hip_repeats_results: *n is exact also beyond max_records or cap (n must not be NULL), counts (n_reads
 * values; may be NULL) is always exact, min(cap, *n) records sorted by (read, start) when *n <= max_records, nothing copied
 * otherwise and no error: repeat trew_hip_satellites with max_records >= *n -- one retry always suffices. */
int trew_hip_satellites_results(trew_hip_ctx *ctx, int slot, trew_hip_satellite *out, uint64_t cap, uint64_t *n, uint32_t *counts, float *ms_kernel);
/* The same on the host, piece by piece from the definition, over packed planes: *n = tracts found, min(cap, *n) records (the
 * first ones of the sorted order), counts as above (may be NULL). */
int trew_satellites_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                         int penalty, uint32_t min_score, trew_hip_satellite *out, uint64_t cap, uint64_t *n, uint32_t *counts);

/* ---- indel-aware motif tract per read: a local alignment of the read against the motif repeated without end ----
 * (how many copies of the unit does this read hold, where do they begin and end when bases are missing or extra, and how
 * many of the errors are substitutions, insertions and deletions?)  Wraparound dynamic programming.  For strand s (fwd: the
 * motif M, rev: its reverse complement) the text is T[j] = M_s[j mod k]; an N in the read matches nothing; 1 <= penalty <= 64.
 * A cell holds a tuple (score, start, consumed, matches); tuples compare lexicographically, score as a signed integer, and
 * the larger tuple wins.  H[0][j] = (0, 0, 0, 0) for 0 <= j < k; for i = 1 .. n, V[i][j] is the largest of
 *   the fresh start             (0, i, 0, 0)
 *   the diagonal                with (s, b, C, m) = H[i-1][(j-1) mod k]: (s + 1, b, C + 1, m + 1) when x[i-1] = M_s[j],
 *                               else (s - penalty, b, C + 1, m)
 *   the inserted read base      with (s, b, C, m) = H[i-1][j]: (s - penalty, b, C, m)
 * and H[i][j] is the largest, over d = 0 .. k-1 deleted motif bases, of (s - penalty d, b, C + d, m) with
 * (s, b, C, m) = V[i][(j-d) mod k].  The record of a strand is the cell with the largest (score, -i, start, consumed,
 * matches): on a tie in score the earliest end wins, then the later start -- the shorter tract at both ends, as for
 * trew_hip_tract.  A largest score of 0 gives zeros.
 *   score_s     matches - penalty * (mismatches + insertions + deletions)
 *   start_s, end_s   the tract is the bases [start, end) of the read
 *   consumed_s  motif bases the alignment went through (matches + mismatches + deletions); copies = consumed / k
 *   matches_s   matching bases
 * Exact consequences, with L = end - start and E = (matches - score) / penalty: deletions = E - (L - matches), insertions =
 * E - (consumed - matches), mismatches = L - matches - insertions.  Every rotation of a motif gives the same record.  One
 * tract per strand, the best one; linear gap cost.  Also additive: TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t score_fwd, start_fwd, end_fwd, consumed_fwd, matches_fwd;
    uint32_t score_rev, start_rev, end_rev, consumed_rev, matches_rev;
} trew_hip_alignment;
/* Like trew_hip_tracts in every respect (batch shapes, staging, asynchronous on the slot's stream, a context of any mode, the
 * motif and penalty checks and their error texts), with a result buffer of its own that the slot's first call allocates and
 * independent of the scan and of the other eight kernels.  Records are laid out out[r * n_motifs + m].  One kernel, a wave
 * per read, for every read length. */
int trew_hip_align(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, int penalty);
/* Waits for the slot and copies the records of its last trew_hip_align; arguments as trew_hip_annotate_results. */
int trew_hip_align_results(trew_hip_ctx *ctx, int slot, trew_hip_alignment *out, uint64_t cap, uint64_t *n, float *ms_kernel);
/* The same records on the host, base by base from the definition, over packed planes. */
int trew_align_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                    const trew_hip_motif *motifs, int n_motifs, int penalty, trew_hip_alignment *out);

/* ---- wraparound alignment for units of up to 256 bases: satellite monomers, given, in noisy reads ----
 * (where in this read is the array of this monomer, how many copies, and how do its errors split, when the copies have
 * diverged from each other by a fifth or more and bases are missing or extra?)  Integer-exact.  The definition is that of
 * trew_hip_alignment, above, word for word: the codes, M_s, an N matches nothing, 1 <= penalty <= 64, the tuple (score, start,
 * consumed, matches), V, H, the maximum over d = 0 .. k-1 deleted unit bases, the record order (score, -end, start, consumed,
 * matches), zeros at score 0, and the derived columns.  The only change is 3 <= k <= TREW_MONOMER_MAX.  The record is
 * trew_hip_alignment, unchanged, laid out out[r * n_monomers + m].
 *   unit   base j of the unit (j < k) lies in bits [2 (j & 15), 2 (j & 15) + 2) of unit[j >> 4], as in trew_hip_satellite;
 *          codes T 0, G 1, C 2, A 3; every bit at or above base k is zero
 * Consequences: for k <= 32 the records equal trew_hip_align's field for field; every rotation of a unit gives the same
 * record; score_rev(x) = score_fwd(reverse complement of x); the derived columns are never negative.
 * Limits: one tract per read, monomer and strand, the best one; linear gap cost; k <= 256; counts only (the traceback is
 * trew_hip_copies, below; the de novo measures built on trew_hip_trace stay at k <= 32); with penalty 1 and long units a random read scores over its whole length
 * (match +1 and every error -1 is the linear phase of local alignment), so use penalty >= 2; higher-order repeat units of
 * kilobases are out of reach.  Also additive: TREW_HIP_ABI_VERSION stays 4. */
#define TREW_MONOMER_MAX 256
#define TREW_MONOMERS_MAX 8 /* monomers a call */
typedef struct {
    int32_t k; /* 3 .. TREW_MONOMER_MAX */
    int32_t reserved;
    uint32_t unit[16];
} trew_hip_monomer; /* 72 bytes */
/* 'ACGT...' (upper or lower case, 3 .. 256 bases) -> monomer.  0 or -1; the text of the error through
 * trew_hip_last_error(NULL).  Touches no device. */
int trew_monomer_parse(const char *text, trew_hip_monomer *out);
/* Like trew_hip_align in every respect (batch shapes including device-resident and pair mode, staging, asynchronous on the
 * slot's stream, a context of any mode, the penalty check and its error text), with 1 <= n_monomers <= 8, a result buffer and
 * a staged monomer table of its own that the slot's first call allocates, and independent of the scan and of the other
 * fifteen kernels.  Argument errors: "n_monomers must be in [1, 8]", "monomers is NULL", "monomer: k must be in [3, 256]",
 * "monomer: unit has bits at or above base k".  One kernel, a wave per read, for every read length; the largest k of the
 * call picks how many phases a lane holds. */
int trew_hip_monomers(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_monomer *monomers, int n_monomers, int penalty);
/* Waits for the slot and copies the records of its last trew_hip_monomers; arguments as trew_hip_annotate_results. */
int trew_hip_monomers_results(trew_hip_ctx *ctx, int slot, trew_hip_alignment *out, uint64_t cap, uint64_t *n, float *ms_kernel);
/* The same records on the host from the definition, over packed planes; the maximum over d in the linear-plus-wrap form
 * (DESIGN 4.7m), O(n k) a strand. */
int trew_monomers_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                       const trew_hip_monomer *monomers, int n_monomers, int penalty, trew_hip_alignment *out);

/* ---- de novo repeats under indels: seed a unit, align against it with wraparound, re-vote the unit from the alignment ----
 * (what repeats in this noisy long read, with which unit, from where to where, and how many copies?)  Integer-exact.  The
 * read x has n bases, with the codes and the N handling of trew_hip_periods; min_period, max_period (<= 32), penalty P and
 * min_score are those of trew_hip_periods, with the same checks and error texts.
 * 1. Periods.  R is the trew_hip_period record of the read.  If R is zero, the record is zero.  Otherwise k = scored_period,
 *    b = start, e = end - k.
 * 2. Seed.  Among i in [b, e) take the longest run of consecutive positions with eq_k[i] true (bases i and i + k both valid
 *    and equal), the first of the longest; rs is its start, or b without one.  S0[j] = x[rs + j] for j < k, an invalid base
 *    replaced by the base of phase (rs + j - start) mod k of the unreduced consensus of trew_hip_periods.  S is S0 reduced to
 *    its primitive root, of length seed_period.  A run of k or more positions is two identical copies: S0 is a literal unit
 *    of the read, not an average over slipped phases.
 * 3. Align.  A1 is the forward-strand record of the wraparound recurrence of trew_hip_alignment, above, of x against S:
 *    the same tuples, tie rules and record, here for every unit length 1 .. 32.
 * 4. Vote.  The same recurrence again over x[A1.start, A1.end) only: H = (0, 0, 0, 0) in every phase at A1.start, positions
 *    count from A1.start.  At each row i, j* is the phase with the largest V[i][j] tuple, the smallest j on a tie (V, not H:
 *    the V cell is where the base was consumed, before any deleted motif bases).  If x[i-1] is valid and the diagonal
 *    candidate of (i, j*) equals V[i][j*], then cnt[j*][x[i-1]] += 1.  A forward decode: no traceback.
 * 5. Re-vote.  U0[j] = S[j] if cnt[j][S[j]] is the largest count of phase j, otherwise the smallest code among the largest
 *    (a phase without votes keeps the seed).  U is U0 reduced to its primitive root.  support = the sum of cnt[j][U0[j]];
 *    changed = the number of phases with U0[j] != S[j].
 * 6. Final.  If U = S, A2 = A1.  Otherwise A2 is the forward record of x against U, and if A2.score < A1.score the seed is
 *    kept: U := S, A2 := A1, changed := 0.  One round only.
 *   period, unit            the length of U and U, packed as trew_hip_period's unit
 *   seed_period, seed_unit  the same of S
 *   scored_period           k of step 1
 *   changed, support        of step 5 (changed: 0 when the seed is kept)
 *   score, start, end, consumed, matches   A2, as in trew_hip_alignment; seed_score = A1.score
 * Consequences: score >= seed_score; unit is primitive; copies = consumed / period and the mismatches, insertions and
 * deletions follow as for trew_hip_alignment with k = period.  Limits: one tract per read, the best one; periods <= 32; linear
 * gap cost; a wrong scored_period (a multiple or a neighbour of the true period) is not repaired; the vote is a forward
 * decode, not a traceback (an indel misplaces the few bases until the penalised path overtakes); one refinement round.
 * trew_hip_resolve, further below, lets the alignment choose between the few best-scoring periods of step 1, and
 * trew_hip_tandems_resolved, trew_hip_decompose_resolved and trew_hip_dissect_resolved do so for every piece.
 * Also additive: TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t period, seed_period, scored_period, changed;
    uint32_t score, start, end, consumed, matches;
    uint32_t seed_score, support, reserved;
    uint64_t unit, seed_unit;
} trew_hip_refined;
/* Like trew_hip_periods in every respect (batch shapes including device-resident and pair mode, staging, asynchronous on the
 * slot's stream, a context of any mode, the checks and their error texts), with a result buffer of its own that the slot's
 * first call allocates and independent of the scan and of the other nine kernels.  One record per read.  One kernel, a wave
 * per read, for every read length. */
int trew_hip_refine(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score);
/* Waits for the slot and copies the records of its last trew_hip_refine; arguments as trew_hip_periods_results. */
int trew_hip_refine_results(trew_hip_ctx *ctx, int slot, trew_hip_refined *out, uint64_t cap, uint64_t *n, float *ms_kernel);
/* The same records on the host, step by step from the definition, over packed planes. */
int trew_refine_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                     int penalty, uint32_t min_score, trew_hip_refined *out);

/* ---- de novo repeats under indels, every tract of a read: trew_hip_repeats' recursion with trew_hip_refine per piece ----
 * (a noisy long read with 900 bases of (AATGG)n beside 600 bases of (TTAGGG)n: both tracts whole, each with its unit)
 * Integer-exact (tests/tandem_ref.py is the reference).  The parameters, checks and error texts are those of
 * trew_hip_refine.  A PIECE is a half-open base range [lo, hi) of a read.  Its REFINED RECORD is the trew_hip_refined record
 * (all six steps) of the bases lo .. hi - 1 taken as a read of their own -- nothing outside the piece is seen, valid or not --
 * with start and end shifted back into read coordinates.  Its PERIODS TRACT is [R.start, R.end) of step 1 of that same
 * computation, shifted likewise.
 *   tandems(piece)  1. if step 1 gives no periods record, the piece yields nothing;
 *                   2. if the refined record X has score >= min_score, the piece yields X, then tandems([lo, X.start)) and
 *                      tandems([X.end, hi));
 *                   3. otherwise (a WEAK piece) it yields no record, then tandems([lo, R.start)) and tandems([R.end, hi)):
 *                      step 1 promised a repeat that no single unit aligns to with min_score (a drifting unit:
 *                      "AAAC" x 5 + "AAAG" x 5 + "AACG" x 5 has a periods score of 48 and a refined score of 23 at the
 *                      defaults); it is used up, and the recursion shrinks.
 * The tracts of a read are tandems([0, n)).  depth is 0 for the read's own piece and parent + 1 below it; a weak piece has a
 * depth but no record.  The other fields are those of trew_hip_refined.  Consequences: the depth-0 record of a read equals its
 * trew_hip_refine record field for field whenever that record's score reaches min_score; a read without a periods record has
 * no tract; the tracts of a read are disjoint and every one scores >= min_score; a read's records do not depend on the rest of
 * the batch; a piece with hi - lo - min_period < min_score cannot have a periods record and need not be walked; on perfect
 * repeats with flanks the (period, unit) pairs are those of trew_hip_repeats, and start, end and score those of
 * trew_hip_align against that unit.  NOT a consequence, unlike trew_hip_repeats: "none scores above the first" -- alignment
 * scores are not ordered by the periods score that picks the tract first.
 * Limits: periods <= 32; linear gap cost; a wrong scored_period is not repaired (trew_hip_tandems_resolved, further below, takes
 * trew_hip_resolve's choice of period for every piece); a weak piece is dropped, with whatever
 * shorter tract a unit of its own would have aligned to inside it; the cost is that of trew_hip_refine per piece.  Also
 * additive: TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t read, depth;
    uint32_t period, seed_period, scored_period, changed;
    uint32_t score, start, end, consumed, matches;
    uint32_t seed_score, support, reserved;
    uint64_t unit, seed_unit;
} trew_hip_tandem; /* 72 bytes: read, depth, the sixteen words of trew_hip_refined */
/* Like trew_hip_repeats in every respect (batch shapes including device-resident and pair mode, staging, asynchronous on the
 * slot's stream, a context of any mode, no motifs, the log of max_records records >= 1 with its counter, one count per read, at
 * most 2^32 - 1 reads a batch), with buffers of its own and independent of the scan and of the other ten kernels.  One kernel,
 * a wave per read, for every read length; the recursion runs inside the wave. */
int trew_hip_tandems(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                     uint64_t max_records);
/* The contract of trew_hip_repeats_results: *n is exact also beyond max_records or cap (n must not be NULL), counts (n_reads
 * values; may be NULL) is always exact, min(cap, *n) records sorted by (read, start) when *n <= max_records; when *n >
 * max_records the log holds an unspecified subset, nothing is copied and the call returns 0: repeat trew_hip_tandems with
 * max_records >= *n -- one retry always suffices. */
int trew_hip_tandems_results(trew_hip_ctx *ctx, int slot, trew_hip_tandem *out, uint64_t cap, uint64_t *n, uint32_t *counts, float *ms_kernel);
/* The same on the host, piece by piece from the definition, over packed planes: *n = tracts found, min(cap, *n) records (the
 * first ones of the sorted order), counts as above (may be NULL). */
int trew_tandems_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                      int penalty, uint32_t min_score, trew_hip_tandem *out, uint64_t cap, uint64_t *n, uint32_t *counts);

/* ---- units in place under indels: the traceback of trew_hip_alignment's wraparound alignment, cut into copies of the motif ----
 * (what is this telomere made of, and in which order, when bases are missing or extra?  trew_hip_chain for reads with indels;
 * its columns also say where the mismatches, insertions and deletions of trew_hip_alignment lie.)  Integer-exact.  Everything
 * is trew_hip_alignment's, unchanged: the codes, M_s, the penalty P, the tuples (score, start, consumed, matches), V, H and the
 * record of a strand.  Three tie rules are added, because equal tuples can come from different cells:
 *   1. V[i][j]: among candidates with equal tuples the fresh start comes first, then the diagonal, then the inserted read
 *      base; op in {F, D, I} names the winner.
 *   2. H[i][j]: d is the smallest d < k that attains the largest tuple.
 *   3. The end cell is the cell (end, j*) of the record; on equal (score, -i, start, consumed, matches) the smallest j wins.
 * The traceback starts at the end cell.  At H[i][j] it emits d columns `del`, for the motif phases j, j - 1, ..., j - d + 1,
 * sets j <- (j - d) mod k and looks at op of V[i][j]: F ends the walk (here i = start); D emits `eq` or `sub`, according to
 * whether x[i-1] = M_s[j], for (read base i - 1, phase j) and goes to H[i-1][(j-1) mod k]; I emits `ins` (read base i - 1, no
 * phase) and goes to H[i-1][j].  Reversed, the columns are the alignment in read order.  A segment begins at the first column
 * and in front of every column whose phase is 0; an `ins` column has no phase and stays in the running segment.  A segment is
 * one item:
 *   start       its first read base
 *   bases       its read bases
 *   phase       the phase of its first phased column
 *   consumed    its phased columns
 *   mismatches, insertions, deletions   as counted in its columns
 *   count       1
 * A segment is a complete exact copy when phase = 0, consumed = k and it has no error; consecutive complete exact copies merge
 * into one item with count = r, bases = consumed = r k and the first copy's start.  A key (read, motif, strand) has items if
 * and only if its alignment score is >= min_score (>= 1).  Consequences: the items of a key tile [start, end) of its record
 * without a gap; their consumed, mismatches, insertions and deletions sum to the record's; every item has bases >= 1; only the
 * first item can have phase != 0.  Limits, as for trew_hip_alignment: one tract per key, linear gaps, k <= 32.  Also
 * additive: TREW_HIP_ABI_VERSION stays 4. */
typedef struct {
    uint32_t read, motif, strand, start, bases, count, phase, consumed, mismatches, insertions, deletions, reserved; /* reserved = 0 */
} trew_hip_trace_item; /* 48 bytes */
/* Like trew_hip_align in every respect (batch shapes including device-resident and pair mode, staging, asynchronous on the
 * slot's stream, a context of any mode, the motif and penalty checks and their error texts), with buffers of its own and
 * independent of the scan and of the other eleven kernels.  Further argument errors: "min_score must be at least 1",
 * "max_items must be at least 1", "max_rows must be at least 1".  The kernel appends items to a log of max_items items and
 * keeps the directions of the traced tracts in a workspace of max_rows rows of 64 bytes; both grow only.  How many rows a
 * (read, motif) claims is internal: at most the read's length, none when neither strand reaches min_score.  At most 2^32 - 1
 * reads a batch.  One kernel, a wave per read, for every read length. */
int trew_hip_trace(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, int penalty,
                   uint32_t min_score, uint64_t max_items, uint64_t max_rows);
/* Waits for the slot.  *n_items and *n_rows (neither may be NULL) are the items found and the rows claimed, exact also beyond
 * max_items, max_rows or cap; counts (n_reads * n_motifs * 2 values at [read][motif][strand]; may be NULL) the items of every
 * key, always exact; records (n_reads * n_motifs; may be NULL) the trew_hip_alignment of every (read, motif), equal to
 * trew_hip_align's.  min(cap, *n_items) items sorted by (read, motif, strand, start) go to `items` when *n_items <= max_items
 * and *n_rows <= max_rows; otherwise nothing is copied into `items` and the call returns 0: repeat trew_hip_trace with both at
 * least what was reported -- one retry always suffices.  (A tract whose rows did not fit is still traced, by recomputing its
 * rows block after block, which costs time quadratic in its length: size max_rows so that this stays the exception.) */
int trew_hip_trace_results(trew_hip_ctx *ctx, int slot, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint64_t *n_rows,
                           uint32_t *counts, trew_hip_alignment *records, float *ms_kernel);
/* The definition on the host with the full table, over packed planes: *n_items = items found, min(cap, *n_items) items (the
 * first ones of the sorted order), counts and records as above (each may be NULL). */
int trew_trace_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                    int n_motifs, int penalty, uint32_t min_score, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint32_t *counts,
                    trew_hip_alignment *records);

/* ---- copies in place for units of up to 256 bases: the traceback of trew_hip_monomers' alignment, cut into copies ----
 * (where does each copy of this satellite monomer begin and end, which copies are intact, and which carry which
 * substitutions, insertions and deletions?)  Integer-exact.  The definition is trew_hip_trace's, above, word for word, with
 * 3 <= k <= TREW_MONOMER_MAX: the tuples, V and H are those of trew_hip_alignment / trew_hip_monomers; the three tie rules
 * hold (op in the order F, D, I; the smallest d; the end cell with the smallest phase on equal (score, -end, start,
 * consumed, matches)); the walk, the segments and the merging of complete exact copies are trew_hip_trace's; the item is
 * trew_hip_trace_item as it is, its word `motif` holding the monomer's index; the alignment records beside the items are
 * trew_hip_monomers', field for field.  A key (read, monomer, strand) has items if and only if its score is >= min_score;
 * items are sorted by (read, monomer, strand, start).  n_rows is defined per key: the sum of end - start over the keys that
 * have items (the strands are walked one after the other, there is no union range as in trew_hip_trace).
 * Consequences: those of trew_hip_trace; for k <= 32 the items equal trew_hip_trace's field for field.
 * Limits: one tract per key, linear gaps, k <= 256; the de novo measures (trew_hip_decompose, trew_hip_dissect,
 * trew_hip_refine) stay at k <= 32.  Also additive: TREW_HIP_ABI_VERSION stays 4.
 *
 * The arguments, checks, error texts, the grow-only log and workspace, the zeroed counters and the retry contract are those of
 * trew_hip_trace; the units are trew_hip_monomers, checked and staged as trew_hip_monomers does (its four argument errors come
 * first).  A row of the workspace is 64 Q bytes, Q = 1, 2, 4 the smallest with 64 Q >= the largest k of the call.  One
 * kernel, a wave per read, for every read length. */
int trew_hip_copies(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_monomer *monomers, int n_monomers, int penalty,
                    uint32_t min_score, uint64_t max_items, uint64_t max_rows);
/* The contract of trew_hip_trace_results, with counts at [read][monomer][strand] and records (n_reads * n_monomers) equal to
 * trew_hip_monomers'.  Argument errors: "trew_hip_copies_results: n_items and n_rows must not be null",
 * "trew_hip_copies_results: items must not be null". */
int trew_hip_copies_results(trew_hip_ctx *ctx, int slot, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint64_t *n_rows,
                            uint32_t *counts, trew_hip_alignment *records, float *ms_kernel);
/* The definition on the host over packed planes: trew_monomers_host's linear-plus-wrap closure with one direction byte a cell
 * of the traced tract only (op, and one bit for "the smallest d is not 0": DESIGN 4.7n), O(n k) a strand.  *n_items = items
 * found, *n_rows (may be NULL) the rows as defined above, min(cap, *n_items) items (the first ones of the sorted order),
 * counts and records as above (each may be NULL). */
int trew_copies_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_monomer *monomers,
                     int n_monomers, int penalty, uint32_t min_score, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint64_t *n_rows,
                     uint32_t *counts, trew_hip_alignment *records);

/* ---- de novo repeats under indels for periods up to 256: trew_hip_refine's seed, align and re-vote with a long unit ----
 * (where does this minisatellite or satellite array begin and end in a noisy long read, how many copies does it hold, how do
 * its errors split, and what is its monomer -- when nobody has typed that monomer?)  Integer-exact (DESIGN 4.7o;
 * tests/polish_ref.py is the reference).  The definition is trew_hip_refine's (steps 1 to 7 above), word for word, with three
 * changes:
 * 1. Periods.  R is the depth-0 record of trew_hip_satellites for the read: the periods record with k over [min_period,
 *    min(max_period, n - 1)], 1 <= min_period <= max_period <= TREW_POLISH_MAX_PERIOD (256); its unreduced consensus serves
 *    the N of a seed window.  The checks and error texts are trew_hip_satellites': "1 <= min_period <= max_period <= 256",
 *    and penalty and min_score as there.
 * 2. The recurrence of steps 3, 4 and 6 is trew_hip_monomers', for every unit length 1 .. 256 (the lower limit of 3 is a
 *    check on typed units, not a property of the recurrence).  The tuples, the tie rules, the vote's V (not H), "the smallest
 *    phase on a tie" and "the diagonal candidate equals V[i][j*]" are unchanged.
 * 3. The record is trew_hip_polished, 176 bytes, one per read: refine's twelve words in refine's order, then unit[16] and
 *    seed_unit[16], packed as trew_hip_satellite.unit: base j in bits [2 (j & 15), 2 (j & 15) + 2) of word j >> 4, zero at
 *    and above period / seed_period.
 * Consequences: with max_period <= 32 the twelve words equal trew_hip_refine's on the same input and arguments and the two
 * units decode to the same strings; score >= seed_score; a zero step-1 record gives a zero record; unit and seed_unit are
 * primitive; the derived columns (trew_hip_alignment's, with k = period) are never negative; whenever seed_period >= 3,
 * seed_score equals the forward score of trew_hip_monomers with the unit S, with changed = 0 all five fields of A2 do, and
 * with changed > 0 the fields of A2 equal those with the unit U; on a perfect repeat period, unit, changed = 0, start, end
 * and score are trew_hip_satellites' depth-0 period and unit and trew_hip_monomers' forward record; (unit) x m with one base
 * removed is one deletion with consumed = m k, with one base added one insertion, the unit unchanged in both.
 * Limits: one tract per read; periods of at most 256; linear gap costs; a wrong scored_period is not repaired, and with the
 * wide range it is wrong more often than in trew_hip_refine (DESIGN 4.7o has the measured figures); the vote is a forward
 * decode, not a traceback; one round; a penalty of 1 is in the linear phase for long units, so use 2 or more, as for
 * trew_hip_monomers; trew_hip_resolve, _tandems, _decompose and _dissect stay at periods <= 32.  Also additive:
 * TREW_HIP_ABI_VERSION stays 4. */
#define TREW_POLISH_MAX_PERIOD 256
typedef struct {
    uint32_t period, seed_period, scored_period, changed; /* of U, of S, of step 1; phases the vote changed */
    uint32_t score, start, end, consumed, matches;        /* A2 */
    uint32_t seed_score, support, reserved;               /* A1.score; the sum of the winning counts; 0 */
    uint32_t unit[16], seed_unit[16];                     /* U and S, packed as trew_hip_satellite.unit */
} trew_hip_polished;
/* Like trew_hip_refine in every respect (batch shapes including device-resident and pair mode, staging, asynchronous on the
 * slot's stream, a context of any mode).  One kernel, a wave per read, for every read length. */
int trew_hip_polish(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score);
/* Waits for the slot and copies the records of its last trew_hip_polish; arguments as trew_hip_refine_results. */
int trew_hip_polish_results(trew_hip_ctx *ctx, int slot, trew_hip_polished *out, uint64_t cap, uint64_t *n, float *ms_kernel);
/* The definition on the host, step by step, over packed planes; out has n_reads records. */
int trew_polish_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                     int penalty, uint32_t min_score, trew_hip_polished *out);

/* ---- units in place with no motif given: trew_hip_refine's unit, anchored at a fixed rotation, and trew_hip_trace against it ----
 * (what is this telomere made of, and in which order, when nobody knows its motif?)  Integer-exact (DESIGN 4.7i;
 * tests/decompose_ref.py is the reference).  The arguments are min_period, max_period (<= 32), the penalty P and min_score: those
 * of trew_hip_refine, with the same checks and error texts.  max_items and max_rows are those of trew_hip_trace; both must be
 * >= 1.
 * 1. Refine.  R is the read's trew_hip_refined record, field for field.
 * 2. Anchor.  If R is zero or R.score < min_score, the read has no items and anchor is 0.  Otherwise k = R.period and U =
 *    R.unit.  U is primitive, so its k rotations are distinct.  M is the smallest rotation of U, in the order in which the
 *    scan compares rotations (as packed words, first base most significant).  No reverse complement is taken here.  anchor =
 *    rho, the one offset with M[j] = U[(j + rho) mod k].
 * 3. Trace.  The items are those of trew_hip_trace_item's definition for the forward strand of the read against the motif M:
 *    the tuples, the three tie rules, the walk, the segments and the merging of complete exact copies are all unchanged.  Unit
 *    lengths 1 and 2 are included: the lower limit of 3 in trew_hip_trace is a check on typed motifs and not a property of the
 *    table.  The item is a trew_hip_trace_item with motif = 0 and strand = 0.
 * 4. Outputs per read: the record R, with its reserved word carrying anchor, and the number of items.
 * Items come sorted by (read, start).  Consequences: the record equals trew_hip_refine's in every field but reserved; a read has
 * items if and only if R.period > 0 and R.score >= min_score; the alignment record of the traced table equals R ((score, start,
 * end, consumed, matches) is the same for every rotation of a unit, only the end phase depends on the rotation); the items tile
 * [R.start, R.end) without a gap; bases sums to end - start, consumed to R.consumed, and the errors to those that follow from R
 * and P; only the first item has phase != 0; for k >= 3 the items equal the forward-strand items of trew_hip_trace with motif
 * M; a perfect repeat begun at each of its k rotations gives the same M, and its first item's phase follows the rotation; a
 * read's items do not depend on the rest of the batch.  Limits: those of trew_hip_refine (one tract per read, periods <= 32,
 * linear gaps, a wrong scored_period not repaired -- trew_hip_decompose_resolved, further below, takes trew_hip_resolve's record);
 * the items are in read orientation and cut at M, and a read of the other
 * strand is cut at the smallest rotation of the reverse complement, so items compare directly only between reads of one
 * strand.  Also additive: TREW_HIP_ABI_VERSION stays 4.
 *
 * Like trew_hip_refine in every respect (batch shapes including device-resident and pair mode, staging, asynchronous on the
 * slot's stream, a context of any mode, no motifs, the checks and their error texts), with buffers of its own and independent of
 * the scan and of the other twelve kernels.  Further argument errors: "max_items must be at least 1", "max_rows must be at
 * least 1".  The log of max_items items, the workspace of max_rows rows -- here of 32 bytes, one strand -- and the two counters
 * are as in trew_hip_trace; a read claims end - start rows when it has items, else none.  At most 2^32 - 1 reads a batch.  One
 * kernel, a wave per read, for every read length. */
int trew_hip_decompose(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                       uint64_t max_items, uint64_t max_rows);
/* The contract of trew_hip_trace_results: *n_items and *n_rows (neither may be NULL) are exact also beyond max_items, max_rows
 * or cap; counts (n_reads values; may be NULL) the items of every read, always exact; records (n_reads; may be NULL) the
 * trew_hip_refined of every read with reserved = anchor.  min(cap, *n_items) items sorted by (read, start) go to `items` when
 * *n_items <= max_items and *n_rows <= max_rows; otherwise nothing is copied into `items` and the call returns 0: repeat
 * trew_hip_decompose with both at least what was reported -- one retry always suffices. */
int trew_hip_decompose_results(trew_hip_ctx *ctx, int slot, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint64_t *n_rows,
                               uint32_t *counts, trew_hip_refined *records, float *ms_kernel);
/* The definition on the host with the full table, over packed planes: *n_items = items found, min(cap, *n_items) items (the
 * first ones of the sorted order), counts and records as above (each may be NULL). */
int trew_decompose_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                        int penalty, uint32_t min_score, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint32_t *counts,
                        trew_hip_refined *records);

/* ---- units in place for every tract of a read, no motif given: trew_hip_tandems with trew_hip_decompose's traceback per tract ----
 * (a long read with a satellite beside a telomere, or two telomeric arrays around a junction: what is each of them made of?)
 * Integer-exact (tests/dissect_ref.py is the reference).  The arguments are those of trew_hip_tandems and
 * trew_hip_decompose, with the same checks and error texts; max_records, max_items and max_rows must each be >= 1.
 * 1. Pieces.  The pieces of a read, their depths, and which pieces give a record are exactly those of trew_hip_tandems,
 *    the weak-piece rule and the pieces too short to repeat included.
 * 2. Records.  A piece [lo, hi) with a record X (score >= min_score) yields a trew_hip_tandem record that equals
 *    trew_hip_tandems' record in every field but reserved, which carries the anchor rho of X.unit as trew_hip_decompose
 *    defines it: M is the smallest rotation of the unit as packed words, no reverse complement taken, M[j] = U[(j + rho) mod k].
 * 3. Items.  The items of that record are those of trew_hip_decompose for the bases lo .. hi - 1 taken as a read of their own,
 *    with lo added to start: trew_hip_trace_items with strand = 0.  motif holds the index of the item's tract among the
 *    read's records in the order of their starts, counting from 0.  Unit lengths 1 and 2 are traced.
 * 4. A weak piece gives no record, no items and claims no rows; its children are walked as in trew_hip_tandems.
 * Records come sorted by (read, start), items by (read, start).  Consequences: the records equal trew_hip_tandems' but for
 * reserved; the depth-0 record and its items equal trew_hip_decompose's record and items of the read whenever that record
 * reaches min_score; the items of a tract tile [start, end) of its record without a gap; their bases, consumed and errors sum
 * to the record's; only the first item of a tract can have phase != 0; a read's output does not depend on the rest of the batch;
 * the rows claimed are the sum of end - start over all records.  Limits: those of trew_hip_tandems and trew_hip_decompose --
 * periods <= 32; linear gaps; a wrong scored_period is not repaired (trew_hip_dissect_resolved, further below, takes
 * trew_hip_resolve's choice for every piece); a weak piece is dropped; signatures compare directly
 * only within one strand value (a tract of the other strand is cut at the smallest rotation of the reverse complement).  Also
 * additive: TREW_HIP_ABI_VERSION stays 4.
 *
 * Like trew_hip_tandems in every respect (batch shapes including device-resident and pair mode, staging, asynchronous on the
 * slot's stream, a context of any mode, no motifs, the checks and their error texts), with buffers of its own and independent of
 * the scan and of the other thirteen kernels.  Further argument errors: "max_records must be at least 1", "max_items must be at
 * least 1", "max_rows must be at least 1".  The kernel appends records to a log of max_records records and items to a log of
 * max_items items and keeps the directions of the traced tracts in a workspace of max_rows rows of 32 bytes; all grow only.  A
 * tract claims end - start rows.  At most 2^32 - 1 reads a batch.  One kernel launch, a wave per read, for every read length;
 * the recursion runs inside the wave. */
int trew_hip_dissect(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                     uint64_t max_records, uint64_t max_items, uint64_t max_rows);
/* Waits for the slot.  *n_records, *n_items and *n_rows (none may be NULL) are the records and items found and the rows claimed,
 * exact also beyond max_records, max_items, max_rows, rec_cap or item_cap; counts (n_reads * 2 values, (tracts, items) of every
 * read; may be NULL) is always exact.  min(rec_cap, *n_records) records and min(item_cap, *n_items) items, each sorted by (read,
 * start), go to `records` and `items` when *n_records <= max_records, *n_items <= max_items and *n_rows <= max_rows; if any of
 * the three capacities is exceeded nothing is copied into `records` or `items` and the call returns 0: repeat trew_hip_dissect
 * with all three at least what was reported -- one retry always suffices.  (A tract whose rows did not fit is still traced, by
 * recomputing its rows block after block: the decision is taken per tract.)  "no trew_hip_dissect on this slot yet" without a
 * call. */
int trew_hip_dissect_results(trew_hip_ctx *ctx, int slot, trew_hip_tandem *records, uint64_t rec_cap, trew_hip_trace_item *items, uint64_t item_cap,
                             uint64_t *n_records, uint64_t *n_items, uint64_t *n_rows, uint32_t *counts, float *ms_kernel);
/* The definition on the host, piece by piece with the full table of every traced piece, over packed planes: *n_records and
 * *n_items (neither may be NULL) as above, *n_rows (may be NULL) the sum of end - start over the records, the first
 * min(rec_cap, *n_records) records and min(item_cap, *n_items) items of the sorted orders, counts as above (may be NULL). */
int trew_dissect_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                      int penalty, uint32_t min_score, trew_hip_tandem *records, uint64_t rec_cap, trew_hip_trace_item *items, uint64_t item_cap,
                      uint64_t *n_records, uint64_t *n_items, uint64_t *n_rows, uint32_t *counts);

/* ---- refine's unit with the period chosen by alignment: the few best-scoring periods each refined, the best record kept ----
 * (step 1 of trew_hip_refine takes the one period with the largest fixed-phase score; on noisy long tracts a multiple or a
 * neighbour of the true period can win there.  Here the alignment decides between the few periods step 1 cannot separate.)
 * Integer-exact.  The read x, its codes, min_period, max_period (<= 32), penalty P and min_score are those of trew_hip_refine,
 * with the same checks and error texts; candidates is C, 1 <= C <= TREW_RESOLVE_MAX_CANDIDATES, anything else is the argument
 * error "resolve: 1 <= candidates <= 4 is required".
 * 1. Scores.  For every admissible k (min_period <= k <= min(max_period, n - 1)) s_k is the trew_hip_periods score of the read
 *    at k.  Order the k by (s_k descending, k ascending); the candidates k_0 .. k_{m-1} are the first C of that order with
 *    s_k >= min_score, so m <= C.  If m = 0 the record is zero.  k_0 is trew_hip_refine's scored_period.
 * 2. Per candidate.  For candidate c, (b, e) is the trew_hip_periods segment of k_c (the smallest e, then the largest b),
 *    start = b and end = e + k_c.  Steps 2 to 6 of trew_hip_refine run with k = k_c and that segment: the seed from the longest
 *    run of eq_{k_c} in [b, e), an N replaced from the unreduced consensus of [start, end) at k_c; align; vote; re-vote; final.
 *    This gives the sixteen words R_c of a trew_hip_refined record with scored_period = k_c and reserved = 0.  R_0 is the read's
 *    trew_hip_refine record word for word.
 * 3. Choice.  The winner is the candidate with the largest R_c.score; on a tie the smaller R_c.period, then the smaller c.
 * 4. Record: the sixteen words of the winner's R_c in trew_hip_refined's layout, then candidates = m, rank = the winner's c,
 *    first_period = R_0.period and first_score = R_0.score.
 * Consequences: with C = 1 the first sixteen words are trew_hip_refine's; score >= first_score >= the seed_score of R_0;
 * rank = 0 implies the sixteen words are trew_hip_refine's; the record is zero exactly when trew_hip_refine's is; score ..
 * matches equal the forward fields of trew_hip_align with the motif `unit` whenever seed_period >= 3; on a perfect repeat
 * rank = 0 (the multiples of the period are the other candidates, their seeds reduce to the same unit and the tie goes to
 * candidate 0).  Limits: the candidates come from the fixed-phase score, so a true period outside the best C is not found; the
 * largest alignment score can prefer a neighbour period over a true-period unit with wrong phases (on one fuzz set of 93 noisy
 * tracts the period alone was right in 77 reads against trew_hip_refine's 79, while the whole unit was right in 77 against 71);
 * the cost is up to C times trew_hip_refine's alignment passes; trew_hip_refine's other limits apply.  Also additive:
 * TREW_HIP_ABI_VERSION stays 4. */
#define TREW_RESOLVE_MAX_CANDIDATES 4
typedef struct {
    uint32_t period, seed_period, scored_period, changed;
    uint32_t score, start, end, consumed, matches;
    uint32_t seed_score, support, reserved;
    uint64_t unit, seed_unit;
    uint32_t candidates, rank, first_period, first_score;
} trew_hip_resolved; /* 80 bytes: the sixteen words of trew_hip_refined, then four of its own */
/* Like trew_hip_refine in every respect (batch shapes including device-resident and pair mode, staging, asynchronous on the
 * slot's stream, a context of any mode, no motifs, the checks and their error texts), with a result buffer of its own that the
 * slot's first call allocates and independent of the scan and of the other fourteen kernels.  One record per read.  One kernel,
 * a wave per read, for every read length. */
int trew_hip_resolve(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                     int candidates);
/* Waits for the slot and copies the records of its last trew_hip_resolve; arguments as trew_hip_refine_results. */
int trew_hip_resolve_results(trew_hip_ctx *ctx, int slot, trew_hip_resolved *out, uint64_t cap, uint64_t *n, float *ms_kernel);
/* The same records on the host, step by step from the definition, over packed planes. */
int trew_resolve_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                      int penalty, uint32_t min_score, int candidates, trew_hip_resolved *out);

/* ---- tandems, decompose and dissect with resolve's period choice: the winner of trew_hip_resolve per piece ----
 * (trew_hip_tandems, trew_hip_decompose and trew_hip_dissect work with trew_hip_refine's record of a piece, whose period is the
 * one with the largest fixed-phase score; for long units that is often a multiple or a neighbour of the true one, and the piece is
 * cut into copies of the wrong unit.  Here every piece gets the record trew_hip_resolve would give it.)
 * Integer-exact (tests/resolved_ref.py is the reference).  The arguments are those of the plain entry point, with
 * the same checks and error texts, then candidates = C as for trew_hip_resolve, with its check and text.
 * resolved(piece, C), for a piece [lo, hi) of a read, is what steps 1 to 3 of trew_hip_resolve give the bases lo .. hi - 1 taken as
 * a read of their own: the number of candidates m; the winner's sixteen words W in trew_hip_refined's layout, start and end
 * shifted by lo, scored_period the winner's k_c; and the trew_hip_periods tract T0 of candidate 0, shifted likewise, which is the
 * tract trew_hip_tandems splits a weak piece around.  m = 0 exactly when the piece has no trew_hip_refine record.
 * trew_hip_tandems_resolved.  tandems(piece): m = 0, nothing; W.score >= min_score, the record W, then tandems([lo, W.start)) and
 *   tandems([W.end, hi)); otherwise (a weak piece) no record, then tandems([lo, T0.start)) and tandems([T0.end, hi)).  Depths, the
 *   sort order, counts, the log and the overflow protocol are trew_hip_tandems'.  W.score >= R_0.score, so a piece that gives
 *   trew_hip_tandems a record gives one here.  The candidates of a piece are periods of the piece, each with its own segment, so
 *   the winner can be another tract than candidate 0's; what is left of the piece is found in the children.
 * trew_hip_decompose_resolved.  trew_hip_decompose with resolved([0, n), C)'s W in the place of trew_hip_refine's record.
 * trew_hip_dissect_resolved.  trew_hip_dissect over the pieces and records of trew_hip_tandems_resolved.
 * In the last two the anchor, the table restarted at W.start, the end phase, the items, the workspace and the three counters are
 * the plain entry point's: (score, start, end, consumed, matches) of W is the alignment of the piece against W.unit.
 * Records keep their types (trew_hip_tandem, trew_hip_refined with reserved = the anchor, trew_hip_trace_item).  Consequences:
 * with C = 1 every result equals the plain entry point's word for word; a read has a depth-0 record exactly when
 * trew_hip_resolve's score reaches min_score, and it is that record.  Limits: candidates, rank, first_period and first_score of
 * trew_hip_resolved are NOT carried by these records (run trew_hip_resolve for them); a tract found at depth 0 here can be one
 * that trew_hip_tandems finds deeper, so depths differ between the two; up to C times the alignment passes per piece; the limits
 * of trew_hip_resolve and of the plain entry points apply.  Also additive: TREW_HIP_ABI_VERSION stays 4.
 * Each call queues on the state of its plain sibling: the results are fetched with trew_hip_tandems_results,
 * trew_hip_decompose_results and trew_hip_dissect_results, the "repeat once with the exact numbers" protocol included, and a
 * plain and a resolved call on one slot replace each other's results. */
int trew_hip_tandems_resolved(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty,
                              uint32_t min_score, int candidates, uint64_t max_records);
int trew_hip_decompose_resolved(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty,
                                uint32_t min_score, int candidates, uint64_t max_items, uint64_t max_rows);
int trew_hip_dissect_resolved(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty,
                              uint32_t min_score, int candidates, uint64_t max_records, uint64_t max_items, uint64_t max_rows);
/* The same on the host, from the definition, over packed planes; arguments as the plain host functions', candidates after min_score. */
int trew_tandems_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                               int max_period, int penalty, uint32_t min_score, int candidates, trew_hip_tandem *out, uint64_t cap, uint64_t *n,
                               uint32_t *counts);
int trew_decompose_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                 int max_period, int penalty, uint32_t min_score, int candidates, trew_hip_trace_item *items, uint64_t cap,
                                 uint64_t *n_items, uint32_t *counts, trew_hip_refined *records);
int trew_dissect_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                               int max_period, int penalty, uint32_t min_score, int candidates, trew_hip_tandem *records, uint64_t rec_cap,
                               trew_hip_trace_item *items, uint64_t item_cap, uint64_t *n_records, uint64_t *n_items, uint64_t *n_rows,
                               uint32_t *counts);

/* ---- host-side packing: the codes[] lookup of kmer.cpp:14-31 applied once per base ---- */
/* words needed for a read of n bases */
uint64_t trew_pack_words(uint64_t n_bases);
/* Packs n reads given as inclusive [st,nd] byte ranges of buf (LocationVector,
 * kmer.h:73) into words/offsets/lengths; returns the words written, or
 * (uint64_t)-1 if words_cap is too small. */
uint64_t trew_pack_reads(const char *buf, const int64_t *st, const int64_t *nd, uint64_t n_reads,
                         uint32_t *words, uint64_t words_cap, uint32_t *offsets, uint32_t *lengths);

/* Same for mate pairs (PairQueueData, kmer.h:98-103): pair i is read i of each buffer; the
 * output holds reads 2i (mate 1) and 2i+1 (mate 2), the layout TREW_MODE_PAIR expects. */
uint64_t trew_pack_pairs(const char *buf1, const int64_t *st1, const int64_t *nd1,
                         const char *buf2, const int64_t *st2, const int64_t *nd2, uint64_t n_pairs,
                         uint32_t *words, uint64_t words_cap, uint32_t *offsets, uint32_t *lengths);

/* ---- synthetic workloads of SURVEY.md section 8(d); identical on host and device ---- */
/* short reads, TTAGGG-seeded: 1.0 % telomeric, 0.5 % junction, 1 % substitutions in those,
 * N with p = 5e-4.  Host: ASCII rows of read_len bytes + '\n'. */
int trew_synth_short_ascii(uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len, char *out);
/* Device: packed triples, read r at word offset r*3*ceil(read_len/32), written to device memory. */
int trew_synth_short_device(trew_hip_ctx *ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                            uint32_t read_len, uint32_t *d_words);
/* paired fragments (config 3): R1 = first read_len bases of a 2*read_len fragment, R2 = revcomp of the rest.
 * Host: mate 1 and mate 2 rows; device: reads 2i, 2i+1 are the mates. */
int trew_synth_pair_ascii(uint64_t seed, uint64_t first_pair, uint64_t n_pairs, uint32_t read_len, char *out1, char *out2);
int trew_synth_pair_device(trew_hip_ctx *ctx, uint64_t seed, uint64_t first_pair, uint64_t n_pairs,
                           uint32_t read_len, uint32_t *d_words);

/* long reads (config 4): lengths from clip(lognormal(9.413, 0.7), 1000, 200000), 5 % with a 2-6 kb
 * (TTAGGG)n 3' tail (5 % substitutions), half reverse-complemented.  lengths first, then the caller
 * lays the reads out (byte offsets of the ASCII rows / u32 word offsets of the packed triples). */
int trew_synth_long_lengths(uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t *lengths);
int trew_synth_long_ascii(uint64_t seed, uint64_t first_read, uint64_t n_reads, const uint64_t *byte_offsets, char *out);
int trew_synth_long_device(trew_hip_ctx *ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                           const uint32_t *d_offsets, uint32_t *d_words);

/* device memory helpers so that a non-C++ host can keep batches resident */
int trew_hip_malloc(trew_hip_ctx *ctx, uint64_t bytes, void **d_ptr);
int trew_hip_free(trew_hip_ctx *ctx, void *d_ptr);
int trew_hip_memcpy_h2d(trew_hip_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int trew_hip_memcpy_d2h(trew_hip_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);
/* pinned host memory for the double-buffered H2D copies of trew_hip_submit */
int trew_hip_host_alloc(trew_hip_ctx *ctx, uint64_t bytes, void **h_ptr);
int trew_hip_host_free(trew_hip_ctx *ctx, void *h_ptr);
int trew_hip_device_count(void);
int trew_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TREW_HIP_H */
