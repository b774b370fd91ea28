// trew_common.hpp -- types shared by the HIP kernels and the C-ABI host layer.
//
// MI355X-native restatement of the hot path of Chemical118/TREW src/kmer.cpp.
// Nothing here is derived from the reference's data structures: per-thread
// direct-address counters / hash maps (ThreadData, kmer.h:132-154) are replaced
// by registers and LDS, the six ResultMaps (kmer.h:79-81) by one device-resident
// open-addressing table with 64-bit CAS keys.
#pragma once
#include <stdint.h>

#include "../../include/trew_hip.h"

namespace trew {

typedef uint32_t u32;
typedef uint64_t u64;

constexpr int kMaxSlots = 6;        // segments per unit: short 3, pair 6, long 2, segment 1
constexpr int kMaxSegBases = 1023;  // longest segment any kernel accepts (short mode rejects reads > 1000, kmer.cpp:1006-1009)
constexpr int kTablePartBits = 9;   // low word bits that select the table partition (see table_add)
constexpr int kThrRows = kMaxSlots + 2;  // rows of the threshold table: one per slot + one per pair of halves of unequal length (joint rows, fill_thresholds)
constexpr int kThrJointRows = 4;    // behind those, four rows of int4 for the loop that judges both halves of a read at once: halves 0/1 and 2/3 of equal length, then of unequal length
constexpr int kThrRow = 66;         // threshold-table entries per slot: k = 1..64, one of read-ahead padding, one to keep rows 16-byte aligned
// (kThrTableBytes, below: those rows and the batch geometry behind them, FilterGeom)
constexpr int kThrNever = 1 << 20;  // a threshold nothing reaches (small enough to be doubled and tripled in the joint rows)

struct DevParams {
    int min_mer, max_mer;
    double low, high;
    float lowf;  // conservative float lower bound of `low` used by the prefilter
    int slice_len;
    int mode;
    u32 flags;
};

struct DevBatch {
    const u32 *words;
    const u32 *offsets;  // nullable
    const u32 *lengths;  // nullable
    u32 uniform_length;
    u32 uniform_stride;
    u64 n_reads;
    u64 n_units;  // reads, or pairs in pair mode
};

// the worklist is a plain array of unit indices (reads / pairs) that survived the prefilter
// One counter block per launch (a slot owns two and alternates, trew_capi.cpp): word 0 = worklist size, then eight 32-word
// lines: word 0 of line s = the exact kernel's queue head of shard s, word kChunkCounterWord = the prefilter's chunk counter of shard s.
constexpr int kChunkCounterWord = 16;
// Two more words of the block's first line belong to the bounds pass (kernels/bounds_pass.inc), which runs between the two kernels:
// the number of leading positions of the exact kernel's list whose packed bounds are stored (the live entries, or with
// TREW_FLAG_DEBUG_NO_LIVE_LIST the worklist entries inside the hand-over buffer), and the entries it found dead.  Both are zero
// where no bounds pass ran: the exact kernel of the launch before cleared the block.
constexpr int kStoredPrefixWord = 1;
constexpr int kDeadEntriesWord = 2;
constexpr int kBoundNeedWords = 97;  // the integer pass thresholds of the bounds pass: one word for every COUNT 0..96 (fill_bound_needs)

// words of DevTable::overflow (one 64-byte line of device counters, cleared by trew_hip_reset_tables)
enum {
    kDiagOverflow = 0,     // a row found the table AND the spill log full: counts were lost, collect fails
    kDiagWorklistDrop = 1, // the prefilter had more survivors than the worklist holds (cannot happen: cap = batch capacity)
    kDiagIntentDrop = 2,   // the pair driver logged more than 32 deferred emissions for one pair (cannot happen: <= 20)
    kDiagInserted = 3,     // keys inserted into the narrow table (occupancy, trew_hip_table_pressure)
    kDiagInsertedWide = 4, // keys inserted into the wide table
    kDiagKernarg = 5,      // TREW_FLAG_DEBUG_POISON_LDS runs: the table descriptor read through the kernarg pointer differed from the by-value argument
    kDiagSpillRows = 6,    // rows in the spill log (DevWide::spill_n points here: one copy reads the whole fill state)
    kDiagG1Drop = 7,       // TREW_FLAG_COMPAT_G1: the stale-row log or its carry was full (collect fails)
    kDiagWords = 16
};

// How often the kernels took their rare fall-back paths (trew_hip_debug_counters).  A module-level device array rather than
// words of DevTable::overflow: decide() and eval_runs() have no table pointer, and the exact kernels have no SGPRs to spare
// for one -- the address of a __device__ variable is a literal.  One array per device, shared by the contexts on it.
enum {
    kFallbackStrictRerun = 0,   // decide(): a speculative skip failed its check and the segment was decided again, every k counted
    kFallbackWindows = 1,       // eval_runs(): more than 64 runs, classes counted per window (eval_k_windows)
    kFallbackWideSpin = 2,      // table_add_wide(): gave up waiting for a slot's ready bit (a duplicate slot may follow; collect merges)
    kFallbackGroupPunt = 3,     // decide_group(): a row gave its segment back (an N, too many heavy k, a failed skip check) and decide() took it
    kFallbackGroupRouted = 4,   // run_short_group(): a read routed and recorded by run_short_routed instead of in row space
    kFallbackGroupTarget = 5,   // run_short_group(): k_mer_target of a read counted by target() (more than 16 runs in the whole read)
    kFallbackHalfDrain = 6,     // filter_kernel<3>: single halves judged by filter_deferred_half (units of which one half was set aside)
    kFallbackUnitDrain = 7,     // filter_kernel<3>: whole units judged by filter_deferred_uni
    kFallbackWords = 8
};

// device scratch of the row-adding entry points (table_check_rows_kernel & co): validation is a pass of its own, so an add is all or nothing
enum { kRowFlagBad = 0, kRowFlagOverflow = 1, kRowFlagMaxLo = 2, kRowFlagMaxHi = 3, kRowFlagWords = 4 };

struct DevTable {
    u64 *keys;    // 0 = empty
    u64 *counts;
    u32 log2_part_slots;  // slots per partition = 1 << log2_part_slots; 512 partitions
    u32 *overflow;        // kDiagWords counters, see above
    const struct DevWide *wide;  // device-resident descriptor of the wide-entry table (k > 32)
};

// TREW_FLAG_COMPAT_G1 (pair mode): what the whole-read block of a pair recorded into temp_result_left stays there in the
// reference's 64-bit branch and is added again by the next pair.  The exact kernel logs those rows and every pair's
// chain flags; g1_apply_kernel adds them again after the batch's exact kernel, rows of the batch's last pair travel to the next
// batch in a carry buffer.  Lives behind the DevTable in the exact kernels' descriptor argument (DevTableG1, defined below DevWide).
struct DevG1 {
    trew_hip_row *log;          // {k, table = forward_high | forward_low, word_lo, word_hi = pair index in the batch, count}
    u32 *counters;              // [0] rows in log, [1] rows in the carry read by this batch, [2] rows in the carry it writes
    unsigned char *pair_flags;  // per pair: bit b = all four segments chained for baseline b (kmer.cpp:378, 389);
                                // bit 2 + b = the whole-read block's `both` condition (kmer.cpp:487, 494); zeroed per batch
    u32 log_cap;
};


// wide entries (k in (32, 64], 128-bit words): tag / word halves / count per slot.  Kept behind a
// pointer so that DevTable stays small enough to travel in registers.
// spill_*: append-only log of (table, k, word, count) rows that found their table partition (or the
// wide table) full; trew_hip_collect merges it, so a skewed key distribution degrades gracefully
// instead of failing.  overflow (DevTable) is only raised when the log itself is full.
struct DevWide {
    u64 *wtag, *wlo, *whi, *wcount;
    u32 wide_log2_slots;
    u32 spill_cap;
    trew_hip_row *spill_rows;
    u32 *spill_n;
    u32 spin_limit;  // polls of a claimed slot's ready bit before table_add_wide gives up on it (0 with TREW_FLAG_DEBUG_WIDE_NO_WAIT)
};

struct DevTableG1 {
    DevTable t;
    DevG1 g;
    DevWide w;  // the wide-table descriptor by value as well: the exact kernels read it where t.wide would point (load_table)
};

// per-read outputs of TREW_MODE_SEGMENT
struct SegResults {
    int32_t *k_high;
    int32_t *k_low;
    u64 *seq_high;     // low 64 bits of MAX_SEQ at k_high
    u64 *seq_low;
    u64 *seq_high_hi;  // high 64 bits (k > 32)
    u64 *seq_low_hi;
};

// one motif of trew_hip_annotate as the kernels read it (kernels/annotate.inc): for strand s (0 = the motif, 1 = its reverse
// complement) and phase q < k, plo/phi[s][q] are the lo / hi plane bits of 32 bases of the endless repetition of the strand's
// target, starting at its base q.  A slot keeps kAnnotMaxMotifs of them in device memory.
constexpr int kAnnotMaxMotifs = TREW_ANNOT_MAX_MOTIFS;
struct AnnotMotifDev {
    u32 k;
    u32 pad[3];
    u32 plo[2][32];
    u32 phi[2][32];
};

// trew_hip_intervals as its kernel reads it (kernels/intervals.inc): the rule of every motif, by value in the kernel's
// arguments, and the slot's append log.
struct IntervalRulesDev {
    u32 max_gap[kAnnotMaxMotifs], min_len[kAnnotMaxMotifs];
};
struct IntervalLog {
    unsigned long long *counter;  // kept intervals found; keeps counting past cap
    u32 *recs;                    // cap records of six u32 (trew_hip_interval)
    u64 cap;
};

// trew_hip_chain's append log (kernels/chain.inc): events, not items -- the host pairs them (trew_capi.cpp).  One event is four
// u32 {read, meta, start, bin}: meta = motif | strand << 4 | kind << 8, kind a set of the bits below (a one-unit run is one
// event with both kChainStart and kChainEnd), bin only for a variant.
constexpr u32 kChainStart = 1u, kChainEnd = 2u, kChainVariant = 4u;
struct ChainLog {
    unsigned long long *counter;  // events found; keeps counting past cap
    uint4 *events;                // cap events
    u64 cap;
};

// trew_hip_repeats' append log (kernels/repeats.inc): records of twelve u32 (trew_hip_repeat); trew_hip_satellites' as well
// (kernels/satellites.inc): records of 26 u32 (trew_hip_satellite); trew_hip_tandems' too (kernels/tandems.inc): records of 18
// u32 (trew_hip_tandem)
struct RepeatLog {
    unsigned long long *counter;  // tracts found; keeps counting past cap
    u32 *recs;                    // cap records
    u64 cap;
};

// trew_hip_trace's item log and direction workspace (kernels/trace.inc): items of twelve u32 (trew_hip_trace_item), rows of 64
// bytes (a direction byte a lane); trew_hip_decompose's as well (kernels/decompose.inc), whose rows have one strand and 32 bytes
struct TraceLog {
    unsigned long long *counter;      // items found; keeps counting past cap
    u32 *recs;                        // cap items
    u64 cap;
    unsigned long long *row_counter;  // rows claimed; keeps counting past max_rows
    unsigned char *rows;              // max_rows rows
    u64 max_rows;
};

struct Segment {
    u32 mate;   // 0 = first read of the unit, 1 = second (pair mode)
    u32 start;  // first base
    u32 len;    // bases
    int kmin, kmax;
    bool valid;
};

#if defined(__HIPCC__)
#define TREW_HD __host__ __device__
#else
#define TREW_HD
#endif

// Segment geometry of every per-read driver of the reference, as a pure
// function of the read length(s).  slot numbering:
//   short  (buffer_task, kmer.cpp:115-171):       0 left half, 1 right half, 2 whole read
//   pair   (buffer_task_pair, kmer.cpp:333-340, 467-480): 0 R1-left 1 R1-right 2 R2-right 3 R2-left 4 R1 whole 5 R2 whole
//   long   (buffer_task_long, kmer.cpp:790-798, 836-838): 0 first slice, 1 last slice (interior slices on demand)
//   segment (k_mer_check, kmer.h:232):            0 whole read
TREW_HD inline Segment get_segment(int mode, int slot, u32 n1, u32 n2, int MIN_MER, int MAX_MER, int SLICE) {
    Segment s;
    s.mate = 0;
    s.start = 0;
    s.len = 0;
    s.kmin = 1;
    s.kmax = 0;
    s.valid = false;
    auto imin = [](int a, int b) { return a < b ? a : b; };
    auto imax = [](int a, int b) { return a > b ? a : b; };
    if (mode == TREW_MODE_SHORT) {
        int n = (int) n1;
        if (2 * MIN_MER > n) return s;
        if (slot <= 1) {
            if (4 * MIN_MER > n) return s;
            s.kmin = MIN_MER;
            s.kmax = imin(n / 4, MAX_MER);
            if (slot == 0) {
                s.start = 0;
                s.len = (u32) (n / 2);
            } else {
                s.start = (u32) (n - (n + 1) / 2);
                s.len = (u32) ((n + 1) / 2);
            }
            s.valid = true;
        } else if (slot == 2) {
            if (4 * MAX_MER <= n) return s;
            s.kmin = imax(n / 4 + 1, MIN_MER);
            s.kmax = imin(n / 2, MAX_MER);
            s.start = 0;
            s.len = (u32) n;
            s.valid = s.kmin <= s.kmax;
        }
    } else if (mode == TREW_MODE_PAIR) {
        int a = (int) n1, b = (int) n2;
        int n = imin(a, b);
        if (2 * MIN_MER > n) return s;
        if (slot <= 3) {
            if (4 * MIN_MER > n) return s;
            s.kmin = MIN_MER;
            s.kmax = imin(n / 4, MAX_MER);
            if (slot == 0) {
                s.mate = 0; s.start = 0; s.len = (u32) (a / 2);
            } else if (slot == 1) {
                s.mate = 0; s.start = (u32) (a - (a + 1) / 2); s.len = (u32) ((a + 1) / 2);
            } else if (slot == 2) {
                s.mate = 1; s.start = (u32) (b - (b + 1) / 2); s.len = (u32) ((b + 1) / 2);
            } else {
                s.mate = 1; s.start = 0; s.len = (u32) (b / 2);
            }
            s.valid = true;
        } else if (slot <= 5) {
            if (4 * MAX_MER <= n) return s;
            s.kmin = imax(n / 4 + 1, MIN_MER);
            s.kmax = imin(n / 2, MAX_MER);
            s.mate = (u32) (slot - 4);
            s.start = 0;
            s.len = slot == 4 ? (u32) a : (u32) b;
            s.valid = s.kmin <= s.kmax;
        }
    } else if (mode == TREW_MODE_LONG) {
        int len = (int) n1;
        int snum = len / SLICE;
        if (snum == 0 || slot > 1) return s;
        int mid = (snum + 1) / 2;
        int bonus = len % SLICE;
        s.kmin = MIN_MER;
        s.kmax = MAX_MER;
        if (slot == 0) {
            s.start = 0;
            s.len = (u32) (SLICE + (1 == mid ? bonus : 0));
        } else {
            int sl = SLICE + (snum == mid ? bonus : 0);
            s.start = (u32) (len - sl);
            s.len = (u32) sl;
        }
        s.valid = true;
    } else {  // TREW_MODE_SEGMENT
        if (slot != 0 || n1 == 0) return s;
        s.kmin = MIN_MER;
        s.kmax = MAX_MER;
        s.start = 0;
        s.len = n1;
        s.valid = true;
    }
    return s;
}

// Windows the prefilter's uniform-geometry fast path LOOKS AT for (segment length L, k) in an nw-word kernel: all COUNT = L-k+1
// of them, except that the 3-word kernel stops at the first 64 when there are 65..kUniSubsetMax (a sound subset bound, see
// filter_k_uni).  fill_thresholds (host) and the kernel both go by this function.
constexpr int kUniSubsetMax = 72;
TREW_HD inline int uni_windows(int nw, int L, int k) {
    const int W = L - k + 1;
    return (nw == 3 && W > 64 && W <= kUniSubsetMax) ? 64 : W;
}

TREW_HD inline int mode_slots(int mode) {
    return mode == TREW_MODE_SHORT ? 3 : mode == TREW_MODE_PAIR ? 6 : mode == TREW_MODE_LONG ? 2 : 1;
}

// ---- the prefilter's batch geometry, worked out on the host once per read length (build_filter_geom below) ----
// A batch of equal-length reads has one segment geometry.  filter_kernel used to derive it in every round of its persistent
// loop (get_segment per slot, the joint loop's admission test, the has-N masks); it now reads the block below, which lies
// behind the joint rows of the threshold table, through wave-uniform scalar loads at the point of use.
// Every struct is a whole number of 32- or 64-byte lines: one s_load_dwordx8 / x16 each.

// the k loop the prefilter runs: MAX_MER, or nothing with TREW_FLAG_DEBUG_NO_KLOOP
TREW_HD inline int filter_gmax_run(const DevParams &P) { return (P.flags & TREW_FLAG_DEBUG_NO_KLOOP) ? P.min_mer - 1 : P.max_mer; }
TREW_HD inline u32 geom_low_mask(int bits) { return bits >= 32 ? 0xffffffffu : (bits <= 0 ? 0u : ((1u << bits) - 1u)); }

// The joint loop (filter_halves_uni, 3-word kernel) takes the halves a, b of slots 2p, 2p + 1: equal length, or a right half
// one base longer (reads of odd length: it is judged by its first L bases against the joint thresholds of row 2 + p), at most 95
// bases, one k range, and every k of the loop with 32..kUniSubsetMax windows.
TREW_HD inline bool joint_loop_admits(const Segment &a, const Segment &b, int klo, int khi) {
    const int L = (int) a.len;
    const bool uneq = b.len == a.len + 1u;
    return a.valid && b.valid && (a.len == b.len || uneq) && a.len <= 95u && a.kmin == b.kmin && a.kmax == b.kmax &&
           klo >= L + 1 - kUniSubsetMax && khi <= L - 32 && klo <= 31;
}

// Geometry the drains of the 3-word kernel need (filter_deferred_uni, filter_deferred_half): the valid segments are exactly the
// 2 (short) or 4 (pair) halves, pairing up as (0, 1) and (2, 3), all with the same [kmin, kmax], at most 95 bases and one base
// apart, k <= length.
TREW_HD inline bool drain_uni_applies(const DevParams &P, u32 UL, int gmax_run) {
    const int n_halves = P.mode == TREW_MODE_PAIR ? 4 : (P.mode == TREW_MODE_SHORT ? 2 : 0);
    if (n_halves == 0) return false;
    for (int slot = n_halves; slot < mode_slots(P.mode); slot++)
        if (get_segment(P.mode, slot, UL, UL, P.min_mer, P.max_mer, P.slice_len).valid) return false;
    const Segment first = get_segment(P.mode, 0, UL, UL, P.min_mer, P.max_mer, P.slice_len);
    for (int p = 0; p < n_halves; p += 2) {
        const Segment a = get_segment(P.mode, p, UL, UL, P.min_mer, P.max_mer, P.slice_len);
        const Segment b = get_segment(P.mode, p + 1, UL, UL, P.min_mer, P.max_mer, P.slice_len);
        const int la = (int) a.len, lb = (int) b.len, lmin = la < lb ? la : lb, lmax = la < lb ? lb : la;
        const int khi = a.kmax < gmax_run ? a.kmax : gmax_run;
        if (!(a.valid && b.valid && a.kmin == b.kmin && a.kmax == b.kmax && lmax <= 95 && lmax - lmin <= 1 && a.kmin >= 1 && khi <= lmin)) return false;
        if (a.kmin != first.kmin || a.kmax != first.kmax) return false;  // filter_deferred_half: one k loop for halves of either pair
    }
    return true;
}

// What a round of the joint loop reads for one pair of halves.  The loop treats both halves alike (one length L, one row of
// thresholds): p and q are the halves as it sees them, of slots slot_p and slot_q (which matters only for the slot handed to
// the half drain).
struct HalvesRound {
    int L, klo, khi;   // length the loop judges both halves by; its k range
    u32 row;           // joint threshold row: p for equal halves, 2 + p for a right half one base longer
    u32 one_load;      // both halves from one load and one prefix parity of the whole read (load_read5), p its left half
    u32 mate;          // one_load: the read that holds both halves
    u32 bs;            // one_load: (first base of the right half) & 31; that base lies in word 2
    u32 slot_p, slot_q;
    // has-N masks.  one_load: of words 0..2 (left half) and words 2..4 (right half) of the read's raw N plane.
    // Otherwise of the three words of half a = p (L bases: its feature mask as well) and of half b = q (its own length: an N in
    // the right half's extra base counts).
    u32 nl[3], nr[3];
    u32 read_words;    // triples of a read of the batch: (uniform_length + 31) / 32
};
// What the two-load path reads on top (halves starting in word 1, reads of 160 bases)
struct HalvesLoads {
    u32 mate_a, start_a, mate_b, start_b;
    u32 pad[4];
};
// one valid slot: get_segment's answer, and whether the segment is too long for the batch's kernel instantiation
struct SlotGeom {
    u32 slot, mate, start, len;
    int kmin, kmax;
    u32 too_long, pad;
};
struct GeomHead {
    u32 nw;         // the kernel instantiation the block was filled for (pick_nw of the longest valid segment)
    u32 n_halves;   // 2 short, 4 pair, else 0
    u32 n_joint;    // leading pairs of halves the joint loop takes (their slots are slot[0 .. 2 n_joint - 1])
    u32 n_slots;    // valid slots, in slot order, in slot[]
    u32 drain_ok;   // drain_uni_applies
    int drain_klo, drain_khi;  // the drains' k loop
    int drain_lmax;            // the longest half
};
struct FilterGeom {  // every member aligned to its own size
    HalvesRound round[2];  // per pair of halves
    HalvesLoads loads[2];
    SlotGeom slot[kMaxSlots];
    GeomHead head;
    u32 pad[8];
};
static_assert(sizeof(HalvesRound) == 64 && sizeof(HalvesLoads) == 32 && sizeof(SlotGeom) == 32 && sizeof(GeomHead) == 32, "one scalar load each");
constexpr size_t kThrGeomOffset = (size_t) kThrRows * kThrRow * 8 + (size_t) kThrJointRows * kThrRow * 16;  // behind the joint rows
static_assert(kThrGeomOffset % 64 == 0 && sizeof(FilterGeom) % 64 == 0, "the block's lines are aligned");
// two blocks: the batch's, and the same with no pair of halves handed to the joint loop -- what a launch that wants the per-slot
// candidate masks (trew_hip_filter_masks) reads, so that no round has to ask
constexpr size_t kThrTableBytes = kThrGeomOffset + 2 * sizeof(FilterGeom);

// The block for reads of uniform_length in an nw-word kernel.  P.flags count: TREW_FLAG_DEBUG_NO_JOINT (no pair goes to the joint
// loop) and TREW_FLAG_DEBUG_NO_KLOOP (the k ranges are empty).
TREW_HD inline void build_filter_geom(const DevParams &P, u32 UL, int nw, FilterGeom *g) {
    const int gmax_run = filter_gmax_run(P);
    const int nslots = mode_slots(P.mode);
    GeomHead &hd = g->head;
    hd.nw = (u32) nw;
    hd.n_halves = P.mode == TREW_MODE_PAIR ? 4u : (P.mode == TREW_MODE_SHORT ? 2u : 0u);
    hd.n_joint = 0;
    hd.n_slots = 0;
    for (int j = 0; j < 8; j++) g->pad[j] = 0;
    for (int i = 0; i < kMaxSlots; i++) {
        SlotGeom &o = g->slot[i];
        o.slot = o.mate = o.start = o.len = 0;
        o.kmin = 1, o.kmax = 0;
        o.too_long = o.pad = 0;
    }
    for (int slot = 0; slot < nslots; slot++) {
        const Segment sg = get_segment(P.mode, slot, UL, UL, P.min_mer, P.max_mer, P.slice_len);
        if (!sg.valid) continue;
        SlotGeom &o = g->slot[hd.n_slots++];
        o.slot = (u32) slot, o.mate = sg.mate, o.start = sg.start, o.len = sg.len;
        o.kmin = sg.kmin, o.kmax = sg.kmax;
        o.too_long = sg.len > (u32) (32 * nw - 1) ? 1u : 0u;
    }
    bool joint = nw == 3 && !(P.flags & TREW_FLAG_DEBUG_NO_JOINT);
    for (int p = 0; p < 2; p++) {
        HalvesRound &r = g->round[p];
        HalvesLoads &l = g->loads[p];
        r.L = r.klo = 0, r.khi = -1;
        r.row = r.one_load = r.mate = r.bs = r.slot_p = r.slot_q = 0;
        r.read_words = (UL + 31u) >> 5;
        for (int j = 0; j < 3; j++) r.nl[j] = r.nr[j] = 0;
        l.mate_a = l.start_a = l.mate_b = l.start_b = 0;
        for (int j = 0; j < 4; j++) l.pad[j] = 0;
        if (2 * p + 1 >= (int) hd.n_halves) joint = false;
        if (!joint) continue;
        const Segment a = get_segment(P.mode, 2 * p, UL, UL, P.min_mer, P.max_mer, P.slice_len);
        const Segment b = get_segment(P.mode, 2 * p + 1, UL, UL, P.min_mer, P.max_mer, P.slice_len);
        const int klo = a.kmin > P.min_mer ? a.kmin : P.min_mer, khi = a.kmax < gmax_run ? a.kmax : gmax_run;
        if (!joint_loop_admits(a, b, klo, khi)) {  // as the kernel's loop over the pairs did: the first pair it does not take ends it
            joint = false;
            continue;
        }
        hd.n_joint = (u32) p + 1u;
        r.L = (int) a.len, r.klo = klo, r.khi = khi;
        const bool uneq = b.len == a.len + 1u;
        r.row = (u32) (uneq ? 2 + p : p);
        l.mate_a = a.mate, l.start_a = a.start, l.mate_b = b.mate, l.start_b = b.start;
        // the halves by position: a is the left one; the first base of the right one; their lengths
        const bool a_left = a.start == 0u;
        const u32 h = a_left ? b.start : a.start, len_l = a_left ? a.len : b.len, len_r = a_left ? b.len : a.len;
        // Both halves lie in one read of at most five triples, one from base 0 and the other from a base in [64, 96).  Not 160
        // bases: bit L of the right half's prefix parity would be bit 160 of the read's (halves_prefix_read5).
        r.one_load = (UL <= 159u && a.mate == b.mate && (a_left ? a.start : b.start) == 0u && (h >> 5) == 2u && h + len_r <= UL) ? 1u : 0u;
        r.mate = a.mate;
        r.bs = h & 31u;
        r.slot_p = (u32) (2 * p), r.slot_q = (u32) (2 * p + 1);
        if (r.one_load) {
            if (!a_left) r.slot_p = (u32) (2 * p + 1), r.slot_q = (u32) (2 * p);
            for (int j = 0; j < 3; j++) {
                r.nl[j] = geom_low_mask((int) len_l - 32 * j);
                r.nr[j] = geom_low_mask((int) (h + len_r) - 32 * (j + 2)) & ~geom_low_mask((int) h - 32 * (j + 2));
            }
        } else {
            for (int j = 0; j < 3; j++) {
                r.nl[j] = geom_low_mask(r.L - 32 * j);
                r.nr[j] = geom_low_mask((int) b.len - 32 * j);
            }
        }
    }
    hd.drain_ok = drain_uni_applies(P, UL, gmax_run) ? 1u : 0u;
    const Segment first = get_segment(P.mode, 0, UL, UL, P.min_mer, P.max_mer, P.slice_len);
    hd.drain_klo = first.kmin > P.min_mer ? first.kmin : P.min_mer;
    hd.drain_khi = first.kmax < gmax_run ? first.kmax : gmax_run;
    hd.drain_lmax = 0;
    for (u32 i = 0; i < hd.n_halves && i < hd.n_slots; i++) hd.drain_lmax = (int) g->slot[i].len > hd.drain_lmax ? (int) g->slot[i].len : hd.drain_lmax;
}

}  // namespace trew
