// trew_capi.cpp -- the extern "C" layer of libtrew_hip.so (see include/trew_hip.h).
//
// Host side only: owns the HIP streams, the per-slot device buffers, the device
// count table, and launches the kernels of trew_kernels.hip.  There is no CPU
// fallback: every compute entry point fails loudly when HIP is unavailable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "trew_common.hpp"
#include "trew_launch.hpp"
#include "trew_measures_host.hpp"
#include "trew_synth.hpp"

using namespace trew;

namespace {

// The per-read measures (trew_hip_annotate, _tracts, _intervals, _variants, _periods, _chain, _repeats, _satellites, _align, _refine, _tandems, _trace, _decompose, _dissect, _resolve, _monomers, _copies, _polish) and what a slot keeps of each.
enum Measure { kAnnotate, kTracts, kIntervals, kVariants, kPeriods, kChain, kRepeats, kSatellites, kAlign, kRefine, kTandems, kTrace, kDecompose, kDissect, kResolve, kMonomers, kCopies, kPolish, kMeasures };
const char *const kMeasureName[kMeasures] = {"annotate", "tracts", "intervals", "variants", "periods", "chain", "repeats", "satellites", "align", "refine", "tandems", "trace", "decompose", "dissect", "resolve", "monomers", "copies", "polish"};
// whether the measure takes motifs: one that takes none has no motif check and no pattern table (measure_begin)
const bool kMeasureHasMotifs[kMeasures] = {true, true, true, true, false, true, false, false, true, false, false, true, false, false, false, false, false, false};  // monomers, copies: their own table (stage_monomers), no pattern table
struct DevBuf {
    void *p = nullptr;
    u64 bytes = 0;  // capacity
};
struct MeasureState {
    DevBuf records;                         // the records of the last call, grown on demand (intervals, chain, repeats, satellites, tandems: the append log)
    DevBuf counts;                          // intervals: one u32 per (read, motif, strand), chain: two; repeats, satellites, tandems: one per read; grown on demand
    unsigned long long *counter = nullptr;  // intervals, chain, repeats, satellites, tandems: the records / events the kernel found, in the log or not
    unsigned long long *hist = nullptr;     // variants: the batch histograms hist, then reads_with, kVarHistLen values each
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool valid = false, timed = false;  // a call was queued / its kernel was launched between the events
    // the numbers of the last call, set in one place each: queue_records (the fixed-size records), queue_log (the append logs)
    u64 n = 0;         // annotate, tracts, variants, align, monomers: its records, n_reads * n_motifs; periods, refine, resolve: n_reads
    u64 max_log = 0;   // intervals: its max_intervals; chain: its max_events; repeats, satellites, tandems: their max_records
    u64 n_counts = 0;  // intervals: n_reads * n_motifs * 2; chain: twice that; repeats, satellites, tandems: n_reads
    int n_motifs = 0;  // variants
    u32 k[kAnnotMaxMotifs] = {};  // chain: the motifs' lengths (pairing a run's events needs start mod k)
    // trace: `records` is its item log, `counter` two values (items, rows), `counts` one u32 per (read, motif, strand); beside them
    // (decompose: the same, `counts` one u32 per read)
    DevBuf rows;       // the direction workspace, 64 bytes a row (decompose: 32), grown on demand
    DevBuf aligned;    // the trew_hip_alignment of every (read, motif) (decompose: the trew_hip_refined of every read)
    u64 max_rows = 0;  // the max_rows of the last call (max_log: its max_items; n: its alignment records)
    // dissect: as decompose, with `aligned` its log of trew_hip_tandem records, `counter` three values (items, rows, records),
    // `counts` two u32 per read; n: the max_records of the last call
};

struct Slot {
    hipStream_t stream = nullptr;
    u32 *d_buf = nullptr;  // one allocation: [offsets max_batch_reads][lengths max_batch_reads][words max_batch_words + slack]
    u32 *d_words = nullptr, *d_offsets = nullptr, *d_lengths = nullptr;  // views into d_buf
    unsigned char *d_ascii = nullptr;  // text batches: [word_offsets][byte_offsets][lengths][bases], max_batch_ascii_bytes + slack
    u32 *d_wl = nullptr;
    u32 *d_wl_count = nullptr;
    // the hand-over of the bounds pass (kernels/bounds_pass.inc): the packed bounds of the first bnd_cap worklist entries of the
    // slot's batch, written between its prefilter and its exact kernel (nullptr / 0: a context whose batches never take that pass)
    u32 *d_bnd = nullptr;
    u32 bnd_cap = 0;
    // the live worklist of the same pass: those of the first bnd_cap entries the exact kernel can still record something for
    // (bnd_cap words; nullptr with TREW_FLAG_DEBUG_NO_LIVE_LIST).  live_launch: the slot's last launch read it.
    u32 *d_live = nullptr;
    bool live_launch = false;
    int2 *d_thr = nullptr;   // pass thresholds of the prefilter's uniform-geometry path (kThrRows * kThrRow)
    int2 *h_thr = nullptr;   // pinned staging of the same
    hipEvent_t ev_tail = nullptr, ev_copied = nullptr;  // order the context's copy stream behind / in front of this slot's stream (BatchCopy)
    u32 *h_seen = nullptr;   // TREW_FLAG_TRACK_PRESSURE: the counter line as of the end of this slot's last batch (pinned, behind h_thr)
    u32 thr_length = 0;      // uniform read length d_thr was computed for (0: none yet)
    u32 thr_flags = 0;       // and the context's flags: the batch geometry behind the thresholds (FilterGeom) folds the debug flags in
    SegResults res = {nullptr, nullptr, nullptr, nullptr};
    // ring of (before filter, between, after exact) events: submits may be queued back to back
    // on the slot's stream without a wait in between, each keeps its own timestamps
    static constexpr int kRing = 128;
    hipEvent_t ev[kRing][3] = {};
    u64 n_launches = 0;  // submits that launched kernels: picks the counter block
    u64 n_submits = 0;   // submits since init
    u64 n_reported = 0;  // submits already averaged by trew_hip_last_timing
    u64 n_units = 0;
    // the pattern tables of the per-read motif measures (stage_motifs) and the state of each measure; all of it is created by
    // the slot's first call of a measure (a context that only scans allocates nothing of it)
    AnnotMotifDev *d_motifs = nullptr, *h_motifs = nullptr;  // kAnnotMaxMotifs pattern tables: device copy and pinned staging
    int motifs_staged = 0;                                   // motifs of h_motifs that d_motifs holds (or will, in stream order)
    trew_hip_monomer *d_monomers = nullptr, *h_monomers = nullptr;  // monomers: TREW_MONOMERS_MAX (k, unit) entries, staged as the pattern tables are
    int monomers_staged = 0;
    MeasureState measure[kMeasures];
};

thread_local std::string g_init_error;  // trew_hip_init failures before a context exists (read back on the same thread)
// Last error of the calling thread.  Several host threads share one context (one slot each); an error string
// inside the context would be written and read concurrently, so the text lives with the thread that got the
// failing status -- the only one that reads it back.
thread_local std::string g_thread_error;
// One counter block: [0] worklist size, then 8 queue heads on separate 128-B lines.  A slot owns TWO blocks and
// alternates between them; the exact kernel of one submit clears the block of the next (see exact_kernel), so a
// submit needs no memset call of its own.  Both are cleared once at init.
constexpr size_t kWlCountWords = 32 + 8 * 32;
constexpr size_t kWlCountBytes = kWlCountWords * 4;

}  // namespace

struct trew_hip_ctx {
    trew_hip_params p;
    DevParams dp;
    DevTable table;
    DevTableG1 table_g1;  // `table` (with TREW_FLAG_DEBUG_NO_EMIT applied) + g1: the exact kernels' descriptor argument
    // TREW_FLAG_COMPAT_G1 (kernels/g1_compat.inc): the stale-row log, the pair flags and the two carry buffers (read / written
    // by a batch, swapped after it)
    DevG1 g1 = {nullptr, nullptr, nullptr, 0};
    trew_hip_row *g1_carry[2] = {nullptr, nullptr};
    u32 g1_carry_cap = 0;
    u64 g1_batches = 0;
    DevWide wide;  // host copy of *table.wide
    u64 table_slots = 0;
    std::vector<Slot> slots;
    // Every host-to-device copy of a batch goes through this ONE stream, whatever slot it is for.  On ROCm 7 the first DMA-engine
    // copy that a stream issues costs 3.5 ms of host time under a process-wide lock (measured: 30 slots = 0.105 s of a 0.22 s
    // file, the workers of the `trew` host queueing up behind each other, profiles/r03/README.md); after that a 16 MB copy is
    // queued in microseconds.  The link carries one copy at a time anyway, so one stream loses no bandwidth.
    hipStream_t copy_stream = nullptr;
    std::mutex copy_mu;  // a batch's copies and the event behind them are queued as one unit
    // Fills of device memory (the tables at init and reset, the buffers at init) are queued on this stream and every other stream
    // of the context is made to wait for the event behind them -- on the device.  hipMemset on the null stream returns at once
    // (2 us for 256 MiB, tools/memset_probe.hip) while the fill takes 0.13 ms, and the slots' non-blocking streams do not wait for
    // the null stream: a batch submitted right behind it scanned into a table that was still being cleared (round 3's "empty
    // tables once in 270 runs").  Stream order instead of a host wait: init / reset do not stall the submitting threads.
    // (The fill stream IS the copy stream: a stream of its own changed which hardware queue the slots' streams landed on -- ROCm
    // spreads a process's streams over four queues in creation order -- and the two batch slots of bench.py stopped overlapping:
    // 1.10 ms a step instead of 0.91.  Fills only happen while no batch copy is in flight.)
    hipStream_t fill_stream = nullptr;  // alias of copy_stream
    hipEvent_t ev_filled = nullptr;
    int n_cu = 256;
    // persistent scratch of trew_hip_collect (device-side compaction)
    unsigned long long *d_collect_n = nullptr;
    trew_hip_row *d_collect_rows = nullptr;
    u64 collect_cap = 0;
    // persistent scratch of trew_hip_add_rows / trew_hip_merge (grow-only)
    trew_hip_row *d_add_rows = nullptr;
    u64 add_cap = 0;
    u32 *d_row_flags = nullptr;  // kRowFlagWords words: verdict of the validation pass of the row-adding entry points
    hipEvent_t ev_producer = nullptr;  // orders slot 0's stream behind a caller's stream (trew_hip_add_gathered_device)
    std::mutex table_mu;  // collect / reset / add_rows / merge are whole-table operations: one at a time
    // TREW_FLAG_TRACK_PRESSURE: the largest value of each fill counter any host thread has read so far (they only grow
    // between resets); trew_hip_table_pressure answers from these
    std::atomic<u32> seen[kDiagWords];
    std::atomic<int> last_slot{-1};  // slot of the most recent submit (launch_batch: is another slot's batch still running?)
    u32 *d_bound_need = nullptr;  // integer pass thresholds of the bounds pass (fill_bound_needs); nullptr: it keeps its doubles
    std::atomic<int> dead_slot{-1};  // the slot whose counter block holds the dead entries of the most recent launch (-1: it had no live list, or the tables were reset since)
    std::mutex seen_mu;  // keeps a reset (which zeroes the copies) apart from a query that folds them
};

// fold one copy of the counter line into ctx->seen
static void note_seen(trew_hip_ctx *ctx, const u32 *diag) {
    for (int i : {(int) kDiagOverflow, (int) kDiagInserted, (int) kDiagInsertedWide, (int) kDiagSpillRows}) {
        u32 cur = ctx->seen[i].load(std::memory_order_relaxed);
        while (cur < diag[i] && !ctx->seen[i].compare_exchange_weak(cur, diag[i], std::memory_order_relaxed)) {
        }
    }
}

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (void) (ctx);                                                                         \
            g_thread_error = std::string(#expr) + ": " + hipGetErrorString(e_);                   \
            return (int) e_ ? (int) e_ : -1;                                                      \
        }                                                                                         \
    } while (0)

static int fail(trew_hip_ctx *, const std::string &msg) {
    g_thread_error = msg;
    return -1;
}

extern "C" int trew_hip_abi_version(void) { return TREW_HIP_ABI_VERSION; }

extern "C" int trew_hip_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int trew_hip_host_alloc(trew_hip_ctx *ctx, uint64_t bytes, void **h_ptr) {
    if (!ctx || !h_ptr) return -1;
    hipError_t e = hipSetDevice(ctx->p.device);
    if (e == hipSuccess) e = hipHostMalloc(h_ptr, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        g_thread_error = std::string("hipHostMalloc: ") + hipGetErrorString(e);
        return (int) e;
    }
    return 0;
}

extern "C" int trew_hip_host_free(trew_hip_ctx *ctx, void *h_ptr) {
    if (!ctx) return -1;
    hipError_t e = hipHostFree(h_ptr);
    if (e != hipSuccess) {
        g_thread_error = std::string("hipHostFree: ") + hipGetErrorString(e);
        return (int) e;
    }
    return 0;
}

extern "C" const char *trew_hip_last_error(const trew_hip_ctx *ctx) {
    return ctx ? g_thread_error.c_str() : g_init_error.c_str();
}

static float conservative_lowf(double low) {
    float f = (float) (low * (1.0 - 1e-6));
    f = std::nextafterf(f, 0.0f);
    return f;
}

// an event behind everything queued on the fill stream so far; the copy stream and every slot's stream wait for it on the device
static int order_behind_fills(trew_hip_ctx *ctx) {
    HIPCHK(ctx, hipEventRecord(ctx->ev_filled, ctx->fill_stream));
    for (auto &s : ctx->slots)
        if (s.stream) HIPCHK(ctx, hipStreamWaitEvent(s.stream, ctx->ev_filled, 0));
    return 0;
}

extern "C" int trew_hip_init(const trew_hip_params *params, trew_hip_ctx **out) {
    if (!params || !out) {
        g_init_error = "trew_hip_init: null argument";
        return -1;
    }
    *out = nullptr;
    const trew_hip_params &p = *params;
    // same limits as the reference CLI (trew.cpp:175-228, 256-304) + this ABI version's device limits
    if (p.min_mer > p.max_mer) { g_init_error = "MIN_MER must not be greater than MAX_MER."; return -1; }
    if (p.min_mer < 3) { g_init_error = "MIN_MER must be greater than or equal to 3."; return -1; }
    if (p.max_mer > 64) { g_init_error = "MAX_MER must be less than or equal to 64."; return -1; }
    if (!(0 < p.low_baseline && p.low_baseline <= 1) || !(0 < p.high_baseline && p.high_baseline <= 1)) { g_init_error = "Baseline must be in range 0 to 1."; return -1; }
    if (p.low_baseline > p.high_baseline) { g_init_error = "Low baseline must be smaller than high baseline."; return -1; }
    if (p.mode < TREW_MODE_SHORT || p.mode > TREW_MODE_SEGMENT) { g_init_error = "unknown mode"; return -1; }
    if (p.mode == TREW_MODE_LONG) {
        if (p.slice_length < 2 * p.max_mer) { g_init_error = "SLICE_LENGTH must be greater than or equal to twice of MAX_MER."; return -1; }
        if (2 * p.slice_length - 1 > kMaxSegBases) { g_init_error = "SLICE_LENGTH must be at most 512 on the HIP path."; return -1; }
    }
    if ((p.flags & TREW_FLAG_COMPAT_G1) && (p.mode != TREW_MODE_PAIR || p.max_mer > 32 || p.n_slots != 1)) {
        g_init_error = "TREW_FLAG_COMPAT_G1 needs pair mode, MAX_MER <= 32 (the 128-bit branch has no stale map) and n_slots = 1 (file order)";
        return -1;
    }
    if (p.n_slots < 1 || p.n_slots > 512) { g_init_error = "n_slots must be in [1,512]"; return -1; }
    if (p.table_log2_slots < 12 || p.table_log2_slots > 30) { g_init_error = "table_log2_slots must be in [12,30]"; return -1; }
    if (p.max_batch_reads == 0 || p.max_batch_reads > 0xfffffff0ull) { g_init_error = "max_batch_reads out of range"; return -1; }

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_init_error = std::string("no HIP device available: ") + hipGetErrorString(e);
        return -2;
    }
    if (p.device < 0 || p.device >= ndev) { g_init_error = "device ordinal out of range"; return -1; }
    e = hipSetDevice(p.device);
    if (e != hipSuccess) { g_init_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return -2; }

    trew_hip_ctx *ctx = new trew_hip_ctx();
    for (auto &v : ctx->seen) v.store(0, std::memory_order_relaxed);
    memset(&ctx->table, 0, sizeof(ctx->table));
    memset(&ctx->wide, 0, sizeof(ctx->wide));
    ctx->p = p;
    ctx->dp.min_mer = p.min_mer;
    ctx->dp.max_mer = p.max_mer;
    ctx->dp.low = p.low_baseline;
    ctx->dp.high = p.high_baseline;
    ctx->dp.lowf = conservative_lowf(p.low_baseline);
    ctx->dp.slice_len = p.slice_length > 0 ? p.slice_length : 150;
    ctx->dp.mode = p.mode;
    ctx->dp.flags = p.flags;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p.device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;

    auto bail = [&](const char *what, hipError_t er) {
        g_init_error = std::string(what) + ": " + hipGetErrorString(er);
        trew_hip_destroy(ctx);
        return -3;
    };
    if ((e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    ctx->fill_stream = ctx->copy_stream;
    if ((e = hipEventCreateWithFlags(&ctx->ev_filled, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    ctx->table_slots = 1ull << p.table_log2_slots;
    ctx->table.log2_part_slots = p.table_log2_slots - kTablePartBits;
    if ((e = hipMalloc((void **) &ctx->table.keys, ctx->table_slots * 8)) != hipSuccess) return bail("hipMalloc(table keys)", e);
    if ((e = hipMalloc((void **) &ctx->table.counts, ctx->table_slots * 8)) != hipSuccess) return bail("hipMalloc(table counts)", e);
    if ((e = hipMalloc((void **) &ctx->table.overflow, kDiagWords * 4)) != hipSuccess) return bail("hipMalloc(overflow)", e);
    if ((e = hipMemsetAsync(ctx->table.keys, 0, ctx->table_slots * 8, ctx->fill_stream)) != hipSuccess) return bail("hipMemsetAsync", e);
    if ((e = hipMemsetAsync(ctx->table.counts, 0, ctx->table_slots * 8, ctx->fill_stream)) != hipSuccess) return bail("hipMemsetAsync", e);
    if ((e = hipMemsetAsync(ctx->table.overflow, 0, kDiagWords * 4, ctx->fill_stream)) != hipSuccess) return bail("hipMemsetAsync", e);
    // wide entries (k > 32) are rare: a quarter of the slots
    ctx->wide.wide_log2_slots = std::max<u32>(10u, p.table_log2_slots - 2u);
    {
        const size_t wb = (size_t) 8 << ctx->wide.wide_log2_slots;
        u64 **arr[4] = {&ctx->wide.wtag, &ctx->wide.wlo, &ctx->wide.whi, &ctx->wide.wcount};
        for (auto a : arr) {
            if ((e = hipMalloc((void **) a, wb)) != hipSuccess) return bail("hipMalloc(wide table)", e);
            if ((e = hipMemsetAsync(*a, 0, wb, ctx->fill_stream)) != hipSuccess) return bail("hipMemsetAsync", e);
        }
        // spill log: 1/16 of the table's slots, at least 64 k rows
        ctx->wide.spill_cap = (u32) std::max<u64>(1ull << 16, ctx->table_slots >> 4);
        ctx->wide.spin_limit = (p.flags & TREW_FLAG_DEBUG_WIDE_NO_WAIT) ? 0u : (1u << 20);
        if ((e = hipMalloc((void **) &ctx->wide.spill_rows, (size_t) ctx->wide.spill_cap * sizeof(trew_hip_row))) != hipSuccess) return bail("hipMalloc(spill log)", e);
        ctx->wide.spill_n = ctx->table.overflow + kDiagSpillRows;  // cleared with the counter line
        DevWide *dw = nullptr;
        if ((e = hipMalloc((void **) &dw, sizeof(DevWide))) != hipSuccess) return bail("hipMalloc(wide descriptor)", e);
        if ((e = hipMemcpy(dw, &ctx->wide, sizeof(DevWide), hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy", e);
        ctx->table.wide = dw;
    }
    {
        if (p.flags & TREW_FLAG_COMPAT_G1) {
            // a pair's whole-read block records the classes of at most two reads for two baselines; the log is sized for
            // every pair of a full batch doing so with a dozen classes each and reports (never hides) an overflow
            ctx->g1.log_cap = (u32) std::min<u64>(std::max<u64>(1ull << 16, 24ull * (p.max_batch_reads / 2)), 1ull << 26);
            ctx->g1_carry_cap = 1u << 16;
            if ((e = hipMalloc((void **) &ctx->g1.log, (size_t) ctx->g1.log_cap * sizeof(trew_hip_row))) != hipSuccess) return bail("hipMalloc(G1 log)", e);
            if ((e = hipMalloc((void **) &ctx->g1.counters, 16)) != hipSuccess) return bail("hipMalloc(G1 counters)", e);
            if ((e = hipMemsetAsync(ctx->g1.counters, 0, 16, ctx->fill_stream)) != hipSuccess) return bail("hipMemsetAsync", e);
            if ((e = hipMalloc((void **) &ctx->g1.pair_flags, (size_t) (p.max_batch_reads / 2 + 64))) != hipSuccess) return bail("hipMalloc(G1 pair flags)", e);
            for (auto &cb : ctx->g1_carry)
                if ((e = hipMalloc((void **) &cb, (size_t) ctx->g1_carry_cap * sizeof(trew_hip_row))) != hipSuccess) return bail("hipMalloc(G1 carry)", e);
        }
        DevTableG1 tbl;
        tbl.t = ctx->table;
        tbl.g = ctx->g1;
        tbl.w = ctx->wide;
        if (p.flags & TREW_FLAG_DEBUG_NO_EMIT) tbl.t.log2_part_slots = 0xffffffffu;  // cached_add drops every row
        ctx->table_g1 = tbl;
    }

    if ((e = hipMalloc((void **) &ctx->d_row_flags, kRowFlagWords * 4)) != hipSuccess) return bail("hipMalloc(row flags)", e);
    if (bounds_pass_applies(ctx->dp, 1)) {
        u32 need[kBoundNeedWords];
        if (fill_bound_needs(ctx->dp, need)) {  // LOW and HIGH are the context's: once
            if ((e = hipMalloc((void **) &ctx->d_bound_need, sizeof(need))) != hipSuccess) return bail("hipMalloc(bound thresholds)", e);
            if ((e = hipMemcpy(ctx->d_bound_need, need, sizeof(need), hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy(bound thresholds)", e);
        }
    }
    if ((e = hipEventCreateWithFlags(&ctx->ev_producer, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    ctx->slots.resize((size_t) p.n_slots);
    for (auto &s : ctx->slots) {
        if ((e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
        if ((e = hipEventCreateWithFlags(&s.ev_tail, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&s.ev_copied, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
        {
            // +8 words of slack: the exact kernel fetches whole 64-word heads of a read
            const size_t words = 2 * (size_t) p.max_batch_reads + (size_t) p.max_batch_words + 8;
            if ((e = hipMalloc((void **) &s.d_buf, words * 4)) != hipSuccess) return bail("hipMalloc(batch buffer)", e);
            if ((e = hipMemsetAsync(s.d_buf, 0, words * 4, ctx->fill_stream)) != hipSuccess) return bail("hipMemsetAsync", e);
            s.d_offsets = s.d_buf;
            s.d_lengths = s.d_buf + p.max_batch_reads;
            s.d_words = s.d_buf + 2 * (size_t) p.max_batch_reads;
        }
        if (p.max_batch_ascii_bytes) {
            if ((e = hipMalloc((void **) &s.d_ascii, p.max_batch_ascii_bytes + 256)) != hipSuccess) return bail("hipMalloc(text buffer)", e);
            if ((e = hipMemsetAsync(s.d_ascii, 0, p.max_batch_ascii_bytes + 256, ctx->fill_stream)) != hipSuccess) return bail("hipMemsetAsync", e);
        }
        if ((e = hipMalloc((void **) &s.d_thr, kThrTableBytes)) != hipSuccess) return bail("hipMalloc(thresholds)", e);
        if ((e = hipHostMalloc((void **) &s.h_thr, kThrTableBytes + kDiagWords * 4, hipHostMallocDefault)) != hipSuccess) return bail("hipHostMalloc(thresholds)", e);
        s.h_seen = (u32 *) ((char *) s.h_thr + kThrTableBytes);
        memset(s.h_seen, 0, kDiagWords * 4);
        if ((e = hipMalloc((void **) &s.d_wl, p.max_batch_reads * sizeof(u32))) != hipSuccess) return bail("hipMalloc(worklist)", e);
        if (bounds_pass_applies(ctx->dp, 1)) {  // (by mode, k range and flags; the batch's geometry decides again at every submit)
            // 256 bytes an entry: not for every read of a batch.  1 to 2 % of WGS-like reads are flagged; a thirty-second of the
            // batch (but room for 64 k entries, a small batch in full) leaves a margin, and entries beyond it are bounded by the
            // exact kernel's rows as before; never more than 4 M entries (1 GiB).  TREW_FLAG_DEBUG_SMALL_BOUNDS: 64 entries, so that a
            // small batch takes both paths.
            const u64 share = std::min<u64>(std::max<u64>(p.max_batch_reads / 32, std::min<u64>(p.max_batch_reads, 1ull << 16)), 1ull << 22);
            s.bnd_cap = (p.flags & TREW_FLAG_DEBUG_SMALL_BOUNDS) ? 64u : (u32) share;
            if ((e = hipMalloc((void **) &s.d_bnd, (size_t) s.bnd_cap * bounds_entry_bytes())) != hipSuccess) return bail("hipMalloc(bounds)", e);
            if (!(p.flags & TREW_FLAG_DEBUG_NO_LIVE_LIST) && (e = hipMalloc((void **) &s.d_live, (size_t) s.bnd_cap * sizeof(u32))) != hipSuccess)
                return bail("hipMalloc(live worklist)", e);
        }
        if ((e = hipMalloc((void **) &s.d_wl_count, 2 * kWlCountBytes)) != hipSuccess) return bail("hipMalloc(wl_count)", e);
        if ((e = hipMemsetAsync(s.d_wl_count, 0, 2 * kWlCountBytes, ctx->fill_stream)) != hipSuccess) return bail("hipMemsetAsync", e);
        if (p.mode == TREW_MODE_SEGMENT) {
            if ((e = hipMalloc((void **) &s.res.k_high, p.max_batch_reads * 4)) != hipSuccess) return bail("hipMalloc", e);
            if ((e = hipMalloc((void **) &s.res.k_low, p.max_batch_reads * 4)) != hipSuccess) return bail("hipMalloc", e);
            if ((e = hipMalloc((void **) &s.res.seq_high, p.max_batch_reads * 8)) != hipSuccess) return bail("hipMalloc", e);
            if ((e = hipMalloc((void **) &s.res.seq_low, p.max_batch_reads * 8)) != hipSuccess) return bail("hipMalloc", e);
            if ((e = hipMalloc((void **) &s.res.seq_high_hi, p.max_batch_reads * 8)) != hipSuccess) return bail("hipMalloc", e);
            if ((e = hipMalloc((void **) &s.res.seq_low_hi, p.max_batch_reads * 8)) != hipSuccess) return bail("hipMalloc", e);
        }
        for (int i = 0; i < Slot::kRing; i++)
            for (int j = 0; j < 3; j++)
                if ((e = hipEventCreate(&s.ev[i][j])) != hipSuccess) return bail("hipEventCreate", e);
    }
    // every stream of the context starts behind the fills (see fill_stream)
    if (int rc = order_behind_fills(ctx)) {
        g_init_error = g_thread_error;
        trew_hip_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return 0;
}

extern "C" void trew_hip_destroy(trew_hip_ctx *ctx) {
    if (!ctx) return;
    (void) hipSetDevice(ctx->p.device);
    for (auto &s : ctx->slots) {
        if (s.stream) (void) hipStreamSynchronize(s.stream);
        if (s.d_buf) (void) hipFree(s.d_buf);
        if (s.d_ascii) (void) hipFree(s.d_ascii);
        if (s.d_thr) (void) hipFree(s.d_thr);
        if (s.h_thr) (void) hipHostFree(s.h_thr);
        if (s.d_wl) (void) hipFree(s.d_wl);
        if (s.d_bnd) (void) hipFree(s.d_bnd);
        if (s.d_live) (void) hipFree(s.d_live);
        if (s.d_wl_count) (void) hipFree(s.d_wl_count);
        if (s.res.k_high) (void) hipFree(s.res.k_high);
        if (s.res.k_low) (void) hipFree(s.res.k_low);
        if (s.res.seq_high) (void) hipFree(s.res.seq_high);
        if (s.res.seq_low) (void) hipFree(s.res.seq_low);
        if (s.res.seq_high_hi) (void) hipFree(s.res.seq_high_hi);
        if (s.res.seq_low_hi) (void) hipFree(s.res.seq_low_hi);
        for (int i = 0; i < Slot::kRing; i++)
            for (int j = 0; j < 3; j++)
                if (s.ev[i][j]) (void) hipEventDestroy(s.ev[i][j]);
        if (s.d_motifs) (void) hipFree(s.d_motifs);
        if (s.h_motifs) (void) hipHostFree(s.h_motifs);
        if (s.d_monomers) (void) hipFree(s.d_monomers);
        if (s.h_monomers) (void) hipHostFree(s.h_monomers);
        for (auto &st : s.measure) {
            for (void *p : {st.records.p, st.counts.p, st.rows.p, st.aligned.p, (void *) st.counter, (void *) st.hist})
                if (p) (void) hipFree(p);
            for (auto e : st.ev)
                if (e) (void) hipEventDestroy(e);
        }
        if (s.ev_tail) (void) hipEventDestroy(s.ev_tail);
        if (s.ev_copied) (void) hipEventDestroy(s.ev_copied);
        if (s.stream) (void) hipStreamDestroy(s.stream);
    }
    if (ctx->copy_stream) (void) hipStreamSynchronize(ctx->copy_stream);
    if (ctx->copy_stream) (void) hipStreamDestroy(ctx->copy_stream);
    if (ctx->ev_filled) (void) hipEventDestroy(ctx->ev_filled);
    if (ctx->table.keys) (void) hipFree(ctx->table.keys);
    if (ctx->table.counts) (void) hipFree(ctx->table.counts);
    if (ctx->table.overflow) (void) hipFree(ctx->table.overflow);
    if (ctx->wide.wtag) (void) hipFree(ctx->wide.wtag);
    if (ctx->wide.wlo) (void) hipFree(ctx->wide.wlo);
    if (ctx->wide.whi) (void) hipFree(ctx->wide.whi);
    if (ctx->wide.wcount) (void) hipFree(ctx->wide.wcount);
    if (ctx->wide.spill_rows) (void) hipFree(ctx->wide.spill_rows);
    if (ctx->table.wide) (void) hipFree((void *) ctx->table.wide);
    if (ctx->g1.log) (void) hipFree(ctx->g1.log);
    if (ctx->g1.counters) (void) hipFree(ctx->g1.counters);
    if (ctx->g1.pair_flags) (void) hipFree(ctx->g1.pair_flags);
    for (auto cb : ctx->g1_carry)
        if (cb) (void) hipFree(cb);
    if (ctx->d_collect_n) (void) hipFree(ctx->d_collect_n);
    if (ctx->d_collect_rows) (void) hipFree(ctx->d_collect_rows);
    if (ctx->d_add_rows) (void) hipFree(ctx->d_add_rows);
    if (ctx->d_row_flags) (void) hipFree(ctx->d_row_flags);
    if (ctx->d_bound_need) (void) hipFree(ctx->d_bound_need);
    if (ctx->ev_producer) (void) hipEventDestroy(ctx->ev_producer);
    delete ctx;
}

// Longest segment any slot of any read of the batch can have, and validation of
// the read-length limits (short mode aborts above MAX_SEQ = 1000, kmer.cpp:1006-1009;
// the build applies the same limit to pair mode).
static int batch_geometry(trew_hip_ctx *ctx, const trew_hip_batch *b, u32 *max_seg, u32 *max_len) {
    const int mode = ctx->p.mode;
    const int MINM = ctx->p.min_mer, MAXM = ctx->p.max_mer, SL = ctx->dp.slice_len;
    u32 maxlen = 0, ms = 0;
    // longest segment of one unit, from the same geometry function the kernels use
    auto unit_seg = [&](u32 n1, u32 n2) {
        u32 m = 0;
        // long mode also walks the interior slices: the middle one carries the remainder (kmer.cpp:790-798)
        if (mode == TREW_MODE_LONG && (int) n1 >= SL) m = (u32) SL + n1 % (u32) SL;
        for (int slot = 0; slot < mode_slots(mode); slot++) {
            const Segment sg = get_segment(mode, slot, n1, n2, MINM, MAXM, SL);
            if (sg.valid) m = std::max(m, sg.len);
        }
        return m;
    };
    if (b->lengths && !b->on_device) {
        // Longest segment over the batch.  It only sizes the kernels (mask words, LDS), so a value that is never
        // too small is what matters; the closed forms below equal unit_seg() except that a whole-read segment is
        // assumed whenever the read is shorter than 4*MAX_MER (get_segment also wants kmin <= kmax).  One pass of
        // a few instructions per read instead of three get_segment() calls: the CLI submits ~10^4 batches a second.
        const u32 two_min = (u32) (2 * MINM), four_min = (u32) (4 * MINM), four_max = (u32) (4 * MAXM);
        if (mode == TREW_MODE_PAIR) {
            for (u64 i = 0; i + 1 < b->n_reads; i += 2) {
                const u32 a = b->lengths[i], c = b->lengths[i + 1], hi = std::max(a, c), lo = std::min(a, c);
                maxlen = std::max(maxlen, hi);
                if (lo >= four_min) ms = std::max(ms, (hi + 1) / 2);
                if (lo >= two_min && lo < four_max) ms = std::max(ms, hi);
            }
        } else if (mode == TREW_MODE_SHORT) {
            for (u64 i = 0; i < b->n_reads; i++) {
                const u32 n = b->lengths[i];
                maxlen = std::max(maxlen, n);
                if (n >= two_min && n < four_max) ms = std::max(ms, n);
            }
            if (maxlen >= four_min) ms = std::max(ms, (maxlen + 1) / 2);
        } else if (mode == TREW_MODE_LONG) {
            for (u64 i = 0; i < b->n_reads; i++) {
                const u32 n = b->lengths[i];
                maxlen = std::max(maxlen, n);
                if ((int) n >= SL) ms = std::max(ms, (u32) SL + n % (u32) SL);  // the middle slice carries the remainder (kmer.cpp:790-798)
            }
        } else {
            for (u64 i = 0; i < b->n_reads; i++) {
                maxlen = std::max(maxlen, b->lengths[i]);
                ms = std::max(ms, unit_seg(b->lengths[i], 0));
            }
        }
    } else if (b->lengths) {
        // device-resident ragged batch: only the caller's max_length hint is known
        maxlen = b->max_length > 0 ? (u32) b->max_length : (u32) kMaxSegBases;
        if (mode == TREW_MODE_SHORT || mode == TREW_MODE_PAIR)
            ms = std::max((maxlen + 1) / 2, std::min<u32>(maxlen, (u32) (4 * MAXM - 1)));
        else if (mode == TREW_MODE_LONG)
            ms = std::min<u32>(maxlen, (u32) (2 * SL - 1));
        else
            ms = maxlen;
    } else {
        maxlen = b->uniform_length;
        ms = unit_seg(maxlen, maxlen);
    }
    // short mode aborts above MAX_SEQ = 1000 (kmer.cpp:1006-1009); the build applies the
    // same limit to pair mode, which the reference leaves unchecked
    if ((mode == TREW_MODE_SHORT || mode == TREW_MODE_PAIR) && maxlen > 1000)
        return fail(ctx, "This mode is designed for short-read sequencing. Please use 'trew long'.");
    if (mode == TREW_MODE_SEGMENT && maxlen > (u32) kMaxSegBases) return fail(ctx, "segment longer than 1023 bases");
    *max_seg = ms;
    *max_len = maxlen;
    return 0;
}

// The host-to-device copies of one batch: queued on the context's copy stream (see trew_hip_ctx::copy_stream), behind whatever
// the slot's stream still has to do with the slot's device buffers and in front of the kernels that follow on it.
struct BatchCopy {
    trew_hip_ctx *ctx;
    Slot &s;
    std::unique_lock<std::mutex> lk;
    BatchCopy(trew_hip_ctx *c, Slot &sl) : ctx(c), s(sl) {}
    int begin() {
        lk = std::unique_lock<std::mutex>(ctx->copy_mu);
        if (hipStreamQuery(s.stream) != hipSuccess) {  // back-to-back submits on one slot: its buffers are still being read
            (void) hipGetLastError();                  // hipErrorNotReady is not an error
            HIPCHK(ctx, hipEventRecord(s.ev_tail, s.stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, s.ev_tail, 0));
        }
        return 0;
    }
    int copy(void *dst, const void *src, u64 bytes) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
        return 0;
    }
    int end() {
        HIPCHK(ctx, hipEventRecord(s.ev_copied, ctx->copy_stream));
        lk.unlock();
        HIPCHK(ctx, hipStreamWaitEvent(s.stream, s.ev_copied, 0));
        return 0;
    }
};

static int stage_batch(trew_hip_ctx *ctx, const trew_hip_batch *b, Slot &s, DevBatch *db) {
    if (b->n_reads > ctx->p.max_batch_reads) return fail(ctx, "batch has more reads than max_batch_reads");
    if (ctx->p.mode == TREW_MODE_PAIR && (b->n_reads & 1)) return fail(ctx, "pair mode needs an even number of reads");
    if (!b->offsets && !b->lengths && b->uniform_stride < 3 * ((b->uniform_length + 31) / 32))
        return fail(ctx, "uniform_stride smaller than the packed read");
    if ((b->offsets == nullptr) != (b->lengths == nullptr)) return fail(ctx, "offsets and lengths must both be given or both be NULL");
    // Index widths of the kernels: worklist entries are u32 unit indices, a read starts at a u32 word offset with explicit
    // offsets and at unit * stride (64-bit arithmetic, get_read) without.  max_batch_reads <= 0xfffffff0 bounds the first for
    // every batch; a uniform batch (device-resident ones included, where no n_words check applies) must also keep the
    // word index of its last read inside what one allocation can hold.
    if (b->n_reads > 0xfffffff0ull) return fail(ctx, "batch has more reads than the kernels' 32-bit unit index holds");
    if (!b->offsets && b->n_reads && (b->n_reads - 1) > (0xffffffffffffffffull / 4ull - 4096ull) / std::max<u64>(1, b->uniform_stride))
        return fail(ctx, "uniform batch: n_reads * uniform_stride overflows the 64-bit word index");
    db->uniform_length = b->uniform_length;
    db->uniform_stride = b->uniform_stride;
    db->n_reads = b->n_reads;
    db->n_units = ctx->p.mode == TREW_MODE_PAIR ? b->n_reads / 2 : b->n_reads;
    if (b->on_device) {
        db->words = b->words;
        db->offsets = b->offsets;
        db->lengths = b->lengths;
    } else {
        if (b->n_words > ctx->p.max_batch_words) return fail(ctx, "batch has more words than max_batch_words");
        if (b->offsets) {
            // the kernels index words[] with these: a read that points outside the batch must never reach the device
            for (u64 i = 0; i < b->n_reads; i++)
                if ((u64) b->offsets[i] + 3ull * (((u64) b->lengths[i] + 31ull) / 32ull) > b->n_words) return fail(ctx, "a read's offset / length points outside the batch's words");
        } else if (b->n_reads && (b->n_reads - 1) * (u64) b->uniform_stride + 3ull * (((u64) b->uniform_length + 31ull) / 32ull) > b->n_words) {
            return fail(ctx, "uniform batch: n_reads * stride exceeds the batch's words");
        }
        // The caller laid the three arrays out back to back in one buffer (see trew_hip.h): ONE copy.  A host that
        // submits thousands of batches a second is bound by HIP API calls, not by bytes.
        BatchCopy bc(ctx, s);
        if (int rc = bc.begin()) return rc;
        if (b->offsets && b->lengths == b->offsets + b->n_reads && b->words == b->lengths + b->n_reads) {  // [offsets][lengths][words]
            if (int rc = bc.copy(s.d_buf, b->offsets, (2 * b->n_reads + b->n_words) * 4)) return rc;
            if (int rc = bc.end()) return rc;
            db->offsets = s.d_buf;
            db->lengths = s.d_buf + b->n_reads;
            db->words = s.d_buf + 2 * b->n_reads;
            return 0;
        }
        if (b->offsets && b->offsets == b->words + b->n_words && b->lengths == b->offsets + b->n_reads) {  // [words][offsets][lengths]
            if (int rc = bc.copy(s.d_buf, b->words, (2 * b->n_reads + b->n_words) * 4)) return rc;
            if (int rc = bc.end()) return rc;
            db->words = s.d_buf;
            db->offsets = s.d_buf + b->n_words;
            db->lengths = s.d_buf + b->n_words + b->n_reads;
            return 0;
        }
        if (int rc = bc.copy(s.d_words, b->words, b->n_words * 4)) return rc;
        db->words = s.d_words;
        db->offsets = nullptr;
        db->lengths = nullptr;
        if (b->offsets) {
            if (int rc = bc.copy(s.d_offsets, b->offsets, b->n_reads * 4)) return rc;
            if (int rc = bc.copy(s.d_lengths, b->lengths, b->n_reads * 4)) return rc;
            db->offsets = s.d_offsets;
            db->lengths = s.d_lengths;
        }
        if (int rc = bc.end()) return rc;
    }
    return 0;
}

// Thresholds of the prefilter's uniform-geometry path for this batch (nullptr: the batch is ragged).  They depend only
// on the read length (and the batch geometry behind them on the context's flags as well), so a slot recomputes and re-sends its
// 9 KB table when the length changes; the copy is queued on
// the slot's stream, in front of the kernel that reads it.
static int stage_thresholds(trew_hip_ctx *ctx, Slot &s, const DevBatch &db, const int2 **out) {
    *out = nullptr;
    if (db.offsets || db.lengths || db.uniform_length == 0) return 0;
    if (s.thr_length != db.uniform_length || s.thr_flags != ctx->dp.flags) {
        HIPCHK(ctx, hipStreamSynchronize(s.stream));  // an earlier copy may still be reading the staging buffer
        fill_thresholds(ctx->dp, db.uniform_length, s.h_thr);
        HIPCHK(ctx, hipMemcpyAsync(s.d_thr, s.h_thr, kThrTableBytes, hipMemcpyHostToDevice, s.stream));
        s.thr_length = db.uniform_length;
        s.thr_flags = ctx->dp.flags;
    }
    *out = s.d_thr;
    return 0;
}

static int sync_all(trew_hip_ctx *ctx);

// the two kernels of one staged batch on the slot's stream (everything trew_hip_submit does after the copy)
static int launch_batch(trew_hip_ctx *ctx, Slot &s, const DevBatch &db, u32 max_seg, u32 max_len) {
    s.n_units = db.n_units;
    if (db.n_units == 0) return 0;
    if (ctx->p.mode == TREW_MODE_SEGMENT) {
        HIPCHK(ctx, hipMemsetAsync(s.res.k_high, 0, db.n_reads * 4, s.stream));
        HIPCHK(ctx, hipMemsetAsync(s.res.k_low, 0, db.n_reads * 4, s.stream));
        HIPCHK(ctx, hipMemsetAsync(s.res.seq_high, 0, db.n_reads * 8, s.stream));
        HIPCHK(ctx, hipMemsetAsync(s.res.seq_low, 0, db.n_reads * 8, s.stream));
        HIPCHK(ctx, hipMemsetAsync(s.res.seq_high_hi, 0, db.n_reads * 8, s.stream));
        HIPCHK(ctx, hipMemsetAsync(s.res.seq_low_hi, 0, db.n_reads * 8, s.stream));
    }
    const u32 wl_cap = (u32) ctx->p.max_batch_reads;
    // Counter block of this launch: clean because the exact kernel of the previous successful launch cleared it (or init did).
    // n_launches only advances once BOTH kernels are queued: if anything below fails, the block may hold a half-built worklist
    // and no exact kernel will clear the other one, so the failing path wipes both before returning (submit_failed).
    u32 *const wl_count = s.d_wl_count + (s.n_launches & 1) * kWlCountWords;
    u32 *const wl_count_next = s.d_wl_count + ((s.n_launches + 1) & 1) * kWlCountWords;  // this launch clears it
    auto submit_failed = [&](int rc) {
        const std::string keep = g_thread_error;  // the clean-up must not replace the text of the failure
        (void) hipMemsetAsync(s.d_wl_count, 0, 2 * kWlCountBytes, s.stream);
        (void) hipStreamSynchronize(s.stream);
        g_thread_error = keep;
        return rc;
    };
#define SUBMIT_CHK(expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            g_thread_error = std::string(#expr) + ": " + hipGetErrorString(e_);               \
            return submit_failed((int) e_);                                                    \
        }                                                                                      \
    } while (0)
    const int2 *d_thr = nullptr;
    if (int rc = stage_thresholds(ctx, s, db, &d_thr)) return submit_failed(rc);
    const bool compat_g1 = (ctx->p.flags & TREW_FLAG_COMPAT_G1) != 0;
    if (compat_g1) SUBMIT_CHK(hipMemsetAsync(ctx->g1.pair_flags, 0, db.n_units, s.stream));
    const bool timed = !(ctx->p.flags & TREW_FLAG_NO_TIMING);
    hipEvent_t *ev = s.ev[s.n_submits % Slot::kRing];
    if (timed) SUBMIT_CHK(hipEventRecord(ev[0], s.stream));
    SUBMIT_CHK(launch_filter(s.stream, (u32) ctx->n_cu, max_seg, ctx->dp, db, s.d_wl, wl_count, wl_cap, nullptr, 0, ctx->table.overflow, d_thr));
    if (timed) SUBMIT_CHK(hipEventRecord(ev[1], s.stream));
    // LDS working set of the exact kernel: the longest segment it may stage (the whole
    // read for k_mer_target / the whole-read check; a slice pair in long mode)
    const u32 exact_seg = ctx->p.mode == TREW_MODE_LONG ? std::min<u32>(max_len, (u32) (2 * ctx->dp.slice_len - 1)) : max_len;
    const u32 cap = std::max<u32>(64u, ((exact_seg + 1 + 63u) / 64u) * 64u);
    const u32 rawwords = ctx->p.mode == TREW_MODE_LONG ? 4u : 3u * ((max_len + 31u) / 32u) + 1u;
    // is the previous submit (on another slot) still running?  Then this batch's kernels will share the chip with it.
    const int me = (int) (&s - ctx->slots.data());
    const int prev = ctx->last_slot.exchange(me, std::memory_order_relaxed);
    bool share = false;
    if (prev >= 0 && prev != me) {
        share = hipStreamQuery(ctx->slots[(size_t) prev].stream) == hipErrorNotReady;
        (void) hipGetLastError();
    }
    // the bounds pass, on the slot's stream between the two kernels (exact_ms of last_timing includes it); no stream of its own
    const bool with_bounds = s.d_bnd != nullptr && bounds_pass_applies(ctx->dp, max_seg);
    if (with_bounds) SUBMIT_CHK(launch_bounds(s.stream, (u32) ctx->n_cu, db.n_units, ctx->dp, db, s.d_wl, wl_count, wl_cap, s.d_bnd, s.bnd_cap, s.d_live, ctx->d_bound_need));
    SUBMIT_CHK(launch_exact(s.stream, (u32) ctx->n_cu, db.n_units, ctx->dp, db, ctx->table_g1, s.d_wl, wl_count, wl_count_next, wl_cap, s.res, cap, rawwords, max_seg, share,
                            with_bounds ? s.d_bnd : nullptr, s.bnd_cap, with_bounds ? s.d_live : nullptr));
    s.live_launch = with_bounds && s.d_live != nullptr;
    ctx->dead_slot.store(s.live_launch ? me : -1, std::memory_order_relaxed);
    if (timed) SUBMIT_CHK(hipEventRecord(ev[2], s.stream));
    if (compat_g1) {  // the stale rows of this batch's pairs (and of the previous batch's tail) are added again, in file order
        SUBMIT_CHK(launch_g1_apply(s.stream, ctx->table, ctx->g1, db, ctx->dp.min_mer, ctx->g1_carry[ctx->g1_batches & 1], ctx->g1_carry[(ctx->g1_batches + 1) & 1],
                                   ctx->g1_carry_cap));
        ctx->g1_batches++;
    }
#undef SUBMIT_CHK
    s.n_launches++;
    s.n_submits++;
    if (ctx->p.flags & TREW_FLAG_TRACK_PRESSURE)  // 64 bytes into pinned memory; trew_hip_table_pressure reads them there
        HIPCHK(ctx, hipMemcpyAsync(s.h_seen, ctx->table.overflow, kDiagWords * 4, hipMemcpyDeviceToHost, s.stream));
    return 0;
}

extern "C" int trew_hip_submit(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot) {
    if (!ctx || !batch) return -1;
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    Slot &s = ctx->slots[(size_t) slot];
    u32 max_seg = 0, max_len = 0;
    if (int rc = batch_geometry(ctx, batch, &max_seg, &max_len)) return rc;
    DevBatch db;
    if (int rc = stage_batch(ctx, batch, s, &db)) return rc;
    return launch_batch(ctx, s, db, max_seg, max_len);
}

// ---- text batches: copy, pack on the device, then the same two kernels
static int stage_ascii(trew_hip_ctx *ctx, const trew_hip_ascii_batch *a, Slot &s, DevBatch *db, u64 *n_words_out) {
    if (!s.d_ascii) return fail(ctx, "the context was created with max_batch_ascii_bytes = 0");
    if (a->n_reads > ctx->p.max_batch_reads) return fail(ctx, "batch has more reads than max_batch_reads");
    if (ctx->p.mode == TREW_MODE_PAIR && (a->n_reads & 1)) return fail(ctx, "pair mode needs an even number of reads");
    const bool ragged = a->word_offsets != nullptr;
    if (ragged != (a->byte_offsets != nullptr) || ragged != (a->lengths != nullptr)) return fail(ctx, "word_offsets, byte_offsets and lengths must all be given or all be NULL");
    u64 n_words = 0;
    if (ragged) {
        // the pack kernel indexes bases[] and words[] with these: validate on the host, as trew_hip_submit does
        u64 w = 0;
        for (u64 i = 0; i < a->n_reads; i++) {
            if (a->word_offsets[i] != w) return fail(ctx, "word_offsets is not the running sum of the packed read sizes");
            if ((u64) a->byte_offsets[i] + a->lengths[i] > a->n_bytes) return fail(ctx, "a read's byte offset / length points outside the batch's bases");
            w += 3ull * (((u64) a->lengths[i] + 31ull) / 32ull);
            if (w > 0xffffffffull) return fail(ctx, "batch packs to more than 2^32 words");
        }
        n_words = w;
        if (a->n_bytes + 12ull * a->n_reads > ctx->p.max_batch_ascii_bytes) return fail(ctx, "text batch larger than max_batch_ascii_bytes");
    } else {
        if (a->uniform_length == 0 && a->n_reads) return fail(ctx, "uniform text batch without uniform_length");
        if (a->n_reads * (u64) a->uniform_length > a->n_bytes) return fail(ctx, "uniform text batch: n_reads * uniform_length exceeds n_bytes");
        if (a->n_bytes > ctx->p.max_batch_ascii_bytes) return fail(ctx, "text batch larger than max_batch_ascii_bytes");
        n_words = a->n_reads * 3ull * (((u64) a->uniform_length + 31ull) / 32ull);
    }
    if (n_words > ctx->p.max_batch_words) return fail(ctx, "batch has more words than max_batch_words");
    *n_words_out = n_words;
    db->n_reads = a->n_reads;
    db->n_units = ctx->p.mode == TREW_MODE_PAIR ? a->n_reads / 2 : a->n_reads;
    db->words = s.d_words;
    if (a->n_reads == 0) return 0;
    const unsigned char *d_bases;
    const u32 *d_wo = nullptr, *d_bo = nullptr, *d_len = nullptr;
    if (ragged) {
        u32 *arr = (u32 *) s.d_ascii;
        d_wo = arr;
        d_bo = arr + a->n_reads;
        d_len = arr + 2 * a->n_reads;
        d_bases = s.d_ascii + 12ull * a->n_reads;
        const bool one = a->byte_offsets == a->word_offsets + a->n_reads && a->lengths == a->byte_offsets + a->n_reads &&
                         (const void *) a->bases == (const void *) (a->lengths + a->n_reads);
        BatchCopy bc(ctx, s);
        if (int rc = bc.begin()) return rc;
        if (one) {  // [word_offsets][byte_offsets][lengths][bases] in one pinned buffer: ONE copy
            if (int rc = bc.copy(s.d_ascii, a->word_offsets, 12ull * a->n_reads + a->n_bytes)) return rc;
        } else {
            if (int rc = bc.copy(arr, a->word_offsets, 4ull * a->n_reads)) return rc;
            if (int rc = bc.copy(arr + a->n_reads, a->byte_offsets, 4ull * a->n_reads)) return rc;
            if (int rc = bc.copy(arr + 2 * a->n_reads, a->lengths, 4ull * a->n_reads)) return rc;
            if (int rc = bc.copy(s.d_ascii + 12ull * a->n_reads, a->bases, a->n_bytes)) return rc;
        }
        if (int rc = bc.end()) return rc;
        db->offsets = d_wo;
        db->lengths = d_len;
        db->uniform_length = 0;
        db->uniform_stride = 0;
    } else {
        d_bases = s.d_ascii;
        BatchCopy bc(ctx, s);
        if (int rc = bc.begin()) return rc;
        if (int rc = bc.copy(s.d_ascii, a->bases, a->n_reads * (u64) a->uniform_length)) return rc;
        if (int rc = bc.end()) return rc;
        db->offsets = nullptr;
        db->lengths = nullptr;
        db->uniform_length = a->uniform_length;
        db->uniform_stride = 3u * ((a->uniform_length + 31u) / 32u);
    }
    HIPCHK(ctx, launch_pack_ascii(s.stream, d_bases, d_bo, d_len, d_wo, a->uniform_length, a->n_reads, n_words / 3ull, s.d_words));
    return 0;
}

static int ascii_geometry(trew_hip_ctx *ctx, const trew_hip_ascii_batch *a, u32 *max_seg, u32 *max_len) {
    trew_hip_batch view;
    memset(&view, 0, sizeof(view));
    view.lengths = a->lengths;
    view.offsets = a->word_offsets;
    view.uniform_length = a->uniform_length;
    view.n_reads = a->n_reads;
    return batch_geometry(ctx, &view, max_seg, max_len);
}

extern "C" int trew_hip_submit_ascii(trew_hip_ctx *ctx, const trew_hip_ascii_batch *batch, int slot) {
    if (!ctx || !batch) return -1;
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    Slot &s = ctx->slots[(size_t) slot];
    u32 max_seg = 0, max_len = 0;
    if (int rc = ascii_geometry(ctx, batch, &max_seg, &max_len)) return rc;
    DevBatch db;
    u64 n_words = 0;
    if (int rc = stage_ascii(ctx, batch, s, &db, &n_words)) return rc;
    return launch_batch(ctx, s, db, max_seg, max_len);
}

extern "C" int trew_hip_pack_ascii(trew_hip_ctx *ctx, const trew_hip_ascii_batch *batch, uint32_t *words, uint64_t words_cap, uint64_t *n_words) {
    if (!ctx || !batch || !n_words) return -1;
    if (int rc = sync_all(ctx)) return rc;
    Slot &s = ctx->slots[0];
    u32 max_seg = 0, max_len = 0;
    if (int rc = ascii_geometry(ctx, batch, &max_seg, &max_len)) return rc;
    DevBatch db;
    if (int rc = stage_ascii(ctx, batch, s, &db, n_words)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s.stream));
    if (words && *n_words && *n_words <= words_cap) HIPCHK(ctx, hipMemcpy(words, s.d_words, *n_words * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int trew_hip_wait(trew_hip_ctx *ctx, int slot) {
    if (!ctx) return -1;
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->slots[(size_t) slot].stream));
    return 0;
}

static int sync_all(trew_hip_ctx *ctx) {
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    for (auto &s : ctx->slots) HIPCHK(ctx, hipStreamSynchronize(s.stream));
    return 0;
}

// reads the device counters; a non-zero "cannot happen" counter is an error, never a silent loss
static int check_diag(trew_hip_ctx *ctx, u32 (&diag)[kDiagWords]) {
    HIPCHK(ctx, hipMemcpy(diag, ctx->table.overflow, sizeof(diag), hipMemcpyDeviceToHost));
    note_seen(ctx, diag);
    if (diag[kDiagOverflow]) return fail(ctx, "device count table and its spill log are full: raise table_log2_slots");
    if (diag[kDiagWorklistDrop]) return fail(ctx, "internal error: the prefilter worklist overflowed (survivors were dropped)");
    if (diag[kDiagIntentDrop]) return fail(ctx, "internal error: a pair logged more than 32 deferred emissions (some were dropped)");
    if (diag[kDiagG1Drop]) return fail(ctx, "TREW_FLAG_COMPAT_G1: the stale-row log of a batch overflowed (submit smaller batches)");
    if (diag[kDiagKernarg]) return fail(ctx, "internal error: the exact kernel's table descriptor differs from its by-value argument (kernarg layout)");
    return 0;
}

static int ensure_rows(trew_hip_ctx *ctx, trew_hip_row **buf, u64 *cap, u64 want) {
    if (want <= *cap) return 0;
    if (*buf) (void) hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    want = std::max<u64>(want + want / 4, 1ull << 16);
    HIPCHK(ctx, hipMalloc((void **) buf, want * sizeof(trew_hip_row)));
    *cap = want;
    return 0;
}

// Compacts the occupied slots of `table` (-1: all) followed by the spill log into d_rows (device memory, capacity
// cap rows) and reports the number of rows there are.  Rows may repeat a key (spilled rows, wide duplicates).
// Caller holds table_mu and has synchronised the slots.
static int compact_to(trew_hip_ctx *ctx, int table, trew_hip_row *d_rows, u64 cap, u64 *n_rows) {
    u32 diag[kDiagWords];
    if (int rc = check_diag(ctx, diag)) return rc;
    u32 n_spill = 0;
    HIPCHK(ctx, hipMemcpy(&n_spill, ctx->wide.spill_n, 4, hipMemcpyDeviceToHost));
    n_spill = std::min(n_spill, ctx->wide.spill_cap);
    if (!ctx->d_collect_n) HIPCHK(ctx, hipMalloc((void **) &ctx->d_collect_n, 8));
    hipStream_t st = ctx->slots[0].stream;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_collect_n, 0, 8, st));
    HIPCHK(ctx, launch_compact(st, ctx->table, ctx->table_slots, ctx->wide.wide_log2_slots, table, d_rows, d_rows ? cap : 0, ctx->d_collect_n));
    unsigned long long n = 0;
    HIPCHK(ctx, hipMemcpyAsync(&n, ctx->d_collect_n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (n_spill) {
        if (table < 0) {  // the log is device-resident: append it as it is
            if (d_rows && n + n_spill <= cap)
                {  // on the stream the compaction ran on, and complete before anyone reads d_rows (callers use other streams)
                    HIPCHK(ctx, hipMemcpyAsync(d_rows + n, ctx->wide.spill_rows, (size_t) n_spill * sizeof(trew_hip_row), hipMemcpyDeviceToDevice, st));
                    HIPCHK(ctx, hipStreamSynchronize(st));
                }
            n += n_spill;
        } else {  // one table only: select on the host (rare path)
            std::vector<trew_hip_row> sp(n_spill);
            HIPCHK(ctx, hipMemcpy(sp.data(), ctx->wide.spill_rows, (size_t) n_spill * sizeof(trew_hip_row), hipMemcpyDeviceToHost));
            for (const auto &r : sp) {
                if (r.table != table) continue;
                if (d_rows && n < cap) HIPCHK(ctx, hipMemcpy(d_rows + n, &r, sizeof(r), hipMemcpyHostToDevice));
                n++;
            }
        }
    }
    *n_rows = n;
    return 0;
}

extern "C" int trew_hip_collect(trew_hip_ctx *ctx, int table, trew_hip_row *rows, uint64_t cap, uint64_t *n_rows) {
    if (!ctx || !n_rows) return -1;
    if (table < -1 || table >= TREW_NUM_TABLES) return fail(ctx, "table out of range");
    std::lock_guard<std::mutex> lk(ctx->table_mu);
    if (int rc = sync_all(ctx)) return rc;
    // compact on the device, copy only the occupied rows (scratch buffers persist across calls)
    const u64 dcap = rows ? cap : 0;
    if (int rc = ensure_rows(ctx, &ctx->d_collect_rows, &ctx->collect_cap, dcap)) return rc;
    u64 n = 0;
    if (int rc = compact_to(ctx, table, dcap ? ctx->d_collect_rows : nullptr, dcap, &n)) return rc;
    if (dcap && n && n <= dcap) {
        HIPCHK(ctx, hipMemcpy(rows, ctx->d_collect_rows, n * sizeof(trew_hip_row), hipMemcpyDeviceToHost));
        // the wide-entry protocol may leave one key in two slots (see table_add_wide), spilled rows repeat
        // keys: counts are sums, merge them
        u32 n_spill = 0;
        HIPCHK(ctx, hipMemcpy(&n_spill, ctx->wide.spill_n, 4, hipMemcpyDeviceToHost));
        bool any_dup = n_spill != 0;
        for (u64 i = 0; i < n && !any_dup; i++) any_dup = rows[i].k > 32;
        if (any_dup) {
            std::sort(rows, rows + n, [](const trew_hip_row &a, const trew_hip_row &b) {
                if (a.table != b.table) return a.table < b.table;
                if (a.k != b.k) return a.k < b.k;
                if (a.word_hi != b.word_hi) return a.word_hi < b.word_hi;
                return a.word_lo < b.word_lo;
            });
            u64 m = 0;
            for (u64 i = 0; i < n; i++) {
                if (m && rows[m - 1].table == rows[i].table && rows[m - 1].k == rows[i].k && rows[m - 1].word_hi == rows[i].word_hi &&
                    rows[m - 1].word_lo == rows[i].word_lo)
                    rows[m - 1].count += rows[i].count;
                else
                    rows[m++] = rows[i];
            }
            // a key whose counts were moved elsewhere (run_long subtracts what it re-files) may sum to zero: not a row
            u64 z = 0;
            for (u64 i = 0; i < m; i++)
                if (rows[i].count) rows[z++] = rows[i];
            n = z;
        }
    }
    *n_rows = n;
    return 0;
}

extern "C" int trew_hip_collect_device(trew_hip_ctx *ctx, trew_hip_row *d_rows, uint64_t cap, uint64_t *n_rows) {
    if (!ctx || !n_rows) return -1;
    std::lock_guard<std::mutex> lk(ctx->table_mu);
    if (int rc = sync_all(ctx)) return rc;
    HIPCHK(ctx, hipDeviceSynchronize());  // the caller's buffer may still be in use on a stream of its own (torch)
    return compact_to(ctx, -1, d_rows, d_rows ? cap : 0, n_rows);
}

extern "C" int trew_hip_collect_slice_device(trew_hip_ctx *ctx, trew_hip_row *d_slice, uint64_t slice_rows, void *consumer_stream, uint64_t *n_rows) {
    if (!ctx || !d_slice) return -1;
    std::lock_guard<std::mutex> lk(ctx->table_mu);
    if (int rc = sync_all(ctx)) return rc;
    hipStream_t st = ctx->slots[0].stream;
    if (consumer_stream) {  // whatever the caller's stream still does with the slice (a previous collective) comes first
        HIPCHK(ctx, hipEventRecord(ctx->ev_producer, (hipStream_t) consumer_stream));
        HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_producer, 0));
    } else {
        HIPCHK(ctx, hipDeviceSynchronize());
    }
    if (!ctx->d_collect_n) HIPCHK(ctx, hipMalloc((void **) &ctx->d_collect_n, 8));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_collect_n, 0, 8, st));
    HIPCHK(ctx, launch_compact(st, ctx->table, ctx->table_slots, ctx->wide.wide_log2_slots, -1, d_slice + 1, slice_rows, ctx->d_collect_n));
    HIPCHK(ctx, launch_slice_finish(st, d_slice, slice_rows, ctx->d_collect_n, ctx->wide.spill_rows, ctx->wide.spill_n, ctx->wide.spill_cap));
    if (consumer_stream) {  // the collective is ordered behind the header on the device: the host is not in the way
        HIPCHK(ctx, hipEventRecord(ctx->ev_producer, st));
        HIPCHK(ctx, hipStreamWaitEvent((hipStream_t) consumer_stream, ctx->ev_producer, 0));
    }
    if (n_rows || !consumer_stream) {
        trew_hip_row h;
        memset(&h, 0, sizeof(h));
        HIPCHK(ctx, hipMemcpyAsync(&h, d_slice, sizeof(h), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (n_rows) *n_rows = h.count;
    }
    return 0;
}

static int reset_locked(trew_hip_ctx *ctx) {
    // the callers have synchronised every slot, so nothing reads or writes the tables; the fills are queued on the fill stream
    // and every stream of the context waits for them on the device (see fill_stream) -- no host wait
    hipStream_t fs = ctx->fill_stream;
    HIPCHK(ctx, hipMemsetAsync(ctx->table.keys, 0, ctx->table_slots * 8, fs));
    HIPCHK(ctx, hipMemsetAsync(ctx->table.counts, 0, ctx->table_slots * 8, fs));
    HIPCHK(ctx, hipMemsetAsync(ctx->table.overflow, 0, kDiagWords * 4, fs));
    const size_t wb = (size_t) 8 << ctx->wide.wide_log2_slots;
    HIPCHK(ctx, hipMemsetAsync(ctx->wide.wtag, 0, wb, fs));
    HIPCHK(ctx, hipMemsetAsync(ctx->wide.wlo, 0, wb, fs));
    HIPCHK(ctx, hipMemsetAsync(ctx->wide.whi, 0, wb, fs));
    HIPCHK(ctx, hipMemsetAsync(ctx->wide.wcount, 0, wb, fs));
    HIPCHK(ctx, fallback_counters_clear(fs));
    if (ctx->g1.counters) HIPCHK(ctx, hipMemsetAsync(ctx->g1.counters, 0, 16, fs));  // a new input: nothing is left in the stale map
    if (int rc = order_behind_fills(ctx)) return rc;
    // the callers have synchronised every slot: no copy into h_seen is in flight
    std::lock_guard<std::mutex> lk(ctx->seen_mu);
    for (auto &sl : ctx->slots) memset(sl.h_seen, 0, kDiagWords * 4);
    for (auto &v : ctx->seen) v.store(0, std::memory_order_relaxed);
    return 0;
}

extern "C" int trew_hip_reset_tables(trew_hip_ctx *ctx) {
    if (!ctx) return -1;
    std::lock_guard<std::mutex> lk(ctx->table_mu);
    if (int rc = sync_all(ctx)) return rc;
    ctx->dead_slot.store(-1, std::memory_order_relaxed);  // trew_hip_debug_counters starts from zero in every slot
    return reset_locked(ctx);
}

extern "C" int trew_hip_table_pressure(trew_hip_ctx *ctx, uint64_t *used_slots, uint64_t *total_slots, uint64_t *spilled_rows,
                                       uint64_t *spill_capacity) {
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    u32 diag[kDiagWords];
    if (ctx->p.flags & TREW_FLAG_TRACK_PRESSURE) {
        // every slot's copy, finished or still being written: the counters only grow between resets and a copy lands a
        // whole word at a time, so any mix of old and new words is a valid (slightly old) reading
        std::lock_guard<std::mutex> lk(ctx->seen_mu);
        for (auto &sl : ctx->slots) {
            u32 copy[kDiagWords];
            for (int i = 0; i < kDiagWords; i++) copy[i] = ((volatile const u32 *) sl.h_seen)[i];
            note_seen(ctx, copy);
        }
        for (int i = 0; i < kDiagWords; i++) diag[i] = ctx->seen[i].load(std::memory_order_relaxed);
    } else {
        // a plain blocking copy: a snapshot of monotonic counters, the slot streams are not waited for (a reset still in flight is)
        HIPCHK(ctx, hipStreamSynchronize(ctx->fill_stream));
        HIPCHK(ctx, hipMemcpy(diag, ctx->table.overflow, sizeof(diag), hipMemcpyDeviceToHost));
    }
    const u32 n_spill = diag[kDiagSpillRows];
    // the narrow and the wide table fill independently: report the fuller one, scaled to the narrow table's size
    const u64 wide_slots = 1ull << ctx->wide.wide_log2_slots;
    const u64 wide_scaled = (u64) ((double) diag[kDiagInsertedWide] / (double) wide_slots * (double) ctx->table_slots);
    if (used_slots) *used_slots = std::max<u64>(diag[kDiagInserted], wide_scaled);
    if (total_slots) *total_slots = ctx->table_slots;
    if (spilled_rows) *spilled_rows = diag[kDiagOverflow] ? (u64) ctx->wide.spill_cap + 1 : n_spill;
    if (spill_capacity) *spill_capacity = ctx->wide.spill_cap;
    return 0;
}

// Adds n_rows device-resident rows on slot 0's stream.  validate: run the device-side check first (rows of unknown origin);
// the add is all or nothing -- with a bad row nothing is added and the call fails, the context stays usable.
static int add_device_rows_locked(trew_hip_ctx *ctx, const trew_hip_row *d_rows, u64 n_rows, bool validate) {
    hipStream_t st = ctx->slots[0].stream;
    if (validate) HIPCHK(ctx, hipMemsetAsync(ctx->d_row_flags, 0, kRowFlagWords * 4, st));
    HIPCHK(ctx, launch_add_rows(st, ctx->table, d_rows, n_rows, validate ? ctx->d_row_flags : nullptr));
    u32 flags[kRowFlagWords] = {0, 0, 0, 0};
    if (validate) HIPCHK(ctx, hipMemcpyAsync(flags, ctx->d_row_flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (flags[kRowFlagBad]) return fail(ctx, "trew_hip_add_rows_device: row out of range (nothing was added)");
    u32 diag[kDiagWords];
    return check_diag(ctx, diag);
}

extern "C" int trew_hip_add_rows(trew_hip_ctx *ctx, const trew_hip_row *rows, uint64_t n_rows) {
    if (!ctx) return -1;
    if (n_rows == 0) return 0;
    for (u64 i = 0; i < n_rows; i++)
        if (rows[i].k < 1 || rows[i].k > 64 || rows[i].table < 0 || rows[i].table >= TREW_NUM_TABLES || (rows[i].k <= 32 && rows[i].word_hi))
            return fail(ctx, "trew_hip_add_rows: row out of range");
    std::lock_guard<std::mutex> lk(ctx->table_mu);
    if (int rc = sync_all(ctx)) return rc;
    if (int rc = ensure_rows(ctx, &ctx->d_add_rows, &ctx->add_cap, n_rows)) return rc;  // persistent scratch: no malloc/free per call
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_add_rows, rows, n_rows * sizeof(trew_hip_row), hipMemcpyHostToDevice, ctx->slots[0].stream));
    return add_device_rows_locked(ctx, ctx->d_add_rows, n_rows, false);  // validated above, on the host
}

extern "C" int trew_hip_add_rows_device(trew_hip_ctx *ctx, const trew_hip_row *d_rows, uint64_t n_rows) {
    if (!ctx) return -1;
    if (n_rows == 0) return 0;
    if (!d_rows) return fail(ctx, "trew_hip_add_rows_device: null rows");
    std::lock_guard<std::mutex> lk(ctx->table_mu);
    if (int rc = sync_all(ctx)) return rc;
    HIPCHK(ctx, hipDeviceSynchronize());  // the rows may have been produced on a stream of the caller's (an RCCL all_gather)
    return add_device_rows_locked(ctx, d_rows, n_rows, true);
}

extern "C" int trew_hip_add_gathered_device(trew_hip_ctx *ctx, const trew_hip_row *d_buf, uint32_t n_slices, uint32_t own_slice,
                                            uint64_t slice_rows, void *producer_stream, uint64_t *max_rows) {
    if (!ctx) return -1;
    if (!d_buf || n_slices == 0 || own_slice >= n_slices) return fail(ctx, "trew_hip_add_gathered_device: bad arguments");
    std::lock_guard<std::mutex> lk(ctx->table_mu);
    if (int rc = sync_all(ctx)) return rc;
    hipStream_t st = ctx->slots[0].stream;
    if (producer_stream) {  // device-side ordering behind the collective: no host synchronisation between the two
        HIPCHK(ctx, hipEventRecord(ctx->ev_producer, (hipStream_t) producer_stream));
        HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_producer, 0));
    } else {
        HIPCHK(ctx, hipDeviceSynchronize());
    }
    HIPCHK(ctx, hipMemsetAsync(ctx->d_row_flags, 0, kRowFlagWords * 4, st));
    HIPCHK(ctx, launch_add_gathered(st, ctx->table, d_buf, n_slices, own_slice, slice_rows, ctx->d_row_flags));
    u32 flags[kRowFlagWords] = {0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(flags, ctx->d_row_flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (max_rows) *max_rows = ((u64) flags[kRowFlagMaxHi] << 32) | flags[kRowFlagMaxLo];
    if (flags[kRowFlagBad]) return fail(ctx, "trew_hip_add_gathered_device: row out of range (nothing was added)");
    if (flags[kRowFlagOverflow]) return 0;  // a slice holds more rows than fit: nothing was added, *max_rows says how many there are
    u32 diag[kDiagWords];
    return check_diag(ctx, diag);
}

extern "C" int trew_hip_debug_worklist(trew_hip_ctx *ctx, int slot, uint32_t *units, uint64_t cap, uint64_t *n) {
    if (!ctx || !n) return -1;
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    Slot &s = ctx->slots[(size_t) slot];
    HIPCHK(ctx, hipStreamSynchronize(s.stream));
    u32 c = 0;
    // the counter block of the last launch keeps its worklist size: the NEXT launch's exact kernel clears it (see exact_kernel)
    if (s.n_launches) HIPCHK(ctx, hipMemcpy(&c, s.d_wl_count + ((s.n_launches - 1) & 1) * kWlCountWords, 4, hipMemcpyDeviceToHost));
    c = (u32) std::min<u64>(c, ctx->p.max_batch_reads);
    *n = c;
    const u64 take = std::min<u64>(c, cap);
    if (units && take) HIPCHK(ctx, hipMemcpy(units, s.d_wl, take * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int trew_hip_debug_live_list(trew_hip_ctx *ctx, int slot, uint32_t *units, uint64_t cap, uint64_t *n) {
    if (!ctx || !n) return -1;
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    Slot &s = ctx->slots[(size_t) slot];
    if (!s.live_launch) return trew_hip_debug_worklist(ctx, slot, units, cap, n);  // the exact kernel read the worklist itself
    HIPCHK(ctx, hipStreamSynchronize(s.stream));
    u32 blk[3] = {0, 0, 0};  // worklist size, stored prefix, dead entries (trew_common.hpp)
    HIPCHK(ctx, hipMemcpy(blk, s.d_wl_count + ((s.n_launches - 1) & 1) * kWlCountWords, sizeof(blk), hipMemcpyDeviceToHost));
    const u64 flagged = std::min<u64>(blk[0], ctx->p.max_batch_reads);
    const u64 pre = std::min<u64>(blk[kStoredPrefixWord], s.bnd_cap), tail = flagged > s.bnd_cap ? flagged - s.bnd_cap : 0;
    *n = pre + tail;
    // the live entries, then the worklist's entries the bounds pass did not look at: what the exact kernel walked, in its order
    const u64 take_pre = std::min<u64>(pre, cap), take_tail = std::min<u64>(tail, cap - take_pre);
    if (units && take_pre) HIPCHK(ctx, hipMemcpy(units, s.d_live, take_pre * 4, hipMemcpyDeviceToHost));
    if (units && take_tail) HIPCHK(ctx, hipMemcpy(units + take_pre, s.d_wl + s.bnd_cap, take_tail * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the compute units the wave-per-read launchers of the per-read measures size their grid by: the device's, or one
// (TREW_FLAG_DEBUG_ONE_CU: every wave of a small batch loops over many reads)
static u32 measure_cu(const trew_hip_ctx *ctx) { return (ctx->p.flags & TREW_FLAG_DEBUG_ONE_CU) ? 1u : (u32) ctx->n_cu; }

extern "C" int trew_hip_debug_measure_grid(trew_hip_ctx *ctx, uint64_t n_reads, uint32_t *blocks) {
    if (!ctx || !blocks) return -1;
    *blocks = wave_per_read_blocks(measure_cu(ctx), n_reads);
    return 0;
}

extern "C" int trew_hip_debug_counters(trew_hip_ctx *ctx, uint64_t *out, int n) {
    if (!ctx || !out || n < 0) return -1;
    if (int rc = sync_all(ctx)) return rc;
    u32 diag[kDiagWords], fb[kFallbackWords];
    HIPCHK(ctx, hipMemcpy(diag, ctx->table.overflow, sizeof(diag), hipMemcpyDeviceToHost));
    HIPCHK(ctx, fallback_counters_read(fb));
    u32 dead = 0;  // of the most recent launch: in the counter block that launch used
    const int ds = ctx->dead_slot.load(std::memory_order_relaxed);
    if (ds >= 0) {
        const Slot &s = ctx->slots[(size_t) ds];
        if (s.n_launches) HIPCHK(ctx, hipMemcpy(&dead, s.d_wl_count + ((s.n_launches - 1) & 1) * kWlCountWords + kDeadEntriesWord, 4, hipMemcpyDeviceToHost));
    }
    const u32 v[TREW_DEBUG_COUNTERS] = {fb[kFallbackStrictRerun], fb[kFallbackWindows], fb[kFallbackWideSpin], diag[kDiagInserted], diag[kDiagInsertedWide], fb[kFallbackGroupPunt], fb[kFallbackGroupRouted], fb[kFallbackGroupTarget], fb[kFallbackHalfDrain], fb[kFallbackUnitDrain], dead};
    for (int i = 0; i < n; i++) out[i] = i < TREW_DEBUG_COUNTERS ? v[i] : 0;
    return 0;
}

extern "C" int trew_hip_merge(trew_hip_ctx *dst, trew_hip_ctx *src) {
    if (!dst || !src) return -1;
    if (dst == src) return fail(dst, "trew_hip_merge: source and destination are the same context");
    // lock order by address: two threads merging in opposite directions cannot deadlock
    std::mutex *m1 = &dst->table_mu, *m2 = &src->table_mu;
    if (m2 < m1) std::swap(m1, m2);
    std::lock_guard<std::mutex> l1(*m1), l2(*m2);
    if (int rc = sync_all(src)) return rc;
    u64 n = 0;
    if (int rc = compact_to(src, -1, nullptr, 0, &n)) return rc;  // size first
    if (n == 0) return 0;
    if (int rc = ensure_rows(src, &src->d_collect_rows, &src->collect_cap, n)) return rc;
    if (int rc = compact_to(src, -1, src->d_collect_rows, src->collect_cap, &n)) return rc;
    if (int rc = sync_all(dst)) return rc;
    if (int rc = ensure_rows(dst, &dst->d_add_rows, &dst->add_cap, n)) return rc;
    // device to device: over xGMI when the contexts sit on two GPUs, a plain copy when they share one
    // (queued on the stream that launches the add kernel, so the kernel is ordered behind the copy by the stream itself;
    // src's rows are complete: compact_to synchronised its stream)
    HIPCHK(dst, hipSetDevice(dst->p.device));
    HIPCHK(dst, hipMemcpyPeerAsync(dst->d_add_rows, dst->p.device, src->d_collect_rows, src->p.device, n * sizeof(trew_hip_row), dst->slots[0].stream));
    return add_device_rows_locked(dst, dst->d_add_rows, n, false);  // rows compacted from a table of this library
}

extern "C" int trew_hip_segment_results(trew_hip_ctx *ctx, int slot, int32_t *k_high, int32_t *k_low,
                                        uint64_t *seq_high, uint64_t *seq_low, uint64_t *seq_high_hi, uint64_t *seq_low_hi,
                                        uint64_t n_reads) {
    if (!ctx) return -1;
    if (ctx->p.mode != TREW_MODE_SEGMENT) return fail(ctx, "segment results exist only in TREW_MODE_SEGMENT");
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    if (int rc = trew_hip_wait(ctx, slot)) return rc;
    Slot &s = ctx->slots[(size_t) slot];
    if (n_reads > s.n_units) return fail(ctx, "n_reads exceeds the last batch");
    if (k_high) HIPCHK(ctx, hipMemcpy(k_high, s.res.k_high, n_reads * 4, hipMemcpyDeviceToHost));
    if (k_low) HIPCHK(ctx, hipMemcpy(k_low, s.res.k_low, n_reads * 4, hipMemcpyDeviceToHost));
    if (seq_high) HIPCHK(ctx, hipMemcpy(seq_high, s.res.seq_high, n_reads * 8, hipMemcpyDeviceToHost));
    if (seq_low) HIPCHK(ctx, hipMemcpy(seq_low, s.res.seq_low, n_reads * 8, hipMemcpyDeviceToHost));
    if (seq_high_hi) HIPCHK(ctx, hipMemcpy(seq_high_hi, s.res.seq_high_hi, n_reads * 8, hipMemcpyDeviceToHost));
    if (seq_low_hi) HIPCHK(ctx, hipMemcpy(seq_low_hi, s.res.seq_low_hi, n_reads * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int trew_hip_filter_masks(trew_hip_ctx *ctx, const trew_hip_batch *batch, uint64_t *cand, int slots_per_read) {
    if (!ctx || !batch || !cand) return -1;
    if (slots_per_read < 1 || slots_per_read > kMaxSlots) return fail(ctx, "slots_per_read out of range");
    if (int rc = sync_all(ctx)) return rc;
    Slot &s = ctx->slots[0];
    u32 max_seg = 0, max_len = 0;
    if (int rc = batch_geometry(ctx, batch, &max_seg, &max_len)) return rc;
    DevBatch db;
    if (int rc = stage_batch(ctx, batch, s, &db)) return rc;
    if (db.n_units == 0) return 0;
    u64 *d = nullptr;
    const u64 bytes = db.n_units * (u64) slots_per_read * 8ull;
    HIPCHK(ctx, hipMalloc((void **) &d, bytes));
    u32 *const wl_count = s.d_wl_count + (s.n_launches & 1) * kWlCountWords;
    const int2 *d_thr = nullptr;
    if (int rc = stage_thresholds(ctx, s, db, &d_thr)) {
        (void) hipFree(d);
        return rc;
    }
    hipError_t e = hipMemsetAsync(d, 0, bytes, s.stream);
    if (e == hipSuccess)
        e = launch_filter(s.stream, (u32) ctx->n_cu, max_seg, ctx->dp, db, s.d_wl, wl_count, (u32) ctx->p.max_batch_reads, d, slots_per_read,
                          ctx->table.overflow, d_thr);
    if (e == hipSuccess) e = hipMemsetAsync(wl_count, 0, kWlCountBytes, s.stream);  // no exact kernel follows: leave the block clean
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    if (e == hipSuccess) e = hipMemcpy(cand, d, bytes, hipMemcpyDeviceToHost);
    (void) hipFree(d);
    HIPCHK(ctx, e);
    return 0;
}

extern "C" int trew_hip_last_timing(trew_hip_ctx *ctx, int slot, float *ms_filter, float *ms_exact, uint64_t *n_flagged) {
    if (!ctx) return -1;
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    if (ctx->p.flags & TREW_FLAG_NO_TIMING) return fail(ctx, "the context was created with TREW_FLAG_NO_TIMING");
    if (int rc = trew_hip_wait(ctx, slot)) return rc;
    Slot &s = ctx->slots[(size_t) slot];
    // mean over the submits since the previous call (at most the last kRing of them)
    u64 first = s.n_reported;
    if (s.n_submits - first > (u64) Slot::kRing) first = s.n_submits - Slot::kRing;
    if (first == s.n_submits) return fail(ctx, "no timed submit on this slot since the last query");
    double sf = 0, se = 0;
    for (u64 i = first; i < s.n_submits; i++) {
        float a = 0, b = 0;
        hipEvent_t *ev = s.ev[i % Slot::kRing];
        HIPCHK(ctx, hipEventElapsedTime(&a, ev[0], ev[1]));
        HIPCHK(ctx, hipEventElapsedTime(&b, ev[1], ev[2]));
        sf += a;
        se += b;
    }
    const double cnt = (double) (s.n_submits - first);
    s.n_reported = s.n_submits;
    if (ms_filter) *ms_filter = (float) (sf / cnt);
    if (ms_exact) *ms_exact = (float) (se / cnt);
    if (n_flagged) {  // optional: costs one blocking 4-byte copy
        u32 c = 0;
        if (s.n_launches) HIPCHK(ctx, hipMemcpy(&c, s.d_wl_count + ((s.n_launches - 1) & 1) * kWlCountWords, 4, hipMemcpyDeviceToHost));
        *n_flagged = c;
    }
    return 0;
}

// ---------------------------------------------------------------- per-read measures: annotate, tracts, intervals, variants, periods, chain, repeats, satellites, align, refine, tandems, trace, decompose, dissect, resolve, monomers, copies, polish
// The eighteen measures share everything on the host side but their kernel and the shape of their results: a queue call stages the
// batch and the motifs and launches one kernel between two events (MeasureState, Slot), a results call waits and copies.
// That shared part exists once: queue_records and results_records for the measures with fixed-size records, queue_log,
// fetch_counted and fetch_log for those with an append log.  An entry point holds what is its measure's own: its argument
// check, what it asks of the helper (record size, capacities) and the launch of its kernel.
// Their definitions on the CPU are in trew_measures_host.cpp; the wrappers here only keep the error text.
extern "C" int trew_motif_parse(const char *text, trew_hip_motif *out) {
    const std::string e = motif_parse(text, out);
    if (!e.empty()) g_thread_error = g_init_error = e;
    return e.empty() ? 0 : -1;
}

// result of a trew_*_host definition -> status; the text goes where trew_hip_last_error finds it with or without a context
static int host_status(const char *e) {
    if (e) g_thread_error = g_init_error = e;
    return e ? -1 : 0;
}

extern "C" int trew_annotate_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                                  const trew_hip_motif *motifs, int n_motifs, trew_hip_annot *out) {
    return host_status(annotate_host(words, offsets, lengths, n_reads, motifs, n_motifs, out));
}

extern "C" int trew_tracts_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                                const trew_hip_motif *motifs, int n_motifs, int penalty, trew_hip_tract *out) {
    return host_status(tracts_host(words, offsets, lengths, n_reads, motifs, n_motifs, penalty, out));
}

extern "C" int trew_intervals_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                                   const trew_hip_motif *motifs, const trew_hip_interval_rule *rules, int n_motifs, trew_hip_interval *out,
                                   uint64_t cap, uint64_t *n, uint32_t *counts) {
    return host_status(intervals_host(words, offsets, lengths, n_reads, motifs, rules, n_motifs, out, cap, n, counts));
}

extern "C" int trew_variants_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                                  const trew_hip_motif *motifs, int n_motifs, trew_hip_variant *out, uint64_t *hist, uint64_t *reads_with) {
    return host_status(variants_host(words, offsets, lengths, n_reads, motifs, n_motifs, out, hist, reads_with));
}

extern "C" int trew_periods_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                 int max_period, int penalty, uint32_t min_score, trew_hip_period *out) {
    return host_status(periods_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, out));
}

extern "C" int trew_chain_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                               int n_motifs, trew_hip_chain_item *out, uint64_t cap, uint64_t *n_items, uint32_t *counts) {
    return host_status(chain_host(words, offsets, lengths, n_reads, motifs, n_motifs, out, cap, n_items, counts));
}

extern "C" int trew_repeats_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                 int max_period, int penalty, uint32_t min_score, trew_hip_repeat *out, uint64_t cap, uint64_t *n, uint32_t *counts) {
    return host_status(repeats_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, out, cap, n, counts));
}

extern "C" int trew_satellites_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                    int max_period, int penalty, uint32_t min_score, trew_hip_satellite *out, uint64_t cap, uint64_t *n,
                                    uint32_t *counts) {
    return host_status(satellites_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, out, cap, n, counts));
}

extern "C" int trew_align_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                               const trew_hip_motif *motifs, int n_motifs, int penalty, trew_hip_alignment *out) {
    return host_status(align_host(words, offsets, lengths, n_reads, motifs, n_motifs, penalty, out));
}

extern "C" int trew_monomer_parse(const char *text, trew_hip_monomer *out) {
    const std::string e = monomer_parse(text, out);
    if (!e.empty()) g_thread_error = g_init_error = e;
    return e.empty() ? 0 : -1;
}

extern "C" int trew_monomers_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                                  const trew_hip_monomer *monomers, int n_monomers, int penalty, trew_hip_alignment *out) {
    return host_status(monomers_host(words, offsets, lengths, n_reads, monomers, n_monomers, penalty, out));
}

extern "C" int trew_copies_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads,
                                const trew_hip_monomer *monomers, int n_monomers, int penalty, uint32_t min_score, trew_hip_trace_item *items,
                                uint64_t cap, uint64_t *n_items, uint64_t *n_rows, uint32_t *counts, trew_hip_alignment *records) {
    return host_status(copies_host(words, offsets, lengths, n_reads, monomers, n_monomers, penalty, min_score, items, cap, n_items, n_rows, counts, records));
}

extern "C" int trew_refine_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                int max_period, int penalty, uint32_t min_score, trew_hip_refined *out) {
    return host_status(refine_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, out));
}

extern "C" int trew_polish_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                int max_period, int penalty, uint32_t min_score, trew_hip_polished *out) {
    return host_status(polish_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, out));
}

extern "C" int trew_tandems_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                 int max_period, int penalty, uint32_t min_score, trew_hip_tandem *out, uint64_t cap, uint64_t *n, uint32_t *counts) {
    return host_status(tandems_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, out, cap, n, counts));
}

extern "C" int trew_trace_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                               int n_motifs, int penalty, uint32_t min_score, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items,
                               uint32_t *counts, trew_hip_alignment *records) {
    return host_status(trace_host(words, offsets, lengths, n_reads, motifs, n_motifs, penalty, min_score, items, cap, n_items, counts, records));
}

extern "C" int trew_decompose_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                   int max_period, int penalty, uint32_t min_score, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items,
                                   uint32_t *counts, trew_hip_refined *records) {
    return host_status(decompose_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, items, cap, n_items, counts, records));
}

extern "C" int trew_dissect_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                 int max_period, int penalty, uint32_t min_score, trew_hip_tandem *records, uint64_t rec_cap,
                                 trew_hip_trace_item *items, uint64_t item_cap, uint64_t *n_records, uint64_t *n_items, uint64_t *n_rows,
                                 uint32_t *counts) {
    return host_status(dissect_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, records, rec_cap, items, item_cap,
                                    n_records, n_items, n_rows, counts));
}

extern "C" int trew_tandems_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                          int max_period, int penalty, uint32_t min_score, int candidates, trew_hip_tandem *out, uint64_t cap,
                                          uint64_t *n, uint32_t *counts) {
    return host_status(tandems_resolved_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, candidates, out, cap, n, counts));
}

extern "C" int trew_decompose_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                            int max_period, int penalty, uint32_t min_score, int candidates, trew_hip_trace_item *items, uint64_t cap,
                                            uint64_t *n_items, uint32_t *counts, trew_hip_refined *records) {
    return host_status(decompose_resolved_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, candidates, items, cap,
                                               n_items, counts, records));
}

extern "C" int trew_dissect_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                          int max_period, int penalty, uint32_t min_score, int candidates, trew_hip_tandem *records, uint64_t rec_cap,
                                          trew_hip_trace_item *items, uint64_t item_cap, uint64_t *n_records, uint64_t *n_items, uint64_t *n_rows,
                                          uint32_t *counts) {
    return host_status(dissect_resolved_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, candidates, records, rec_cap,
                                             items, item_cap, n_records, n_items, n_rows, counts));
}

extern "C" int trew_resolve_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                 int max_period, int penalty, uint32_t min_score, int candidates, trew_hip_resolved *out) {
    return host_status(resolve_host(words, offsets, lengths, n_reads, min_period, max_period, penalty, min_score, candidates, out));
}

// the pattern words of one motif (AnnotMotifDev, trew_common.hpp)
static void fill_motif(const trew_hip_motif &m, AnnotMotifDev *d) {
    memset(d, 0, sizeof(*d));
    d->k = (u32) m.k;
    const u64 target[2] = {m.word, motif_revcomp(m.word, m.k)};
    for (int s = 0; s < 2; s++)
        for (int q = 0; q < m.k; q++) {
            u32 lo = 0, hi = 0;
            for (int i = 0; i < 32; i++) {
                const int j = (i + q) % m.k;  // base j of the target, first base most significant
                const u32 c = (u32) (target[s] >> (2 * (m.k - 1 - j))) & 3u;
                lo |= (c & 1u) << i;
                hi |= (c >> 1) << i;
            }
            d->plo[s][q] = lo;
            d->phi[s][q] = hi;
        }
}

// The pattern tables of a slot, shared by the measures with motifs: created by the first call that needs them (each piece on its
// own, so that a failed call can simply be repeated); they travel on the slot's stream in front of the kernel, and only when
// they changed.
static int stage_motifs(trew_hip_ctx *ctx, Slot &s, const trew_hip_motif *motifs, int n_motifs) {
    if (!s.d_motifs) HIPCHK(ctx, hipMalloc((void **) &s.d_motifs, sizeof(AnnotMotifDev) * kAnnotMaxMotifs));
    if (!s.h_motifs) HIPCHK(ctx, hipHostMalloc((void **) &s.h_motifs, sizeof(AnnotMotifDev) * kAnnotMaxMotifs, hipHostMallocDefault));
    AnnotMotifDev tab[kAnnotMaxMotifs];
    for (int m = 0; m < n_motifs; m++) fill_motif(motifs[m], &tab[m]);
    if (s.motifs_staged < n_motifs || memcmp(tab, s.h_motifs, sizeof(AnnotMotifDev) * (size_t) n_motifs) != 0) {
        HIPCHK(ctx, hipStreamSynchronize(s.stream));  // an earlier copy may still be reading the staging buffer
        memcpy(s.h_motifs, tab, sizeof(AnnotMotifDev) * (size_t) n_motifs);
        HIPCHK(ctx, hipMemcpyAsync(s.d_motifs, s.h_motifs, sizeof(AnnotMotifDev) * (size_t) n_motifs, hipMemcpyHostToDevice, s.stream));
        s.motifs_staged = n_motifs;
    }
    return 0;
}

// What every queue call does before anything of its own: the argument checks in the order callers see them (`own` holds
// the measure's own checks; it runs behind the motifs' check and in front of the first HIP call), the batch and the motifs onto the slot's stream, and the measure's two events on its first use.
// The measures without motifs are known by kMeasureHasMotifs, not by their arguments: for them there is no motif check
// and no pattern table, and they pass no motifs.  For the others, no motifs stays the argument error it always was.
template <class Own>
static int measure_begin(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, Measure which,
                         Own own, Slot **slot_out, DevBatch *db) {
    if (!ctx || !batch) return -1;
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    if (kMeasureHasMotifs[which])
        if (const char *e = motifs_error(motifs, n_motifs)) return fail(ctx, e);
    if (const char *e = own()) return fail(ctx, e);
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    Slot &s = ctx->slots[(size_t) slot];
    if (int rc = stage_batch(ctx, batch, s, db)) return rc;  // also: the read index fits a record's u32
    if (kMeasureHasMotifs[which])
        if (int rc = stage_motifs(ctx, s, motifs, n_motifs)) return rc;
    for (auto &e : s.measure[which].ev)
        if (!e) HIPCHK(ctx, hipEventCreate(&e));
    *slot_out = &s;
    return 0;
}
static const char *no_own_checks() { return nullptr; }
static int no_setup(Slot &, MeasureState &) { return 0; }

// A device buffer that only grows.  The fields are zeroed between free and malloc, so that a call that fails here can
// simply be repeated.
static int grow(trew_hip_ctx *ctx, Slot &s, DevBuf &b, u64 want) {
    if (want <= b.bytes) return 0;
    HIPCHK(ctx, hipStreamSynchronize(s.stream));  // nothing may still be writing the old buffer
    if (b.p) HIPCHK(ctx, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    HIPCHK(ctx, hipMalloc(&b.p, want));
    b.bytes = want;
    return 0;
}

// the measure's kernel between its two events; `launch` returns a status and sets the error text like every other step
template <class Launch>
static int timed_launch(trew_hip_ctx *ctx, Slot &s, MeasureState &st, Launch launch) {
    HIPCHK(ctx, hipEventRecord(st.ev[0], s.stream));
    if (int rc = launch()) return rc;
    HIPCHK(ctx, hipEventRecord(st.ev[1], s.stream));
    st.timed = true;
    return 0;
}

// The queue call of the measures with one fixed-size record per (read, motif) or per read (annotate, tracts, align, periods,
// refine, resolve, variants; per_read: n_motifs or 1): measure_begin, room for the records, `setup` (what else the measure keeps on the
// device: the histograms of variants), then the numbers of the call, all in one place, and `launch` between the events unless
// the batch is empty.  Every call starts from zero, and one that fails on the way can simply be repeated.
template <class Own, class Setup, class Launch>
static int queue_records(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, Measure which,
                         int per_read, size_t rec_bytes, Own own, Setup setup, Launch launch) {
    Slot *sp = nullptr;
    DevBatch db;
    if (int rc = measure_begin(ctx, batch, slot, motifs, n_motifs, which, own, &sp, &db)) return rc;
    Slot &s = *sp;
    MeasureState &st = s.measure[which];
    const u64 need = db.n_reads * (u64) per_read;
    if (int rc = grow(ctx, s, st.records, need * rec_bytes)) return rc;
    if (int rc = setup(s, st)) return rc;
    st.valid = true;
    st.timed = false;
    st.n = need;
    if (need == 0) return 0;
    return timed_launch(ctx, s, st, [&]() -> int { return launch(s, st, db); });
}

// What a measure with an append log asks of queue_log besides its kernel.
struct LogShape {
    size_t rec_bytes;        // of one record of the log (chain: one event)
    u64 max_log;             // the capacity of the log for this call
    u64 counts_per_read;     // u32 counts: n_motifs * 2 (intervals, trace), n_motifs * 4 (chain), 1 (repeats, satellites, tandems)
    bool zero_counts;        // the kernel adds to its counts (repeats, satellites, tandems); the others store every one of them
    u64 max_rows;            // trace, decompose: the rows of the direction workspace for this call, and a second counter for them; else 0
    u64 aligned_per_read;    // trace: n_motifs alignment records; decompose: one refined record; else 0
    size_t row_bytes;        // trace: 64, decompose: 32, copies: 64 Q (the call's phases a lane); else 0
    size_t aligned_bytes;    // of one of the records beside the log; else 0
    u64 max_tracts;          // dissect: the capacity of its second log, the records kept in `aligned`, and a third counter for them; else 0
};

// The queue call of the measures with an append log (intervals, chain, repeats, satellites, tandems, trace, decompose, dissect, copies): measure_begin, the
// counter (one word, trace and decompose two, dissect three: a fixed size, allocated on first use), room for the counts, the log and trace's two buffers,
// then the numbers of the call, all in one place, the counter back to zero -- every call starts from zero, also one without
// reads, whose results then report nothing found -- and `launch` between the events unless the batch is empty.  `setup`: what
// else the measure keeps on the device (the monomers of copies), as in queue_records.
template <class Own, class Setup, class Launch>
static int queue_log(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, Measure which,
                     const LogShape &shape, Own own, Setup setup, Launch launch) {
    Slot *sp = nullptr;
    DevBatch db;
    if (int rc = measure_begin(ctx, batch, slot, motifs, n_motifs, which, own, &sp, &db)) return rc;
    Slot &s = *sp;
    MeasureState &st = s.measure[which];
    const size_t counter_bytes = (shape.max_tracts ? 3 : shape.max_rows ? 2 : 1) * sizeof(unsigned long long);
    const u64 n_counts = db.n_reads * shape.counts_per_read, n_aligned = shape.max_tracts ? shape.max_tracts : db.n_reads * shape.aligned_per_read;
    if (!st.counter) HIPCHK(ctx, hipMalloc((void **) &st.counter, counter_bytes));
    if (int rc = grow(ctx, s, st.aligned, n_aligned * shape.aligned_bytes)) return rc;
    if (int rc = grow(ctx, s, st.counts, n_counts * sizeof(u32))) return rc;
    if (int rc = grow(ctx, s, st.records, shape.max_log * shape.rec_bytes)) return rc;
    if (int rc = grow(ctx, s, st.rows, shape.max_rows * shape.row_bytes)) return rc;
    if (int rc = setup(s, st)) return rc;
    st.valid = true;
    st.timed = false;
    st.n = n_aligned;
    st.n_counts = n_counts;
    st.max_log = shape.max_log;  // this call's capacity, not the (possibly larger) buffer's: the overflow contract is per call
    st.max_rows = shape.max_rows;
    HIPCHK(ctx, hipMemsetAsync(st.counter, 0, counter_bytes, s.stream));
    if (n_counts == 0) return 0;
    if (shape.zero_counts) HIPCHK(ctx, hipMemsetAsync(st.counts.p, 0, n_counts * sizeof(u32), s.stream));
    return timed_launch(ctx, s, st, [&]() -> int { return launch(s, st, db); });
}

// What every results call does first: the checks (`arg_error`: the text of the measure's own argument check, which comes
// behind the slot's), then the wait for the slot's stream.
static int fetch_begin(trew_hip_ctx *ctx, int slot, Measure which, const char *arg_error, Slot **slot_out) {
    if (!ctx) return -1;
    if (slot < 0 || slot >= (int) ctx->slots.size()) return fail(ctx, "slot out of range");
    if (arg_error) return fail(ctx, arg_error);
    Slot &s = ctx->slots[(size_t) slot];
    if (!s.measure[which].valid) return fail(ctx, std::string("no trew_hip_") + kMeasureName[which] + " on this slot yet");
    *slot_out = &s;
    return trew_hip_wait(ctx, slot);
}

// the fixed-size records of a measure: min(n, cap) of them; without `out` none (no error)
static int fetch_records(trew_hip_ctx *ctx, const MeasureState &st, void *out, u64 cap, size_t rec_bytes, uint64_t *n) {
    if (n) *n = st.n;
    const u64 take = std::min<u64>(st.n, cap);
    if (out && take) HIPCHK(ctx, hipMemcpy(out, st.records.p, take * rec_bytes, hipMemcpyDeviceToHost));
    return 0;
}

static int fetch_end(trew_hip_ctx *ctx, const MeasureState &st, float *ms_kernel) {
    if (ms_kernel) {
        *ms_kernel = 0.0f;
        if (st.timed) HIPCHK(ctx, hipEventElapsedTime(ms_kernel, st.ev[0], st.ev[1]));
    }
    return 0;
}

// the results call of annotate, tracts, align, periods, refine and resolve, whole
static int results_records(trew_hip_ctx *ctx, int slot, Measure which, void *out, u64 cap, size_t rec_bytes, uint64_t *n, float *ms_kernel) {
    Slot *sp = nullptr;
    if (int rc = fetch_begin(ctx, slot, which, nullptr, &sp)) return rc;
    const MeasureState &st = sp->measure[which];
    if (int rc = fetch_records(ctx, st, out, cap, rec_bytes, n)) return rc;
    return fetch_end(ctx, st, ms_kernel);
}

// what the kernel of a log measure counted: `words` counter values (trace: two), and the counts where the caller wants them
static int fetch_counted(trew_hip_ctx *ctx, const MeasureState &st, unsigned long long *found, int words, uint32_t *counts) {
    HIPCHK(ctx, hipMemcpy(found, st.counter, (size_t) words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (counts && st.n_counts) HIPCHK(ctx, hipMemcpy(counts, st.counts.p, st.n_counts * sizeof(u32), hipMemcpyDeviceToHost));
    return 0;
}

// an overflowed log holds an unspecified subset: nothing of it is copied (only intervals, whose records stand each for itself,
// hands out what its log holds)
static u64 whole_log(const MeasureState &st, u64 found) { return found <= st.max_log ? found : 0; }

// min(cap, n_in_log) records of the log, the first ones in the order of `sort`: sorted on the host, so the records do not depend
// on the order in which the waves appended them.  A buffer smaller than the log gets the first `cap` of the sorted log.
template <class Rec>
static int fetch_log(trew_hip_ctx *ctx, const MeasureState &st, Rec *out, u64 cap, u64 n_in_log, void (*sort)(Rec *, uint64_t)) {
    const u64 take = std::min<u64>(n_in_log, cap);
    if (!take) return 0;
    if (take == n_in_log) {
        HIPCHK(ctx, hipMemcpy(out, st.records.p, take * sizeof(Rec), hipMemcpyDeviceToHost));
        sort(out, take);
    } else {
        std::vector<Rec> all((size_t) n_in_log);
        HIPCHK(ctx, hipMemcpy(all.data(), st.records.p, n_in_log * sizeof(Rec), hipMemcpyDeviceToHost));
        sort(all.data(), n_in_log);
        memcpy(out, all.data(), take * sizeof(Rec));
    }
    return 0;
}

// ---------------------------------------------------------------- per-read annotation against given motifs
extern "C" int trew_hip_annotate(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs) {
    if (!ctx || !batch) return -1;
    // the longest read picks the kernel; none of the scan's read-length rules applies (no batch_geometry)
    u32 max_len = 0;
    bool general = (ctx->p.flags & TREW_FLAG_DEBUG_ANNOT_GENERAL) != 0;
    if (!batch->lengths) {
        max_len = batch->uniform_length;
    } else if (!batch->on_device) {
        for (u64 i = 0; i < batch->n_reads; i++) max_len = std::max(max_len, batch->lengths[i]);
    } else if (batch->max_length > 0) {
        max_len = (u32) batch->max_length;
    } else {
        general = true;  // unknown
    }
    return queue_records(ctx, batch, slot, motifs, n_motifs, kAnnotate, n_motifs, sizeof(trew_hip_annot), no_own_checks, no_setup,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             HIPCHK(ctx, launch_annotate(s.stream, measure_cu(ctx), db, s.d_motifs, n_motifs, max_len, general, (trew_hip_annot *) st.records.p));
                             return 0;
                         });
}

extern "C" int trew_hip_annotate_results(trew_hip_ctx *ctx, int slot, trew_hip_annot *out, uint64_t cap, uint64_t *n, float *ms_kernel) {
    return results_records(ctx, slot, kAnnotate, out, cap, sizeof(trew_hip_annot), n, ms_kernel);
}

// ---------------------------------------------------------------- per-read error-tolerant terminal tracts
extern "C" int trew_hip_tracts(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, int penalty) {
    auto own = [&]() -> const char * { return penalty < 1 || penalty > 64 ? "penalty must be in [1, 64]" : nullptr; };
    return queue_records(ctx, batch, slot, motifs, n_motifs, kTracts, n_motifs, sizeof(trew_hip_tract), own, no_setup,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             HIPCHK(ctx, launch_tracts(s.stream, measure_cu(ctx), db, s.d_motifs, n_motifs, penalty, (trew_hip_tract *) st.records.p));
                             return 0;
                         });
}

extern "C" int trew_hip_tracts_results(trew_hip_ctx *ctx, int slot, trew_hip_tract *out, uint64_t cap, uint64_t *n, float *ms_kernel) {
    return results_records(ctx, slot, kTracts, out, cap, sizeof(trew_hip_tract), n, ms_kernel);
}

// ---------------------------------------------------------------- indel-aware motif tract per read (wraparound alignment)
extern "C" int trew_hip_align(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, int penalty) {
    auto own = [&]() -> const char * { return penalty < 1 || penalty > 64 ? "penalty must be in [1, 64]" : nullptr; };
    return queue_records(ctx, batch, slot, motifs, n_motifs, kAlign, n_motifs, sizeof(trew_hip_alignment), own, no_setup,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             HIPCHK(ctx, launch_align(s.stream, measure_cu(ctx), db, s.d_motifs, n_motifs, penalty, (trew_hip_alignment *) st.records.p));
                             return 0;
                         });
}

extern "C" int trew_hip_align_results(trew_hip_ctx *ctx, int slot, trew_hip_alignment *out, uint64_t cap, uint64_t *n, float *ms_kernel) {
    return results_records(ctx, slot, kAlign, out, cap, sizeof(trew_hip_alignment), n, ms_kernel);
}

// ---------------------------------------------------------------- wraparound alignment for units of up to 256 bases
// The (k, unit[16]) entries of a slot, beside the pattern tables and staged as they are (stage_motifs): created by the first
// call, on the slot's stream in front of the kernel, and only when they changed.
static int stage_monomers(trew_hip_ctx *ctx, Slot &s, const trew_hip_monomer *monomers, int n_monomers) {
    const size_t bytes = sizeof(trew_hip_monomer) * (size_t) n_monomers;
    if (!s.d_monomers) HIPCHK(ctx, hipMalloc((void **) &s.d_monomers, sizeof(trew_hip_monomer) * TREW_MONOMERS_MAX));
    if (!s.h_monomers) HIPCHK(ctx, hipHostMalloc((void **) &s.h_monomers, sizeof(trew_hip_monomer) * TREW_MONOMERS_MAX, hipHostMallocDefault));
    trew_hip_monomer tab[TREW_MONOMERS_MAX];
    for (int m = 0; m < n_monomers; m++) {
        tab[m] = monomers[m];
        tab[m].reserved = 0;
    }
    if (s.monomers_staged < n_monomers || memcmp(tab, s.h_monomers, bytes) != 0) {
        HIPCHK(ctx, hipStreamSynchronize(s.stream));  // an earlier copy may still be reading the staging buffer
        memcpy(s.h_monomers, tab, bytes);
        HIPCHK(ctx, hipMemcpyAsync(s.d_monomers, s.h_monomers, bytes, hipMemcpyHostToDevice, s.stream));
        s.monomers_staged = n_monomers;
    }
    return 0;
}

// Enters through the motif-less path of measure_begin: the monomers' check is one of the measure's own.
extern "C" int trew_hip_monomers(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_monomer *monomers, int n_monomers, int penalty) {
    auto own = [&]() -> const char * {
        if (const char *e = monomers_error(monomers, n_monomers)) return e;
        return penalty < 1 || penalty > 64 ? "penalty must be in [1, 64]" : nullptr;
    };
    auto setup = [&](Slot &s, MeasureState &) -> int { return stage_monomers(ctx, s, monomers, n_monomers); };
    return queue_records(ctx, batch, slot, nullptr, 0, kMonomers, n_monomers > 0 ? n_monomers : 0, sizeof(trew_hip_alignment), own, setup,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             u32 max_k = 0;
                             for (int m = 0; m < n_monomers; m++) max_k = std::max(max_k, (u32) monomers[m].k);
                             HIPCHK(ctx, launch_monomers(s.stream, measure_cu(ctx), db, s.d_monomers, n_monomers, max_k, penalty, (trew_hip_alignment *) st.records.p));
                             return 0;
                         });
}

extern "C" int trew_hip_monomers_results(trew_hip_ctx *ctx, int slot, trew_hip_alignment *out, uint64_t cap, uint64_t *n, float *ms_kernel) {
    return results_records(ctx, slot, kMonomers, out, cap, sizeof(trew_hip_alignment), n, ms_kernel);
}

// ---------------------------------------------------------------- units in place under indels: the traceback of the alignment
// `records` is the item log, `counter` two values (items, rows), `aligned` the trew_hip_alignment of every (read, motif).
static_assert(sizeof(trew_hip_trace_item) == 48, "twelve words: what trace_wave_kernel stores");
extern "C" int trew_hip_trace(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, int penalty,
                              uint32_t min_score, uint64_t max_items, uint64_t max_rows) {
    auto own = [&]() -> const char * {
        return penalty < 1 || penalty > 64 ? "penalty must be in [1, 64]"
               : min_score < 1             ? "min_score must be at least 1"
               : max_items < 1             ? "max_items must be at least 1"
               : max_rows < 1              ? "max_rows must be at least 1"
                                           : nullptr;
    };
    const LogShape shape = {sizeof(trew_hip_trace_item), max_items, (u64) n_motifs * 2ull, false, max_rows, (u64) n_motifs, 64, sizeof(trew_hip_alignment)};
    return queue_log(ctx, batch, slot, motifs, n_motifs, kTrace, shape, own, no_setup, [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
        const TraceLog lg = {st.counter, (u32 *) st.records.p, st.max_log, st.counter + 1, (unsigned char *) st.rows.p, st.max_rows};
        HIPCHK(ctx, launch_trace(s.stream, measure_cu(ctx), db, s.d_motifs, n_motifs, penalty, min_score, lg, (trew_hip_alignment *) st.aligned.p,
                                 (u32 *) st.counts.p));
        return 0;
    });
}

// the results call of trace and copies, whole; null_error, items_error: the texts of the two argument checks
static int results_traced(trew_hip_ctx *ctx, int slot, Measure which, const char *null_error, const char *items_error, trew_hip_trace_item *items,
                          uint64_t cap, uint64_t *n_items, uint64_t *n_rows, uint32_t *counts, trew_hip_alignment *records, float *ms_kernel) {
    const char *arg_error = !n_items || !n_rows ? null_error : cap && !items ? items_error : nullptr;
    Slot *sp = nullptr;
    if (int rc = fetch_begin(ctx, slot, which, arg_error, &sp)) return rc;
    const MeasureState &st = sp->measure[which];
    unsigned long long found[2] = {0, 0};
    if (int rc = fetch_counted(ctx, st, found, 2, counts)) return rc;
    *n_items = found[0];
    *n_rows = found[1];
    if (records && st.n) HIPCHK(ctx, hipMemcpy(records, st.aligned.p, st.n * sizeof(trew_hip_alignment), hipMemcpyDeviceToHost));
    // a workspace that overflowed did not stop the walk, but the contract is one: both fit, or no items
    if (int rc = fetch_log(ctx, st, items, cap, found[1] <= st.max_rows ? whole_log(st, found[0]) : 0, sort_trace_items)) return rc;
    return fetch_end(ctx, st, ms_kernel);
}

extern "C" int trew_hip_trace_results(trew_hip_ctx *ctx, int slot, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint64_t *n_rows,
                                      uint32_t *counts, trew_hip_alignment *records, float *ms_kernel) {
    return results_traced(ctx, slot, kTrace, "trew_hip_trace_results: n_items and n_rows must not be null", "trew_hip_trace_results: items must not be null",
                          items, cap, n_items, n_rows, counts, records, ms_kernel);
}

// ---------------------------------------------------------------- copies in place for units of up to 256 bases: the traceback of monomers' alignment
// As trace: `records` is the item log, `counter` two values (items, rows), `aligned` the trew_hip_alignment of every (read,
// monomer), `counts` one u32 per (read, monomer, strand); `rows` 64 Q bytes a row, Q the phases a lane holds in this call (the
// largest k picks it, as in launch_monomers).  Enters through the motif-less path as monomers does; the staged table is the slot's.
extern "C" int trew_hip_copies(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_monomer *monomers, int n_monomers, int penalty,
                               uint32_t min_score, uint64_t max_items, uint64_t max_rows) {
    auto own = [&]() -> const char * {
        if (const char *e = monomers_error(monomers, n_monomers)) return e;
        return penalty < 1 || penalty > 64 ? "penalty must be in [1, 64]"
               : min_score < 1             ? "min_score must be at least 1"
               : max_items < 1             ? "max_items must be at least 1"
               : max_rows < 1              ? "max_rows must be at least 1"
                                           : nullptr;
    };
    u32 max_k = 0;
    for (int m = 0; monomers && m < n_monomers && m < TREW_MONOMERS_MAX; m++) max_k = std::max(max_k, (u32) monomers[m].k);
    const size_t row_bytes = max_k <= 64u ? 64 : max_k <= 128u ? 128 : 256;
    const u64 per_read = n_monomers > 0 ? (u64) n_monomers : 0;
    const LogShape shape = {sizeof(trew_hip_trace_item), max_items, per_read * 2ull, false, max_rows, per_read, row_bytes, sizeof(trew_hip_alignment)};
    auto setup = [&](Slot &s, MeasureState &) -> int { return stage_monomers(ctx, s, monomers, n_monomers); };
    return queue_log(ctx, batch, slot, nullptr, 0, kCopies, shape, own, setup, [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
        const TraceLog lg = {st.counter, (u32 *) st.records.p, st.max_log, st.counter + 1, (unsigned char *) st.rows.p, st.max_rows};
        HIPCHK(ctx, launch_copies(s.stream, measure_cu(ctx), db, s.d_monomers, n_monomers, max_k, penalty, min_score, lg, (trew_hip_alignment *) st.aligned.p,
                                  (u32 *) st.counts.p));
        return 0;
    });
}

extern "C" int trew_hip_copies_results(trew_hip_ctx *ctx, int slot, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint64_t *n_rows,
                                       uint32_t *counts, trew_hip_alignment *records, float *ms_kernel) {
    return results_traced(ctx, slot, kCopies, "trew_hip_copies_results: n_items and n_rows must not be null",
                          "trew_hip_copies_results: items must not be null", items, cap, n_items, n_rows, counts, records, ms_kernel);
}

// ---------------------------------------------------------------- units in place with no motif given: refine's unit, anchored, traced
// As trace: `records` is the item log, `counter` two values (items, rows); `counts` one u32 per read, `aligned` the
// trew_hip_refined of every read (its reserved word the anchor), `rows` 32 bytes a row.
// candidates 0: trew_hip_decompose and its kernel; otherwise trew_hip_decompose_resolved (the sibling's checks, then resolve_error's)
static int queue_decompose(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                           bool resolved, int candidates, uint64_t max_items, uint64_t max_rows) {
    auto own = [&]() -> const char * {
        if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
        if (const char *e = max_items < 1 ? "max_items must be at least 1" : max_rows < 1 ? "max_rows must be at least 1" : nullptr) return e;
        return resolved ? resolve_error(min_period, max_period, penalty, min_score, candidates) : nullptr;
    };
    const LogShape shape = {sizeof(trew_hip_trace_item), max_items, 1, false, max_rows, 1, 32, sizeof(trew_hip_refined)};
    return queue_log(ctx, batch, slot, nullptr, 0, kDecompose, shape, own, no_setup, [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
        const TraceLog lg = {st.counter, (u32 *) st.records.p, st.max_log, st.counter + 1, (unsigned char *) st.rows.p, st.max_rows};
        if (resolved)
            HIPCHK(ctx, launch_decompose_resolved(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, candidates, lg,
                                                  (trew_hip_refined *) st.aligned.p, (u32 *) st.counts.p));
        else
            HIPCHK(ctx, launch_decompose(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, lg, (trew_hip_refined *) st.aligned.p,
                                         (u32 *) st.counts.p));
        return 0;
    });
}

extern "C" int trew_hip_decompose(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty,
                                  uint32_t min_score, uint64_t max_items, uint64_t max_rows) {
    return queue_decompose(ctx, batch, slot, min_period, max_period, penalty, min_score, false, 0, max_items, max_rows);
}

extern "C" int trew_hip_decompose_resolved(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty,
                                           uint32_t min_score, int candidates, uint64_t max_items, uint64_t max_rows) {
    return queue_decompose(ctx, batch, slot, min_period, max_period, penalty, min_score, true, candidates, max_items, max_rows);
}

extern "C" int trew_hip_decompose_results(trew_hip_ctx *ctx, int slot, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint64_t *n_rows,
                                          uint32_t *counts, trew_hip_refined *records, float *ms_kernel) {
    const char *arg_error = !n_items || !n_rows ? "trew_hip_decompose_results: n_items and n_rows must not be null"
                            : cap && !items     ? "trew_hip_decompose_results: items must not be null"
                                                : nullptr;
    Slot *sp = nullptr;
    if (int rc = fetch_begin(ctx, slot, kDecompose, arg_error, &sp)) return rc;
    const MeasureState &st = sp->measure[kDecompose];
    unsigned long long found[2] = {0, 0};
    if (int rc = fetch_counted(ctx, st, found, 2, counts)) return rc;
    *n_items = found[0];
    *n_rows = found[1];
    if (records && st.n) HIPCHK(ctx, hipMemcpy(records, st.aligned.p, st.n * sizeof(trew_hip_refined), hipMemcpyDeviceToHost));
    // trace's contract: both fit, or no items
    if (int rc = fetch_log(ctx, st, items, cap, found[1] <= st.max_rows ? whole_log(st, found[0]) : 0, sort_trace_items)) return rc;
    return fetch_end(ctx, st, ms_kernel);
}

// ---------------------------------------------------------------- units in place for every tract of a read, no motif given
// As decompose: `records` is the item log, `rows` 32 bytes a row; `aligned` is the log of trew_hip_tandem records (reserved: the
// anchor), `counter` three values (items, rows, records), `counts` two u32 per read (tracts, items).
static int queue_dissect(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                         bool resolved, int candidates, uint64_t max_records, uint64_t max_items, uint64_t max_rows) {
    auto own = [&]() -> const char * {
        if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
        if (const char *e = max_records < 1 ? "max_records must be at least 1"
                            : max_items < 1 ? "max_items must be at least 1"
                            : max_rows < 1  ? "max_rows must be at least 1"
                                            : nullptr)
            return e;
        return resolved ? resolve_error(min_period, max_period, penalty, min_score, candidates) : nullptr;
    };
    const LogShape shape = {sizeof(trew_hip_trace_item), max_items, 2, false, max_rows, 0, 32, sizeof(trew_hip_tandem), max_records};
    return queue_log(ctx, batch, slot, nullptr, 0, kDissect, shape, own, no_setup, [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
        const TraceLog lg = {st.counter, (u32 *) st.records.p, st.max_log, st.counter + 1, (unsigned char *) st.rows.p, st.max_rows};
        const RepeatLog rl = {st.counter + 2, (u32 *) st.aligned.p, st.n};
        if (resolved)
            HIPCHK(ctx, launch_dissect_resolved(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, candidates, rl, lg,
                                                (u32 *) st.counts.p));
        else
            HIPCHK(ctx, launch_dissect(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, rl, lg, (u32 *) st.counts.p));
        return 0;
    });
}

extern "C" int trew_hip_dissect(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                                uint64_t max_records, uint64_t max_items, uint64_t max_rows) {
    return queue_dissect(ctx, batch, slot, min_period, max_period, penalty, min_score, false, 0, max_records, max_items, max_rows);
}

extern "C" int trew_hip_dissect_resolved(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty,
                                         uint32_t min_score, int candidates, uint64_t max_records, uint64_t max_items, uint64_t max_rows) {
    return queue_dissect(ctx, batch, slot, min_period, max_period, penalty, min_score, true, candidates, max_records, max_items, max_rows);
}

extern "C" int trew_hip_dissect_results(trew_hip_ctx *ctx, int slot, trew_hip_tandem *records, uint64_t rec_cap, trew_hip_trace_item *items,
                                        uint64_t item_cap, uint64_t *n_records, uint64_t *n_items, uint64_t *n_rows, uint32_t *counts,
                                        float *ms_kernel) {
    const char *arg_error = !n_records || !n_items || !n_rows ? "trew_hip_dissect_results: n_records, n_items and n_rows must not be null"
                            : rec_cap && !records             ? "trew_hip_dissect_results: records must not be null"
                            : item_cap && !items              ? "trew_hip_dissect_results: items must not be null"
                                                              : nullptr;
    Slot *sp = nullptr;
    if (int rc = fetch_begin(ctx, slot, kDissect, arg_error, &sp)) return rc;
    const MeasureState &st = sp->measure[kDissect];
    unsigned long long found[3] = {0, 0, 0};
    if (int rc = fetch_counted(ctx, st, found, 3, counts)) return rc;
    *n_items = found[0];
    *n_rows = found[1];
    *n_records = found[2];
    // one contract for the three: all fit, or nothing is copied.  The items are numbered against all the records, so both logs
    // come whole to the host whatever the caller's buffers hold.
    if (found[0] <= st.max_log && found[1] <= st.max_rows && found[2] <= st.n && (rec_cap || item_cap) && found[2]) {
        std::vector<trew_hip_tandem> recs((size_t) found[2]);
        std::vector<trew_hip_trace_item> its((size_t) found[0]);
        HIPCHK(ctx, hipMemcpy(recs.data(), st.aligned.p, recs.size() * sizeof(trew_hip_tandem), hipMemcpyDeviceToHost));
        if (!its.empty()) HIPCHK(ctx, hipMemcpy(its.data(), st.records.p, its.size() * sizeof(trew_hip_trace_item), hipMemcpyDeviceToHost));
        sort_tandems(recs.data(), recs.size());
        sort_dissect_items(its.data(), its.size());
        number_dissect_items(recs.data(), recs.size(), its.data(), its.size());
        if (const u64 take = std::min<u64>(rec_cap, recs.size())) memcpy(records, recs.data(), take * sizeof(trew_hip_tandem));
        if (const u64 take = std::min<u64>(item_cap, its.size())) memcpy(items, its.data(), take * sizeof(trew_hip_trace_item));
    }
    return fetch_end(ctx, st, ms_kernel);
}

// ---------------------------------------------------------------- gap-tolerant motif intervals anywhere in a read
extern "C" int trew_hip_intervals(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs,
                                  const trew_hip_interval_rule *rules, int n_motifs, uint64_t max_intervals) {
    auto own = [&]() -> const char * {
        if (const char *e = rules_error(rules, n_motifs)) return e;
        return max_intervals < 1 ? "max_intervals must be at least 1" : nullptr;
    };
    const LogShape shape = {sizeof(trew_hip_interval), max_intervals, (u64) n_motifs * 2ull, false, 0, 0, 0, 0};
    return queue_log(ctx, batch, slot, motifs, n_motifs, kIntervals, shape, own, no_setup, [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
        IntervalRulesDev rd;
        memset(&rd, 0, sizeof(rd));
        for (int m = 0; m < n_motifs; m++) {
            rd.max_gap[m] = rules[m].max_gap;
            rd.min_len[m] = rules[m].min_len;
        }
        const IntervalLog lg = {st.counter, (u32 *) st.records.p, st.max_log};
        HIPCHK(ctx, launch_intervals(s.stream, measure_cu(ctx), db, s.d_motifs, n_motifs, rd, lg, (u32 *) st.counts.p));
        return 0;
    });
}

extern "C" int trew_hip_intervals_results(trew_hip_ctx *ctx, int slot, trew_hip_interval *out, uint64_t cap, uint64_t *n, uint32_t *counts,
                                          float *ms_kernel) {
    // unlike the fixed-size ones, this call needs `n` (the only way to learn of an overflow), and like variants it refuses a
    // capacity without a buffer
    const char *arg_error = !n ? "trew_hip_intervals_results: n must not be null" : cap && !out ? "trew_hip_intervals_results: out must not be null" : nullptr;
    Slot *sp = nullptr;
    if (int rc = fetch_begin(ctx, slot, kIntervals, arg_error, &sp)) return rc;
    const MeasureState &st = sp->measure[kIntervals];
    unsigned long long found = 0;
    if (int rc = fetch_counted(ctx, st, &found, 1, counts)) return rc;
    *n = found;
    if (int rc = fetch_log(ctx, st, out, cap, std::min<u64>(found, st.max_log), sort_intervals)) return rc;
    return fetch_end(ctx, st, ms_kernel);
}

// ---------------------------------------------------------------- telomere variant repeats
constexpr u64 kVarHistLen = (u64) kAnnotMaxMotifs * 2ull * TREW_VARIANT_BINS;  // values of one histogram of a slot

extern "C" int trew_hip_variants(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs) {
    // both histograms (a fixed size: allocated on first use, never grown) start every call at zero, also a call without reads
    auto hists = [&](Slot &s, MeasureState &st) -> int {
        if (!st.hist) HIPCHK(ctx, hipMalloc((void **) &st.hist, 2ull * kVarHistLen * sizeof(unsigned long long)));
        HIPCHK(ctx, hipMemsetAsync(st.hist, 0, 2ull * kVarHistLen * sizeof(unsigned long long), s.stream));
        st.n_motifs = n_motifs;
        return 0;
    };
    return queue_records(ctx, batch, slot, motifs, n_motifs, kVariants, n_motifs, sizeof(trew_hip_variant), no_own_checks, hists,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             HIPCHK(ctx, launch_variants(s.stream, measure_cu(ctx), db, s.d_motifs, n_motifs, (trew_hip_variant *) st.records.p, st.hist, st.hist + kVarHistLen));
                             return 0;
                         });
}

extern "C" int trew_hip_variants_results(trew_hip_ctx *ctx, int slot, trew_hip_variant *out, uint64_t cap, uint64_t *n, uint64_t *hist,
                                         uint64_t *reads_with, float *ms_kernel) {
    // unlike annotate and tracts, which copy nothing when `out` is NULL, a capacity without a buffer is an error here
    const char *arg_error = cap && !out ? "trew_hip_variants_results: out must not be null" : nullptr;
    Slot *sp = nullptr;
    if (int rc = fetch_begin(ctx, slot, kVariants, arg_error, &sp)) return rc;
    const MeasureState &st = sp->measure[kVariants];
    if (int rc = fetch_records(ctx, st, out, cap, sizeof(trew_hip_variant), n)) return rc;
    const size_t hb = (size_t) st.n_motifs * 2 * TREW_VARIANT_BINS * sizeof(uint64_t);
    if (hist && hb) HIPCHK(ctx, hipMemcpy(hist, st.hist, hb, hipMemcpyDeviceToHost));
    if (reads_with && hb) HIPCHK(ctx, hipMemcpy(reads_with, st.hist + kVarHistLen, hb, hipMemcpyDeviceToHost));
    return fetch_end(ctx, st, ms_kernel);
}

// ---------------------------------------------------------------- de novo repeat period and unit per read
extern "C" int trew_hip_periods(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score) {
    auto own = [&]() -> const char * { return periods_error(min_period, max_period, penalty, min_score); };
    return queue_records(ctx, batch, slot, nullptr, 0, kPeriods, 1, sizeof(trew_hip_period), own, no_setup,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             HIPCHK(ctx, launch_periods(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, (trew_hip_period *) st.records.p));
                             return 0;
                         });
}

extern "C" int trew_hip_periods_results(trew_hip_ctx *ctx, int slot, trew_hip_period *out, uint64_t cap, uint64_t *n, float *ms_kernel) {
    return results_records(ctx, slot, kPeriods, out, cap, sizeof(trew_hip_period), n, ms_kernel);
}

// ---------------------------------------------------------------- de novo repeats under indels: seed, align, re-vote
extern "C" int trew_hip_refine(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score) {
    auto own = [&]() -> const char * { return periods_error(min_period, max_period, penalty, min_score); };
    return queue_records(ctx, batch, slot, nullptr, 0, kRefine, 1, sizeof(trew_hip_refined), own, no_setup,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             HIPCHK(ctx, launch_refine(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, (trew_hip_refined *) st.records.p));
                             return 0;
                         });
}

extern "C" int trew_hip_refine_results(trew_hip_ctx *ctx, int slot, trew_hip_refined *out, uint64_t cap, uint64_t *n, float *ms_kernel) {
    return results_records(ctx, slot, kRefine, out, cap, sizeof(trew_hip_refined), n, ms_kernel);
}

// ---------------------------------------------------------------- de novo repeats under indels for periods up to 256
extern "C" int trew_hip_polish(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score) {
    auto own = [&]() -> const char * { return satellites_error(min_period, max_period, penalty, min_score); };
    return queue_records(ctx, batch, slot, nullptr, 0, kPolish, 1, sizeof(trew_hip_polished), own, no_setup,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             HIPCHK(ctx, launch_polish(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, (trew_hip_polished *) st.records.p));
                             return 0;
                         });
}

extern "C" int trew_hip_polish_results(trew_hip_ctx *ctx, int slot, trew_hip_polished *out, uint64_t cap, uint64_t *n, float *ms_kernel) {
    return results_records(ctx, slot, kPolish, out, cap, sizeof(trew_hip_polished), n, ms_kernel);
}

// ---------------------------------------------------------------- refine's unit with the period chosen by alignment
extern "C" int trew_hip_resolve(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                                int candidates) {
    auto own = [&]() -> const char * { return resolve_error(min_period, max_period, penalty, min_score, candidates); };
    return queue_records(ctx, batch, slot, nullptr, 0, kResolve, 1, sizeof(trew_hip_resolved), own, no_setup,
                         [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
                             HIPCHK(ctx, launch_resolve(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, candidates,
                                                        (trew_hip_resolved *) st.records.p));
                             return 0;
                         });
}

extern "C" int trew_hip_resolve_results(trew_hip_ctx *ctx, int slot, trew_hip_resolved *out, uint64_t cap, uint64_t *n, float *ms_kernel) {
    return results_records(ctx, slot, kResolve, out, cap, sizeof(trew_hip_resolved), n, ms_kernel);
}

// ---------------------------------------------------------------- ordered unit chain per read
// The log holds events, not items; the results call pairs them, for which it keeps the motifs' lengths.
extern "C" int trew_hip_chain(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, const trew_hip_motif *motifs, int n_motifs, uint64_t max_events) {
    auto own = [&]() -> const char * { return max_events < 1 ? "max_events must be at least 1" : nullptr; };
    const LogShape shape = {sizeof(uint4), max_events, (u64) n_motifs * 4ull, false, 0, 0, 0, 0};
    return queue_log(ctx, batch, slot, motifs, n_motifs, kChain, shape, own, no_setup, [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
        for (int m = 0; m < n_motifs; m++) st.k[m] = (u32) motifs[m].k;  // a batch without reads has no events to pair
        const ChainLog lg = {st.counter, (uint4 *) st.records.p, st.max_log};
        HIPCHK(ctx, launch_chain(s.stream, measure_cu(ctx), db, s.d_motifs, n_motifs, lg, (u32 *) st.counts.p));
        return 0;
    });
}

extern "C" int trew_hip_chain_results(trew_hip_ctx *ctx, int slot, trew_hip_chain_item *out, uint64_t cap, uint64_t *n_items, uint64_t *n_events,
                                      uint32_t *counts, float *ms_kernel) {
    const char *arg_error = !n_items || !n_events ? "trew_hip_chain_results: n_items and n_events must not be null"
                            : cap && !out         ? "trew_hip_chain_results: out must not be null"
                                                  : nullptr;
    Slot *sp = nullptr;
    if (int rc = fetch_begin(ctx, slot, kChain, arg_error, &sp)) return rc;
    const MeasureState &st = sp->measure[kChain];
    // the number of items is the sum of the counts, which the kernel stores whether or not the log fitted
    std::vector<u32> own_counts;
    if (!counts && st.n_counts) {
        own_counts.resize((size_t) st.n_counts);
        counts = own_counts.data();
    }
    unsigned long long found = 0;
    if (int rc = fetch_counted(ctx, st, &found, 1, counts)) return rc;
    *n_events = found;
    u64 items = 0;
    for (u64 i = 0; i < st.n_counts; i++) items += counts[i];
    *n_items = items;
    const u64 take = std::min<u64>(items, cap);
    if (found <= st.max_log && take) {
        // Pairing on the host, so the items do not depend on the order in which the waves appended the events: ordered by
        // (read, motif, strand, start mod k, start), the starts and ends of a residue class alternate.
        std::vector<uint4> ev((size_t) found);
        HIPCHK(ctx, hipMemcpy(ev.data(), st.records.p, found * sizeof(uint4), hipMemcpyDeviceToHost));
        const u32 *kk = st.k;
        auto motif_of = [](const uint4 &e) { return e.y & 15u; };
        std::sort(ev.begin(), ev.end(), [&](const uint4 &a, const uint4 &b) {
            if (a.x != b.x) return a.x < b.x;
            if ((a.y & 255u) != (b.y & 255u)) return (a.y & 255u) < (b.y & 255u);  // motif, then strand
            const u32 k = kk[a.y & 15u];
            if (a.z % k != b.z % k) return a.z % k < b.z % k;
            return a.z < b.z;
        });
        std::vector<trew_hip_chain_item> all;
        all.reserve((size_t) items);
        u32 open = 0;  // the start of the residue class's open run
        for (const uint4 &e : ev) {
            const u32 kind = e.y >> 8, m = motif_of(e), strand = (e.y >> 4) & 1u;
            if (kind & kChainVariant) all.push_back(trew_hip_chain_item{e.x, m, strand, e.z, 1, e.w});
            if (kind & kChainStart) open = e.z;
            if (kind & kChainEnd) all.push_back(trew_hip_chain_item{e.x, m, strand, open, (e.z - open) / kk[m] + 1u, TREW_VARIANT_NONE});
        }
        if (all.size() != items) return fail(ctx, "trew_hip_chain_results: the events do not pair into the counted items");
        sort_chain_items(all.data(), all.size());
        memcpy(out, all.data(), take * sizeof(trew_hip_chain_item));
    }
    return fetch_end(ctx, st, ms_kernel);
}

// ---------------------------------------------------------------- de novo repeats: every tract of a read (repeats), with periods up to 256 (satellites), under indels (tandems)
// Three kernels, three record types and one host path: a log of one record per tract, one count per read that the kernel adds
// to, and a MeasureState each.
template <class Own, class Launch>
static int queue_tracts(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, Measure which, size_t rec_bytes, uint64_t max_records, Own error,
                        Launch launch) {
    auto own = [&]() -> const char * {
        if (const char *e = error()) return e;
        return max_records < 1 ? "max_records must be at least 1" : nullptr;
    };
    const LogShape shape = {rec_bytes, max_records, 1, true, 0, 0, 0, 0};
    return queue_log(ctx, batch, slot, nullptr, 0, which, shape, own, no_setup, [&](Slot &s, MeasureState &st, const DevBatch &db) -> int {
        return launch(s, db, RepeatLog{st.counter, (u32 *) st.records.p, st.max_log}, (u32 *) st.counts.p);
    });
}

// like intervals, their results call needs `n` (the only way to learn of an overflow) and refuses a capacity without a buffer:
// `arg_error` is the text of that check
template <class Rec>
static int results_tracts(trew_hip_ctx *ctx, int slot, Measure which, const char *arg_error, Rec *out, uint64_t cap, uint64_t *n, uint32_t *counts,
                          float *ms_kernel, void (*sort)(Rec *, uint64_t)) {
    Slot *sp = nullptr;
    if (int rc = fetch_begin(ctx, slot, which, arg_error, &sp)) return rc;
    const MeasureState &st = sp->measure[which];
    unsigned long long found = 0;
    if (int rc = fetch_counted(ctx, st, &found, 1, counts)) return rc;
    *n = found;
    if (int rc = fetch_log(ctx, st, out, cap, whole_log(st, found), sort)) return rc;
    return fetch_end(ctx, st, ms_kernel);
}

extern "C" int trew_hip_repeats(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                                uint64_t max_records) {
    auto error = [&]() { return periods_error(min_period, max_period, penalty, min_score); };
    return queue_tracts(ctx, batch, slot, kRepeats, sizeof(trew_hip_repeat), max_records, error, [&](Slot &s, const DevBatch &db, const RepeatLog &lg, u32 *counts) -> int {
        HIPCHK(ctx, launch_repeats(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, lg, counts));
        return 0;
    });
}

extern "C" int trew_hip_repeats_results(trew_hip_ctx *ctx, int slot, trew_hip_repeat *out, uint64_t cap, uint64_t *n, uint32_t *counts, float *ms_kernel) {
    const char *arg_error = !n ? "trew_hip_repeats_results: n must not be null" : cap && !out ? "trew_hip_repeats_results: out must not be null" : nullptr;
    return results_tracts(ctx, slot, kRepeats, arg_error, out, cap, n, counts, ms_kernel, sort_repeats);
}

static_assert(sizeof(trew_hip_satellite) == 104, "26 words: what satellites_wave_kernel stores");
extern "C" int trew_hip_satellites(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty,
                                   uint32_t min_score, uint64_t max_records) {
    auto error = [&]() { return satellites_error(min_period, max_period, penalty, min_score); };
    return queue_tracts(ctx, batch, slot, kSatellites, sizeof(trew_hip_satellite), max_records, error, [&](Slot &s, const DevBatch &db, const RepeatLog &lg, u32 *counts) -> int {
        HIPCHK(ctx, launch_satellites(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, lg, counts));
        return 0;
    });
}

extern "C" int trew_hip_satellites_results(trew_hip_ctx *ctx, int slot, trew_hip_satellite *out, uint64_t cap, uint64_t *n, uint32_t *counts,
                                           float *ms_kernel) {
    const char *arg_error = !n ? "trew_hip_satellites_results: n must not be null" : cap && !out ? "trew_hip_satellites_results: out must not be null" : nullptr;
    return results_tracts(ctx, slot, kSatellites, arg_error, out, cap, n, counts, ms_kernel, sort_satellites);
}

static_assert(sizeof(trew_hip_tandem) == 72, "18 words: what tandems_wave_kernel stores");
extern "C" int trew_hip_tandems(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                                uint64_t max_records) {
    auto error = [&]() { return periods_error(min_period, max_period, penalty, min_score); };
    return queue_tracts(ctx, batch, slot, kTandems, sizeof(trew_hip_tandem), max_records, error, [&](Slot &s, const DevBatch &db, const RepeatLog &lg, u32 *counts) -> int {
        HIPCHK(ctx, launch_tandems(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, lg, counts));
        return 0;
    });
}

// the sibling's checks (queue_tracts adds max_records) come first, then resolve_error's check of the candidates
extern "C" int trew_hip_tandems_resolved(trew_hip_ctx *ctx, const trew_hip_batch *batch, int slot, int min_period, int max_period, int penalty,
                                         uint32_t min_score, int candidates, uint64_t max_records) {
    auto error = [&]() -> const char * {
        if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
        if (max_records < 1) return "max_records must be at least 1";
        return resolve_error(min_period, max_period, penalty, min_score, candidates);
    };
    return queue_tracts(ctx, batch, slot, kTandems, sizeof(trew_hip_tandem), max_records, error, [&](Slot &s, const DevBatch &db, const RepeatLog &lg, u32 *counts) -> int {
        HIPCHK(ctx, launch_tandems_resolved(s.stream, measure_cu(ctx), db, min_period, max_period, penalty, min_score, candidates, lg, counts));
        return 0;
    });
}

extern "C" int trew_hip_tandems_results(trew_hip_ctx *ctx, int slot, trew_hip_tandem *out, uint64_t cap, uint64_t *n, uint32_t *counts, float *ms_kernel) {
    const char *arg_error = !n ? "trew_hip_tandems_results: n must not be null" : cap && !out ? "trew_hip_tandems_results: out must not be null" : nullptr;
    return results_tracts(ctx, slot, kTandems, arg_error, out, cap, n, counts, ms_kernel, sort_tandems);
}

// ---------------------------------------------------------------- host packing
extern "C" uint64_t trew_pack_words(uint64_t n_bases) { return 3ull * ((n_bases + 31ull) / 32ull); }

namespace {
struct PackLut {
    unsigned char v[256];
    PackLut() {
        // codes[], kmer.cpp:14-31: T=0 G=1 C=2 A=3, either case; everything else is "N"
        for (int i = 0; i < 256; i++) v[i] = 4;
        v[(int) 'T'] = v[(int) 't'] = 0;
        v[(int) 'G'] = v[(int) 'g'] = 1;
        v[(int) 'C'] = v[(int) 'c'] = 2;
        v[(int) 'A'] = v[(int) 'a'] = 3;
    }
};
const PackLut g_lut;

// 32 bases -> {lo, hi, nmask} with AVX2 compares + movemask (about 10x the table loop)
#if defined(__x86_64__)
#include <immintrin.h>
__attribute__((target("avx2"))) inline void pack32_avx2(const unsigned char *q, uint32_t *out) {
    const __m256i c = _mm256_and_si256(_mm256_loadu_si256((const __m256i *) q), _mm256_set1_epi8((char) 0xDF));  // upper-case
    const __m256i a = _mm256_cmpeq_epi8(c, _mm256_set1_epi8('A')), cc = _mm256_cmpeq_epi8(c, _mm256_set1_epi8('C'));
    const __m256i g = _mm256_cmpeq_epi8(c, _mm256_set1_epi8('G')), t = _mm256_cmpeq_epi8(c, _mm256_set1_epi8('T'));
    // letters only: 0xDF folding must not turn e.g. 'a'-0x20 twins of non-letters into hits: A/C/G/T & a/c/g/t are the only preimages
    const uint32_t ma = (uint32_t) _mm256_movemask_epi8(a), mc = (uint32_t) _mm256_movemask_epi8(cc);
    const uint32_t mg = (uint32_t) _mm256_movemask_epi8(g), mt = (uint32_t) _mm256_movemask_epi8(t);
    out[0] = mg | ma;             // lo bit: G=1, A=3
    out[1] = mc | ma;             // hi bit: C=2, A=3
    out[2] = ~(ma | mc | mg | mt);  // everything else is "N"
}
// 64 bases -> two triples with AVX-512BW byte compares straight into mask registers
__attribute__((target("avx512f,avx512bw"))) inline void pack64_avx512(const unsigned char *q, uint32_t *out) {
    const __m512i c = _mm512_and_si512(_mm512_loadu_si512((const void *) q), _mm512_set1_epi8((char) 0xDF));
    const uint64_t ma = _mm512_cmpeq_epi8_mask(c, _mm512_set1_epi8('A')), mc = _mm512_cmpeq_epi8_mask(c, _mm512_set1_epi8('C'));
    const uint64_t mg = _mm512_cmpeq_epi8_mask(c, _mm512_set1_epi8('G')), mt = _mm512_cmpeq_epi8_mask(c, _mm512_set1_epi8('T'));
    const uint64_t lo = mg | ma, hi = mc | ma, nm = ~(ma | mc | mg | mt);
    out[0] = (uint32_t) lo;
    out[1] = (uint32_t) hi;
    out[2] = (uint32_t) nm;
    out[3] = (uint32_t) (lo >> 32);
    out[4] = (uint32_t) (hi >> 32);
    out[5] = (uint32_t) (nm >> 32);
}
#endif

// one read -> triples; returns words written
inline uint64_t pack_one(const unsigned char *p, uint64_t len, uint32_t *out) {
    const uint64_t nw = (len + 31) / 32;
    uint64_t j = 0;
#if defined(__x86_64__)
    static const bool have_avx512 = __builtin_cpu_supports("avx512bw") && !getenv("TREW_NO_AVX512");
    static const bool have_avx2 = __builtin_cpu_supports("avx2");
    if (have_avx512)
        for (; 32 * (j + 2) <= len; j += 2) pack64_avx512(p + 32 * j, out + 3 * j);
    if (have_avx2)
        for (; 32 * (j + 1) <= len; j++) pack32_avx2(p + 32 * j, out + 3 * j);
#endif
    for (; j < nw; j++) {
        uint32_t lo = 0, hi = 0, nm = 0;
        const uint64_t m = std::min<uint64_t>(32, len - 32 * j);
        const unsigned char *q = p + 32 * j;
        for (uint64_t i = 0; i < m; i++) {
            const unsigned c = g_lut.v[q[i]];
            lo |= (uint32_t) (c & 1u) << i;
            hi |= (uint32_t) ((c >> 1) & 1u) << i;
            nm |= (uint32_t) (c >> 2) << i;
        }
        out[3 * j + 0] = lo & ~nm;
        out[3 * j + 1] = hi & ~nm;
        out[3 * j + 2] = nm;
    }
    return 3 * nw;
}
}  // namespace

extern "C" uint64_t trew_pack_reads(const char *buf, const int64_t *st, const int64_t *nd, uint64_t n_reads,
                                    uint32_t *words, uint64_t words_cap, uint32_t *offsets, uint32_t *lengths) {
    uint64_t w = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const int64_t n = nd[r] - st[r] + 1;
        const uint64_t len = n > 0 ? (uint64_t) n : 0;
        if (w + 3 * ((len + 31) / 32) > words_cap || w > 0xffffffffull) return (uint64_t) -1;
        offsets[r] = (uint32_t) w;
        lengths[r] = (uint32_t) len;
        w += pack_one((const unsigned char *) buf + st[r], len, words + w);
    }
    return w;
}

extern "C" uint64_t trew_pack_pairs(const char *buf1, const int64_t *st1, const int64_t *nd1,
                                    const char *buf2, const int64_t *st2, const int64_t *nd2, uint64_t n_pairs,
                                    uint32_t *words, uint64_t words_cap, uint32_t *offsets, uint32_t *lengths) {
    uint64_t w = 0;
    for (uint64_t r = 0; r < n_pairs; r++) {
        for (int mate = 0; mate < 2; mate++) {
            const char *buf = mate ? buf2 : buf1;
            const int64_t s = mate ? st2[r] : st1[r], e = mate ? nd2[r] : nd1[r];
            const uint64_t len = e - s + 1 > 0 ? (uint64_t) (e - s + 1) : 0;
            if (w + 3 * ((len + 31) / 32) > words_cap || w > 0xffffffffull) return (uint64_t) -1;
            offsets[2 * r + mate] = (uint32_t) w;
            lengths[2 * r + mate] = (uint32_t) len;
            w += pack_one((const unsigned char *) buf + s, len, words + w);
        }
    }
    return w;
}

// ---------------------------------------------------------------- synthetic workloads
template <typename F>
static void parallel_reads(uint64_t n, F fn) {
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 1;
    if (n < 4096 || nt == 1) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> th;
    const uint64_t per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        const uint64_t lo = std::min<uint64_t>(n, per * t), hi = std::min<uint64_t>(n, lo + per);
        if (lo < hi) th.emplace_back([=] { fn(lo, hi); });
    }
    for (auto &x : th) x.join();
}

extern "C" int trew_synth_short_ascii(uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len, char *out) {
    parallel_reads(n_reads, [=](uint64_t lo, uint64_t hi) {
        for (uint64_t r = lo; r < hi; r++) {
            const trew_synth::ReadClass c = trew_synth::read_class(seed, first_read + r);
            char *o = out + r * (uint64_t) (read_len + 1);
            for (uint32_t p = 0; p < read_len; p++)
                o[p] = trew_synth::base_char(trew_synth::short_base(seed, first_read + r, c, p, read_len));
            o[read_len] = '\n';
        }
    });
    return 0;
}

extern "C" int trew_synth_pair_ascii(uint64_t seed, uint64_t first_pair, uint64_t n_pairs, uint32_t read_len, char *out1, char *out2) {
    parallel_reads(n_pairs, [=](uint64_t lo, uint64_t hi) {
        for (uint64_t r = lo; r < hi; r++) {
            const trew_synth::ReadClass c = trew_synth::read_class(seed, first_pair + r);
            char *o1 = out1 + r * (uint64_t) (read_len + 1);
            char *o2 = out2 + r * (uint64_t) (read_len + 1);
            for (uint32_t p = 0; p < read_len; p++) {
                o1[p] = trew_synth::base_char(trew_synth::pair_base(seed, first_pair + r, c, 0, p, read_len));
                o2[p] = trew_synth::base_char(trew_synth::pair_base(seed, first_pair + r, c, 1, p, read_len));
            }
            o1[read_len] = '\n';
            o2[read_len] = '\n';
        }
    });
    return 0;
}

// ---- long reads: quantile table of clip(lognormal(9.413, 0.7), 1000, 200000), host double math only
static double inv_norm_cdf(double p) {  // Acklam's rational approximation (|rel err| < 1.2e-9)
    static const double a[] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
    static const double b[] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01};
    static const double c[] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
    static const double d[] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
    const double pl = 0.02425;
    if (p < pl) {
        const double q = std::sqrt(-2 * std::log(p));
        return (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
    }
    if (p > 1 - pl) return -inv_norm_cdf(1 - p);
    const double q = p - 0.5, r = q * q;
    return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1);
}

static const uint32_t *long_quantiles() {
    static uint32_t table[trew_synth::kLongQuantiles];
    static bool init = false;
    if (!init) {
        for (int i = 0; i < trew_synth::kLongQuantiles; i++) {
            const double z = inv_norm_cdf((i + 0.5) / trew_synth::kLongQuantiles);
            double len = std::exp(9.413 + 0.7 * z);
            len = std::min(200000.0, std::max(1000.0, len));
            table[i] = (uint32_t) len;
        }
        init = true;
    }
    return table;
}

extern "C" int trew_synth_long_lengths(uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t *lengths) {
    const uint32_t *qt = long_quantiles();
    for (uint64_t r = 0; r < n_reads; r++) lengths[r] = trew_synth::long_class(seed, first_read + r, qt).len;
    return 0;
}

extern "C" int trew_synth_long_ascii(uint64_t seed, uint64_t first_read, uint64_t n_reads, const uint64_t *byte_offsets, char *out) {
    const uint32_t *qt = long_quantiles();
    parallel_reads(n_reads, [=](uint64_t lo, uint64_t hi) {
        for (uint64_t r = lo; r < hi; r++) {
            const trew_synth::LongClass c = trew_synth::long_class(seed, first_read + r, qt);
            char *o = out + byte_offsets[r];
            for (uint32_t p = 0; p < c.len; p++) o[p] = trew_synth::base_char(trew_synth::long_base(seed, first_read + r, c, p));
            o[c.len] = '\n';
        }
    });
    return 0;
}

extern "C" int trew_synth_long_device(trew_hip_ctx *ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                                      const uint32_t *d_offsets, uint32_t *d_words) {
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    uint32_t *d_qt = nullptr;
    HIPCHK(ctx, hipMalloc((void **) &d_qt, trew_synth::kLongQuantiles * 4));
    hipError_t e = hipMemcpy(d_qt, long_quantiles(), trew_synth::kLongQuantiles * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_synth_long(ctx->slots[0].stream, seed, first_read, n_reads, d_qt, d_offsets, d_words);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->slots[0].stream);
    (void) hipFree(d_qt);
    HIPCHK(ctx, e);
    return 0;
}

extern "C" int trew_synth_short_device(trew_hip_ctx *ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                                       uint32_t read_len, uint32_t *d_words) {
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    HIPCHK(ctx, launch_synth_short(ctx->slots[0].stream, seed, first_read, n_reads, read_len, d_words));
    HIPCHK(ctx, hipStreamSynchronize(ctx->slots[0].stream));
    return 0;
}

extern "C" int trew_synth_pair_device(trew_hip_ctx *ctx, uint64_t seed, uint64_t first_pair, uint64_t n_pairs,
                                      uint32_t read_len, uint32_t *d_words) {
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    HIPCHK(ctx, launch_synth_pair(ctx->slots[0].stream, seed, first_pair, n_pairs, read_len, d_words));
    HIPCHK(ctx, hipStreamSynchronize(ctx->slots[0].stream));
    return 0;
}

// ---------------------------------------------------------------- device memory helpers
extern "C" int trew_hip_malloc(trew_hip_ctx *ctx, uint64_t bytes, void **d_ptr) {
    if (!ctx || !d_ptr) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    HIPCHK(ctx, hipMalloc(d_ptr, bytes));
    return 0;
}
extern "C" int trew_hip_free(trew_hip_ctx *ctx, void *d_ptr) {
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    HIPCHK(ctx, hipFree(d_ptr));
    return 0;
}
extern "C" int trew_hip_memcpy_h2d(trew_hip_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes) {
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    HIPCHK(ctx, hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return 0;
}
extern "C" int trew_hip_memcpy_d2h(trew_hip_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes) {
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->p.device));
    HIPCHK(ctx, hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return 0;
}
