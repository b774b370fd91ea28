// kernels/dissect.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Units in place for every tract of a read, no motif given (trew_hip_dissect): tandems.inc's pieces of a read, and for every
// piece that gives a record decompose.inc's anchor and traceback of that piece against its own unit.  A kernel beside the scan
// and beside the other thirteen measures: it reads the same bit planes, takes no pattern table and writes only buffers of its
// own (a log of records, a log of items, a direction workspace, their three counters, two counts per read).  refine_piece is
// refine.inc's; the rows and the walk are wrap_fill<32>, wrap_fetch<32> and wrap_walk<32> of kernels/wraparound.inc.
//
// Definition (DESIGN 4.7j, include/trew_hip.h).  The pieces of a read, their depths and which of them give a record are those
// of trew_hip_tandems (4.7g), the weak-piece rule and repeat_worth included.  A piece [lo, hi) with a record X (score >=
// min_score) yields X with its reserved word the anchor rho of X.unit (4.7i: the smallest rotation as packed words, no reverse
// complement) and the items of 4.7i for the bases [lo, hi) taken as a read of their own, in read coordinates.  A weak piece
// yields nothing and claims no rows.
//
// The piece loop is tandems.inc's, written out once more: the wave-uniform stack of (lo, hi, depth) across the lanes of three
// VGPRs, the LONGER child pushed, the SHORTER continued, both children of a weak piece as well; a fix to the walk there or in
// pieces.inc has to be made here too.  The stack stays live across a trace; the piece at hand, the stack pointer and the
// record are wave-uniform.  For a strong piece, in the order of decompose.inc: the anchor (lane j < k forms rotation j of the
// packed unit, two wave maxima and a ballot name the smallest), the claim of end - start rows of 32 bytes with one returning
// atomic, the rows by wrap_fill<32> from `start` -- refine_piece saw nothing outside the piece and X lies inside it, so the
// table restarted at X.start holds the path (fact (b) of trace.inc) whatever lies in front of the piece -- the end phase from
// row `end`, and wrap_walk<32>.  Every cell's start is a read coordinate, as X.start is: the items come out in read
// coordinates.  `fits` is decided per tract; a tract whose rows do not fit is traced by recomputing its blocks.  The word
// `motif` of an item holds the tract's start here; the host turns it into the tract's index where it sorts (trew_capi.cpp).
//
// Append.  One returning 64-bit vector-memory atomic per record and per item on its log's counter, wave-uniform; eighteen
// lanes store a record, twelve an item, nothing at or beyond a capacity while the counters keep counting.  counts[read] =
// (tracts, items), stored for every read.  All stores are vector stores; no inline assembly.
//
// Registers.  Left to itself the compiler takes 131 VGPRs here (decompose.inc's 126 and the stack), one wave a SIMD fewer than
// the kernels beside it; asked for four waves it finds 127 without a spill and without scratch, so the kernel asks.  Keeping lo
// and hi of an entry in the two halves of one register instead saves one VGPR (130): not enough, and not kept.

// kResolved (trew_hip_dissect_resolved, DESIGN 4.7l): resolve_piece (kernels/resolve_piece.inc) in the place of refine_piece, with
// `candidates` its C; the record stays word i in lane i, the words the walk, the anchor and the rows need are read out of it and the
// store moves it two lanes up.  <false> is trew_hip_dissect's kernel as it was; it ignores `candidates`.
// Registers.  <true> under the four-wave request spills (128 VGPRs, 4 spilled, 20 bytes of scratch; 2 and 12 with the stack, and
// with the candidate list as well, in LDS: the pressure is in SGPRs), so it does not ask ((1, 8) is a 256-thread block's default):
// 137 VGPRs, three waves a SIMD, no scratch (DESIGN 4.7l).
template <bool kResolved>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kResolved ? 1 : 4, kResolved ? 8 : 4)))
dissect_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, RepeatLog rl, TraceLog lg, u32 *__restrict__ counts,
                    u32 candidates) {
    __shared__ u32 bins[4][kPeriodBins];
    __shared__ uint4 dis_lds[4][kTraceBlock * 2u];
    const u32 lane = lane_id();
    u32 *h = bins[threadIdx.x >> 6];
    h[lane] = 0;
    h[lane + 64u] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    const u32 kmin = (u32) rfl_i(min_period), kmax = (u32) rfl_i(max_period);
    const u32 smin = rfl(min_score);
    const u32 j = lane & 31u;
    uint4 *const blk4 = dis_lds[(threadIdx.x >> 6) & 3u];
    unsigned char *const blk = (unsigned char *) blk4;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        u32 st_lo = 0, st_hi = 0, st_d = 0;  // the stack: entry i in lane i
        u32 sp = 0;                          // entries pending (wave-uniform, at most 32: kernels/pieces.inc)
        u32 lo = 0, hi = rd.len, depth = 0;  // the piece at hand
        u32 found = 0, n_items = 0;
        bool have = repeat_worth(lo, hi, kmin, smin);
        while (have) {  // wave-uniform
            u32 rec[16], r_start = 0, r_end = 0;
            u32 won = 0;  // kResolved: the record, word i in lane i
            bool split;
            if constexpr (kResolved) {
                u32 m;
                split = resolve_piece(rd, Piece{lo, hi}, kmin, kmax, P, smin, rfl(candidates), h, won, r_start, r_end, m, [](u32, u32, u32, bool) {});
                rec[0] = record_word(won, 0), rec[4] = record_word(won, 4), rec[5] = record_word(won, 5), rec[6] = record_word(won, 6);
                rec[7] = record_word(won, 7), rec[8] = record_word(won, 8), rec[12] = record_word(won, 12), rec[13] = record_word(won, 13);
            } else {
                split = refine_piece(rd, Piece{lo, hi}, kmin, kmax, P, smin, h, rec, r_start, r_end);
            }
            u32 a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;  // the children; a the shorter
            if (split) {
                const u32 score = rfl(rec[4]);
                const bool strong = score >= smin;
                // the children lie around the refined tract, or around the periods tract of a weak piece
                const u32 start = strong ? rfl(rec[5]) : rfl(r_start), en = strong ? rfl(rec[6]) : rfl(r_end);
                // a tract lies inside its piece; the pieces below are formed from it, the rows are claimed by it
                if (!(start >= lo && en <= hi && start < en)) break;
                const u32 k = rfl(rec[0]);
                if (strong && k != 0u) {
                    found++;
                    const u32 consumed_r = rfl(rec[7]), matches_r = rfl(rec[8]);
                    // ---- anchor: the smallest rotation of the packed unit, first base most significant
                    const u64 unit = ((u64) rfl(rec[13]) << 32) | rfl(rec[12]);
                    const u64 mask = k >= 32u ? ~0ull : (1ull << (2u * k)) - 1ull;
                    const bool live = lane < k;  // one half forms the rotations
                    const u32 sh = live ? 2u * lane : 0u;
                    const u64 rot = sh ? ((unit << sh) | (unit >> ((2u * k - sh) & 63u))) & mask : unit;  // rotation `lane`
                    const u32 nhi = ~(u32) (rot >> 32), nlo = ~(u32) rot;
                    bool tie = live & (nhi == wave_max_u32(live ? nhi : 0u));
                    tie &= nlo == wave_max_u32(tie ? nlo : 0u);
                    u32 rho = (u32) __builtin_ctzll(__ballot(tie) | (1ull << 63));  // the unit is primitive: one lane is left
                    rho = rho < k ? rho : 0u;
                    // ---- the record: read, depth, refine's sixteen words with the anchor in the reserved one
                    {
                        u32 x;
                        if constexpr (kResolved) {
                            x = lane_read(won, ((lane - 2u) & 63u) << 2);  // word i into lane i + 2
                            x = lane == 13u ? rho : x;
                        } else {
                            x = rec[15];
#pragma unroll
                            for (int i = 14; i >= 0; i--) x = lane == (u32) (i + 2) ? (i == 11 ? rho : rec[i]) : x;
                        }
                        x = lane == 1u ? depth : x;
                        x = lane == 0u ? (u32) r : x;
                        log_append<kTandemWords>(rl.counter, rl.recs, rl.cap, x);
                    }
                    const u32 at = j >= k ? 0u : j + rho >= k ? j + rho - k : j + rho;  // (j + rho) mod k for the lanes j < k
                    const u32 tb = j < k ? (u32) (unit >> (2u * (k - 1u - at))) & 3u : 8u;  // M[j]; both halves alike
                    u32 src[5];
                    wrap_sources(k, src);
                    // ---- rows
                    const u32 rows = en - start;  // >= 1
                    u64 first = 0;
                    if (lane == 0) first = atomicAdd(lg.row_counter, (unsigned long long) rows);
                    first = rfl64(first);
                    const bool fits = first + (u64) rows <= lg.max_rows;
                    unsigned char *const ws = lg.rows + first * 32ull;  // formed, not touched, when the rows do not fit
                    // the end cell: the lowest phase whose cell of row `end` is the record's tuple
                    auto end_phase = [&](const AlignCell &H) {
                        const bool is_end = (lane < k) & (H.score == score) & (H.start == start) & (H.consumed == consumed_r) & (H.matches == matches_r);
                        const u32 p = (u32) __builtin_ctzll(__ballot(is_end) | (1ull << 63));
                        return p < k ? p : 0u;  // never: the cell exists (fact (b) of trace.inc)
                    };
                    u32 jj = 0;
                    if (fits) {
                        jj = end_phase(wrap_fill<32>(rd, start, en, start, tb, P, k, src, ws, start));
                        __threadfence();  // other lanes of this wave read the rows back
                    }
                    // ---- the walk and the items, one strand; the item's motif word: the tract's start
                    n_items += wrap_walk<32>(lg, (u32) r, start, 0u, k, start, en, jj, blk, [&](u32 blk_lo, u32 i) {
                        if (fits) {
                            wrap_fetch<32>(ws, start, blk4, blk_lo, i);
                        } else {
                            const AlignCell H = wrap_fill<32>(rd, start, i, start, tb, P, k, src, blk, blk_lo);
                            if (i == en) jj = end_phase(H);  // the first block ends at row `end`
                        }
                    });
                }
                const bool left_short = start - lo <= hi - en;
                a_lo = left_short ? lo : en;
                a_hi = left_short ? start : hi;
                b_lo = left_short ? en : lo;
                b_hi = left_short ? hi : start;
                depth++;
                if (repeat_worth(b_lo, b_hi, kmin, smin)) {  // push the longer child
                    if (lane == sp) {
                        st_lo = b_lo;
                        st_hi = b_hi;
                        st_d = depth;
                    }
                    sp++;
                }
            }
            if (split && repeat_worth(a_lo, a_hi, kmin, smin)) {  // go on with the shorter child
                lo = a_lo;
                hi = a_hi;
            } else if (sp != 0u) {  // pop
                sp--;
                sp = rfl(sp);
                lo = (u32) __builtin_amdgcn_readlane((int) st_lo, sp);
                hi = (u32) __builtin_amdgcn_readlane((int) st_hi, sp);
                depth = (u32) __builtin_amdgcn_readlane((int) st_d, sp);
            } else {
                have = false;
            }
        }
        if (lane < 2) counts[r * 2ull + lane] = lane ? n_items : found;
    }
}
