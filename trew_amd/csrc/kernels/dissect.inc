// kernels/dissect.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Units in place for every tract of a read, no motif given (trew_hip_dissect): tandems.inc's pieces of a read, and for every
// piece that gives a record decompose.inc's anchor and traceback of that piece against its own unit.  A kernel beside the scan
// and beside the other thirteen measures: it reads the same bit planes, takes no pattern table and writes only buffers of its
// own (a log of records, a log of items, a direction workspace, their three counters, two counts per read).  refine_piece is
// refine.inc's, the recursion over the pieces kernels/pieces.inc's, the anchor and the trace of a tract decompose.inc's.
//
// Definition (DESIGN 4.7j, include/trew_hip.h).  The pieces of a read, their depths and which of them give a record are those
// of trew_hip_tandems (4.7g), the weak-piece rule and repeat_worth included.  A piece [lo, hi) with a record X (score >=
// min_score) yields X with its reserved word the anchor rho of X.unit (4.7i: the smallest rotation as packed words, no reverse
// complement) and the items of 4.7i for the bases [lo, hi) taken as a read of their own, in read coordinates.  A weak piece
// yields nothing and claims no rows.
//
// The piece loop is walk_pieces of kernels/pieces.inc: the wave-uniform stack of (lo, hi, depth) across the lanes of three
// VGPRs, the LONGER child pushed, the SHORTER continued, both children of a weak piece as well.  This file is the eval of a
// piece: refine_piece (or resolve_piece), and for a strong piece whose tract lies inside it unit_anchor and trace_tract of
// kernels/decompose.inc, where the account of the anchor, the rows, the end phase and the walk stands.  refine_piece saw
// nothing outside the piece and X lies inside it, so the table restarted at X.start holds the path (fact (b) of trace.inc)
// whatever lies in front of the piece.  Every cell's start is a read coordinate, as X.start is: the items come out in read
// coordinates.  The stack stays live across a trace.  The eval hands back the tract and this lane's word of the record from
// lane 2 on; walk_pieces checks the tract, adds read and depth and appends the record, so a record goes out after its tract's
// items and not before them: the two logs have counters of their own and the host sorts both, so no result, count or overflow
// number depends on that order.  walk_pieces checks a tract only after the eval returns, so the eval checks it too: a tract
// that does not lie inside its piece claims no rows, is handed back without a record, and walk_pieces ends the read.  A weak
// piece, and a strong one with k = 0, split without a record.  The word `motif` of an item holds the tract's start here; the
// host turns it into the tract's index where it sorts (trew_capi.cpp).
//
// The eval returns at once for a piece without a tract, in front of the words it reads out of a record.  That is for the
// registers, not for the work: without that return <false> took 55.0 .. 55.1 ms for the long reads of tools/dissect_bench.py
// on the MI355X against 53.4 on its own walk (76 SGPR spills against 68); with one return behind the if constexpr <true> took
// 56.0 .. 56.2 against 54.4 .. 54.5 (112 spills against 95); as it stands 53.1 .. 53.2 and 53.9 .. 54.1, 77 and 92 spills
// (profiles/unit_walk/README.md).
//
// Append.  One returning 64-bit vector-memory atomic per record and per item on its log's counter, wave-uniform; eighteen
// lanes store a record, twelve an item, nothing at or beyond a capacity while the counters keep counting.  counts[read] =
// (tracts, items), stored for every read.  All stores are vector stores; no inline assembly.
//
// Registers.  Left to itself the compiler takes 131 VGPRs here (decompose.inc's 126 and the stack), one wave a SIMD fewer than
// the kernels beside it; asked for four waves it finds 127 without a spill and without scratch, so the kernel asks.  Keeping lo
// and hi of an entry in the two halves of one register instead saves one VGPR (130): not enough, and not kept.

// kResolved (trew_hip_dissect_resolved, DESIGN 4.7l): resolve_piece (kernels/resolve_piece.inc) in the place of refine_piece, with
// `candidates` its C; the record stays word i in lane i, the words the eval, the anchor and the rows need are read out of it and the
// record's word is taken two lanes up.  <false> is trew_hip_dissect's kernel as it was; it ignores `candidates`.
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
    uint4 *const blk4 = dis_lds[(threadIdx.x >> 6) & 3u];
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        u32 n_items = 0;
        const u32 found = walk_pieces<kTandemWords>(r, rd.len, kmin, smin, rl, [&](u32 lo, u32 hi) __attribute__((always_inline)) {
            u32 rec[16], r_start = 0, r_end = 0;
            u32 won = 0;  // kResolved: the record, word i in lane i
            bool split;
            if constexpr (kResolved) {
                u32 m;
                split = resolve_piece(rd, Piece{lo, hi}, kmin, kmax, P, smin, rfl(candidates), h, won, r_start, r_end, m, [](u32, u32, u32, bool) {});
                if (!split) return PieceEval{false, false, 0u, 0u, 0u};
                rec[0] = record_word(won, 0), rec[4] = record_word(won, 4), rec[5] = record_word(won, 5), rec[6] = record_word(won, 6);
                rec[7] = record_word(won, 7), rec[8] = record_word(won, 8), rec[12] = record_word(won, 12), rec[13] = record_word(won, 13);
            } else {
                split = refine_piece(rd, Piece{lo, hi}, kmin, kmax, P, smin, h, rec, r_start, r_end);
                if (!split) return PieceEval{false, false, 0u, 0u, 0u};
            }
            const u32 score = rfl(rec[4]), k = rfl(rec[0]);
            const bool strong = score >= smin;
            // the children lie around the refined tract, or around the periods tract of a weak piece
            const u32 start = strong ? rfl(rec[5]) : rfl(r_start), en = strong ? rfl(rec[6]) : rfl(r_end);
            // a tract lies inside its piece: one that does not claims no rows, has no record, and walk_pieces ends the read
            const bool record = split && strong && k != 0u && start >= lo && en <= hi && start < en;
            u32 x = 0;
            if (record) {  // wave-uniform
                const u64 unit = ((u64) rfl(rec[13]) << 32) | rfl(rec[12]);
                const u32 rho = unit_anchor(unit, k);
                // the record's words from lane 2 on: refine's sixteen with the anchor in the reserved one
                if constexpr (kResolved) {
                    x = lane_read(won, ((lane - 2u) & 63u) << 2);  // word i into lane i + 2
                    x = lane == 13u ? rho : x;
                } else {
                    x = rec[15];
#pragma unroll
                    for (int i = 14; i >= 0; i--) x = lane == (u32) (i + 2) ? (i == 11 ? rho : rec[i]) : x;
                }
                // the items, the word `motif` of each the tract's start
                n_items += trace_tract(rd, lg, (u32) r, start, unit, k, rho, score, start, en, rfl(rec[7]), rfl(rec[8]), P, blk4);
            }
            return PieceEval{split, record, start, en, x};
        });
        if (lane < 2) counts[r * 2ull + lane] = lane ? n_items : found;
    }
}
