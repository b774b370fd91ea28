// kernels/copies.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Copies in place for units of up to 256 bases (trew_hip_copies): the traceback of monomers.inc's wraparound alignment, cut
// into copies of the monomer -- trew_hip_trace's definition, word for word, with 3 <= k <= TREW_MONOMER_MAX.  A kernel beside
// the scan and beside the other sixteen measures: it reads the batch's bit planes and the staged (k, unit[16]) entries and
// writes its own records, counts, item log and direction workspace.  The cell, the row step with and without directions and
// the butterfly are monomers.inc's (mono_row<Q, kDirs>, mono_reduce_wave<kPhase>), the walk and the items wraparound.inc's
// (wrap_walk with the del-bit decoder); this file is pass 1 with the end phase, the claim of the rows, their fill and fetch.
//
// The direction of a cell is one bit, not d.  A byte op | d << 2 | hit << 7 cannot hold d < 256, and need not.  In the closed
// row H[j] = max(V[j], H[(j - 1) mod k] shifted by 1): the maximum over d >= 1 of V[(j - d) mod k] shifted by d is the maximum
// over d' = d - 1 >= 0 of V[((j - 1) - d') mod k] shifted by d', shifted once more (shifting is monotone and composes; d' = k - 1
// is the cell V[j] a whole turn round, P k lower, which never wins and may stand in either maximum).  Let the smallest d that
// attains H[j] be d0 >= 1.  Then H[j - 1] is H[j] un-shifted by one: H[j - 1] shifted by 1 is a candidate of H[j], so it is
// not larger; and V[j - d0] shifted by d0 - 1 is a candidate of H[j - 1], so it is not smaller.  The smallest d of H[j - 1] is
// d0 - 1: a smaller d' there would give d' + 1 < d0 at j with the same tuple.  So a cell stores op (2 bits), hit (1 bit) and
// del = "H[j] is strictly larger than V[j] was before the closure", that is d0 >= 1, and the walk emits one `del` column and
// steps j <- (j - 1) mod k while del is set, d0 times in all, then reads op: rule (2) of 4.7h, one step at a time.  (A cell
// with del set scores: it is strictly larger than a V, which is at least the fresh start; so the dropped candidates of
// mono_take change nothing here.)  tests/copies_ref.py compares (op, d) of the O(n k^2) definition with this on every cell.
// Rule (1), op in the order F, D, I, is the order of mono_row's selects as it is of wrap_row's (trace.inc, (a)); rule (3), the
// end cell with the smallest phase, is the lowest live slot inside a lane (strict compares going up the slots) and the smaller
// phase last in the butterfly.  Fact (b) of trace.inc does not depend on k: the traceback needs only the tract's rows, started
// again from (0, start, 0, 0) in row start.
//
// Wave per read on the grid of launch_tracts, the blocked layout of monomers.inc: lane l holds the phases Q l .. Q l + Q - 1.
// The strands of a monomer are walked one after the other, each whole: pass 1 is monomers' loop and keeps the end phase; pass
// 2 runs when the strand reached min_score: the wave claims end - start rows of 64 Q bytes with one returning atomic on the row
// counter and computes the rows start + 1 .. end again; every lane stores the bytes of its Q cells with one vector store
// (phase j at byte j of the row).  The walk is wave-uniform; the rows come a block of kCopiesLds / (64 Q) at a time into LDS,
// 4 KB a wave as in trace.inc, the block being one contiguous piece of the workspace (a lane fetches 64 bytes).
//
// When the claimed rows lie beyond max_rows nothing is stored in the workspace, and the walk fills its LDS block by computing
// the strand's rows from its start up to the block again, as trace.inc does: the items' number stays exact.  No scalar
// memory writes, no inline assembly, no scratch.

constexpr u32 kCopiesLds = 4096;  // bytes of the walk's LDS block a wave: 64 / Q rows

template <int Q>
struct CopiesCells;  // the direction bytes of a lane's Q cells as one store
template <>
struct CopiesCells<1> {
    using T = unsigned char;
};
template <>
struct CopiesCells<2> {
    using T = unsigned short;
};
template <>
struct CopiesCells<4> {
    using T = u32;
};

// the strand's target base of every slot of the lane (a dead phase matches nothing) and which slots are live
template <int Q>
__device__ __forceinline__ void mono_target(const trew_hip_monomer *mm, u32 k, u32 strand, u32 lane, u32 (&tb)[Q], bool (&live)[Q]) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const u32 p = (u32) Q * lane + (u32) q;
        live[q] = p < k;
        const u32 j = !live[q] ? 0u : strand ? k - 1u - p : p;  // < 256
        const u32 code = (mm->unit[j >> 4] >> (2u * (j & 15u))) & 3u;
        tb[q] = !live[q] ? 8u : strand ? 3u - code : code;
    }
}

// Rows start + 1 .. to of the table that starts from (0, start, 0, 0) in row start; every lane stores the Q bytes of row i >
// keep at dst[(i - keep - 1) * 64 Q + Q lane]: the whole row, dead phases included.
template <int Q>
__device__ __forceinline__ void copies_fill(const ReadRef &rd, u32 start, u32 to, const u32 (&tb)[Q], int P, u32 lane, u32 diag_src, u32 last_lane,
                                            u32 last_slot, unsigned char *dst, u32 keep) {
    using T = typename CopiesCells<Q>::T;
    AlignCell H[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) H[q] = AlignCell{0, start, 0, 0};
    u32 lo = 0, hi = 0, nm = 0;
    for (u32 i = start + 1u; i <= to; i++) {
        const u32 p = i - 1u, b = p & 31u;
        if (b == 0u || p == start) {
            const u64 w = p >> 5;
            lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
        }
        const u32 dirs = mono_row<Q, true>(H, base_code(lo, hi, nm, b), tb, i, P, lane, diag_src, last_lane, last_slot);
        if (i > keep) *(T *) (dst + (u64) (i - keep - 1u) * (64u * (u32) Q) + (u32) Q * lane) = (T) dirs;
    }
}

// Rows blk_lo + 1 .. i (at most a block) out of the workspace whose first row is start + 1 into the wave's LDS block: they
// are one piece of (i - blk_lo) Q times 64 bytes, a lane fetches 64 of them
template <int Q>
__device__ __forceinline__ void copies_fetch(const unsigned char *ws, u32 start, uint4 *blk4, u32 blk_lo, u32 i) {
    struct alignas(16) Piece {
        uint4 q[4];
    };
    const u32 lane = lane_id();
    const Piece *src = (const Piece *) (ws + (u64) (blk_lo - start) * (64u * (u32) Q));
    if (lane < (i - blk_lo) * (u32) Q) ((Piece *) blk4)[lane] = src[lane];
}

template <int Q>
__global__ void __launch_bounds__(256) copies_wave_kernel(DevBatch B, const trew_hip_monomer *__restrict__ mt, int n_monomers, int penalty, u32 min_score,
                                                          TraceLog lg, u32 *__restrict__ out, u32 *__restrict__ counts) {
    constexpr u32 kRowBytes = 64u * (u32) Q, kBlock = kCopiesLds / kRowBytes;
    __shared__ uint4 copies_lds[4][kCopiesLds / 16u];
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    const u32 lane = lane_id();
    uint4 *const blk4 = copies_lds[(threadIdx.x >> 6) & 3u];
    unsigned char *const blk = (unsigned char *) blk4;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_monomers; m++) {
            const trew_hip_monomer *mm = mt + m;
            const u32 k = rfl((u32) mm->k);  // 3 .. 64 Q
            const u32 last_lane = (k - 1u) / (u32) Q, last_slot = (k - 1u) % (u32) Q;
            const u32 diag_src = (lane == 0u ? last_lane : lane - 1u) << 2;
            for (u32 strand = 0; strand < 2u; strand++) {
                u32 tb[Q];
                bool live[Q];
                mono_target<Q>(mm, k, strand, lane, tb, live);
                // ---- pass 1: monomers' loop; the best cell of a lane also keeps its phase, the lowest live slot on equal tuples
                AlignCell H[Q], best{0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < Q; q++) H[q] = AlignCell{0, 0, 0, 0};
                u32 best_end = 0, best_j = (u32) Q * lane;
                for (u32 w = 0; w < rd.nw; w++) {
                    const u32 lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
                    const u32 left = rd.len - (w << 5);  // >= 1
                    const u32 nb = left < 32u ? left : 32u;
                    for (u32 b = 0; b < nb; b++) {
                        const u32 i = (w << 5) + b + 1u;
                        mono_row<Q, false>(H, base_code(lo, hi, nm, b), tb, i, P, lane, diag_src, last_lane, last_slot);
                        AlignCell top = H[0];
                        u32 top_q = 0;
#pragma unroll
                        for (int q = 1; q < Q; q++) {
                            const bool up = live[q] & align_gt(H[q], top);
                            top = align_pick(up, H[q], top);
                            top_q = up ? (u32) q : top_q;
                        }
                        const bool up = live[0] & (top.score > best.score);
                        wrap_keep_best(top, i, live[0], best, best_end);
                        best_j = up ? (u32) Q * lane + top_q : best_j;
                    }
                }
                mono_reduce_wave<true>(best, best_end, best_j);
                const u32 x = lane == 0u ? best.score : lane == 1u ? best.start : lane == 2u ? best_end : lane == 3u ? best.consumed : best.matches;
                if (lane < 5u) out[(r * (u64) n_monomers + (u64) m) * 10ull + 5ull * strand + lane] = x;

                // ---- pass 2 and the walk: every lane holds the strand's record after the butterfly
                const u32 score = rfl(best.score), start = rfl(best.start), en = rfl(best_end);
                u32 n_items = 0;
                if (score >= min_score) {
                    const u32 rows = en - start;  // >= 1
                    u64 first = 0;
                    if (lane == 0) first = atomicAdd(lg.row_counter, (unsigned long long) rows);
                    first = rfl64(first);
                    const bool fits = first + (u64) rows <= lg.max_rows;
                    unsigned char *const ws = lg.rows + first * (u64) kRowBytes;
                    if (fits) {
                        copies_fill<Q>(rd, start, en, tb, P, lane, diag_src, last_lane, last_slot, ws, start);
                        __threadfence();  // other lanes of this wave read the rows back
                    }
                    u32 jj = rfl(best_j);
                    n_items = wrap_walk<kRowBytes, kBlock, true>(lg, (u32) r, (u32) m, strand, k, start, en, jj, blk, [&](u32 blk_lo, u32 i) {
                        if (fits) copies_fetch<Q>(ws, start, blk4, blk_lo, i);
                        else copies_fill<Q>(rd, start, i, tb, P, lane, diag_src, last_lane, last_slot, blk, blk_lo);  // the strand's rows from its start again
                    });
                }
                if (lane == 0) counts[(r * (u64) n_monomers + (u64) m) * 2ull + strand] = n_items;
            }
        }
    }
}
