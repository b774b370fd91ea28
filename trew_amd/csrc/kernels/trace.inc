// kernels/trace.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Units in place under indels (trew_hip_trace): the traceback of align.inc's wraparound alignment, cut into copies of the
// motif.  A kernel beside the scan and beside the other eleven measures: it reads the same bit planes and pattern tables and
// writes its own records, counts, item log and direction workspace.  The cells, the row step with and without directions, the
// rows of direction bytes (wrap_fill, wrap_fetch) and the walk (wrap_walk) are kernels/wraparound.inc's, shared with
// decompose.inc; this file is pass 1, the claim of the rows and a walk per traced strand.
//
// Definition (DESIGN 4.7h, include/trew_hip.h).  The table of 4.7e with three tie rules: op of V[i][j] is the fresh start
// before the diagonal before the inserted read base on equal tuples, d of H[i][j] the smallest d that attains the largest
// tuple, and the end cell has the smallest phase among equal cells.  The walk goes from the end cell to the fresh start.
//
// (a) The doubling steps give the defined directions.  op: the row step takes the diagonal only when its score is positive
// (a tuple with score <= 0 from an earlier row has start < i and loses to the fresh start (0, i, 0, 0); it cannot equal it) and
// the inserted base only when it is strictly larger than what stands -- F, D, I in this order on equal tuples.  d: before step
// s every lane holds the largest tuple over d < s with the smallest such d (true for s = 1: d = 0).  Step s offers lane j the
// cell of lane (j - s) mod k as it was before the step: the largest over d' < s with the smallest d', now d = d' + s in
// [s, 2 s).  Taken only when strictly larger, the lane keeps the smaller d on equal tuples (every d < s is smaller than every
// d >= s), and takes the smallest d of [s, 2 s) otherwise: the claim for 2 s.  The last step may offer d >= k: the same cell
// as d - k, P k cheaper, strictly smaller in score, never taken.  tests/trace_ref.py checks every cell, k = 3 .. 32.
//
// (b) The traceback needs only the tract's rows.  Every cell on the walked path carries the record's start in its tuple (a
// candidate hands its start on), and so does every candidate that ties with one, since start is a field of the tuple.  A cell
// whose start field is b was reached from the fresh start of row b through rows > b alone, so the table that begins with
// H[b][.] = (0, b, 0, 0) holds each of these cells with the same tuple; and it holds nothing larger than the full table does,
// cell by cell (its row b is not larger, and the recurrence is monotone).  So in every cell of the path the winner and what
// ties with it are the same in both tables, and the directions agree there.
//
// Wave per read on the grid of launch_tracts, the row layout of align.inc: lanes 0 .. 31 hold the phases of strand fwd, lanes
// 32 .. 63 those of strand rev.  Pass 1 is align's loop and keeps the end phase.  Pass 2 runs only when a strand reached
// min_score: the wave claims hi - lo rows of 64 bytes (lo the smaller start, hi the larger end of the strands that reached it)
// with one returning atomic on the row counter and computes the rows lo + 1 .. hi again, each strand's half starting from
// (0, start, 0, 0) at its own start; every lane stores one byte a row, op | d << 2 | hit << 7 (hit: the read base equals the
// lane's motif base, which spares the walk a look at the read).  The walk is wave-uniform and goes down a row a step, so the
// rows come a block of kTraceBlock at a time into LDS (a lane fetches a row, 4 x 16 bytes), and a step is two LDS byte reads,
// not two dependent loads from HBM.  Items appear last to first: a segment closes at its first column, a run of complete exact
// copies is emitted when a segment that is none closes behind it.  One returning atomic an item on the log's counter, twelve
// lanes store its words, nothing at or beyond the capacity while the counter keeps counting.
//
// When the claimed rows lie beyond max_rows nothing is stored in the workspace, and the walk fills its LDS block by computing
// the strand's rows from its start up to the block again: the items' number stays exact, which the retry contract needs, at a
// cost quadratic in the tract (tract^2 / (2 kTraceBlock) row steps).  No scalar stores, no inline assembly.

__global__ void __launch_bounds__(256) trace_wave_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, int penalty, u32 min_score,
                                                         TraceLog lg, u32 *__restrict__ out, u32 *__restrict__ counts) {
    __shared__ uint4 trace_lds[4][kTraceBlock * 4u];
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    const u32 lane = lane_id();
    const u32 j = lane & 31u, half = lane & 32u;
    uint4 *const blk4 = trace_lds[(threadIdx.x >> 6) & 3u];
    unsigned char *const blk = (unsigned char *) blk4;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_motifs; m++) {
            const AnnotMotifDev *mm = mt + m;
            const u32 k = rfl(mm->k);
            const bool live = j < k;
            const u32 strand = lane >> 5;
            const u32 tb = live ? ((mm->plo[strand][0] >> j) & 1u) | (((mm->phi[strand][0] >> j) & 1u) << 1) : 8u;
            u32 src[5];
            wrap_sources(k, src);
            // ---- pass 1: align's loop; the best cell of a lane also keeps its phase
            AlignCell H{0, 0, 0, 0}, best{0, 0, 0, 0};
            u32 best_end = 0, best_j = j;
            for (u32 w = 0; w < rd.nw; w++) {
                const u32 lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
                const u32 left = rd.len - (w << 5);  // >= 1
                const u32 nb = left < 32u ? left : 32u;
                for (u32 b = 0; b < nb; b++) {
                    const u32 i = (w << 5) + b + 1u;
                    wrap_row<false>(H, base_code(lo, hi, nm, b), tb, i, P, k, src);
                    wrap_keep_best(H, i, live, best, best_end);
                }
            }
            wrap_reduce_half<true>(best, best_end, best_j);
            wrap_store_alignment(out + (r * (u64) n_motifs + (u64) m) * 10ull, best, best_end);

            // ---- pass 2 and the walk
            const u32 sc[2] = {(u32) __builtin_amdgcn_readlane((int) best.score, 0), (u32) __builtin_amdgcn_readlane((int) best.score, 32)};
            const u32 st[2] = {(u32) __builtin_amdgcn_readlane((int) best.start, 0), (u32) __builtin_amdgcn_readlane((int) best.start, 32)};
            const u32 en[2] = {(u32) __builtin_amdgcn_readlane((int) best_end, 0), (u32) __builtin_amdgcn_readlane((int) best_end, 32)};
            const u32 js[2] = {(u32) __builtin_amdgcn_readlane((int) best_j, 0), (u32) __builtin_amdgcn_readlane((int) best_j, 32)};
            const bool traced[2] = {sc[0] >= min_score, sc[1] >= min_score};
            u32 n_items[2] = {0, 0};
            if (traced[0] | traced[1]) {
                const u32 lo = traced[0] && traced[1] ? (st[0] < st[1] ? st[0] : st[1]) : traced[0] ? st[0] : st[1];
                const u32 hi = traced[0] && traced[1] ? (en[0] > en[1] ? en[0] : en[1]) : traced[0] ? en[0] : en[1];
                const u32 rows = hi - lo;  // >= 1
                u64 first = 0;
                if (lane == 0) first = atomicAdd(lg.row_counter, (unsigned long long) rows);
                first = rfl64(first);
                const bool fits = first + (u64) rows <= lg.max_rows;
                // a half that is not traced starts with the other one: its bytes are never read
                const u32 my_start = half ? (traced[1] ? st[1] : lo) : (traced[0] ? st[0] : lo);
                unsigned char *const ws = lg.rows + first * 64ull;
                if (fits) {
                    wrap_fill<64>(rd, lo, hi, my_start, tb, P, k, src, ws, lo);
                    __threadfence();  // other lanes of this wave read the rows back
                }
                for (u32 s = 0; s < 2; s++) {
                    if (!traced[s]) continue;
                    const u32 start = st[s];
                    u32 jj = js[s];
                    n_items[s] = wrap_walk<64>(lg, (u32) r, (u32) m, s, k, start, en[s], jj, blk + (s << 5), [&](u32 blk_lo, u32 i) {
                        if (fits) wrap_fetch<64>(ws, lo, blk4, blk_lo, i);
                        else wrap_fill<64>(rd, start, i, my_start, tb, P, k, src, blk, blk_lo);  // the strand's rows from its start again
                    });
                }
            }
            if (lane < 2) counts[(r * (u64) n_motifs + (u64) m) * 2ull + lane] = lane ? n_items[1] : n_items[0];
        }
    }
}
