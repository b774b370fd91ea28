// kernels/trace.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Units in place under indels (trew_hip_trace): the traceback of align.inc's wraparound alignment, cut into copies of the
// motif.  A kernel beside the scan and beside the other eleven measures: it reads the same bit planes and pattern tables and
// writes its own records, counts, item log and direction workspace.  The cells, their order and the lane reads are align.inc's
// (AlignCell, align_gt, align_pick, align_from: used, not changed); the row step is written again here because it carries the
// directions.
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

constexpr u32 kTraceBlock = 64;  // rows of the walk's LDS block: 4 KB a wave
constexpr u32 kTraceWords = 12;  // trew_hip_trace_item

// One row: H of row i - 1 -> H of row i; returns op | d << 2 | hit << 7 of the lane's cell.
__device__ __forceinline__ u32 trace_row(AlignCell &H, u32 c, u32 tb, u32 i, int P, u32 k, const u32 (&src)[5]) {
    const bool hit = c == tb;
    const AlignCell d = align_from(H, src[0]);
    const int ds = hit ? (int) d.score + 1 : (int) d.score - P;
    AlignCell V = align_pick(ds > 0, AlignCell{(u32) ds, d.start, d.consumed + 1u, d.matches + (hit ? 1u : 0u)}, AlignCell{0, i, 0, 0});
    u32 op = ds > 0 ? 1u : 0u;
    const int is = (int) H.score - P;
    const AlignCell ins{(u32) is, H.start, H.consumed, H.matches};
    const bool ti = (is > 0) & align_gt(ins, V);
    V = align_pick(ti, ins, V);
    op = ti ? 2u : op;
    u32 dd = 0;
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const u32 s = 1u << t;
        if (s < k) {  // wave-uniform
            const AlignCell v = align_from(V, src[t]);
            const u32 vd = lane_read(dd, src[t]);
            const int cs = (int) v.score - P * (int) s;
            const AlignCell cand{(u32) cs, v.start, v.consumed + s, v.matches};
            const bool take = (cs > 0) & align_gt(cand, V);
            V = align_pick(take, cand, V);
            dd = take ? vd + s : dd;
        }
    }
    H = V;
    return op | (dd << 2) | (hit ? 128u : 0u);
}

// Rows from + 1 .. to of the table in which the lane's half starts from (0, my_start, 0, 0) at row my_start (from <=
// my_start); the byte of row i > keep goes to dst[(i - keep - 1) * 64 + lane].
__device__ __forceinline__ void trace_fill(const ReadRef &rd, u32 from, u32 to, u32 my_start, u32 tb, int P, u32 k, const u32 (&src)[5],
                                           unsigned char *dst, u32 keep, u32 lane) {
    AlignCell H{0, my_start, 0, 0};
    u32 lo = 0, hi = 0, nm = 0;
    for (u32 i = from + 1u; i <= to; i++) {
        const u32 p = i - 1u, b = p & 31u;
        if (b == 0u || p == from) {
            const u64 w = p >> 5;
            lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
        }
        const u32 c = ((lo >> b) & 1u) | (((hi >> b) & 1u) << 1) | (((nm >> b) & 1u) << 2);
        const u32 byte = trace_row(H, c, tb, i, P, k, src);
        H = align_pick(i <= my_start, AlignCell{0, my_start, 0, 0}, H);
        if (i > keep) dst[(u64) (i - keep - 1u) * 64ull + lane] = (unsigned char) byte;
    }
}

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
#pragma unroll
            for (int t = 0; t < 5; t++) {
                int q = ((int) j - (1 << t)) % (int) k;
                q = q < 0 ? q + (int) k : q;
                src[t] = (half | (u32) q) << 2;
            }
            // ---- pass 1: align's loop; the best cell of a lane also keeps its phase
            AlignCell H{0, 0, 0, 0}, best{0, 0, 0, 0};
            u32 best_end = 0, best_j = j;
            for (u32 w = 0; w < rd.nw; w++) {
                const u32 lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
                const u32 left = rd.len - (w << 5);  // >= 1
                const u32 nb = left < 32u ? left : 32u;
                for (u32 b = 0; b < nb; b++) {
                    const u32 i = (w << 5) + b + 1u;
                    const u32 c = ((lo >> b) & 1u) | (((hi >> b) & 1u) << 1) | (((nm >> b) & 1u) << 2);  // 4: an N
                    (void) trace_row(H, c, tb, i, P, k, src);
                    const bool up = live & (H.score > best.score);  // strictly: the earliest end stays
                    best = align_pick(up, H, best);
                    best_end = up ? i : best_end;
                }
            }
            // the largest (score, -end, start, consumed, matches, -phase) of each half, in every lane of the half
#pragma unroll
            for (u32 off = 16; off >= 1; off >>= 1) {
                const u32 from = (lane ^ off) << 2;
                const AlignCell o = align_from(best, from);
                const u32 o_end = lane_read(best_end, from), o_j = lane_read(best_j, from);
                const bool take = o.score != best.score ? o.score > best.score
                                : o_end != best_end     ? o_end < best_end
                                : align_gt(o, best)     ? true
                                : align_gt(best, o)     ? false
                                                        : o_j < best_j;
                best = align_pick(take, o, best);
                best_end = take ? o_end : best_end;
                best_j = take ? o_j : best_j;
            }
            u32 x = 0;
            auto put = [&](u32 q, u32 v) {
                const u32 rev = (u32) __builtin_amdgcn_readlane((int) v, 32);
                x = lane == q ? v : lane == 5u + q ? rev : x;
            };
            put(0, best.score);
            put(1, best.start);
            put(2, best_end);
            put(3, best.consumed);
            put(4, best.matches);
            if (lane < 10) out[(r * (u64) n_motifs + (u64) m) * 10ull + lane] = x;

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
                    trace_fill(rd, lo, hi, my_start, tb, P, k, src, ws, lo, lane);
                    __threadfence();  // other lanes of this wave read the rows back
                }
                for (u32 s = 0; s < 2; s++) {
                    if (!traced[s]) continue;
                    const u32 start = st[s], lane0 = s << 5;
                    u32 i = en[s], jj = js[s], seg_end = i, consumed = 0, sub = 0, ins = 0, del = 0, phase = 0, cols = 0, run = 0, run_start = 0;
                    u32 blk_lo = i;  // the block holds the rows blk_lo + 1 .. : none yet
                    u32 found = 0;
                    auto emit = [&](u32 e_start, u32 e_bases, u32 e_count, u32 e_phase, u32 e_consumed, u32 e_sub, u32 e_ins, u32 e_del) {
                        found++;
                        const u32 v = lane == 0u ? (u32) r : lane == 1u ? (u32) m : lane == 2u ? s : lane == 3u ? e_start : lane == 4u ? e_bases
                                    : lane == 5u ? e_count : lane == 6u ? e_phase : lane == 7u ? e_consumed : lane == 8u ? e_sub
                                    : lane == 9u ? e_ins : lane == 10u ? e_del : 0u;
                        log_append<kTraceWords>(lg.counter, lg.recs, lg.cap, v);
                    };
                    auto flush_run = [&]() {
                        if (run) emit(run_start, run * k, run, 0, run * k, 0, 0, 0);
                        run = 0;
                    };
                    auto close = [&]() {  // the running segment begins at read base i
                        if (phase == 0 && consumed == k && (sub | ins | del) == 0) {
                            run++;
                            run_start = i;
                        } else {
                            flush_run();
                            emit(i, seg_end - i, 1, phase, consumed, sub, ins, del);
                        }
                        seg_end = i;
                        consumed = sub = ins = del = phase = cols = 0;
                    };
                    while (i > start) {
                        if (i <= blk_lo) {  // the next block: the rows blk_lo + 1 .. i
                            blk_lo = i - start > kTraceBlock ? i - kTraceBlock : start;
                            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            if (fits) {
                                const u32 row = blk_lo + 1u + lane;
                                if (row <= i) {
                                    const uint4 *g = (const uint4 *) (ws + (u64) (row - lo - 1u) * 64ull);
                                    const uint4 a = g[0], b = g[1], c = g[2], d = g[3];
                                    blk4[lane * 4u + 0u] = a;
                                    blk4[lane * 4u + 1u] = b;
                                    blk4[lane * 4u + 2u] = c;
                                    blk4[lane * 4u + 3u] = d;
                                }
                            } else {
                                trace_fill(rd, start, i, my_start, tb, P, k, src, blk, blk_lo, lane);
                            }
                            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                        }
                        const unsigned char *row = blk + (i - blk_lo - 1u) * 64u + lane0;
                        const u32 d = rfl((u32) row[jj]) >> 2 & 31u;
                        for (u32 q = 0; q < d; q++) {
                            phase = jj;
                            consumed++, del++, cols++;
                            if (jj == 0) close();
                            jj = jj ? jj - 1u : k - 1u;
                        }
                        const u32 cell = rfl((u32) row[jj]);
                        const u32 op = cell & 3u;
                        if (op == 0) break;  // never: the fresh start lies in row `start`
                        i--;
                        cols++;
                        if (op == 1) {
                            phase = jj;
                            consumed++;
                            sub += (cell >> 7) ^ 1u;
                            if (jj == 0) close();
                            jj = jj ? jj - 1u : k - 1u;
                        } else {
                            ins++;
                        }
                    }
                    if (cols) close();
                    flush_run();
                    n_items[s] = found;
                }
            }
            if (lane < 2) counts[(r * (u64) n_motifs + (u64) m) * 2ull + lane] = lane ? n_items[1] : n_items[0];
        }
    }
}
