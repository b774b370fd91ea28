// kernels/wraparound.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// The wraparound alignment of DESIGN 4.7e as the measures of its family use it (align.inc, refine.inc and through it
// tandems.inc, trace.inc, decompose.inc): the cell, the row step, the best cell of a half, and for the measures that walk the
// path back (4.7h, 4.7i) the rows of direction bytes and the walk over them.  No kernel here; plain C++ and builtins.
//
//   AlignCell, align_gt, align_pick, lane_read, align_from   the cell, its order, selects and lane reads
//   wrap_sources, base_code    the lanes a lane reads from; a read base's code out of its plane words
//   wrap_row                   H of row i - 1 -> H of row i, with the direction byte when asked for
//   wrap_keep_best, wrap_reduce_half, wrap_store_alignment   the best cell: per lane, per half, as a trew_hip_alignment
//   wrap_fill, wrap_fetch      the direction bytes of a range of rows: computed, or brought from the workspace into LDS
//   wrap_walk                  from the end cell down to the fresh start: the items of trew_hip_trace_item (copies.inc walks
//                              its own rows with it: the row size, the rows of a block and the decoder are template parameters)
//
// Layout.  The row lives in registers: lanes 0 .. 31 hold the phases j of one strand, lanes 32 .. 63 those of the other (or
// mirror them), lanes with (lane & 31) >= k are idle: no lane ever reads from them and they keep no best cell.  No lane read
// leaves its half.  Everything around a lane read is a select, so the lanes of a wave stay together.

struct AlignCell {
    u32 score, start, consumed, matches;
};

// a > b, field by field in the order of the struct
__device__ __forceinline__ bool align_gt(const AlignCell &a, const AlignCell &b) {
    const u64 a0 = ((u64) a.score << 32) | a.start, b0 = ((u64) b.score << 32) | b.start;
    const u64 a1 = ((u64) a.consumed << 32) | a.matches, b1 = ((u64) b.consumed << 32) | b.matches;
    return (a0 > b0) | ((a0 == b0) & (a1 > b1));
}

// t ? a : b, field by field: selects, no control flow (the lanes of a wave stay together for the lane reads)
__device__ __forceinline__ AlignCell align_pick(bool t, const AlignCell &a, const AlignCell &b) {
    return AlignCell{t ? a.score : b.score, t ? a.start : b.start, t ? a.consumed : b.consumed, t ? a.matches : b.matches};
}

__device__ __forceinline__ u32 lane_read(u32 v, u32 byte_index) { return (u32) __builtin_amdgcn_ds_bpermute((int) byte_index, (int) v); }
// the cell of the lane whose index is byte_index / 4
__device__ __forceinline__ AlignCell align_from(const AlignCell &c, u32 byte_index) {
    return AlignCell{lane_read(c.score, byte_index), lane_read(c.start, byte_index), lane_read(c.consumed, byte_index), lane_read(c.matches, byte_index)};
}

// the lanes this one reads from, as byte indices: (j - 1) mod k for the diagonal, (j - s) mod k for the doubling steps s = 2^t
__device__ __forceinline__ void wrap_sources(u32 k, u32 (&src)[5]) {
    const u32 j = lane_id() & 31u, half = lane_id() & 32u;
#pragma unroll
    for (int t = 0; t < 5; t++) {
        int q = ((int) j - (1 << t)) % (int) k;
        q = q < 0 ? q + (int) k : q;
        src[t] = (half | (u32) q) << 2;
    }
}

// the code of base b of a 32-base word of the planes: 0 .. 3, 4: an N
__device__ __forceinline__ u32 base_code(u32 lo, u32 hi, u32 nm, u32 b) { return ((lo >> b) & 1u) | (((hi >> b) & 1u) << 1) | (((nm >> b) & 1u) << 2); }

// One row: H of row i - 1 -> H of row i for the read base c against the lane's unit base tb, the doubling steps below k only.
// One cyclic neighbour read for the diagonal, then the maximum over d deleted unit bases as steps s = 1, 2, 4, ... < k,
// H[j] = max(H[j], H[(j - s) mod k] shifted by s); a candidate whose score is not positive is dropped (it loses to the fresh
// start).  kDirs: the directions are kept and op | d << 2 | hit << 7 of the lane's cell is returned (0 without), under the tie
// rules whose proof stands at the head of trace.inc.  mid(V, diagonal taken, inserted base taken, c) runs between the
// inserted-base select and the doubling steps (refine.inc's vote).
struct WrapNoMid {
    __device__ __forceinline__ void operator()(const AlignCell &, bool, bool, u32) const {}
};
template <bool kDirs, class Mid = WrapNoMid>
__device__ __forceinline__ u32 wrap_row(AlignCell &H, u32 c, u32 tb, u32 i, int P, u32 k, const u32 (&src)[5], Mid mid = Mid{}) {
    const bool hit = c == tb;
    const AlignCell d = align_from(H, src[0]);
    const int ds = hit ? (int) d.score + 1 : (int) d.score - P;
    AlignCell V = align_pick(ds > 0, AlignCell{(u32) ds, d.start, d.consumed + 1u, d.matches + (hit ? 1u : 0u)}, AlignCell{0, i, 0, 0});
    const int is = (int) H.score - P;
    const AlignCell ins{(u32) is, H.start, H.consumed, H.matches};
    const bool by_ins = (is > 0) & align_gt(ins, V);
    V = align_pick(by_ins, ins, V);
    mid(V, ds > 0, by_ins, c);
    u32 dd = 0;
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const u32 s = 1u << t;
        if (s < k) {  // wave-uniform
            const AlignCell v = align_from(V, src[t]);
            const int cs = (int) v.score - P * (int) s;
            const AlignCell cand{(u32) cs, v.start, v.consumed + s, v.matches};
            const bool take = (cs > 0) & align_gt(cand, V);
            V = align_pick(take, cand, V);
            if constexpr (kDirs) {
                const u32 vd = lane_read(dd, src[t]);
                dd = take ? vd + s : dd;
            }
        }
    }
    H = V;
    if constexpr (!kDirs) return 0u;
    return (by_ins ? 2u : ds > 0 ? 1u : 0u) | (dd << 2) | (hit ? 128u : 0u);
}

// a live lane keeps its own best cell, taking a new one only when it scores strictly higher: the earliest end stays
__device__ __forceinline__ void wrap_keep_best(const AlignCell &H, u32 i, bool live, AlignCell &best, u32 &best_end) {
    const bool up = live & (H.score > best.score);
    best = align_pick(up, H, best);
    best_end = up ? i : best_end;
}

// the largest (score, -end, start, consumed, matches[, -phase]) of each half, in every lane of the half: one butterfly
template <bool kPhase>
__device__ __forceinline__ void wrap_reduce_half(AlignCell &best, u32 &best_end, u32 &best_j) {
    const u32 lane = lane_id();
#pragma unroll
    for (u32 off = 16; off >= 1; off >>= 1) {
        const u32 from = (lane ^ off) << 2;
        const AlignCell o = align_from(best, from);
        const u32 o_end = lane_read(best_end, from);
        const u32 o_j = kPhase ? lane_read(best_j, from) : 0u;
        const bool take = o.score != best.score ? o.score > best.score
                        : o_end != best_end     ? o_end < best_end
                        : align_gt(o, best)     ? true
                        : !kPhase               ? false
                        : align_gt(best, o)     ? false
                                                : o_j < best_j;
        best = align_pick(take, o, best);
        best_end = take ? o_end : best_end;
        if constexpr (kPhase) best_j = take ? o_j : best_j;
    }
}

// ten lanes write the ten words of a trew_hip_alignment (lanes 0 .. 4 the half of lane 0, lanes 5 .. 9 that of lane 32): one vector store
__device__ __forceinline__ void wrap_store_alignment(u32 *__restrict__ out, const AlignCell &best, u32 best_end) {
    const u32 lane = lane_id();
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
    if (lane < 10) out[lane] = x;
}

constexpr u32 kTraceBlock = 64;  // rows of the walk's LDS block: kRowBytes * 64 bytes a wave
constexpr u32 kTraceWords = 12;  // trew_hip_trace_item

// Rows from + 1 .. to of the table in which the lane's half starts from (0, my_start, 0, 0) at row my_start (from <=
// my_start); the lanes below kRowBytes store the byte of row i > keep at dst[(i - keep - 1) * kRowBytes + lane].  Returns H of
// row `to`.
template <u32 kRowBytes>
__device__ __forceinline__ AlignCell wrap_fill(const ReadRef &rd, u32 from, u32 to, u32 my_start, u32 tb, int P, u32 k, const u32 (&src)[5],
                                               unsigned char *dst, u32 keep) {
    const u32 lane = lane_id();
    AlignCell H{0, my_start, 0, 0};
    u32 lo = 0, hi = 0, nm = 0;
    for (u32 i = from + 1u; i <= to; i++) {
        const u32 p = i - 1u, b = p & 31u;
        if (b == 0u || p == from) {
            const u64 w = p >> 5;
            lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
        }
        const u32 byte = wrap_row<true>(H, base_code(lo, hi, nm, b), tb, i, P, k, src);
        H = align_pick(i <= my_start, AlignCell{0, my_start, 0, 0}, H);
        if (i > keep && lane < kRowBytes) dst[(u64) (i - keep - 1u) * kRowBytes + lane] = (unsigned char) byte;
    }
    return H;
}

// Rows blk_lo + 1 .. i out of the workspace whose first row is ws_lo + 1 into the wave's LDS block: a lane fetches a row
template <u32 kRowBytes>
__device__ __forceinline__ void wrap_fetch(const unsigned char *ws, u32 ws_lo, uint4 *blk4, u32 blk_lo, u32 i) {
    struct alignas(16) Row {
        uint4 q[kRowBytes / 16u];
    };
    const u32 lane = lane_id(), row = blk_lo + 1u + lane;
    if (row <= i) ((Row *) blk4)[lane] = *(const Row *) (ws + (u64) (row - ws_lo - 1u) * kRowBytes);
}

// The walk from the end cell (row en, phase jj) down to the fresh start in row `start`, wave-uniform, and its items: words 0
// .. 2 of each are (w_read, w_motif, w_strand).  It goes down a row a step, so the rows come a block of kTraceBlock at a time
// into LDS and a step is two LDS byte reads: refill(blk_lo, i) brings the rows blk_lo + 1 .. i to blk (row x at (x - blk_lo -
// 1) * kRowBytes), and may set jj while it brings the first block.  Items appear last to first: a segment closes at its first
// column, a run of complete exact copies is emitted when a segment that is none closes behind it.  One returning atomic an
// item on the log's counter, twelve lanes store its words, nothing at or beyond the capacity while the counter keeps
// counting.  Returns the number of items.
// kBlock: the rows of a block.  kDelBit (copies.inc): bits 2 .. 6 of a byte hold not d but whether d > 0, and the walk emits one
// `del` column and looks again until the bit is clear.
template <u32 kRowBytes, u32 kBlock = kTraceBlock, bool kDelBit = false, class Refill>
__device__ __forceinline__ u32 wrap_walk(const TraceLog &lg, u32 w_read, u32 w_motif, u32 w_strand, u32 k, u32 start, u32 en, u32 &jj,
                                         const unsigned char *blk, Refill refill) {
    const u32 lane = lane_id();
    u32 i = en, seg_end = i, consumed = 0, sub = 0, ins = 0, del = 0, phase = 0, cols = 0, run = 0, run_start = 0;
    u32 blk_lo = i;  // the block holds the rows blk_lo + 1 .. : none yet
    u32 found = 0;
    auto emit = [&](u32 e_start, u32 e_bases, u32 e_count, u32 e_phase, u32 e_consumed, u32 e_sub, u32 e_ins, u32 e_del) {
        found++;
        const u32 v = lane == 0u ? w_read : lane == 1u ? w_motif : lane == 2u ? w_strand : lane == 3u ? e_start : lane == 4u ? e_bases
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
            blk_lo = i - start > kBlock ? i - kBlock : start;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            refill(blk_lo, i);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        const unsigned char *row = blk + (i - blk_lo - 1u) * kRowBytes;
        auto del_column = [&]() {
            phase = jj;
            consumed++, del++, cols++;
            if (jj == 0) close();
            jj = jj ? jj - 1u : k - 1u;
        };
        if constexpr (kDelBit) {
            while (rfl((u32) row[jj]) >> 2 & 31u) del_column();
        } else {
            const u32 d = rfl((u32) row[jj]) >> 2 & 31u;
            for (u32 q = 0; q < d; q++) del_column();
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
    return found;
}
