// kernels/align.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Indel-aware motif tract per read (trew_hip_align): a local alignment of the read against the motif repeated without end,
// wraparound dynamic programming.  A kernel beside the scan and beside the other eight measures: it reads the same bit planes
// and pattern tables, writes only its own result buffer, uses no LDS memory, no worklist, no counter and no table.
//
// Definition (DESIGN 4.7e, include/trew_hip.h).  A cell holds (score, start, consumed, matches), compared in this order, the
// larger wins.  Row i of the table follows from row i - 1 alone: V[i][j] is the largest of the fresh start (0, i, 0, 0), the
// diagonal from H[i-1][(j-1) mod k] (+1 on a match, -P otherwise, one motif base consumed) and the inserted read base from
// H[i-1][j] (-P); H[i][j] is the largest of V[i][(j-d) mod k] with d < k deleted motif bases at -P each.
//
// Wave per read, for every length.  The row lives in registers: lanes 0 .. 31 hold the phases j of strand fwd, lanes 32 .. 63
// those of strand rev, lanes with (lane & 31) >= k are idle (no lane ever reads from them and they keep no best cell).  The
// read's base is wave-uniform, its plane words are read once per 32 bases.  Per base one row step, wrap_row of
// kernels/wraparound.inc: one cyclic neighbour read for the diagonal (ds_bpermute moves registers between lanes through the
// LDS crossbar without touching LDS memory), then the maximum over d as doubling steps s = 1, 2, 4, ... < k on the cyclic
// order, H[j] = max(H[j], H[(j-s) mod k] shifted by s): every d < k is a sum of distinct steps below k, and a candidate that
// went more than once round the motif is the same cell P k cheaper, so it never wins.  Scores in a row are never negative
// (the fresh start is always a candidate): a candidate whose score is not positive is dropped, which is exact because
// (0, b, ., .) with b < i loses to the fresh start (0, i, 0, 0).  Each lane keeps its own best cell, taking a new one only
// when it scores strictly higher, so the earliest end survives inside a lane (wrap_keep_best); one butterfly over the 32
// lanes of each half applies (score, -end, start, consumed, matches) at the end (wrap_reduce_half).  The cell, the row step,
// the butterfly and the record's store are wraparound.inc's, shared with refine.inc, trace.inc and decompose.inc.

__global__ void __launch_bounds__(256) align_wave_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, int penalty,
                                                         u32 *__restrict__ out) {
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    const u32 lane = lane_id();
    const u32 j = lane & 31u;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_motifs; m++) {
            const AnnotMotifDev *mm = mt + m;
            const u32 k = rfl(mm->k);
            const bool live = j < k;
            // base j of the strand's target: phase 0 of the pattern table holds it in bit j; an idle lane matches nothing
            const u32 strand = lane >> 5;
            const u32 tb = live ? ((mm->plo[strand][0] >> j) & 1u) | (((mm->phi[strand][0] >> j) & 1u) << 1) : 8u;
            u32 src[5];
            wrap_sources(k, src);
            AlignCell H{0, 0, 0, 0}, best{0, 0, 0, 0};
            u32 best_end = 0;
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
            u32 none = 0;
            wrap_reduce_half<false>(best, best_end, none);
            wrap_store_alignment(out + (r * (u64) n_motifs + (u64) m) * 10ull, best, best_end);
        }
    }
}
