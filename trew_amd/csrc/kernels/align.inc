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
// read's base is wave-uniform, its plane words are read once per 32 bases.  Per base: one cyclic neighbour read for the
// diagonal (ds_bpermute moves registers between lanes through the LDS crossbar without touching LDS memory), then the maximum
// over d as doubling steps s = 1, 2, 4, ... < k on the cyclic order, H[j] = max(H[j], H[(j-s) mod k] shifted by s): every
// d < k is a sum of distinct steps below k, and a candidate that went more than once round the motif is the same cell P k
// cheaper, so it never wins.  Scores in a row are never negative (the fresh start is always a candidate): a candidate whose
// score is not positive is dropped, which is exact because (0, b, ., .) with b < i loses to the fresh start (0, i, 0, 0).
// Each lane keeps its own best cell, taking a new one only when it scores strictly higher, so the earliest end survives
// inside a lane; one butterfly over the 32 lanes of each half applies (score, -end, start, consumed, matches) at the end.

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

__global__ void __launch_bounds__(256) align_wave_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, int penalty,
                                                         u32 *__restrict__ out) {
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    const u32 lane = lane_id();
    const u32 j = lane & 31u, half = lane & 32u;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_motifs; m++) {
            const AnnotMotifDev *mm = mt + m;
            const u32 k = rfl(mm->k);
            const bool live = j < k;
            // base j of the strand's target: phase 0 of the pattern table holds it in bit j; an idle lane matches nothing
            const u32 strand = lane >> 5;
            const u32 tb = live ? ((mm->plo[strand][0] >> j) & 1u) | (((mm->phi[strand][0] >> j) & 1u) << 1) : 8u;
            // the lanes this one reads from: (j - 1) mod k for the diagonal, (j - s) mod k for the doubling steps
            u32 src[5];
#pragma unroll
            for (int t = 0; t < 5; t++) {
                int q = ((int) j - (1 << t)) % (int) k;
                q = q < 0 ? q + (int) k : q;
                src[t] = (half | (u32) q) << 2;
            }
            AlignCell H{0, 0, 0, 0}, best{0, 0, 0, 0};
            u32 best_end = 0;
            for (u32 w = 0; w < rd.nw; w++) {
                const u32 lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
                const u32 left = rd.len - (w << 5);  // >= 1
                const u32 nb = left < 32u ? left : 32u;
                for (u32 b = 0; b < nb; b++) {
                    const u32 i = (w << 5) + b + 1u;
                    const u32 c = ((lo >> b) & 1u) | (((hi >> b) & 1u) << 1) | (((nm >> b) & 1u) << 2);  // 4: an N
                    const bool hit = c == tb;
                    const AlignCell d = align_from(H, src[0]);
                    const int ds = hit ? (int) d.score + 1 : (int) d.score - P;
                    AlignCell V = align_pick(ds > 0, AlignCell{(u32) ds, d.start, d.consumed + 1u, d.matches + (hit ? 1u : 0u)}, AlignCell{0, i, 0, 0});
                    const int is = (int) H.score - P;
                    const AlignCell ins{(u32) is, H.start, H.consumed, H.matches};
                    V = align_pick((is > 0) & align_gt(ins, V), ins, V);
#pragma unroll
                    for (int t = 0; t < 5; t++) {
                        const u32 s = 1u << t;
                        if (s < k) {  // wave-uniform
                            const AlignCell v = align_from(V, src[t]);
                            const int cs = (int) v.score - P * (int) s;
                            const AlignCell cand{(u32) cs, v.start, v.consumed + s, v.matches};
                            V = align_pick((cs > 0) & align_gt(cand, V), cand, V);
                        }
                    }
                    H = V;
                    const bool up = live & (H.score > best.score);  // strictly: the earliest end stays
                    best = align_pick(up, H, best);
                    best_end = up ? i : best_end;
                }
            }
            // the largest (score, -end, start, consumed, matches) of each half, in every lane of the half
#pragma unroll
            for (u32 off = 16; off >= 1; off >>= 1) {
                const u32 from = (lane ^ off) << 2;
                const AlignCell o = align_from(best, from);
                const u32 o_end = lane_read(best_end, from);
                const bool take = o.score != best.score ? o.score > best.score
                                : o_end != best_end     ? o_end < best_end
                                                        : align_gt(o, best);
                best = align_pick(take, o, best);
                best_end = take ? o_end : best_end;
            }
            // ten lanes write the record's ten words (trew_hip_alignment): one vector store
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
        }
    }
}
