// kernels/monomers.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Wraparound alignment for units of up to 256 bases (trew_hip_monomers): trew_hip_alignment's definition, word for word, with
// 3 <= k <= TREW_MONOMER_MAX.  A kernel beside the scan and beside the other fifteen measures: it reads the batch's bit planes
// and its own table of (k, unit[16]) entries, writes only its own result buffer, uses no LDS memory, no worklist, no counter,
// no atomic and no pattern table.  The cell, its order, the selects, the lane read and the base's code are wraparound.inc's.
//
// Layout.  One strand's row is spread over all 64 lanes, Q phases a lane, blocked: lane l holds the phases Q l .. Q l + Q - 1
// in a register array that only unrolled constants index, a phase is live when it is below k.  Q = 1, 2, 4 is the smallest
// with 64 Q >= the largest k of the call.  The two strands of a monomer are walked one after the other.  No live phase ever
// reads a dead one: every source below is a lower phase, or phase k - 1.
//
// Row step (mono_row).  The diagonal of slot q > 0 is the lane's own slot q - 1 of the previous row; slot 0 reads slot Q - 1
// of lane l - 1; phase 0 reads phase k - 1, which sits in a wave-uniform lane and slot: that lane hands out this slot instead of
// its slot Q - 1 (nobody else reads that one: the lanes above it are dead), so the diagonal is one cell read a base whatever Q.
//
// Closure over d deleted unit bases, H[j] = max over d < k of V[(j - d) mod k] shifted by d (score - P d, consumed + d), in
// the linear-plus-wrap form:
//   (a) the linear prefix closure over the phases 0 .. k - 1 without the wrap, L[j] = max over j' <= j of V[j'] shifted by
//       j - j': serially over the slots of a lane; then the closed cell arriving at phase Q l - 1 for every lane l, an
//       exclusive scan of the lanes' last slots across lanes (the cell of lane l - 1, then doubling steps t = 1, 2, 4, ... below
//       the last live lane, a step shifts by Q t); then that carry, shifted by q + 1, into slot q;
//   (b) W = L[k - 1], wave-uniform (a v_readlane of the wave-uniform lane, the slot picked by wave-uniform selects);
//   (c) H[j] = max(L[j], W shifted by j + 1).
// Exactness.  Shifting by d is monotone in the tuple order (it changes score and consumed by the same amount on both sides),
// so the largest of shifted cells is the shifted largest cell, and steps compose: shifted by a, then by b, is shifted by
// a + b.  A source j' <= j is in L[j] with exactly d = j - j'; through W it would have gone a whole turn further, d + k, which
// scores P k lower and loses strictly.  A source j' > j is in W with k - 1 - j' and arrives with exactly d = j + k - j' < k.  So
// every d of the definition occurs and nothing else can win.  A candidate whose score is not positive is dropped at every step,
// as in wrap_row: it loses to the fresh start (0, i, 0, 0), which every V already holds, and it stays not positive under any
// further shift, so dropping early and dropping late are the same.
// The last live lane may have fewer than Q live slots: W is taken at its slot (k - 1) mod Q, and its dead slots, like the dead
// lanes, take part in nothing (they compute, nobody reads them, they keep no best cell).
//
// Best cell.  A lane first reduces its live slots of the row by the full tuple order (the end is the same), then keeps its
// own best under wrap_keep_best's strictly-larger-score rule, so the earliest end stays; one butterfly over the 64 lanes
// applies (score, -end, start, consumed, matches) at the end of the strand, and five lanes store the strand's half of the
// record: one vector store.

// V = max(V, v shifted by d deleted unit bases) where ok; a candidate that does not score is dropped
__device__ __forceinline__ void mono_take(AlignCell &V, const AlignCell &v, int P, u32 d, bool ok) {
    const int cs = (int) v.score - P * (int) d;
    const AlignCell cand{(u32) cs, v.start, v.consumed + d, v.matches};
    const bool take = ok & (cs > 0) & align_gt(cand, V);
    V = align_pick(take, cand, V);
}

// bit positions of a cell's direction byte (copies.inc): op in bits 0 .. 1 and hit in bit 7 as in wrap_row's byte, del in bit 2
constexpr u32 kMonoDel = 4u, kMonoHit = 128u;

// slot `slot` (wave-uniform) of a lane's cells: selects over the unrolled slots
template <int Q>
__device__ __forceinline__ AlignCell mono_slot(const AlignCell (&X)[Q], u32 slot) {
    AlignCell c = X[Q - 1];
#pragma unroll
    for (int q = 0; q < Q - 1; q++) c = align_pick(slot == (u32) q, X[q], c);
    return c;
}

// One row: H of row i - 1 -> H of row i for the read base c against the lane's unit bases tb.  last_lane, last_slot: where
// phase k - 1 sits; diag_src: the lane slot 0 takes its diagonal from, as a byte index (lane 0: last_lane).
// kDirs: the directions are kept and the byte of slot q is returned in bits [8 q, 8 q + 8) (0 without): op | del << 2 |
// hit << 7, op by the order of the selects as in wrap_row, del: H is strictly larger than V was in front of step (a) -- the
// smallest d of the cell is not 0 (the proof that one bit carries d stands at the head of copies.inc).
// mid(q, V[q], the diagonal was taken with a positive score and the inserted base did not beat it) runs per slot between the
// inserted-base select and step (a), where wrap_row has its own (polish.inc's vote); the default does nothing.
struct MonoNoMid {
    __device__ __forceinline__ void operator()(int, const AlignCell &, bool) const {}
};
template <int Q, bool kDirs, class Mid = MonoNoMid>
__device__ __forceinline__ u32 mono_row(AlignCell (&H)[Q], u32 c, const u32 (&tb)[Q], u32 i, int P, u32 lane, u32 diag_src, u32 last_lane,
                                         u32 last_slot, Mid mid = Mid{}) {
    const AlignCell mine = align_pick(lane == last_lane, mono_slot<Q>(H, last_slot), H[Q - 1]);
    const AlignCell prev = align_from(mine, diag_src);
    AlignCell V[Q], V0[kDirs ? Q : 1];
    u32 dirs = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const AlignCell d = q ? H[q ? q - 1 : 0] : prev;
        const bool hit = c == tb[q];
        const int ds = hit ? (int) d.score + 1 : (int) d.score - P;
        V[q] = align_pick(ds > 0, AlignCell{(u32) ds, d.start, d.consumed + 1u, d.matches + (hit ? 1u : 0u)}, AlignCell{0, i, 0, 0});
        const int is = (int) H[q].score - P;
        const AlignCell ins{(u32) is, H[q].start, H[q].consumed, H[q].matches};
        const bool by_ins = (is > 0) & align_gt(ins, V[q]);
        V[q] = align_pick(by_ins, ins, V[q]);
        mid(q, V[q], (ds > 0) & !by_ins);
        if constexpr (kDirs) {
            V0[q] = V[q];
            dirs |= ((by_ins ? 2u : ds > 0 ? 1u : 0u) | (hit ? kMonoHit : 0u)) << (8 * q);
        }
    }
    // (a) inside the lane, then across the lanes: C is the closed cell of phase Q lane - 1 (lane 0: none)
#pragma unroll
    for (int q = 1; q < Q; q++) mono_take(V[q], V[q - 1], P, 1u, true);
    AlignCell C = align_from(V[Q - 1], (lane - 1u) << 2);
    C = align_pick(lane == 0u, AlignCell{0, 0, 0, 0}, C);
#pragma unroll
    for (u32 t = 1; t < 64u; t <<= 1)
        if (t < last_lane) {  // wave-uniform
            const AlignCell o = align_from(C, (lane - t) << 2);
            mono_take(C, o, P, (u32) Q * t, lane >= t);
        }
#pragma unroll
    for (int q = 0; q < Q; q++) mono_take(V[q], C, P, (u32) q + 1u, true);
    // (b) the closed cell of phase k - 1, (c) round the wrap
    const AlignCell wl = mono_slot<Q>(V, last_slot);
    const AlignCell W{(u32) __builtin_amdgcn_readlane((int) wl.score, (int) last_lane), (u32) __builtin_amdgcn_readlane((int) wl.start, (int) last_lane),
                      (u32) __builtin_amdgcn_readlane((int) wl.consumed, (int) last_lane),
                      (u32) __builtin_amdgcn_readlane((int) wl.matches, (int) last_lane)};
#pragma unroll
    for (int q = 0; q < Q; q++) {
        mono_take(V[q], W, P, (u32) Q * lane + (u32) q + 1u, true);
        H[q] = V[q];
        if constexpr (kDirs) dirs |= (align_gt(V[q], V0[q]) ? kMonoDel : 0u) << (8 * q);
    }
    return dirs;
}

// the largest (score, -end, start, consumed, matches[, -phase]) of the wave, in every lane: one butterfly
template <bool kPhase>
__device__ __forceinline__ void mono_reduce_wave(AlignCell &best, u32 &best_end, u32 &best_j) {
    const u32 lane = lane_id();
#pragma unroll
    for (u32 off = 32; off >= 1; off >>= 1) {
        const u32 from = (lane ^ off) << 2;
        const AlignCell o = align_from(best, from);
        const u32 o_end = lane_read(best_end, from);
        bool take = o.score != best.score ? o.score > best.score : o_end != best_end ? o_end < best_end : align_gt(o, best);
        if constexpr (kPhase) {
            const u32 o_j = lane_read(best_j, from);
            const bool same = (o.score == best.score) & (o_end == best_end) & !align_gt(o, best) & !align_gt(best, o);
            take = same ? o_j < best_j : take;
            best_j = take ? o_j : best_j;
        }
        best = align_pick(take, o, best);
        best_end = take ? o_end : best_end;
    }
}

template <int Q>
__global__ void __launch_bounds__(256) monomers_wave_kernel(DevBatch B, const trew_hip_monomer *__restrict__ mt, int n_monomers, int penalty,
                                                            u32 *__restrict__ out) {
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    const u32 lane = lane_id();
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_monomers; m++) {
            const trew_hip_monomer *mm = mt + m;
            const u32 k = rfl((u32) mm->k);  // 3 .. 64 Q
            const u32 last_lane = (k - 1u) / (u32) Q, last_slot = (k - 1u) % (u32) Q;
            const u32 diag_src = (lane == 0u ? last_lane : lane - 1u) << 2;
            for (u32 strand = 0; strand < 2u; strand++) {
                // base p of the strand's target: the unit's base p, or the complement of its base k - 1 - p; a dead phase matches nothing
                u32 tb[Q];
                bool live[Q];
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const u32 p = (u32) Q * lane + (u32) q;
                    live[q] = p < k;
                    const u32 j = !live[q] ? 0u : strand ? k - 1u - p : p;  // < 256
                    const u32 code = (mm->unit[j >> 4] >> (2u * (j & 15u))) & 3u;
                    tb[q] = !live[q] ? 8u : strand ? 3u - code : code;
                }
                AlignCell H[Q], best{0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < Q; q++) H[q] = AlignCell{0, 0, 0, 0};
                u32 best_end = 0, no_phase = 0;
                for (u32 w = 0; w < rd.nw; w++) {
                    const u32 lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
                    const u32 left = rd.len - (w << 5);  // >= 1
                    const u32 nb = left < 32u ? left : 32u;
                    for (u32 b = 0; b < nb; b++) {
                        const u32 i = (w << 5) + b + 1u;
                        mono_row<Q, false>(H, base_code(lo, hi, nm, b), tb, i, P, lane, diag_src, last_lane, last_slot);
                        AlignCell top = H[0];
#pragma unroll
                        for (int q = 1; q < Q; q++) top = align_pick(live[q] & align_gt(H[q], top), H[q], top);
                        wrap_keep_best(top, i, live[0], best, best_end);
                    }
                }
                mono_reduce_wave<false>(best, best_end, no_phase);
                const u32 x = lane == 0u ? best.score : lane == 1u ? best.start : lane == 2u ? best_end : lane == 3u ? best.consumed : best.matches;
                if (lane < 5u) out[(r * (u64) n_monomers + (u64) m) * 10ull + 5ull * strand + lane] = x;
            }
        }
    }
}
