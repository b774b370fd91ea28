// kernels/polish.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// De novo repeats under indels for periods up to 256 (trew_hip_polish): refine.inc's seed, align, vote and re-vote with
// satellites.inc's step 1 and monomers.inc's row.  A kernel beside the scan and beside the other seventeen measures: it reads
// the same bit planes, takes no pattern table and writes only its own records.  4 KiB of LDS per wave (the consensus bins of
// satellites.inc), all zero on entry and on exit of every stage; no worklist, no counter, no atomic of its own.
//
// Definition: DESIGN 4.7o, include/trew_hip.h (trew_hip_polished).  Wave per read, for every length.
//
// Layout.  monomers.inc's: Q = 1, 2, 4 phases a lane, blocked (lane l: phases Q l .. Q l + Q - 1), Q the smallest with
// 64 Q >= max_period of the call; a read whose period is small runs on the call's layout, its last live lane then has fewer
// than Q live slots and the lanes above it are dead.
//
// Stage 1 is satellite_record's k loop with period_score<true>, then period_locate<true> and satellite_consensus, as they are.
// The unreduced consensus is in the lanes, phase lane + 64 s in bits [2 s, 2 s + 2).
//
// Stage 2 (seed).  refine_longest_run<true> over the eq words of the scored k.  The consensus codes go to the first 256 words
// of the bins, one word a phase (as satellite_record does for its root); lane l loads the bases rs + Q l + q of its slots from
// the planes, an N takes word (pos - start) mod k.  S0 goes to the words 256 .. 511, where every lane reaches phase
// (j + c) mod k for the divisor loop of satellite_record.  tb[q] = S0's base below seed_period, 8 above.
//
// Stages 3 to 6.  polish_pass is the base loop of monomers_wave_kernel with mono_row<Q, false> over [lo, hi) of the read taken
// as a read of its own; the kernel holds one copy of it in a loop of three wave-uniform passes (align against S, vote over
// A1's tract, align against U), not three inlined copies.  The vote runs in mono_row's `mid`: a lane reduces the V cells of its
// live slots by the tuple order, the smallest slot on a tie; four wave maxima, field by field over the lanes still tied
// (refine_pass's), and the lowest set bit of the ballot give the lane; its smallest tied slot is the phase, which the blocked
// layout makes the smallest phase.  A dead slot of the last live lane and the dead lanes never take part.  The counters
// cnt[Q][4] live in the lane; slots are indexed by unrolled selects only.
//
// Re-vote, root and pack go through the bins; 44 lanes store the record with one vector store.

constexpr u32 kPolishWords = 44;  // trew_hip_polished: twelve words, unit[16], seed_unit[16]
static_assert(TREW_POLISH_MAX_PERIOD == kSatelliteMaxPeriod, "step 1, the bins and the layouts are satellites' and monomers'");
static_assert(sizeof(trew_hip_polished) == 4u * kPolishWords, "the record's words");

__device__ __forceinline__ void polish_sync() {
    // the wave's own LDS operations complete in program order; the fences keep the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the length of the primitive root of the unit whose base j is word j of g (j < k) and x[q] in its lane's slot q; wave-uniform
template <int Q>
__device__ __forceinline__ u32 polish_root(const u32 *g, const u32 (&x)[Q], u32 k) {
    const u32 lane = lane_id();
    for (u32 c = 1; 2u * c <= k; c++) {  // a proper divisor is at most k / 2
        if (k % c) continue;
        bool differs = false;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const u32 j = (u32) Q * lane + (u32) q;
            if (j < k) {
                const u32 src = j + c >= k ? j + c - k : j + c;  // (j + c) mod k
                differs |= g[src] != x[q];
            }
        }
        if (__ballot(differs) == 0ull) return c;
    }
    return k;
}

// One pass of monomers' recurrence over the bases [lo_pos, hi_pos) of the read, taken as a read of their own, against the
// unit tb (8 in a dead slot) of length k: the best cell as monomers_wave_kernel finds it, in every lane; start and end count
// from lo_pos.  vote (wave-uniform): the pass decodes into cnt.  The one copy of the row step serves all three passes, so the
// lane's reduction of its slots (selects) runs in the two alignment passes as well; only the wave maxima, the ballot and the
// counters are behind `vote`.
template <int Q>
__device__ __forceinline__ void polish_pass(const ReadRef &rd, u32 lo_pos, u32 hi_pos, const u32 (&tb)[Q], u32 k, int P, bool vote, AlignCell &best,
                                            u32 &best_end, u32 (&cnt)[Q][4]) {
    const u32 lane = lane_id();
    const u32 last_lane = (k - 1u) / (u32) Q, last_slot = (k - 1u) % (u32) Q;
    const u32 diag_src = (lane == 0u ? last_lane : lane - 1u) << 2;
    bool live[Q];
    AlignCell H[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        live[q] = (u32) Q * lane + (u32) q < k;
        H[q] = AlignCell{0, 0, 0, 0};
    }
    best = AlignCell{0, 0, 0, 0};
    best_end = 0;
    u32 no_phase = 0;
    for (u32 w = lo_pos >> 5; ((u64) w << 5) < (u64) hi_pos; w++) {
        const u32 lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
        const u32 b0 = w == (lo_pos >> 5) ? lo_pos & 31u : 0u;
        const u32 left = hi_pos - (w << 5);  // >= 1
        const u32 nb = left < 32u ? left : 32u;
        for (u32 b = b0; b < nb; b++) {
            const u32 i = (w << 5) + b + 1u - lo_pos;
            const u32 c = base_code(lo, hi, nm, b);
            AlignCell bv{0, 0, 0, 0};  // the lane's largest V, its slot, and whether the diagonal is that cell
            u32 bs = 0;
            bool bd = false;
            mono_row<Q, false>(H, c, tb, i, P, lane, diag_src, last_lane, last_slot, [&](int q, const AlignCell &V, bool diag) __attribute__((always_inline)) {
                bool mine = false;
#pragma unroll
                for (int s = 0; s < Q; s++) mine |= (q == s) & live[s];
                const bool take = q == 0 || (mine & align_gt(V, bv));  // strictly: the smallest slot keeps a tie
                bv = align_pick(take, V, bv);
                bs = take ? (u32) q : bs;
                bd = take ? diag : bd;
                if (q == Q - 1 && vote) {  // every slot seen; wave-uniform
                    // the phase with the largest V, the smallest on a tie: the lanes still tied, field by field
                    bool tie = live[0] & (bv.score == wave_max_u32(live[0] ? bv.score : 0u));
                    tie &= bv.start == wave_max_u32(tie ? bv.start : 0u);
                    tie &= bv.consumed == wave_max_u32(tie ? bv.consumed : 0u);
                    tie &= bv.matches == wave_max_u32(tie ? bv.matches : 0u);
                    const u32 ls = (u32) __builtin_ctzll(__ballot(tie));  // a live lane is always left
                    const bool voted = (lane == ls) & bd;
#pragma unroll
                    for (int s = 0; s < Q; s++)
#pragma unroll
                        for (u32 x = 0; x < 4u; x++) cnt[s][x] += (voted & (bs == (u32) s) & (c == x)) ? 1u : 0u;
                }
            });
            AlignCell top = H[0];
#pragma unroll
            for (int q = 1; q < Q; q++) top = align_pick(live[q] & align_gt(H[q], top), H[q], top);
            wrap_keep_best(top, i, live[0], best, best_end);
        }
    }
    mono_reduce_wave<false>(best, best_end, no_phase);
}

template <int Q>
__global__ void __launch_bounds__(256) polish_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, u32 *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) u32 bins[4][kSatelliteBins];
    const u32 lane = lane_id();
    u32 *h = bins[threadIdx.x >> 6];
    satellite_clear(h);
    polish_sync();
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    const u32 kmin = (u32) rfl_i(min_period), kmax = min((u32) rfl_i(max_period), 64u * (u32) Q);  // the layout holds no more
    const u32 smin = rfl(min_score);
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        const Piece pc{0u, rd.len};
        u32 rec[12];
#pragma unroll
        for (int i = 0; i < 12; i++) rec[i] = 0;
        u32 unit_word = 0;  // lanes 12 .. 43: unit[lane - 12], seed_unit[lane - 28]
        // 1. periods: the scored k
        u32 score = 0, k = 0;
        for (u32 kk = kmin; kk <= kmax && kk < rd.len; kk++) {
            const u32 sc = period_score<true>(rd, pc, kk, P);
            if (sc > score) {  // strictly: the smallest k keeps a tie
                score = sc;
                k = kk;
            }
        }
        if (k != 0u && score >= smin) {  // wave-uniform; a zero record otherwise
            u32 b, e;
            period_locate<true>(rd, pc, k, P, score, b, e);
            const u32 start = b, end = e + k;
            u32 cons, cons_support;
            satellite_consensus(rd, k, start, end, h, cons, cons_support);
            // 2. seed: the k bases at the longest run, an N replaced by its phase of the consensus
            const u32 rs = refine_longest_run<true>(rd, pc, k, b, e);
#pragma unroll
            for (u32 s = 0; s < 4u; s++) h[lane + 64u * s] = (cons >> (2u * s)) & 3u;
            polish_sync();
            u32 S[Q], tb[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const u32 j = (u32) Q * lane + (u32) q;
                S[q] = 8u;
                if (j < k) {
                    const u32 pos = rs + j;  // < end <= n
                    const u32 w = pos >> 5, bit = pos & 31u;
                    const u32 c0 = rd.w[3ull * w + 0], c1 = rd.w[3ull * w + 1], c2 = rd.w[3ull * w + 2];
                    const u32 cu = h[(pos - start) % k];
                    S[q] = (c2 >> bit) & 1u ? cu : ((c0 >> bit) & 1u) | (((c1 >> bit) & 1u) << 1);
                    h[kSatelliteMaxPeriod + j] = S[q];
                }
            }
            polish_sync();
            const u32 ks = polish_root<Q>(h + kSatelliteMaxPeriod, S, k);
            polish_sync();
            satellite_clear(h);
            polish_sync();
            u32 ku = ks, changed = 0, support = 0;
            u32 U[Q], cnt[Q][4];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                S[q] = (u32) Q * lane + (u32) q < ks ? S[q] : 8u;
                tb[q] = U[q] = S[q];
#pragma unroll
                for (u32 x = 0; x < 4u; x++) cnt[q][x] = 0;
            }
            // 3 to 6: align against the seed, vote over the tract alone, align against the re-voted unit
            AlignCell a1{0, 0, 0, 0}, a2{0, 0, 0, 0};
            u32 a1_end = 0, a2_end = 0, lo_pos = 0, hi_pos = rd.len, kt = ks;
            for (u32 pass = 0; pass < 3u; pass++) {
                AlignCell best;
                u32 best_end;
                polish_pass<Q>(rd, lo_pos, hi_pos, tb, kt, P, pass == 1u, best, best_end, cnt);
                const AlignCell found{rfl(best.score), rfl(best.start), rfl(best.consumed), rfl(best.matches)};  // the best cell is in every lane
                best_end = rfl(best_end);
                if (pass == 0u) {
                    a2 = a1 = found;
                    a2_end = a1_end = best_end;
                    lo_pos = a1.start;
                    hi_pos = a1_end;
                } else if (pass == 1u) {
                    // 5. re-vote: the seed's base where its count is the largest, else the smallest code among the largest
                    u32 U0[Q];
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        const u32 j = (u32) Q * lane + (u32) q;
                        u32 top = 0, ctop = cnt[q][0];
#pragma unroll
                        for (u32 x = 1; x < 4u; x++) {
                            const bool up = cnt[q][x] > ctop;  // strictly
                            top = up ? x : top;
                            ctop = up ? cnt[q][x] : ctop;
                        }
                        u32 cs = 0;
#pragma unroll
                        for (u32 x = 0; x < 4u; x++) cs = (S[q] & 3u) == x ? cnt[q][x] : cs;
                        const bool in = j < ks;
                        U0[q] = in ? (cs == ctop ? S[q] : top) : 8u;
                        changed += (u32) __popcll(__ballot(in && U0[q] != S[q]));
                        support += in ? (U0[q] == S[q] ? cs : ctop) : 0u;
                        if (in) h[j] = U0[q];
                    }
                    support = wave_sum_u32(support);
                    if (changed == 0u) {  // wave-uniform: U = S, A2 = A1
                        polish_sync();
                        satellite_clear(h);
                        polish_sync();
                        break;
                    }
                    polish_sync();
                    ku = polish_root<Q>(h, U0, ks);
                    polish_sync();
                    satellite_clear(h);
                    polish_sync();
#pragma unroll
                    for (int q = 0; q < Q; q++) tb[q] = U[q] = (u32) Q * lane + (u32) q < ku ? U0[q] : 8u;
                    kt = ku;
                    lo_pos = 0;
                    hi_pos = rd.len;
                } else {
                    // 6. final: a lower score keeps the seed
                    a2 = found;
                    a2_end = best_end;
                    if (a2.score < a1.score) {
                        a2 = a1;
                        a2_end = a1_end;
                        ku = ks;
                        changed = 0;
#pragma unroll
                        for (int q = 0; q < Q; q++) U[q] = S[q];
                    }
                }
            }
            rec[0] = ku;
            rec[1] = ks;
            rec[2] = k;
            rec[3] = changed;
            rec[4] = a2.score;
            rec[5] = a2.start;
            rec[6] = a2_end;
            rec[7] = a2.consumed;
            rec[8] = a2.matches;
            rec[9] = a1.score;
            rec[10] = support;
            // pack: U's codes in the words 0 .. 255 of the cleared bins, S's in 256 .. 511; word i of a unit is its codes 16 i .. 16 i + 15
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const u32 j = (u32) Q * lane + (u32) q;
                if (j < ku) h[j] = U[q];
                if (j < ks) h[kSatelliteMaxPeriod + j] = S[q];
            }
            polish_sync();
            if (lane >= 12u && lane < kPolishWords) {
                const u32 j0 = 16u * (lane - 12u);  // < 512
#pragma unroll 1
                for (u32 q = 0; q < 4u; q++) {
                    const uint4 v = reinterpret_cast<const uint4 *>(h)[(j0 >> 2) + q];  // nothing at or above the unit's length
                    unit_word |= (v.x << (8u * q)) | (v.y << (8u * q + 2u)) | (v.z << (8u * q + 4u)) | (v.w << (8u * q + 6u));
                }
            }
            polish_sync();
            satellite_clear(h);
            polish_sync();
        }
        // 44 lanes write the record's 44 words (trew_hip_polished): one vector store
        const u32 x = lane_words<12>(rec, unit_word);
        if (lane < kPolishWords) out[r * (u64) kPolishWords + lane] = x;
    }
}
