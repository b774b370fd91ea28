// kernels/refine.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// De novo repeats under indels (trew_hip_refine): the period and tract of trew_hip_periods, a literal seed unit from the longest
// run of eq_k, the wraparound alignment of the read against it, a forward-decoded vote per phase and the alignment against
// the re-voted unit.  A kernel beside the scan and beside the other nine measures: it reads the same bit planes, takes no
// pattern table and writes only its own records.  512 bytes of LDS per wave (the consensus bins of periods.inc), no worklist.
//
// Definition: DESIGN 4.7f, include/trew_hip.h (trew_hip_refined).  Wave per read, for every length.
//
// Stage 1 (periods) is periods.inc's period_score, period_locate and period_consensus as they are; the unreduced consensus
// stays in the lanes (lane j: phase j) for the N of a seed window.
//
// Stage 2 (seed).  One more walk over the eq words of the scored k, masked to [b, e): lane l takes word 64 t + l.  A run that
// crosses words is measured where it ends: a lane's first run is lengthened by the run that ends at the end of the word in
// front, which is 32 for every all-ones word directly in front (a ballot and a count of leading set bits) plus the trailing
// run of the first word that is not all ones (one ds_bpermute), or plus the wave-uniform carry of the iteration in front when
// every word in front is all ones.  A lane that a run passes through sees a shorter piece of it with the same start, which
// never wins.  The longest run, the smallest start among the longest: two wave maxima an iteration; a later iteration must be
// strictly longer.
//
// Stages 3 to 6 (align, vote, align) are the row step of kernels/wraparound.inc, kept written out in refine_pass because the
// shared form was 3 % slower on long reads (profiles/wraparound/README.md): the row in registers, a phase per lane, the cyclic neighbour
// by ds_bpermute, the doubling steps below the unit length only, everything selects.  The unit length is wave-uniform per
// read, so the source-lane tables are computed per pass.  Only one strand is needed: lanes 32 .. 63 mirror lanes 0 .. 31
// (same phase, same unit, same cells), which keeps every lane read inside its half as in align.inc and costs nothing.  The
// vote's argmax over the row is four wave maxima (DPP), field by field over the lanes still tied, and a ballot whose lowest
// bit is the smallest phase; the four counters of a phase live in its lane.

// the length of the primitive root of the unit u (lane j < k: its base j), wave-uniform; the loop of period_record
__device__ __forceinline__ u32 refine_root(u32 u, u32 k) {
    const u32 lane = lane_id();
    for (u32 c = 1; c < k; c++) {
        if (k % c) continue;
        const u32 src = lane + c >= k ? lane + c - k : lane + c;  // (j + c) mod k for the lanes j < k
        const u32 other = lane_read(u, (src & 63u) << 2);
        if (__ballot(lane < k && other != u) == 0ull) return c;
    }
    return k;
}

// u[0 .. d - 1] packed first base most significant (lane j < d: base j), as period_record packs its unit
__device__ __forceinline__ void refine_pack(u32 u, u32 d, u32 &lo, u32 &hi) {
    const u32 lane = lane_id();
    const u32 sh = lane < d ? 2u * (d - 1u - lane) : 0u;
    const u64 term = lane < d ? (u64) u << sh : 0ull;
    lo = wave_sum_u32((u32) term);  // the lanes' terms have no bit in common: their sum is their OR
    hi = wave_sum_u32((u32) (term >> 32));
}

// the start of the longest run of set bits of the piece's eq_k among the positions [b, e), the first of the longest; b without one.
// kWide (kernels/polish.inc): k may exceed 32, handed on to period_eq_word; the instantiation without it is the code as it was.
template <bool kWide = false>
__device__ __forceinline__ u32 refine_longest_run(const ReadRef &rd, Piece pc, u32 k, u32 b, u32 e) {
    const u32 lane = lane_id();
    u32 best_len = 0, best_start = b, carry = 0;  // carry: the run that ends at the end of the iteration in front
    for (u32 t0 = b >> 5; ((u64) t0 << 5) < (u64) e; t0 += 64u) {
        const u32 w = t0 + lane;
        const u64 p0 = (u64) w << 5;
        u32 vm;
        u32 eq = period_eq_word<kWide>(rd, pc, k, w, vm);
        const u32 first = p0 >= (u64) b ? 0u : (u64) b - p0 >= 32u ? 32u : b - (u32) p0;   // bits in front of b
        const u32 last = p0 >= (u64) e ? 0u : (u64) e - p0 >= 32u ? 32u : e - (u32) p0;    // one past the last bit in front of e
        eq &= (last >= 32u ? 0xffffffffu : (1u << last) - 1u) & (first >= 32u ? 0u : 0xffffffffu << first);
        const bool all = eq == 0xffffffffu;
        const u32 sfx = all ? 32u : (u32) __clz((int) ~eq);  // the run that ends at the word's last bit
        // the run that ends at the end of the word in front
        const u64 below = ~__ballot(all) & ((1ull << lane) - 1ull);  // the words in front that are not all ones
        const u32 hb = below ? 63u - (u32) __clzll((long long) below) : 0u;
        const u32 sfx_hb = lane_read(sfx, hb << 2);
        const u32 cin = below ? 32u * (lane - 1u - hb) + sfx_hb : 32u * lane + carry;
        u32 cur = cin, bl = 0, bs = 0;
#pragma unroll
        for (u32 i = 0; i < 32u; i++) {
            cur = (eq >> i) & 1u ? cur + 1u : 0u;
            const bool up = cur > bl;  // strictly: the first of the longest
            bs = up ? (u32) p0 + i + 1u - cur : bs;
            bl = up ? cur : bl;
        }
        const u32 mlen = wave_max_u32(bl);
        const u32 mstart = 0xffffffffu - wave_max_u32(bl == mlen ? 0xffffffffu - bs : 0u);
        if (mlen > best_len) {  // wave-uniform
            best_len = mlen;
            best_start = mstart;
        }
        carry = (u32) __builtin_amdgcn_readlane((int) cur, 63);
    }
    return best_len ? best_start : b;
}

// One pass of the wraparound recurrence over the bases [lo, hi) of the read, taken as a read of their own, against the unit
// whose base j is tb in the lanes with (lane & 31) = j < k (8 in the others): the best cell of the row's lanes as
// align_wave_kernel finds it, in every lane; start and end count from lo.  kVote: the forward decode into cnt.
// Repeats wrap_sources, base_code, wrap_row<false> (the vote where its `mid` runs), wrap_keep_best and wrap_reduce_half<false>.
template <bool kVote>
__device__ __forceinline__ void refine_pass(const ReadRef &rd, u32 lo_pos, u32 hi_pos, u32 tb, u32 k, int P, AlignCell &best, u32 &best_end,
                                            u32 (&cnt)[4]) {
    const u32 lane = lane_id();
    const u32 j = lane & 31u, half = lane & 32u;
    const bool live = j < k;
    u32 src[5];
#pragma unroll
    for (int t = 0; t < 5; t++) {
        int q = ((int) j - (1 << t)) % (int) k;
        q = q < 0 ? q + (int) k : q;
        src[t] = (half | (u32) q) << 2;
    }
    AlignCell H{0, 0, 0, 0};
    best = AlignCell{0, 0, 0, 0};
    best_end = 0;
    for (u32 w = lo_pos >> 5; ((u64) w << 5) < (u64) hi_pos; w++) {
        const u32 lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
        const u32 b0 = w == (lo_pos >> 5) ? lo_pos & 31u : 0u;
        const u32 left = hi_pos - (w << 5);  // >= 1
        const u32 nb = left < 32u ? left : 32u;
        for (u32 b = b0; b < nb; b++) {
            const u32 i = (w << 5) + b + 1u - lo_pos;
            const u32 c = ((lo >> b) & 1u) | (((hi >> b) & 1u) << 1) | (((nm >> b) & 1u) << 2);  // 4: an N
            const bool hit = c == tb;
            const AlignCell d = align_from(H, src[0]);
            const int ds = hit ? (int) d.score + 1 : (int) d.score - P;
            AlignCell V = align_pick(ds > 0, AlignCell{(u32) ds, d.start, d.consumed + 1u, d.matches + (hit ? 1u : 0u)}, AlignCell{0, i, 0, 0});
            const int is = (int) H.score - P;
            const AlignCell ins{(u32) is, H.start, H.consumed, H.matches};
            const bool by_ins = (is > 0) & align_gt(ins, V);
            V = align_pick(by_ins, ins, V);
            if constexpr (kVote) {
                // the phase with the largest V, the smallest on a tie: the lanes still tied, field by field
                bool tie = live & (V.score == wave_max_u32(live ? V.score : 0u));
                tie &= V.start == wave_max_u32(tie ? V.start : 0u);
                tie &= V.consumed == wave_max_u32(tie ? V.consumed : 0u);
                tie &= V.matches == wave_max_u32(tie ? V.matches : 0u);
                const u32 js = (u32) __builtin_ctzll(__ballot(tie));  // a live lane is always left; < 32: the halves are alike
                // the diagonal is that cell: it was taken (a score of 0 or less is never the cell) and the inserted base did not beat it
                const bool voted = (j == js) & (ds > 0) & !by_ins;
#pragma unroll
                for (u32 x = 0; x < 4u; x++) cnt[x] += (voted & (c == x)) ? 1u : 0u;
            }
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
}

// Steps 2 to 6 of DESIGN 4.7f for the period k of the piece pc and its periods score (> 0): the segment of k and its consensus,
// the seed, align, vote, re-vote, final.  rec[0 .. 15] = the sixteen words of trew_hip_refined with scored_period = k, start and
// end in read coordinates; r_start and r_end the periods tract of k, in read coordinates as well.  What refine_piece does with the
// one period of its step 1 and resolve_wave_kernel (kernels/resolve.inc) with each of its candidates.  skip(S): asked once, with
// the primitive seed in the lanes (base j in the lanes with (lane & 31) = j < seed_period, 8 in the others), in front of the three
// passes; wave-uniform; true: the passes walk no base (their range is empty: a branch around them cost resolve_wave_kernel 22
// VGPRs and a wave per SIMD), rec is of no use and the result is false.  Wave-uniform.  h: the wave's bins, all zero on entry and
// on exit.
template <class Skip>
__device__ __forceinline__ bool refine_at(const ReadRef &rd, Piece pc, u32 k, u32 score, int P, u32 *h, u32 (&rec)[16], u32 &r_start, u32 &r_end, Skip skip) {
    const u32 lane = lane_id();
    const u32 j = lane & 31u;
    u32 b, e;
    period_locate(rd, pc, k, P, score, b, e);
    const u32 start = b, end = e + k;
    r_start = start;
    r_end = end;
    u32 cons, cons_cnt;
    period_consensus(rd, k, start, end, h, cons, cons_cnt);
    // 2. seed: the k bases at the longest run, an N replaced by its phase of the consensus
    const u32 rs = refine_longest_run(rd, pc, k, b, e);
    u32 s0 = 8;
    {
        const u32 pos = rs + j;  // < end for j < k
        const u32 ph = (pos - start) % k;
        const u32 cu = lane_read(cons, ph << 2);
        if (j < k && pos < pc.hi) {
            const u32 w = pos >> 5, bit = pos & 31u;
            const u32 c0 = rd.w[3ull * w + 0], c1 = rd.w[3ull * w + 1], c2 = rd.w[3ull * w + 2];
            s0 = (c2 >> bit) & 1u ? cu : ((c0 >> bit) & 1u) | (((c1 >> bit) & 1u) << 1);
        }
    }
    const u32 ks = refine_root(s0, k);
    const u32 S = j < ks ? lane_read(s0, j << 2) : 8u;  // both halves alike
    const bool skipped = skip(S);                 // wave-uniform
    const u32 p_hi = skipped ? pc.lo : pc.hi;    // skipped: the passes walk no base
    u32 cnt[4] = {0, 0, 0, 0};
    // 3. align against the seed
    AlignCell a1;
    u32 a1_end;
    refine_pass<false>(rd, pc.lo, p_hi, S, ks, P, a1, a1_end, cnt);
    const u32 a1_start = rfl(a1.start);  // the best cell is in every lane; 0 and 0 without one
    a1_end = rfl(a1_end);
    // 4. vote over the tract alone
    {
        AlignCell av;
        u32 av_end;
        refine_pass<true>(rd, pc.lo + a1_start, pc.lo + a1_end, S, ks, P, av, av_end, cnt);
    }
    // 5. re-vote: the seed's base where its count is the largest, else the smallest code among the largest
    u32 top = 0;
#pragma unroll
    for (u32 x = 1; x < 4u; x++) top = cnt[x] > cnt[top] ? x : top;  // strictly
    u32 cs = 0;
#pragma unroll
    for (u32 x = 0; x < 4u; x++) cs = (S & 3u) == x ? cnt[x] : cs;
    const bool lane_k = lane < ks;  // one half counts
    const u32 U0 = j < ks ? (cs == cnt[top] ? S : top) : 8u;
    u32 changed = (u32) __popcll(__ballot(lane_k && U0 != S));
    const u32 support = wave_sum_u32(lane_k ? (U0 == S ? cs : cnt[top]) : 0u);
    u32 ku = ks;
    u32 U = S;
    AlignCell a2 = a1;
    u32 a2_end = a1_end;
    // 6. final: align against the re-voted unit; a lower score keeps the seed
    if (changed) {  // wave-uniform
        ku = refine_root(U0, ks);
        U = j < ku ? U0 : 8u;
        refine_pass<false>(rd, pc.lo, p_hi, U, ku, P, a2, a2_end, cnt);
        if (rfl(a2.score) < rfl(a1.score)) {
            a2 = a1;
            a2_end = a1_end;
            U = S;
            ku = ks;
            changed = 0;
        }
    }
    rec[0] = ku;
    rec[1] = ks;
    rec[2] = k;
    rec[3] = changed;
    rec[4] = a2.score;
    rec[5] = pc.lo + a2.start;  // refine_pass counts from the piece's first base
    rec[6] = pc.lo + a2_end;
    rec[7] = a2.consumed;
    rec[8] = a2.matches;
    rec[9] = a1.score;
    rec[10] = support;
    rec[11] = 0;
    refine_pack(U, ku, rec[12], rec[13]);
    refine_pack(S, ks, rec[14], rec[15]);
    return !skipped;
}

// The refined record of one piece (DESIGN 4.7f, all six steps, over the bases [pc.lo, pc.hi) taken as a read of their own; nothing
// outside the piece is seen): rec[0 .. 15] = the sixteen words of trew_hip_refined, start and end in read coordinates.  False
// without a periods record (step 1), rec all zero; otherwise r_start and r_end hold the periods tract of step 1, in read
// coordinates as well (kernels/tandems.inc splits a weak piece there).  Wave-uniform.  h: the wave's bins.
__device__ __forceinline__ bool refine_piece(const ReadRef &rd, Piece pc, u32 kmin, u32 kmax, int P, u32 min_score, u32 *h, u32 (&rec)[16], u32 &r_start,
                                             u32 &r_end) {
    // 1. periods: the scored k
    u32 score = 0, k = 0;
    for (u32 kk = kmin; kk <= kmax && kk < pc.hi - pc.lo; kk++) {
        const u32 sc = period_score(rd, pc, kk, P);
        if (sc > score) {  // strictly: the smallest k keeps a tie
            score = sc;
            k = kk;
        }
    }
    if (k == 0u || score < min_score) {  // wave-uniform: a zero record
#pragma unroll
        for (int i = 0; i < 16; i++) rec[i] = 0;
        return false;
    }
    return refine_at(rd, pc, k, score, P, h, rec, r_start, r_end, [](u32) { return false; });
}

__global__ void __launch_bounds__(256) refine_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, u32 *__restrict__ out) {
    __shared__ u32 bins[4][kPeriodBins];
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
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        u32 rec[16], r_start, r_end;  // the periods tract and the returned flag are for kernels/tandems.inc: not used here
        refine_piece(rd, Piece{0u, rd.len}, kmin, kmax, P, min_score, h, rec, r_start, r_end);  // the whole read; all zero without a record
        // sixteen lanes write the record's sixteen words (trew_hip_refined): one vector store
        const u32 x = lane_words(rec, rec[15]);
        if (lane < 16) out[r * 16ull + lane] = x;
    }
}
