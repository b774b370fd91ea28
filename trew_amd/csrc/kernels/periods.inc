// kernels/periods.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// De novo repeat period and unit per read (trew_hip_periods): what repeats in a read, with which unit, and where, without a
// motif.  A kernel beside the scan and beside the four motif measures: it reads the same bit planes, takes no pattern
// table, and writes only its own records.  512 bytes of LDS per wave (the consensus bins), no worklist, no table.
//
// Definition (DESIGN 4.7a).  eq_k[i] (i < n - k) = bases i and i + k are both valid and equal; score(i) = +1 / -P;
// S_k(e) = sum over i < e; V_k(e) = S_k(e) - min over b <= e of S_k(b); score_k = max V_k, e_k the smallest e that attains
// it, b_k the largest b <= e_k at which S_k is smallest.  k* = the smallest k with the largest score_k.  The consensus unit
// of [b, e + k*) by majority per phase, its primitive root, and the record.
//
// Wave per read, for every length: lane l takes 32-base word 64 t + l in iteration t.  Its eq_k word comes from the three
// planes of the word and of the word behind it (one v_alignbit by k per plane; for k = 32 the next word itself), masked to
// i < n - k.  Lane 63's look-ahead word is loaded like every other, so an iteration seam carries no planes.
//
// Pass 1, values only, every k.  One in-word walk gives a word's total T, its smallest prefix m and largest prefix M (both
// over e = 0 .. 32, so <= 0 and >= 0) and its best segment W = max_e (s(e) - min_{b <= e} s(b)).  With g the smallest S in
// front of the word relative to the word's start (g <= 0: the start itself counts),
//     max over e in the word of V(e) = max over e of max(s(e) - g, s(e) - min_{b <= e, in word} s(b)) = max(M - g, W),
// so no second walk is needed for the value.  g has two sources: the words in front inside the iteration -- an exclusive
// DPP prefix maximum over keys kBias - (off + m), off from wave_scan_u32 of the totals -- and the iterations in front, the
// wave-uniform 64-bit gmin - run.  The second is applied to the wave maximum of off + M, in 64 bits, because S - gmin can
// reach n.  Inside an iteration |S| <= 64 words * 32 bases * 64 = 2^17 (kBias = 2^18); the running sum and the smallest
// prefix travel between iterations in 64 bits (|S| <= 64 n).
//
// Pass 2, positions, k* only.  e*: the same placement, then a second in-word walk, in 64 bits, that starts from the
// smallest S in front of the word and stops at the first e with V(e) = score; the lowest lane of the first iteration with
// such an e has the smallest.  b*: S(e*) - score is the smallest S over [0, e*], so b* is the largest b <= e* with S(b)
// equal to it: a third loop compares every prefix with that value and takes a wave maximum of b + 1.
//
// Consensus.  Every lane walks the valid bases of its word inside [start, end), the phase (p - start) mod k* counted along,
// and adds one to bin 4 phase + code with an LDS atomic (4 k* <= 128 bins per wave, the mechanism of kernels/variants.inc).
// Lane j < k* then reads its phase's four bins and takes the majority; the bins are cleared for the wave's next user.  The
// primitive root compares u with itself rotated by every divisor d of k* (one ds_bpermute a divisor).
//
// period_eq_word, period_score and period_locate take a template parameter kWide for kernels/satellites.inc (k up to 256); the
// kernels of this file and of repeats.inc use the instantiation without it, which is the code as it was.

constexpr u32 kPeriodBins = 128;

// A piece [lo, hi) of a read (0 <= lo <= hi <= n) is scored as a read of its own: position p exists only for lo <= p and
// p + k < hi, and nothing outside the piece is seen.  The whole read is the piece [0, n) (periods_wave_kernel); the children of
// a tract are pieces (kernels/repeats.inc).  The iteration grid of a piece starts at word lo >> 5.
struct Piece {
    u32 lo, hi;
};

// eq_k word of 32-base word w (w >= lo >> 5): bit i = bases 32 w + i and 32 w + i + k are both valid and equal, and
// lo <= 32 w + i < hi - k.  vm = the positions of the word that exist.  Reads word w and word w + 1 where they exist; what a
// plane holds in front of lo or at and past hi never shows (lo <= i and i + k < hi for every bit kept).
//
// kWide (kernels/satellites.inc): k may exceed 32.  For k = 32 q + r the partner of word w is word w + q and word w + q + 1,
// aligned by r (for r = 0 word w + q itself: v_alignbit by 0 returns its low operand); a partner word at or past rd.nw reads
// as all N.  Every lane loads its own partners, so an iteration seam still carries only sums.  The instantiation without
// kWide is the code as it was for k <= 32: q = 0, and k = 32 takes the next word.
template <bool kWide = false>
__device__ __forceinline__ u32 period_eq_word(const ReadRef &rd, Piece pc, u32 k, u32 w, u32 &vm) {
    const long long left = (long long) pc.hi - (long long) k - 32ll * (long long) w;  // positions i >= 32 w with i < hi - k
    const u32 nv = left >= 32 ? 32u : left > 0 ? (u32) left : 0u;
    const u32 first = w == (pc.lo >> 5) ? pc.lo & 31u : 0u;  // the bits of the piece's first word in front of lo
    vm = (nv >= 32u ? 0xffffffffu : (1u << nv) - 1u) & (0xffffffffu << first);
    if (vm == 0u) return 0u;  // also: w >= rd.nw
    const u32 c0 = rd.w[3ull * w + 0], c1 = rd.w[3ull * w + 1], c2 = rd.w[3ull * w + 2];
    if constexpr (kWide) {
        const u32 q = k >> 5, wa = w + q, wb = wa + 1u;  // w < rd.nw <= 2^27 and q <= 8: no wrap
        u32 a0 = c0, a1 = c1, a2 = c2, b0 = 0, b1 = 0, b2 = 0xffffffffu;
        if (q != 0u) {
            a0 = a1 = 0;
            a2 = 0xffffffffu;
            if (wa < rd.nw) {
                a0 = rd.w[3ull * wa + 0];
                a1 = rd.w[3ull * wa + 1];
                a2 = rd.w[3ull * wa + 2];
            }
        }
        if (wb < rd.nw) {
            b0 = rd.w[3ull * wb + 0];
            b1 = rd.w[3ull * wb + 1];
            b2 = rd.w[3ull * wb + 2];
        }
        const u32 t0 = alignbit(b0, a0, k), t1 = alignbit(b1, a1, k), t2 = alignbit(b2, a2, k);
        return ~((c0 ^ t0) | (c1 ^ t1) | c2 | t2) & vm;
    }
    u32 n0 = 0, n1 = 0, n2 = 0xffffffffu;
    if (w + 1u < rd.nw) {
        n0 = rd.w[3ull * (w + 1u) + 0];
        n1 = rd.w[3ull * (w + 1u) + 1];
        n2 = rd.w[3ull * (w + 1u) + 2];
    }
    const u32 s0 = k >= 32u ? n0 : alignbit(n0, c0, k), s1 = k >= 32u ? n1 : alignbit(n1, c1, k), s2 = k >= 32u ? n2 : alignbit(n2, c2, k);
    return ~((c0 ^ s0) | (c1 ^ s1) | c2 | s2) & vm;
}

// in-word walk over the prefixes e = 1 .. 32 (e = 0: value 0): total, smallest and largest prefix, best segment.  A position
// that does not exist (no bit in vm) scores 0 and changes none of the four.
__device__ __forceinline__ void period_walk(u32 eq, u32 vm, int P, int &T, int &m, int &M, int &W) {
    const u32 ne = vm & ~eq;
    int s = 0, mn = 0, mx = 0, bw = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        s += (int) ((eq >> i) & 1u) - P * (int) ((ne >> i) & 1u);
        mn = min(mn, s);
        mx = max(mx, s);
        bw = max(bw, s - mn);
    }
    T = s;
    m = mn;
    M = mx;
    W = bw;
}

constexpr int kPeriodBias = 1 << 18;  // above every |S| inside an iteration

// what one iteration of one k knows after the walk and the placement
struct PeriodPlace {
    int off;      // S at the start of the lane's word, relative to the start of the iteration
    int total;    // S at the end of the iteration, likewise (wave-uniform)
    int pmin;     // the smallest S of the words in front of the lane's inside the iteration, likewise; kPeriodBias for lane 0
    int itmin;    // the smallest S of the whole iteration, likewise (wave-uniform)
};
__device__ __forceinline__ PeriodPlace period_place(int T, int m) {
    PeriodPlace p;
    const u32 incl = wave_scan_u32((u32) T);
    p.off = (int) (incl - (u32) T);
    p.total = __builtin_amdgcn_readlane((int) incl, 63);
    const u32 sc = wave_scan_max_u32((u32) (kPeriodBias - (p.off + m)));  // idle lanes: T = m = 0, a prefix that exists
    p.pmin = kPeriodBias - (int) wave_prev_lane_u32(sc);
    p.itmin = kPeriodBias - __builtin_amdgcn_readlane((int) sc, 63);
    return p;
}

// score_k of one piece: the largest V_k(e)
template <bool kWide = false>
__device__ __forceinline__ u32 period_score(const ReadRef &rd, Piece pc, u32 k, int P) {
    long long run = 0, gmin = 0, best = 0;  // S at the start of the iteration; the smallest S so far; the largest V so far
    const u32 wend = (u32) (((u64) pc.hi + 31ull) >> 5);  // one past the piece's last word
    for (u32 t0 = pc.lo >> 5; t0 < wend; t0 += 64u) {
        u32 vm;
        const u32 eq = period_eq_word<kWide>(rd, pc, k, t0 + lane_id(), vm);
        int T, m, M, W;
        period_walk(eq, vm, P, T, m, M, W);
        const PeriodPlace pl = period_place(T, m);
        const int hi = pl.off + M;
        const u32 v_in = wave_max_u32((u32) max(W, hi - pl.pmin));         // against the words of this iteration; W >= 0
        const int hi_all = (int) wave_max_u32((u32) (hi + kPeriodBias)) - kPeriodBias;
        best = max(best, max((long long) v_in, (long long) hi_all - (gmin - run)));  // against the iterations in front
        gmin = min(gmin, run + (long long) pl.itmin);
        run += (long long) pl.total;
    }
    return (u32) best;
}

// the segment of score_k (score > 0): e = the smallest e with V_k(e) = score, b = the largest b in [lo, e] with S_k(b)
// smallest over [lo, e]; both in read coordinates
template <bool kWide = false>
__device__ __forceinline__ void period_locate(const ReadRef &rd, Piece pc, u32 k, int P, u32 score, u32 &b_out, u32 &e_out) {
    const u32 lane = lane_id();
    long long run = 0, gmin = 0, s_end = 0;
    u32 e_star = 0;
    const u32 wlo = pc.lo >> 5, wend = (u32) (((u64) pc.hi + 31ull) >> 5);
    for (u32 t0 = wlo; t0 < wend; t0 += 64u) {
        u32 vm;
        const u32 eq = period_eq_word<kWide>(rd, pc, k, t0 + lane, vm);
        int T, m, M, W;
        period_walk(eq, vm, P, T, m, M, W);
        const PeriodPlace pl = period_place(T, m);
        // second walk, relative to the word's start: mn = the smallest S in front (the start itself included, so <= 0)
        long long s = 0, mn = min(gmin - run, (long long) pl.pmin) - (long long) pl.off;
        u32 e_loc = 0;
        long long s_loc = 0;
#pragma unroll
        for (u32 i = 0; i < 32u; i++) {
            if ((vm >> i) & 1u) {
                s += ((eq >> i) & 1u) ? 1ll : -(long long) P;
                mn = min(mn, s);
                if (e_loc == 0u && s - mn == (long long) score) {
                    e_loc = i + 1u;
                    s_loc = s;
                }
            }
        }
        const u64 hit = __ballot(e_loc != 0u);
        if (hit) {  // wave-uniform
            const u32 L = (u32) __builtin_ctzll(hit);
            e_star = ((t0 + L) << 5) + (u32) __builtin_amdgcn_readlane((int) e_loc, L);
            const long long rel = (long long) pl.off + s_loc;  // |rel| < 2^18
            s_end = run + (long long) __builtin_amdgcn_readlane((int) rel, L);
            break;
        }
        gmin = min(gmin, run + (long long) pl.itmin);
        run += (long long) pl.total;
    }
    const long long lowest = s_end - (long long) score;  // min over lo <= b <= e* of S(b)
    u32 b1 = 0;                                          // b + 1 of the latest prefix found at that value
    run = 0;
    for (u32 t0 = wlo; t0 <= (e_star >> 5) && t0 < wend; t0 += 64u) {
        const u32 w = t0 + lane;
        u32 vm;
        const u32 eq = period_eq_word<kWide>(rd, pc, k, w, vm);
        int T, m, M, W;
        period_walk(eq, vm, P, T, m, M, W);
        const u32 incl = wave_scan_u32((u32) T);
        long long s = run + (long long) (int) (incl - (u32) T);
        u32 mine = 0;
        const u64 b0 = (u64) w << 5;
        // b exists for lo <= b <= e*; S does not move in front of lo, so b = lo is found with the value 0 wherever lo lies in its word
        if (b0 >= (u64) pc.lo && b0 <= (u64) e_star && s == lowest) mine = (u32) b0 + 1u;  // the word's start: the end of the word in front, or b = lo
#pragma unroll
        for (u32 i = 0; i < 32u; i++) {
            if ((vm >> i) & 1u) s += ((eq >> i) & 1u) ? 1ll : -(long long) P;
            if (b0 + i + 1u >= (u64) pc.lo && b0 + i + 1u <= (u64) e_star && s == lowest) mine = (u32) b0 + i + 2u;
        }
        b1 = max(b1, wave_max_u32(mine));
        run += (long long) __builtin_amdgcn_readlane((int) incl, 63);
    }
    b_out = b1 - 1u;  // b1 >= 1: the minimum over [lo, e*] is attained
    e_out = e_star;
}

// consensus of [start, end) at period k: u = lane j's majority code (j < k), cnt_u its count; h = the wave's bins, all zero
// on entry and on exit
__device__ __forceinline__ void period_consensus(const ReadRef &rd, u32 k, u32 start, u32 end, u32 *h, u32 &u, u32 &cnt_u) {
    const u32 lane = lane_id();
    for (u32 t0 = (start >> 5) & ~63u; t0 < rd.nw && ((u64) t0 << 5) < (u64) end; t0 += 64u) {
        const u32 w = t0 + lane;
        const u64 p0 = (u64) w << 5;
        if (w >= rd.nw || p0 >= (u64) end || p0 + 32u <= (u64) start) continue;
        const u32 c0 = rd.w[3ull * w + 0], c1 = rd.w[3ull * w + 1], c2 = rd.w[3ull * w + 2];
        const u32 lo = p0 < (u64) start ? start - (u32) p0 : 0u;                   // first bit inside the span
        const u32 hi = (u64) end - p0 >= 32u ? 32u : (u32) ((u64) end - p0);       // one past the last
        u32 phase = ((u32) p0 + lo - start) % k;
        for (u32 i = lo; i < hi; i++) {
            if (!((c2 >> i) & 1u)) atomicAdd(&h[(4u * phase + (((c0 >> i) & 1u) | (((c1 >> i) & 1u) << 1))) & (kPeriodBins - 1u)], 1u);  // phase < 32: the mask never bites
            phase = phase + 1u == k ? 0u : phase + 1u;
        }
    }
    // the wave's own LDS operations complete in program order; the fences keep the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const u32 j4 = (lane & 31u) * 4u;
    const u32 a0 = h[j4], a1 = h[j4 + 1u], a2 = h[j4 + 2u], a3 = h[j4 + 3u];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    h[lane] = 0;
    h[lane + 64u] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    u = 0;
    cnt_u = a0;
    if (a1 > cnt_u) { u = 1; cnt_u = a1; }  // strictly: the smallest code keeps a tie
    if (a2 > cnt_u) { u = 2; cnt_u = a2; }
    if (a3 > cnt_u) { u = 3; cnt_u = a3; }
    if (lane >= k) u = cnt_u = 0;
}

// The record of one piece: rec[0 .. 9] = the ten words of trew_hip_period (period, scored_period, score, start, end, matches,
// support, reserved, unit), start and end in read coordinates; all zero and false without a record (no admissible k, or
// score < min_score).  Wave-uniform.  h: the wave's bins.
__device__ __forceinline__ bool period_record(const ReadRef &rd, Piece pc, u32 kmin, u32 kmax, int P, u32 min_score, u32 *h, u32 (&rec)[10]) {
    const u32 lane = lane_id();
    const u32 len = pc.hi - pc.lo;
    u32 best = 0, ks = 0;
    for (u32 k = kmin; k <= kmax && k < len; k++) {
        const u32 sc = period_score(rd, pc, k, P);
        if (sc > best) {  // strictly: the smallest k keeps a tie
            best = sc;
            ks = k;
        }
    }
#pragma unroll
    for (int i = 0; i < 10; i++) rec[i] = 0;
    if (ks == 0u || best < min_score) return false;  // wave-uniform
    u32 b, e;
    period_locate(rd, pc, ks, P, best, b, e);
    const u32 start = b, end = e + ks;
    u32 u, cnt_u;
    period_consensus(rd, ks, start, end, h, u, cnt_u);
    u32 d = ks;
    for (u32 c = 1; c < ks; c++) {
        if (ks % c) continue;
        const u32 src = lane + c >= ks ? lane + c - ks : lane + c;  // (j + c) mod k* for the lanes j < k*
        const u32 other = (u32) __builtin_amdgcn_ds_bpermute((int) ((src & 63u) << 2), (int) u);
        if (__ballot(lane < ks && other != u) == 0ull) {
            d = c;
            break;
        }
    }
    // unit: u[0 .. d - 1], first base most significant; the lanes' terms have no bit in common, so their sum is their OR
    const u32 sh = lane < d ? 2u * (d - 1u - lane) : 0u;
    const u64 term = lane < d ? (u64) u << sh : 0ull;
    rec[0] = d;
    rec[1] = ks;
    rec[2] = best;
    rec[3] = start;
    rec[4] = end;
    rec[5] = tract_div((u64) best + (u64) (u32) P * (u64) (e - b), (u32) P + 1u);
    rec[6] = wave_sum_u32(cnt_u);
    rec[8] = wave_sum_u32((u32) term);
    rec[9] = wave_sum_u32((u32) (term >> 32));
    return true;
}

__global__ void __launch_bounds__(256) periods_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, u32 *__restrict__ out) {
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
        u32 rec[10];
        period_record(rd, Piece{0u, rd.len}, kmin, kmax, P, min_score, h, rec);  // the whole read
        const u32 x = lane_words(rec, rec[9]);
        if (lane < 10) out[r * 10ull + lane] = x;
    }
}
