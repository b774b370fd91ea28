// kernels/repeats.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// De novo repeats: every tract of a read, not only the best one (trew_hip_repeats).  A kernel beside periods_wave_kernel, which
// stays as it is: it reads the same bit planes, takes no pattern table and writes only buffers of its own (an append log of
// records with its counter, one count per read).  512 bytes of LDS per wave (the consensus bins), no worklist, no table.
//
// Definition (DESIGN 4.7c).  A piece [lo, hi) of a read has the record that trew_hip_periods gives its bases taken as a read
// of their own (period_record, kernels/periods.inc, which sees nothing outside the piece), start and end in read coordinates.
// repeats(piece): no record, nothing; else the record R, then repeats([lo, R.start)) and repeats([R.end, hi)).  The tracts of
// a read are repeats([0, n)); depth is 0 for the read's own record and parent + 1 below it.
//
// The recursion runs inside the wave, over a wave-uniform stack of (lo, hi, depth) kept across the lanes of three VGPRs
// (entry i in lane i; a push is a store by one lane, a pop a v_readlane with a uniform index).  After a record the LONGER child
// is pushed and the wave continues with the SHORTER, so the piece at hand is at most half the piece its pending sibling came
// from: with f(L) the entries a piece of L bases can add to the stack, f(L) <= 1 + f(L / 2), and a read of fewer than 2^32
// bases never has more than 32 entries pending -- half the 64 lanes.  A piece with hi - lo - min_period < min_score cannot
// have a record (score_k <= len - k) and is neither pushed nor walked, which changes no result.
//
// Append.  One returning 64-bit vector-memory atomic per record on the log's counter, wave-uniform (lane 0 adds, the others
// get the index through readfirstlane, as in kernels/chain.inc); the record's twelve words go out from twelve lanes, those of
// a record at or beyond the capacity not at all while the counter keeps counting.  counts[read] is stored for every read.

constexpr u32 kRepeatWords = 12;  // trew_hip_repeat: read, depth, the ten words of trew_hip_period

// a piece that may have a record: score_k <= hi - lo - k <= hi - lo - min_period
__device__ __forceinline__ bool repeat_worth(u32 lo, u32 hi, u32 kmin, u32 min_score) {
    const u32 len = hi - lo;
    return len > kmin && len - kmin >= min_score;
}

// counts: one u32 per read; the counter of lg is zero when the kernel starts (the caller's memset on the same stream)
__global__ void __launch_bounds__(256) repeats_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, RepeatLog lg,
                                                           u32 *__restrict__ counts) {
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
    const u32 smin = rfl(min_score);
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        u32 st_lo = 0, st_hi = 0, st_d = 0;  // the stack: entry i in lane i
        u32 sp = 0;                          // entries pending (wave-uniform, at most 32: see above)
        u32 lo = 0, hi = rd.len, depth = 0;  // the piece at hand
        u32 found = 0;
        bool have = repeat_worth(lo, hi, kmin, smin);
        while (have) {  // wave-uniform
            u32 rec[10];
            bool split = period_record(rd, Piece{lo, hi}, kmin, kmax, P, smin, h, rec);
            // a tract lies inside its piece; the pieces below are formed from it, so nothing else may ever reach them
            if (split && !(rec[3] >= lo && rec[4] <= hi && rec[3] < rec[4])) break;
            u32 a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;  // the children; a the shorter
            if (split) {
                found++;
                u64 idx = 0;
                if (lane == 0) idx = atomicAdd(lg.counter, 1ull);
                idx = rfl64(idx);
                u32 x = rec[9];
#pragma unroll
                for (int i = 8; i >= 0; i--) x = lane == (u32) (i + 2) ? rec[i] : x;
                x = lane == 1u ? depth : x;
                x = lane == 0u ? (u32) r : x;
                if (idx < lg.cap && lane < kRepeatWords) lg.recs[idx * (u64) kRepeatWords + lane] = x;
                const u32 start = rfl(rec[3]), end = rfl(rec[4]);
                const bool left_short = start - lo <= hi - end;
                a_lo = left_short ? lo : end;
                a_hi = left_short ? start : hi;
                b_lo = left_short ? end : lo;
                b_hi = left_short ? hi : start;
                depth++;
                if (repeat_worth(b_lo, b_hi, kmin, smin)) {  // push the longer child
                    if (lane == sp) {
                        st_lo = b_lo;
                        st_hi = b_hi;
                        st_d = depth;
                    }
                    sp++;
                }
            }
            if (split && repeat_worth(a_lo, a_hi, kmin, smin)) {  // go on with the shorter child
                lo = a_lo;
                hi = a_hi;
            } else if (sp != 0u) {  // pop
                sp--;
                sp = rfl(sp);
                lo = (u32) __builtin_amdgcn_readlane((int) st_lo, sp);
                hi = (u32) __builtin_amdgcn_readlane((int) st_hi, sp);
                depth = (u32) __builtin_amdgcn_readlane((int) st_d, sp);
            } else {
                have = false;
            }
        }
        if (lane == 0) counts[r] = found;
    }
}
