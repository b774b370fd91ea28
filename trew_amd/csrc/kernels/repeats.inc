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
// The recursion (the stack inside the wave, the order of the children, the pruning) and the append of a record's twelve words
// to the log are those of kernels/pieces.inc; this file says what a piece gives.  counts[read] is stored for every read.

constexpr u32 kRepeatWords = 12;  // trew_hip_repeat: read, depth, the ten words of trew_hip_period

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
        const u32 found = walk_pieces<kRepeatWords>(r, rd.len, kmin, smin, lg, [&](u32 lo, u32 hi) __attribute__((always_inline)) {
            u32 rec[10];
            const bool split = period_record(rd, Piece{lo, hi}, kmin, kmax, P, smin, h, rec);
            return PieceEval{split, split, rec[3], rec[4], lane_words<10, 2>(rec, rec[9])};
        });
        if (lane == 0) counts[r] = found;
    }
}
