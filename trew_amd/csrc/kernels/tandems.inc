// kernels/tandems.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// De novo repeats under indels, every tract of a read (trew_hip_tandems): the recursion of repeats.inc over pieces with the
// work of refine.inc per piece.  A kernel beside repeats_wave_kernel and refine_wave_kernel, which stay as they are: it reads the
// same bit planes, takes no pattern table and writes only buffers of its own (an append log of records with its counter, one
// count per read).  512 bytes of LDS per wave (the consensus bins), no worklist, no table.
//
// Definition (DESIGN 4.7g).  A piece [lo, hi) of a read has the refined record that trew_hip_refine gives its bases taken as
// a read of their own (refine_piece, kernels/refine.inc, which sees nothing outside the piece), start and end in read
// coordinates, and the periods tract of step 1 of that computation.  tandems(piece): no periods record, nothing; a refined
// record X with score >= min_score, X, then tandems([lo, X.start)) and tandems([X.end, hi)); otherwise (a weak piece) no
// record, then tandems([lo, R.start)) and tandems([R.end, hi)) around the periods tract R, which is used up.  The tracts of a
// read are tandems([0, n)); depth is 0 for the read's own piece and parent + 1 below it, whether the parent gave a record or not.
//
// The piece loop is that of walk_pieces (kernels/pieces.inc): the wave-uniform stack of (lo, hi, depth) across the lanes of three
// VGPRs, the LONGER child pushed and the SHORTER continued (both children of a weak piece as well: R is not empty, so they
// shrink), hence at most 32 entries pending; a piece that repeat_worth rules out can have no periods record and is neither
// pushed nor walked.  It is written out here and does not call walk_pieces, lane_words or log_append: with any of them this
// kernel's registers come out differently (113 VGPRs instead of 119 with the walk, the hot loops of refine_piece the same
// instructions on other registers) and long reads take 2.1 to 2.9 % longer on the MI355X (profiles/piece_walk/README.md).  So
// the walk stands twice, there and here (dissect.inc calls walk_pieces: profiles/unit_walk/README.md): a fix to it there has to
// be made here as well.
//
// Append.  One returning 64-bit vector-memory atomic per record on the log's counter, wave-uniform (lane 0 adds, the others
// get the index through readfirstlane); the record's eighteen words go out from eighteen lanes, those of a record at or beyond
// the capacity not at all while the counter keeps counting.  counts[read] is stored for every read.

constexpr u32 kTandemWords = 18;  // trew_hip_tandem: read, depth, the sixteen words of trew_hip_refined

// counts: one u32 per read; the counter of lg is zero when the kernel starts (the caller's memset on the same stream)
// kResolved (trew_hip_tandems_resolved, DESIGN 4.7l): resolve_piece (kernels/resolve_piece.inc) in the place of refine_piece, with
// `candidates` its C; the record stays word i in lane i, three words are read out of it and the store moves it two lanes up.
// <false> is trew_hip_tandems' kernel, instruction for instruction what it was without the parameter; it ignores `candidates`.
template <bool kResolved>
__global__ void __launch_bounds__(256) tandems_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, RepeatLog lg,
                                                           u32 *__restrict__ counts, u32 candidates) {
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
            u32 rec[16], r_start = 0, r_end = 0;
            u32 won = 0;  // kResolved: the record, word i in lane i
            bool split;
            if constexpr (kResolved) {
                u32 m;
                split = resolve_piece(rd, Piece{lo, hi}, kmin, kmax, P, smin, rfl(candidates), h, won, r_start, r_end, m, [](u32, u32, u32, bool) {});
                rec[4] = record_word(won, 4), rec[5] = record_word(won, 5), rec[6] = record_word(won, 6);
            } else {
                split = refine_piece(rd, Piece{lo, hi}, kmin, kmax, P, smin, h, rec, r_start, r_end);
            }
            u32 a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;  // the children; a the shorter
            if (split) {
                const bool strong = rfl(rec[4]) >= smin;
                // the children lie around the refined tract, or around the periods tract of a weak piece
                const u32 start = strong ? rfl(rec[5]) : rfl(r_start), end = strong ? rfl(rec[6]) : rfl(r_end);
                // a tract lies inside its piece; the pieces below are formed from it, so nothing else may ever reach them
                if (!(start >= lo && end <= hi && start < end)) break;
                if (strong) {
                    found++;
                    u64 idx = 0;
                    if (lane == 0) idx = atomicAdd(lg.counter, 1ull);
                    idx = rfl64(idx);
                    u32 x;
                    if constexpr (kResolved) {
                        x = lane_read(won, ((lane - 2u) & 63u) << 2);  // word i into lane i + 2
                    } else {
                        x = rec[15];
#pragma unroll
                        for (int i = 14; i >= 0; i--) x = lane == (u32) (i + 2) ? rec[i] : x;
                    }
                    x = lane == 1u ? depth : x;
                    x = lane == 0u ? (u32) r : x;
                    if (idx < lg.cap && lane < kTandemWords) lg.recs[idx * (u64) kTandemWords + lane] = x;
                }
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
