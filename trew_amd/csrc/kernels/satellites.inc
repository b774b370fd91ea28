// kernels/satellites.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// De novo repeats with periods up to 256 (trew_hip_satellites): the measure of kernels/repeats.inc with
// 1 <= min_period <= max_period <= kSatelliteMaxPeriod and a unit of sixteen words.  A kernel beside periods_wave_kernel and
// repeats_wave_kernel, which stay as they are: it reads the same bit planes, takes no pattern table and writes only buffers
// of its own (an append log of records with its counter, one count per read).  4 KiB of LDS per wave (the consensus bins).
//
// Definition (DESIGN 4.7d): that of 4.7a for a piece and of 4.7c for the recursion, k over [min_period, min(max_period, len - 1)].
//
// What is wide here and what is shared:
//   eq word      period_eq_word<true> (kernels/periods.inc): the partner of word w is word w + (k >> 5) and the one behind it.
//                period_walk, period_place, period_score<true> and period_locate<true> are the code of periods.inc: their
//                bounds (|S| <= 2^17 inside an iteration, kPeriodBias) do not depend on k.
//   consensus    4 * 256 bins per wave; lane l takes the majority of the phases l, l + 64, l + 128 and l + 192.
//   root         the majority codes go to the first 256 words of the (cleared) bins, one word a phase, where every lane
//                reaches phase (j + d) mod k*; the proper divisors d of k* in ascending order.
//   record       26 words from 26 lanes with one vector store: lanes 0 .. 9 the header, lane 10 + i unit word i, packed from
//                the sixteen codes 16 i .. 16 i + 15 in LDS (no carry between words; nothing at or above base `period`).
//   recursion    the stack in the lanes of three VGPRs, the pruning (repeat_worth) and the append are kernels/pieces.inc's.

constexpr u32 kSatelliteMaxPeriod = 256;                  // the one place the upper limit of a period is written down
constexpr u32 kSatelliteBins = 4u * kSatelliteMaxPeriod;  // u32 per wave
constexpr u32 kSatelliteWords = 26;                       // trew_hip_satellite: ten words and unit[16]
static_assert(kSatelliteMaxPeriod == 256u, "four phases a lane, sixteen unit words and uint4 bin rows are written for 256");
static_assert(kSatelliteMaxPeriod == TREW_SATELLITE_MAX_PERIOD, "the header's limit");

// the wave's bins, all zero: sixteen words a lane
__device__ __forceinline__ void satellite_clear(u32 *h) {
    const u32 lane = lane_id();
#pragma unroll
    for (u32 s = 0; s < 4u; s++) reinterpret_cast<uint4 *>(h)[lane + 64u * s] = make_uint4(0u, 0u, 0u, 0u);
}

// consensus of [start, end) at period k <= 256: u = the majority codes of the phases lane + 64 s, two bits each (s = 0 in the
// lowest), support = the sum of their counts over the lane's phases (a phase >= k has neither); h = the wave's bins, all zero
// on entry and on exit.  Once per record: the loops over s stay rolled, which keeps the registers of the k loop free.
__device__ __forceinline__ void satellite_consensus(const ReadRef &rd, u32 k, u32 start, u32 end, u32 *h, u32 &u, u32 &support) {
    const u32 lane = lane_id();
    for (u32 t0 = (start >> 5) & ~63u; t0 < rd.nw && ((u64) t0 << 5) < (u64) end; t0 += 64u) {
        const u32 w = t0 + lane;
        const u64 p0 = (u64) w << 5;
        if (w >= rd.nw || p0 >= (u64) end || p0 + 32u <= (u64) start) continue;
        const u32 c0 = rd.w[3ull * w + 0], c1 = rd.w[3ull * w + 1], c2 = rd.w[3ull * w + 2];
        const u32 lo = p0 < (u64) start ? start - (u32) p0 : 0u;              // first bit inside the span
        const u32 hi = (u64) end - p0 >= 32u ? 32u : (u32) ((u64) end - p0);  // one past the last
        u32 phase = ((u32) p0 + lo - start) % k;
        for (u32 i = lo; i < hi; i++) {
            if (!((c2 >> i) & 1u)) atomicAdd(&h[4u * phase + (((c0 >> i) & 1u) | (((c1 >> i) & 1u) << 1))], 1u);  // phase < k <= 256
            phase = phase + 1u == k ? 0u : phase + 1u;
        }
    }
    // the wave's own LDS operations complete in program order; the fences keep the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    u = 0;
    support = 0;
#pragma unroll 1
    for (u32 s = 0; s < 4u; s++) {
        const uint4 a = reinterpret_cast<const uint4 *>(h)[lane + 64u * s];
        u32 code = 0, cnt = a.x;
        if (a.y > cnt) { code = 1; cnt = a.y; }  // strictly: the smallest code keeps a tie
        if (a.z > cnt) { code = 2; cnt = a.z; }
        if (a.w > cnt) { code = 3; cnt = a.w; }
        if (lane + 64u * s < k) {
            u |= code << (2u * s);
            support += cnt;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    satellite_clear(h);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The record of one piece, as period_record gives it for k <= 32: rec[0 .. 7] = period, scored_period, score, start, end,
// matches, support, reserved (wave-uniform); unit_word = unit[lane - 10] in the lanes 10 .. 25, 0 elsewhere.  All zero and
// false without a record.  h: the wave's bins.
__device__ __forceinline__ bool satellite_record(const ReadRef &rd, Piece pc, u32 kmin, u32 kmax, int P, u32 min_score, u32 *h, u32 (&rec)[8],
                                                 u32 &unit_word) {
    const u32 lane = lane_id();
    const u32 len = pc.hi - pc.lo;
    u32 best = 0, ks = 0;
    for (u32 k = kmin; k <= kmax && k < len; k++) {
        const u32 sc = period_score<true>(rd, pc, k, P);
        if (sc > best) {  // strictly: the smallest k keeps a tie
            best = sc;
            ks = k;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) rec[i] = 0;
    unit_word = 0;
    if (ks == 0u || best < min_score) return false;  // wave-uniform
    u32 b, e;
    period_locate<true>(rd, pc, ks, P, best, b, e);
    const u32 start = b, end = e + ks;
    u32 u, support;
    satellite_consensus(rd, ks, start, end, h, u, support);
    // the codes where every lane reaches every phase: word j of the cleared bins holds phase j's
#pragma unroll
    for (u32 s = 0; s < 4u; s++) h[lane + 64u * s] = (u >> (2u * s)) & 3u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    u32 d = ks;
    for (u32 c = 1; 2u * c <= ks; c++) {  // a proper divisor is at most k* / 2
        if (ks % c) continue;
        bool differs = false;
#pragma unroll 1
        for (u32 s = 0; s < 4u; s++) {
            const u32 j = lane + 64u * s;
            if (j < ks) {
                const u32 src = j + c >= ks ? j + c - ks : j + c;  // (j + c) mod k*
                differs |= h[src] != ((u >> (2u * s)) & 3u);
            }
        }
        if (__ballot(differs) == 0ull) {
            d = c;
            break;
        }
    }
    // unit word i = lane - 10: bases 16 i .. 16 i + 15, base j in bits [2 (j & 15), 2 (j & 15) + 2); nothing at or above base d
    if (lane >= 10u && lane < kSatelliteWords) {
        const u32 j0 = 16u * (lane - 10u);
#pragma unroll 1
        for (u32 q = 0; q < 4u; q++) {
            const uint4 v = reinterpret_cast<const uint4 *>(h)[(j0 >> 2) + q];
            const u32 j = j0 + 4u * q;
            unit_word |= (j + 0u < d ? v.x << (8u * q + 0u) : 0u) | (j + 1u < d ? v.y << (8u * q + 2u) : 0u) |
                         (j + 2u < d ? v.z << (8u * q + 4u) : 0u) | (j + 3u < d ? v.w << (8u * q + 6u) : 0u);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (u32 s = 0; s < 4u; s++) h[lane + 64u * s] = 0;  // the bins are all zero again
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    rec[0] = d;
    rec[1] = ks;
    rec[2] = best;
    rec[3] = start;
    rec[4] = end;
    rec[5] = tract_div((u64) best + (u64) (u32) P * (u64) (e - b), (u32) P + 1u);
    rec[6] = wave_sum_u32(support);
    return true;
}

// counts: one u32 per read; the counter of lg is zero when the kernel starts (the caller's memset on the same stream)
__global__ void __launch_bounds__(256, 5) satellites_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, RepeatLog lg,
                                                              u32 *__restrict__ counts) {
    __shared__ __attribute__((aligned(16))) u32 bins[4][kSatelliteBins];
    const u32 lane = lane_id();
    u32 *h = bins[threadIdx.x >> 6];
    satellite_clear(h);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    const u32 kmin = (u32) rfl_i(min_period), kmax = min((u32) rfl_i(max_period), kSatelliteMaxPeriod);  // the bins hold no more
    const u32 smin = rfl(min_score);
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        const u32 found = walk_pieces<kSatelliteWords>(r, rd.len, kmin, smin, lg, [&](u32 lo, u32 hi) __attribute__((always_inline)) {
            u32 rec[8], unit_word;  // unit_word: lanes 10 .. 25
            const bool split = satellite_record(rd, Piece{lo, hi}, kmin, kmax, P, smin, h, rec, unit_word);
            return PieceEval{split, split, rec[3], rec[4], lane_words<8, 2>(rec, unit_word)};
        });
        if (lane == 0) counts[r] = found;
    }
}
