// kernels/resolve.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Refine's unit with the period chosen by alignment (trew_hip_resolve): the few best-scoring periods of periods.inc's fixed-phase
// score are the candidates, refine.inc's steps 2 to 6 (refine_at) run for each, and the record with the largest final score is
// kept.  A kernel beside the scan and beside the other fourteen measures: it reads the same bit planes, takes no pattern table and
// writes only its own records.  512 bytes of LDS per wave (the consensus bins of periods.inc), no worklist.
//
// Definition: DESIGN 4.7k, include/trew_hip.h (trew_hip_resolved).  Wave per read, for every length.
//
// Stage 1, the candidate loop around one inlined refine_at, the duplicate-seed skip and the best record held word i in lane i are
// resolve_piece (kernels/resolve_piece.inc), which the resolved forms of tandems, decompose and dissect call per piece; this kernel
// calls it for the whole read and keeps, through its `note`, the record's own words: rank, first_period and first_score.  Lanes
// 16 .. 19 take the record's own four words, and twenty lanes store the record at once.

__global__ void __launch_bounds__(256) resolve_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, u32 candidates,
                                                           u32 *__restrict__ out) {
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
    const u32 kmin = (u32) rfl_i(min_period), kmax = (u32) rfl_i(max_period), C = rfl(candidates);
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        const Piece pc{0u, rd.len};  // the whole read
        // steps 1 to 3: the winner word i in lane i, and the record's own four words
        u32 best, r_start, r_end, m, rank = 0, first_period = 0, first_score = 0;  // the periods tract is for kernels/tandems.inc: not used here
        resolve_piece(rd, pc, kmin, kmax, P, min_score, C, h, best, r_start, r_end, m, [&](u32 c, u32 sc, u32 pd, bool taken) {
            if (c == 0u) {
                first_period = pd;
                first_score = sc;
            }
            rank = taken ? c : rank;
        });
        // twenty lanes write the record's twenty words (trew_hip_resolved): one vector store; all zero without a candidate
        const u32 own[4] = {m, rank, first_period, first_score};
        const u32 x = lane_words<4, 16>(own, best);
        if (lane < 20) out[r * 20ull + lane] = x;
    }
}
