// kernels/resolve.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Refine's unit with the period chosen by alignment (trew_hip_resolve): the few best-scoring periods of periods.inc's fixed-phase
// score are the candidates, refine.inc's steps 2 to 6 (refine_at) run for each, and the record with the largest final score is
// kept.  A kernel beside the scan and beside the other fourteen measures: it reads the same bit planes, takes no pattern table and
// writes only its own records.  512 bytes of LDS per wave (the consensus bins of periods.inc), no worklist.
//
// Definition: DESIGN 4.7k, include/trew_hip.h (trew_hip_resolved).  Wave per read, for every length.
//
// Stage 1 is refine_piece's loop over k with period_score; it keeps the four best (score, k) pairs in wave-uniform registers, an
// insertion into a sorted list written out: strictly greater displaces, so the smaller k keeps a tie.  The first C of the four
// are the first C of the whole order.  No extra pass over the read.
//
// The candidate loop is a runtime loop around one inlined refine_at.  period_consensus wants the wave's bins zero on entry and
// leaves them zero, so the loop clears nothing.  A candidate whose primitive seed equals an earlier candidate's code for code
// gives the same record up to scored_period and loses the tie: its three passes walk no base (refine_at's skip).  The earlier
// seeds are kept four bits a candidate in one register (lane j: base j, 8 past the seed's length, both halves alike), the
// compare is a ballot.  A rotation of an earlier seed differs in some lane and is aligned.
//
// Best so far: the winner's sixteen words in one register, word i in lane i (lane_words), with its score, period and rank
// wave-uniform beside it.  Lanes 16 .. 19 take the record's own four words, and twenty lanes store the record at once.

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
        // 1. scores: the four best (score, k) with score >= min_score (>= 1), score descending, k ascending; k = 0: no entry
        u32 s0 = 0, s1 = 0, s2 = 0, s3 = 0, k0 = 0, k1 = 0, k2 = 0, k3 = 0;
        for (u32 kk = kmin; kk <= kmax && kk < rd.len; kk++) {
            const u32 sc = period_score(rd, pc, kk, P);
            if (sc < min_score) continue;  // wave-uniform, as every branch below
            if (sc > s0) {
                s3 = s2, k3 = k2, s2 = s1, k2 = k1, s1 = s0, k1 = k0, s0 = sc, k0 = kk;
            } else if (sc > s1) {
                s3 = s2, k3 = k2, s2 = s1, k2 = k1, s1 = sc, k1 = kk;
            } else if (sc > s2) {
                s3 = s2, k3 = k2, s2 = sc, k2 = kk;
            } else if (sc > s3) {
                s3 = sc, k3 = kk;
            }
        }
        const u32 found = (k0 != 0u) + (k1 != 0u) + (k2 != 0u) + (k3 != 0u);
        const u32 m = found < C ? found : C;
        // 2. and 3. per candidate the refined record; the largest score, then the smaller period, then the smaller c
        u32 best = 0, best_score = 0, best_period = 0, rank = 0, first_period = 0, first_score = 0;  // best: word i in lane i
        u32 seen = 0;                                                                                // the seed of candidate c in bits 4 c .. 4 c + 3
        for (u32 c = 0; c < m; c++) {
            const u32 k = c == 0u ? k0 : c == 1u ? k1 : c == 2u ? k2 : k3;
            const u32 score = c == 0u ? s0 : c == 1u ? s1 : c == 2u ? s2 : s3;
            u32 rec[16], r_start, r_end;  // the periods tract is for kernels/tandems.inc: not used here
            const bool done = refine_at(rd, pc, k, score, P, h, rec, r_start, r_end, [&](u32 S) {
                bool dup = false;
                for (u32 q = 0; q < c; q++) dup |= __ballot(((seen >> (4u * q)) & 15u) != S) == 0ull;
                seen |= S << (4u * c);  // S <= 8
                return dup;
            });
            if (!done) continue;  // wave-uniform: the record of an earlier candidate but for scored_period, which loses the tie
            const u32 sc = rfl(rec[4]), pd = rfl(rec[0]);
            const u32 x = lane_words(rec, rec[15]);
            if (c == 0u) {
                first_period = pd;
                first_score = sc;
            }
            if (c == 0u || sc > best_score || (sc == best_score && pd < best_period)) {
                best = x;
                best_score = sc;
                best_period = pd;
                rank = c;
            }
        }
        // twenty lanes write the record's twenty words (trew_hip_resolved): one vector store; all zero without a candidate
        const u32 own[4] = {m, rank, first_period, first_score};
        const u32 x = lane_words<4, 16>(own, best);
        if (lane < 20) out[r * 20ull + lane] = x;
    }
}
