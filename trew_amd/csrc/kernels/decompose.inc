// kernels/decompose.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Units in place with no motif given (trew_hip_decompose): refine.inc's unit of the read, anchored at its smallest rotation,
// and trace.inc's traceback of the read against that rotation on the one strand the unit was found on.  A kernel beside the scan
// and beside the other twelve measures: it reads the same bit planes, takes no pattern table and writes its own records,
// counts, item log and direction workspace.  refine_piece, the cells and the lane reads of align.inc and trace_row are used,
// not changed; the fill is written again here because a row has one strand.
//
// Definition (DESIGN 4.7i, include/trew_hip.h).  R is the read's trew_hip_refined record.  Without one, or with R.score <
// min_score, the read has no items and anchor 0.  Otherwise M is the smallest of the k = R.period rotations of U = R.unit as
// packed words (the order of the scan's min_rotation; U is primitive, so there is one), anchor the rho with M[j] = U[(j + rho)
// mod k], and the items are those of 4.7h for the forward strand of the read against M, for every k >= 1.
//
// Wave per read on the grid of launch_tracts.  Refine: refine_piece over the whole read, as refine_wave_kernel calls it.
// Anchor: lane j < k forms rotation j of the packed unit as a 2k-bit rotate of the 64-bit word; two wave maxima over the
// complemented halves of the word leave the lanes that hold the smallest, a ballot names the one; every lane then takes its
// base of M out of the packed unit, lanes 32 .. 63 mirror lanes 0 .. 31 as in refine.inc.  Rows: the alignment record of the
// read against M is R in (score, start, end, consumed, matches) -- these do not depend on the rotation, only the end phase does
// -- so there is no pass 1: by fact (b) of trace.inc the table that begins with H = (0, start, 0, 0) at row start holds the
// path, and the wave claims end - start rows of 32 bytes (lanes 0 .. 31 store a byte each: half of trace's workspace a base)
// with one returning atomic and computes them.  End phase: in row `end` of that table the lanes whose cell is (R.score, R.start,
// R.consumed, R.matches) are the end cells of the full table (R is the largest tuple of that row there, and the restarted
// table holds nothing larger), the lowest bit of their ballot is rule 3's.  The walk and the items are trace.inc's for one
// strand: blocks of kTraceBlock rows in 2 KB of LDS a wave, a lane fetches a row as two 16-byte loads; one returning atomic an
// item, twelve lanes store it, nothing at or beyond the capacity while the counter keeps counting.  Rows claimed beyond max_rows
// are not stored; the walk then fills its block by computing the rows from `start` again, as in trace.inc.  No scalar
// stores, no inline assembly.

// Rows from + 1 .. to of the table that starts from (0, from, 0, 0) in every phase at row from; lanes 0 .. 31 store the byte of
// row i > keep at dst[(i - keep - 1) * 32 + lane].  Returns H of row `to`.
__device__ __forceinline__ AlignCell decompose_fill(const ReadRef &rd, u32 from, u32 to, u32 tb, int P, u32 k, const u32 (&src)[5], unsigned char *dst,
                                                    u32 keep, u32 lane) {
    AlignCell H{0, from, 0, 0};
    u32 lo = 0, hi = 0, nm = 0;
    for (u32 i = from + 1u; i <= to; i++) {
        const u32 p = i - 1u, b = p & 31u;
        if (b == 0u || p == from) {
            const u64 w = p >> 5;
            lo = rfl(rd.w[3ull * w + 0]), hi = rfl(rd.w[3ull * w + 1]), nm = rfl(rd.w[3ull * w + 2]);
        }
        const u32 c = ((lo >> b) & 1u) | (((hi >> b) & 1u) << 1) | (((nm >> b) & 1u) << 2);
        const u32 byte = trace_row(H, c, tb, i, P, k, src);
        if (i > keep && lane < 32u) dst[(u64) (i - keep - 1u) * 32ull + lane] = (unsigned char) byte;
    }
    return H;
}

__global__ void __launch_bounds__(256) decompose_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, TraceLog lg,
                                                             u32 *__restrict__ out, u32 *__restrict__ counts) {
    __shared__ u32 bins[4][kPeriodBins];
    __shared__ uint4 dec_lds[4][kTraceBlock * 2u];
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
    const u32 j = lane & 31u, half = lane & 32u;
    uint4 *const blk4 = dec_lds[(threadIdx.x >> 6) & 3u];
    unsigned char *const blk = (unsigned char *) blk4;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        u32 rec[16], r_start, r_end;  // the periods tract is for kernels/tandems.inc: not used here
        refine_piece(rd, Piece{0u, rd.len}, kmin, kmax, P, smin, h, rec, r_start, r_end);  // the whole read; all zero without a record
        const u32 k = rfl(rec[0]), score = rfl(rec[4]), start = rfl(rec[5]), en = rfl(rec[6]), consumed_r = rfl(rec[7]), matches_r = rfl(rec[8]);
        u32 rho = 0, found = 0;
        if (k != 0u && score >= smin && en > start && en <= rd.len) {  // wave-uniform; a record's tract lies inside its read
            // ---- anchor: the smallest rotation of the packed unit, first base most significant
            const u64 unit = ((u64) rfl(rec[13]) << 32) | rfl(rec[12]);
            const u64 mask = k >= 32u ? ~0ull : (1ull << (2u * k)) - 1ull;
            const bool live = lane < k;  // one half forms the rotations
            const u32 sh = live ? 2u * lane : 0u;
            const u64 rot = sh ? ((unit << sh) | (unit >> ((2u * k - sh) & 63u))) & mask : unit;  // rotation `lane`: its base i is U[(i + lane) mod k]
            const u32 nhi = ~(u32) (rot >> 32), nlo = ~(u32) rot;
            bool tie = live & (nhi == wave_max_u32(live ? nhi : 0u));
            tie &= nlo == wave_max_u32(tie ? nlo : 0u);
            rho = (u32) __builtin_ctzll(__ballot(tie) | (1ull << 63));  // U is primitive: one lane is left
            rho = rho < k ? rho : 0u;
            const u32 at = j >= k ? 0u : j + rho >= k ? j + rho - k : j + rho;  // (j + rho) mod k for the lanes j < k
            const u32 tb = j < k ? (u32) (unit >> (2u * (k - 1u - at))) & 3u : 8u;  // M[j]; both halves alike, an idle lane matches nothing
            u32 src[5];
#pragma unroll
            for (int t = 0; t < 5; t++) {
                int q = ((int) j - (1 << t)) % (int) k;
                q = q < 0 ? q + (int) k : q;
                src[t] = (half | (u32) q) << 2;
            }
            // ---- rows
            const u32 rows = en - start;  // >= 1
            u64 first = 0;
            if (lane == 0) first = atomicAdd(lg.row_counter, (unsigned long long) rows);
            first = rfl64(first);
            const bool fits = first + (u64) rows <= lg.max_rows;
            unsigned char *const ws = lg.rows + first * 32ull;
            // the end cell: the lowest phase whose cell of row `end` is the record's tuple
            auto end_phase = [&](const AlignCell &H) {
                const bool is_end = (lane < k) & (H.score == score) & (H.start == start) & (H.consumed == consumed_r) & (H.matches == matches_r);
                const u32 p = (u32) __builtin_ctzll(__ballot(is_end) | (1ull << 63));
                return p < k ? p : 0u;  // never: the cell exists (fact (b) of trace.inc)
            };
            u32 jj = 0;
            if (fits) {
                jj = end_phase(decompose_fill(rd, start, en, tb, P, k, src, ws, start, lane));
                __threadfence();  // other lanes of this wave read the rows back
            }
            // ---- the walk and the items: trace.inc's, one strand
            u32 i = en, seg_end = i, consumed = 0, sub = 0, ins = 0, del = 0, phase = 0, cols = 0, run = 0, run_start = 0;
            u32 blk_lo = i;  // the block holds the rows blk_lo + 1 .. : none yet
            auto emit = [&](u32 e_start, u32 e_bases, u32 e_count, u32 e_phase, u32 e_consumed, u32 e_sub, u32 e_ins, u32 e_del) {
                found++;
                const u32 v = lane == 0u ? (u32) r : lane == 3u ? e_start : lane == 4u ? e_bases : lane == 5u ? e_count : lane == 6u ? e_phase
                            : lane == 7u ? e_consumed : lane == 8u ? e_sub : lane == 9u ? e_ins : lane == 10u ? e_del : 0u;  // motif = strand = 0
                log_append<kTraceWords>(lg.counter, lg.recs, lg.cap, v);
            };
            auto flush_run = [&]() {
                if (run) emit(run_start, run * k, run, 0, run * k, 0, 0, 0);
                run = 0;
            };
            auto close = [&]() {  // the running segment begins at read base i
                if (phase == 0 && consumed == k && (sub | ins | del) == 0) {
                    run++;
                    run_start = i;
                } else {
                    flush_run();
                    emit(i, seg_end - i, 1, phase, consumed, sub, ins, del);
                }
                seg_end = i;
                consumed = sub = ins = del = phase = cols = 0;
            };
            while (i > start) {
                if (i <= blk_lo) {  // the next block: the rows blk_lo + 1 .. i
                    blk_lo = i - start > kTraceBlock ? i - kTraceBlock : start;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    if (fits) {
                        const u32 row = blk_lo + 1u + lane;
                        if (row <= i) {
                            const uint4 *g = (const uint4 *) (ws + (u64) (row - start - 1u) * 32ull);
                            const uint4 a = g[0], b = g[1];
                            blk4[lane * 2u + 0u] = a;
                            blk4[lane * 2u + 1u] = b;
                        }
                    } else {
                        const AlignCell H = decompose_fill(rd, start, i, tb, P, k, src, blk, blk_lo, lane);
                        if (i == en) jj = end_phase(H);  // the first block ends at row `end`
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                const unsigned char *row = blk + (i - blk_lo - 1u) * 32u;
                const u32 d = rfl((u32) row[jj]) >> 2 & 31u;
                for (u32 q = 0; q < d; q++) {
                    phase = jj;
                    consumed++, del++, cols++;
                    if (jj == 0) close();
                    jj = jj ? jj - 1u : k - 1u;
                }
                const u32 cell = rfl((u32) row[jj]);
                const u32 op = cell & 3u;
                if (op == 0) break;  // never: the fresh start lies in row `start`
                i--;
                cols++;
                if (op == 1) {
                    phase = jj;
                    consumed++;
                    sub += (cell >> 7) ^ 1u;
                    if (jj == 0) close();
                    jj = jj ? jj - 1u : k - 1u;
                } else {
                    ins++;
                }
            }
            if (cols) close();
            flush_run();
        }
        // sixteen lanes write the record's sixteen words (trew_hip_refined), its reserved word the anchor: one vector store
        u32 x = rec[15];
#pragma unroll
        for (int w = 14; w >= 0; w--) x = lane == (u32) w ? (w == 11 ? rho : rec[w]) : x;
        if (lane < 16) out[r * 16ull + lane] = x;
        if (lane == 0) counts[r] = found;
    }
}
