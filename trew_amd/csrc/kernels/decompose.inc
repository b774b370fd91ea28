// kernels/decompose.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Units in place with no motif given (trew_hip_decompose): refine.inc's unit of the read, anchored at its smallest rotation,
// and trace.inc's traceback of the read against that rotation on the one strand the unit was found on.  A kernel beside the scan
// and beside the other twelve measures: it reads the same bit planes, takes no pattern table and writes its own records,
// counts, item log and direction workspace.  refine_piece is refine.inc's; the rows and the walk are wrap_fill<32>, wrap_fetch<32>
// and wrap_walk<32> of kernels/wraparound.inc, which trace.inc calls with 64 bytes a row.  This file holds the anchor
// (unit_anchor) and the claim of the rows, the end phase and one walk (trace_tract), which dissect.inc calls as well, and the
// kernel: refine, the two calls, the store.
//
// Definition (DESIGN 4.7i, include/trew_hip.h).  R is the read's trew_hip_refined record.  Without one, or with R.score <
// min_score, the read has no items and anchor 0.  Otherwise M is the smallest of the k = R.period rotations of U = R.unit as
// packed words (the order of the scan's min_rotation; U is primitive, so there is one), anchor the rho with M[j] = U[(j + rho)
// mod k], and the items are those of 4.7h for the forward strand of the read against M, for every k >= 1.
//
// Wave per read on the grid of launch_tracts.  Refine: refine_piece over the whole read, as refine_wave_kernel calls it; then
// unit_anchor and trace_tract below, where the account of the anchor, the rows, the end phase and the walk stands.  No scalar
// stores, no inline assembly.

// The anchor of a record's unit: the rho whose rotation of the k packed bases of `unit` (first base most significant) is the
// smallest as packed words.  Lane j < k forms rotation j as a 2k-bit rotate of the 64-bit word; two wave maxima over the
// complemented halves of the word leave the lanes that hold the smallest, a ballot names the one.  Wave-uniform in and out.
__device__ __forceinline__ u32 unit_anchor(u64 unit, u32 k) {
    const u32 lane = lane_id();
    const u64 mask = k >= 32u ? ~0ull : (1ull << (2u * k)) - 1ull;
    const bool live = lane < k;  // one half forms the rotations
    const u32 sh = live ? 2u * lane : 0u;
    const u64 rot = sh ? ((unit << sh) | (unit >> ((2u * k - sh) & 63u))) & mask : unit;  // rotation `lane`: its base i is U[(i + lane) mod k]
    const u32 nhi = ~(u32) (rot >> 32), nlo = ~(u32) rot;
    bool tie = live & (nhi == wave_max_u32(live ? nhi : 0u));
    tie &= nlo == wave_max_u32(tie ? nlo : 0u);
    const u32 rho = (u32) __builtin_ctzll(__ballot(tie) | (1ull << 63));  // U is primitive: one lane is left
    return rho < k ? rho : 0u;
}

// The items of the tract [start, en) of read rd against M, the rotation rho of `unit`, on one strand, for a record (score, start,
// en, consumed, matches) of a refinement that saw nothing in front of `start` it could have used: the whole read for decompose, a
// piece that holds the tract for dissect.  Words 0 and 1 of an item are w_read and w_motif; every coordinate is the read's.
// Returns the items (counted past lg.cap as well).
//
// Every lane takes its base of M out of the packed unit, lanes 32 .. 63 mirror lanes 0 .. 31 as in refine.inc.  Rows: the
// alignment record of the bases against M is the record in (score, start, end, consumed, matches) -- these do not depend on
// the rotation, only the end phase does -- so there is no pass 1: by fact (b) of trace.inc the table that begins with H = (0,
// start, 0, 0) at row start holds the path, and the wave claims end - start rows of 32 bytes (lanes 0 .. 31 store a byte each:
// half of trace's workspace a base) with one returning atomic and computes them.  End phase: in row `end` of that table the
// lanes whose cell is (score, start, consumed, matches) are the end cells of the full table (the record is the largest tuple
// of that row there, and the restarted table holds nothing larger), the lowest bit of their ballot is rule 3's.  The walk and
// the items are trace.inc's for one strand: blocks of kTraceBlock rows in 2 KB of LDS a wave (blk4), a lane fetches a row as
// two 16-byte loads; one returning atomic an item, twelve lanes store it, nothing at or beyond the capacity while the counter
// keeps counting.  `fits` is decided per tract: rows claimed beyond max_rows are not stored; the walk then fills its block by
// computing the rows from `start` again, as in trace.inc.
__device__ __forceinline__ u32 trace_tract(const ReadRef &rd, const TraceLog &lg, u32 w_read, u32 w_motif, u64 unit, u32 k, u32 rho, u32 score, u32 start,
                                           u32 en, u32 consumed, u32 matches, int P, uint4 *blk4) {
    const u32 lane = lane_id(), j = lane & 31u;
    unsigned char *const blk = (unsigned char *) blk4;
    const u32 at = j >= k ? 0u : j + rho >= k ? j + rho - k : j + rho;  // (j + rho) mod k for the lanes j < k
    const u32 tb = j < k ? (u32) (unit >> (2u * (k - 1u - at))) & 3u : 8u;  // M[j]; both halves alike, an idle lane matches nothing
    u32 src[5];
    wrap_sources(k, src);
    // ---- rows
    const u32 rows = en - start;  // >= 1
    u64 first = 0;
    if (lane == 0) first = atomicAdd(lg.row_counter, (unsigned long long) rows);
    first = rfl64(first);
    const bool fits = first + (u64) rows <= lg.max_rows;
    unsigned char *const ws = lg.rows + first * 32ull;  // formed, not touched, when the rows do not fit
    // the end cell: the lowest phase whose cell of row `end` is the record's tuple
    auto end_phase = [&](const AlignCell &H) {
        const bool is_end = (lane < k) & (H.score == score) & (H.start == start) & (H.consumed == consumed) & (H.matches == matches);
        const u32 p = (u32) __builtin_ctzll(__ballot(is_end) | (1ull << 63));
        return p < k ? p : 0u;  // never: the cell exists (fact (b) of trace.inc)
    };
    u32 jj = 0;
    if (fits) {
        jj = end_phase(wrap_fill<32>(rd, start, en, start, tb, P, k, src, ws, start));
        __threadfence();  // other lanes of this wave read the rows back
    }
    // ---- the walk and the items, one strand
    return wrap_walk<32>(lg, w_read, w_motif, 0u, k, start, en, jj, blk, [&](u32 blk_lo, u32 i) {
        if (fits) {
            wrap_fetch<32>(ws, start, blk4, blk_lo, i);
        } else {
            const AlignCell H = wrap_fill<32>(rd, start, i, start, tb, P, k, src, blk, blk_lo);
            if (i == en) jj = end_phase(H);  // the first block ends at row `end`
        }
    });
}


// kResolved (trew_hip_decompose_resolved, DESIGN 4.7l): resolve_piece (kernels/resolve_piece.inc) over the whole read in the place
// of refine_piece, with `candidates` its C; the record stays word i in lane i, the words the anchor and the rows need are read out
// of it and the store takes it as it is.  <false> is trew_hip_decompose's kernel as it was; it ignores `candidates`.
// Registers.  Left to itself <true> takes 132 VGPRs and three waves a SIMD; asked for four it finds 128 without a spill and without
// scratch, so it asks.  <false> gets (1, 8), which is what a 256-thread block has without the attribute: 126 VGPRs as before.
template <bool kResolved>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kResolved ? 4 : 1, kResolved ? 4 : 8)))
decompose_wave_kernel(DevBatch B, int min_period, int max_period, int penalty, u32 min_score, TraceLog lg,
                                                             u32 *__restrict__ out, u32 *__restrict__ counts, u32 candidates) {
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
    uint4 *const blk4 = dec_lds[(threadIdx.x >> 6) & 3u];
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        u32 rec[16], r_start, r_end;  // the periods tract is for kernels/tandems.inc: not used here
        u32 won = 0;  // kResolved: the record, word i in lane i
        if constexpr (kResolved) {
            u32 m;
            resolve_piece(rd, Piece{0u, rd.len}, kmin, kmax, P, smin, rfl(candidates), h, won, r_start, r_end, m, [](u32, u32, u32, bool) {});
            rec[0] = record_word(won, 0), rec[4] = record_word(won, 4), rec[5] = record_word(won, 5), rec[6] = record_word(won, 6);
            rec[7] = record_word(won, 7), rec[8] = record_word(won, 8), rec[12] = record_word(won, 12), rec[13] = record_word(won, 13);
        } else {
            refine_piece(rd, Piece{0u, rd.len}, kmin, kmax, P, smin, h, rec, r_start, r_end);  // the whole read; all zero without a record
        }
        const u32 k = rfl(rec[0]), score = rfl(rec[4]), start = rfl(rec[5]), en = rfl(rec[6]), consumed_r = rfl(rec[7]), matches_r = rfl(rec[8]);
        u32 rho = 0, found = 0;
        if (k != 0u && score >= smin && en > start && en <= rd.len) {  // wave-uniform; a record's tract lies inside its read
            const u64 unit = ((u64) rfl(rec[13]) << 32) | rfl(rec[12]);
            rho = unit_anchor(unit, k);
            found = trace_tract(rd, lg, (u32) r, 0u, unit, k, rho, score, start, en, consumed_r, matches_r, P, blk4);
        }
        // sixteen lanes write the record's sixteen words (trew_hip_refined), its reserved word the anchor: one vector store
        u32 x;
        if constexpr (kResolved) {
            x = lane == 11u ? rho : won;
        } else {
            x = rec[15];
#pragma unroll
            for (int w = 14; w >= 0; w--) x = lane == (u32) w ? (w == 11 ? rho : rec[w]) : x;
        }
        if (lane < 16) out[r * 16ull + lane] = x;
        if (lane == 0) counts[r] = found;
    }
}
