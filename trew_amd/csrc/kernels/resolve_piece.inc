// kernels/resolve_piece.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// resolve's period choice for one piece of a read (DESIGN 4.7l): what trew_hip_resolve's steps 1 to 3 give the bases [lo, hi) taken
// as a read of their own.  No kernel here: the device function that the <true> instantiations of tandems_wave_kernel,
// decompose_wave_kernel and dissect_wave_kernel call where their <false> instantiations call refine_piece, and that
// resolve_wave_kernel calls for the whole read.  Plain C++ and builtins.
//
// Stage 1 is refine_piece's loop over k with period_score; it keeps the four best (score, k) pairs in wave-uniform registers, an
// insertion into a sorted list written out: strictly greater displaces, so the smaller k keeps a tie.  The first C of the four
// are the first C of the whole order.  No extra pass over the piece.
//
// The candidate loop is a runtime loop around one inlined refine_at.  period_consensus wants the wave's bins zero on entry and
// leaves them zero, so the loop clears nothing, across candidates and across pieces.  A candidate whose primitive seed equals an
// earlier candidate's code for code gives the same record up to scored_period and loses the tie: its three passes walk no base
// (refine_at's skip).  The earlier seeds are kept four bits a candidate in one register (lane j: base j, 8 past the seed's
// length, both halves alike), the compare is a ballot.  A rotation of an earlier seed differs in some lane and is aligned.
//
// Best so far: the winner's sixteen words in one register, word i in lane i (lane_words), with its score and period wave-uniform
// beside it.  The record stays in the lanes: a caller reads the few words it computes with by v_readlane and stores the
// register as it is (or moved two lanes up, behind read and depth), instead of sixteen wave-uniform values held across its own work.

// The resolved record of one piece: `best` = the winner's sixteen words of trew_hip_refined, word i in lane i (lanes 16 .. 63: word
// 15), start and end in read coordinates, scored_period the winner's k; all zero without a candidate, and false.  Otherwise true,
// with r_start and r_end the periods tract of candidate 0, in read coordinates: the tract refine_piece hands out (a weak piece is
// split there).  note(c, score, period, taken): called once per aligned candidate, wave-uniform, for what resolve's own record
// keeps beside the winner.  Returns the number of candidates through m.  Wave-uniform.  h: the wave's bins, zero on entry and exit.
template <class Note>
__device__ __forceinline__ bool resolve_piece(const ReadRef &rd, Piece pc, u32 kmin, u32 kmax, int P, u32 min_score, u32 C, u32 *h, u32 &best, u32 &r_start,
                                              u32 &r_end, u32 &m, Note note) {
    // 1. scores: the four best (score, k) with score >= min_score (>= 1), score descending, k ascending; k = 0: no entry
    u32 s0 = 0, s1 = 0, s2 = 0, s3 = 0, k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    for (u32 kk = kmin; kk <= kmax && kk < pc.hi - pc.lo; kk++) {
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
    m = found < C ? found : C;
    // 2. and 3. per candidate the refined record; the largest score, then the smaller period, then the smaller c
    u32 best_score = 0, best_period = 0;
    u32 seen = 0;  // the seed of candidate c in bits 4 c .. 4 c + 3
    best = 0;
    r_start = 0;
    r_end = 0;
    for (u32 c = 0; c < m; c++) {
        const u32 k = c == 0u ? k0 : c == 1u ? k1 : c == 2u ? k2 : k3;
        const u32 score = c == 0u ? s0 : c == 1u ? s1 : c == 2u ? s2 : s3;
        u32 rec[16], c_start, c_end;
        const bool done = refine_at(rd, pc, k, score, P, h, rec, c_start, c_end, [&](u32 S) {
            bool dup = false;
            for (u32 q = 0; q < c; q++) dup |= __ballot(((seen >> (4u * q)) & 15u) != S) == 0ull;
            seen |= S << (4u * c);  // S <= 8
            return dup;
        });
        if (c == 0u) {  // candidate 0 is never skipped
            r_start = rfl(c_start);
            r_end = rfl(c_end);
        }
        if (!done) continue;  // wave-uniform: the record of an earlier candidate but for scored_period, which loses the tie
        const u32 sc = rfl(rec[4]), pd = rfl(rec[0]);
        const u32 x = lane_words(rec, rec[15]);
        const bool taken = c == 0u || sc > best_score || (sc == best_score && pd < best_period);
        if (taken) {
            best = x;
            best_score = sc;
            best_period = pd;
        }
        note(c, sc, pd, taken);
    }
    return m != 0u;
}

// word i of a record held word i in lane i, wave-uniform
__device__ __forceinline__ u32 record_word(u32 rec, u32 i) { return (u32) __builtin_amdgcn_readlane((int) rec, (int) i); }
