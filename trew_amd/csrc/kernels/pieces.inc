// kernels/pieces.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// What the every-tract measures share below their own work on a piece (repeats.inc, satellites.inc, dissect.inc), and the two
// smaller things that the other wave-per-read kernels share with them: a record's words spread over lanes (periods.inc,
// refine.inc) and the append of one record to a log (wraparound.inc's wrap_walk for trace.inc, decompose.inc and dissect.inc).
// No kernel here; plain C++ and builtins.  tandems.inc keeps a walk and an append of its own, the one other copy of the walk,
// for the reason given at its head.
//
//   lane_words    rec[N] -> one word per lane, for one vector store of the record
//   log_append    one record into an append log: one returning atomic on the counter, kWords lanes store
//   repeat_worth  a piece that may have a record at all
//   walk_pieces   the recursion over the pieces of one read: the stack, the child order, the containment check, `found`

// this lane's word of a record held wave-uniformly in rec: rec[i] in lane kFirstLane + i, `tail` in every other lane (words
// that follow the record's, as satellites' unit; a caller with none passes rec[N - 1], which costs no select of its own)
template <u32 N, u32 kFirstLane = 0>
__device__ __forceinline__ u32 lane_words(const u32 (&rec)[N], u32 tail) {
    const u32 lane = lane_id();
    u32 x = tail;
#pragma unroll
    for (int i = (int) N - 1; i >= 0; i--) x = lane == kFirstLane + (u32) i ? rec[i] : x;
    return x;
}

// Append one record of kWords words to a log, the whole wave at once: one returning 64-bit vector-memory atomic on the
// counter (lane 0 adds, the others get the index through readfirstlane, as in kernels/chain.inc), then lane i stores `word` as
// word i of the record.  A record at or beyond `cap` is not stored at all while the counter keeps counting.
template <u32 kWords>
__device__ __forceinline__ void log_append(unsigned long long *counter, u32 *recs, u64 cap, u32 word) {
    const u32 lane = lane_id();
    u64 idx = 0;
    if (lane == 0) idx = atomicAdd(counter, 1ull);
    idx = rfl64(idx);
    if (idx < cap && lane < kWords) recs[idx * (u64) kWords + lane] = word;
}

// a piece that may have a record: score_k <= hi - lo - k <= hi - lo - min_period
__device__ __forceinline__ bool repeat_worth(u32 lo, u32 hi, u32 kmin, u32 min_score) {
    const u32 len = hi - lo;
    return len > kmin && len - kmin >= min_score;
}

// what a measure's eval(lo, hi) says of the piece [lo, hi); all but `word` wave-uniform
struct PieceEval {
    bool split;      // the piece has a tract [start, end): its children [lo, start) and [end, hi) are formed
    bool record;     // and a record of that tract (dissect.inc's weak piece has none: it splits around a tract that is used up)
    u32 start, end;  // the tract, in read coordinates
    u32 word;        // this lane's word of the record from lane 2 on; lanes 0 and 1 get the read and the depth here
};

// The pieces of read r of `len` bases, depth first: eval(lo, hi) judges a piece, its record if it has one goes to lg as
// {read, depth, eval's words}, and the walk goes on below it.  Returns the records of the read (counted past lg.cap as well).
// The tract of a split piece is checked here, after eval returns: an eval that does more with a tract than hand it back checks
// it as well, and hands a tract that fails back without a record, which ends the read.
//
// The recursion runs inside the wave, over a wave-uniform stack of (lo, hi, depth) kept across the lanes of three VGPRs
// (entry i in lane i; a push is a store by one lane, a pop a v_readlane with a uniform index).  After a split the LONGER child
// is pushed and the wave continues with the SHORTER, so the piece at hand is at most half the piece its pending sibling came
// from: with f(L) the entries a piece of L bases can add to the stack, f(L) <= 1 + f(L / 2), and a read of fewer than 2^32
// bases never has more than 32 entries pending -- half the 64 lanes.  A piece with hi - lo - min_period < min_score cannot
// have a record (score_k <= len - k) and is neither pushed nor walked, which changes no result.
template <u32 kWords, class Eval>
__device__ __forceinline__ u32 walk_pieces(u64 r, u32 len, u32 kmin, u32 smin, const RepeatLog &lg, Eval &&eval) {
    const u32 lane = lane_id();
    u32 st_lo = 0, st_hi = 0, st_d = 0;  // the stack: entry i in lane i
    u32 sp = 0;                          // entries pending (wave-uniform, at most 32: see above)
    u32 lo = 0, hi = len, depth = 0;     // the piece at hand
    u32 found = 0;
    bool have = repeat_worth(lo, hi, kmin, smin);
    while (have) {  // wave-uniform
        const PieceEval e = eval(lo, hi);
        u32 a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;  // the children; a the shorter
        if (e.split) {
            const u32 start = rfl(e.start), end = rfl(e.end);
            // a tract lies inside its piece; the pieces below are formed from it, so nothing else may ever reach them
            if (!(start >= lo && end <= hi && start < end)) break;
            if (e.record) {
                found++;
                u32 x = e.word;
                x = lane == 1u ? depth : x;
                x = lane == 0u ? (u32) r : x;
                log_append<kWords>(lg.counter, lg.recs, lg.cap, x);
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
        if (e.split && repeat_worth(a_lo, a_hi, kmin, smin)) {  // go on with the shorter child
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
    return found;
}
