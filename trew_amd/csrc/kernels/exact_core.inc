// kernels/exact_core.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// The exact path of one segment: LDS working set, class counting by runs (Lemma A), lane bounds, decide (the selection loops), emission; run_short / run_segment.

// ------------------------------------------------------------------ exact path
// LDS working set of one wave, carved from dynamic LDS and sized by the longest
// segment of the batch (cap bases, a multiple of 64): 2.6 KB for 150-bp reads, so
// 8 waves per SIMD stay resident and hide the global/LDS latency chains.
// The struct only carries the two sizes (it travels in SGPRs); every array is an
// offset from the dynamic-LDS base so that accesses compile to ds_* instructions.
//   seq   [2][cap/32+2] u64  2-bit bases, first base most significant (KmerSeq orientation, kmer.h:77)
//   vmask [cap/64+2] u64  bit i: window i has no N
//   emask [cap/64+2] u64  bit i: base i == base i+k (Lemma A: windows i, i+1 share a class)
//   nmask [2][cap/32+2] u32  bit i = base i is not A/C/G/T or lies past the end of the staged range
// seq/nmask hold a whole read (two of them: both mates of a pair), staged ONCE per read; a segment
// is a view: s0 = its first base inside the staged bases.  Windows never reach past the segment
// (i < L-k+1), so the view needs no end mask of its own.  Long reads do not fit: the long driver
// stages one slice at a time at base 0.
//   raw   [kRawReads][rawwords] u32  packed triples of the reads of two chunks (short driver) or of the two mates, staged once
//   cnt   [cap] u16  class size at the class's first item, else 0
//   start [cap] u16  first window of each run
//   intent [kIntentWords] u32  per-chunk read descriptors of the short/segment/pair drivers' chunk pipeline (two buffers)
//   group  [kGroupWords] u32  working set of decide_group (packed bounds, multiples masks, results)
//   ckey/cpart/ccnt [kCacheSlots]  the wave's private count cache (see cached_add)
//   canon [cap]  WT   per run (fast path) or per window (fallback); WT = u64 (k <= 32) or u128
struct ExactSmem {
    u32 lds;  // LDS offset of the wave's dynamic-LDS working set, taken in the kernel (see lds_at)
    u32 cap, rawwords;
    u32 s0;         // first base of the current segment within the staged bases
    u32 rs, rnw;    // the same segment in the read's packed triples: first base, triples of the read
    const u32 *rw;  // the read's triples (LDS copy or global), nullptr when unknown
};
__host__ __device__ inline u32 exact_rangewords(u32 cap) { return cap / 32 + 2; }  // words of one staged range (+ read-ahead)

constexpr u32 kCacheSlots = 128;
constexpr u32 kRawReads = 8;      // raw[]: two buffers of four reads (the short driver's chunk pipeline; the pair driver uses the first two)
constexpr u32 kIntentWords = 64;  // intent[]: two buffers of 32 words of chunk descriptors
// decide_group (kernels/decide_group.inc): bnd [4][32] packed lane bounds of the four segments of a pass, mult [32] the k-index
// masks of the multiples of every k of the run, gres [4][8] what the pass decided per segment
constexpr u32 kGroupBnd = 0, kGroupMult = 128, kGroupRes = 160, kGroupWords = 192;
constexpr u32 kGroupPairIndex = kGroupRes + 31;  // TREW_FLAG_COMPAT_G1: the index of the pair whose whole-read block emit_k is logging (gres is the short driver's)
__host__ __device__ inline u32 exact_lds_precache(u32 cap, u32 rawwords) {  // everything before the count cache, 16-byte aligned
    const u32 b = 2 * exact_rangewords(cap) * 8 + 2 * (cap / 64 + 2) * 8 + 2 * exact_rangewords(cap) * 4 + kRawReads * rawwords * 4 + 2 * cap * 2 + (kIntentWords + kGroupWords) * 4;
    return (b + 15u) & ~15u;
}
__host__ __device__ inline u32 exact_lds_fixed(u32 cap, u32 rawwords) {  // everything before canon[], 16-byte aligned
    return exact_lds_precache(cap, rawwords) + kCacheSlots * 16u;
}
constexpr u32 kSaveItems = 16, kSaveSlots = 6;  // pair driver: class tables kept per slot between decide and flush
__host__ __device__ inline u32 exact_lds_bytes(u32 cap, u32 rawwords, u32 wordbytes) {
    return exact_lds_fixed(cap, rawwords) + cap * wordbytes + 16 + kSaveSlots * kSaveItems * (wordbytes + 2u);
}

__device__ __forceinline__ unsigned char *lds0() {
    extern __shared__ __attribute__((aligned(16))) unsigned char trew_lds[];
    return trew_lds;
}
// The same address inside the noinline device functions.  There the compiler does not know which kernel called, so naming
// the extern __shared__ array costs a look-up of the kernel's dynamic-LDS offset in a table in memory (s_getpc + s_load +
// s_waitcnt, up to three times per function: eval_runs did it three times per call).  The kernel takes the offset once
// (lds_offset_in_kernel, a compile-time constant there) and hands it down in ExactSmem.
typedef __attribute__((address_space(3))) unsigned char lds_byte;
__device__ __forceinline__ u32 lds_offset_in_kernel() { return (u32) (unsigned long) (lds_byte *) lds0(); }
__device__ __forceinline__ unsigned char *lds_at(ExactSmem sm) { return (unsigned char *) (lds_byte *) (unsigned long) sm.lds; }
// Phase profile (tools/phase_profile.py, built with -DTREW_PHASE_PROFILE only): lane 0 of each wave
// accumulates s_memtime deltas per phase in LDS and adds them to g_phase when the wave retires.
#ifdef TREW_PHASE_PROFILE
__device__ unsigned long long g_phase[32];
__device__ __forceinline__ unsigned long long *ph_lds() {
    __shared__ unsigned long long ph[32];
    return ph;
}
#define PH_T0(v) const unsigned long long v = (unsigned long long) clock64()
#define PH_ADD(i, v)                                                                  \
    do {                                                                              \
        if (lane_id() == 0) ph_lds()[i] += (unsigned long long) clock64() - (v);      \
    } while (0)
#define PH_CNT(i, c)                                   \
    do {                                               \
        if (lane_id() == 0) ph_lds()[i] += (c);        \
    } while (0)
#else
#define PH_T0(v)
#define PH_ADD(i, v)
#define PH_CNT(i, c)
#endif
enum { PH_TOTAL = 0, PH_STAGE, PH_LOADSEG, PH_BOUNDS, PH_DECIDE, PH_RUNS, PH_WINDOWS, PH_RECORD_EVAL, PH_EMIT, PH_FLUSH, PH_EVALK_A, PH_PAIR_STAGE, PH_PAIR_FLUSH, PH_PAIR_FWD, PH_PAIR_BWD, PH_PAIR_WHOLE,
       PH_N_READS = 16, PH_N_RUNS_CALLS, PH_N_WINDOWS_CALLS, PH_N_RECORD, PH_N_RUNS_TOTAL, PH_N_K5 };

__device__ __forceinline__ u64 *sm_seq(ExactSmem sm) { return (u64 *) lds_at(sm); }
__device__ __forceinline__ u64 *sm_vmask(ExactSmem sm) { return sm_seq(sm) + 2 * exact_rangewords(sm.cap); }
__device__ __forceinline__ u64 *sm_emask(ExactSmem sm) { return sm_vmask(sm) + (sm.cap / 64 + 2); }
__device__ __forceinline__ u32 *sm_nmask(ExactSmem sm) { return (u32 *) (sm_emask(sm) + (sm.cap / 64 + 2)); }
__device__ __forceinline__ u32 *sm_raw(ExactSmem sm) { return sm_nmask(sm) + 2 * exact_rangewords(sm.cap); }
__device__ __forceinline__ unsigned short *sm_cnt(ExactSmem sm) { return (unsigned short *) (sm_raw(sm) + kRawReads * sm.rawwords); }
__device__ __forceinline__ unsigned short *sm_start(ExactSmem sm) { return sm_cnt(sm) + sm.cap; }
__device__ __forceinline__ u32 *sm_intent(ExactSmem sm) { return (u32 *) (sm_start(sm) + sm.cap); }
__device__ __forceinline__ u32 *sm_group(ExactSmem sm) { return sm_intent(sm) + kIntentWords; }  // kGroupWords words, see kGroup*
__device__ __forceinline__ u64 *sm_ckey(ExactSmem sm) { return (u64 *) (lds_at(sm) + exact_lds_precache(sm.cap, sm.rawwords)); }
__device__ __forceinline__ u32 *sm_cpart(ExactSmem sm) { return (u32 *) (sm_ckey(sm) + kCacheSlots); }
__device__ __forceinline__ u32 *sm_ccnt(ExactSmem sm) { return sm_cpart(sm) + kCacheSlots; }
template <typename WT>
__device__ __forceinline__ WT *sm_canon(ExactSmem sm) { return (WT *) (lds_at(sm) + exact_lds_fixed(sm.cap, sm.rawwords)); }
template <typename WT>
__device__ __forceinline__ WT *sm_save_canon(ExactSmem sm) { return sm_canon<WT>(sm) + sm.cap + 16 / sizeof(WT); }  // [kSaveSlots][kSaveItems]
template <typename WT>
__device__ __forceinline__ unsigned short *sm_save_cnt(ExactSmem sm) { return (unsigned short *) (sm_save_canon<WT>(sm) + kSaveSlots * kSaveItems); }

__device__ __forceinline__ ExactSmem uni(ExactSmem sm) {
    sm.lds = rfl(sm.lds);
    sm.cap = rfl(sm.cap);
    sm.rawwords = rfl(sm.rawwords);
    sm.s0 = rfl(sm.s0);
    sm.rs = rfl(sm.rs);
    sm.rnw = rfl(sm.rnw);
    sm.rw = rfl_ptr(sm.rw);
    return sm;
}
// the same for the run's parameters where a noinline function takes them by value
__device__ __forceinline__ DevParams uni(DevParams p) {
    p.min_mer = rfl_i(p.min_mer);
    p.max_mer = rfl_i(p.max_mer);
    p.low = rfl_f64(p.low);
    p.high = rfl_f64(p.high);
    p.lowf = __int_as_float(rfl_i(__float_as_int(p.lowf)));
    p.slice_len = rfl_i(p.slice_len);
    p.mode = rfl_i(p.mode);
    p.flags = rfl(p.flags);
    return p;
}
// The exact kernels carry the table descriptor as a POINTER (two SGPRs) to their own by-value copy of it in the kernarg segment
// (exact_kernel) and read its nine dwords with scalar loads where rows are actually added (emit_k, cache_flush, the pair driver's merged flush).  Passed
// by value it was live across the whole read loop: the register allocator kept it in spill lanes and reloaded all nine
// dwords in front of each of the 21 call sites that forward it (250 of the short-read kernel's 570 static v_readlane
// reloads, profiles/r03/README.md).
typedef const DevTable *TableRef;
__device__ __forceinline__ DevTable load_table(TableRef p) {
    // the constant address space: read-only for the kernel's lifetime, so a wave-uniform load is an s_load (cf. load_thr8)
    typedef const __attribute__((address_space(4))) u64 *c64;
    typedef const __attribute__((address_space(4))) u32 *c32;
    const u64 a = rfl64((u64) p);
    DevTable T;
    T.keys = (u64 *) *(c64) (a + offsetof(DevTable, keys));
    T.counts = (u64 *) *(c64) (a + offsetof(DevTable, counts));
    T.log2_part_slots = *(c32) (a + offsetof(DevTable, log2_part_slots));
    T.overflow = (u32 *) *(c64) (a + offsetof(DevTable, overflow));
    // the wide-table descriptor sits in the same kernel argument (DevTableG1::w): the kernels read the dispatch's own copy of it,
    // as they do for the narrow table, not the device-resident one t.wide points to (that one serves the table kernels)
    T.wide = (const DevWide *) (a + offsetof(DevTableG1, w));
    return T;
}

__device__ __forceinline__ u64 spread32(u32 v) {
    u64 x = v;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// stage bases [s, s+L) of a read into LDS (one wave)
// copy a read's triples into LDS once; later segment staging reads LDS, not HBM
__device__ ReadRef stage_read(ExactSmem sm, const ReadRef &rd, int mate) {
    u32 *dst = sm_raw(sm) + (u32) mate * sm.rawwords;
    const u32 n = 3u * rd.nw;
    if (n > sm.rawwords) return rd;  // does not fit (long mode): keep reading global memory
    for (u32 j = lane_id(); j < n; j += 64) dst[j] = rd.w[j];
    ReadRef r = rd;
    r.w = dst;
    return r;
}

// stage bases [s, s+L) of a read as range `range` (0 or 1) of seq[] / nmask[] (one wave)
__attribute__((noinline)) __device__ void stage_bases(ExactSmem sm, ReadRef rd, u32 s, u32 L, u32 range) {
    PH_T0(t_ph);
    sm = uni(sm);
    rd.w = rfl_ptr(rd.w);
    rd.len = rfl(rd.len);
    rd.nw = rfl(rd.nw);
    s = rfl(s);
    L = rfl(L);
    range = rfl(range);
    __syncthreads();
    const u32 nwords = (L + 31u) >> 5;
    const u32 segwords = exact_rangewords(sm.cap);
    u64 *seq = sm_seq(sm) + range * segwords;
    u32 *nmk = sm_nmask(sm) + range * segwords;
    for (u32 lane = lane_id(); lane < segwords; lane += 64) {
        u64 sq = 0;
        u32 nmv = 0xffffffffu;
        if (lane < nwords) {
            u32 lo[1], hi[1], nm[1];
            load_planes<1>(rd, s + 32u * lane, lo, hi, nm);
            nmv = nm[0] | ~low_mask<true>((int) L - 32 * (int) lane);
            const u32 l = lo[0] & ~nmv, h = hi[0] & ~nmv;
            sq = spread32(__brev(l)) | (spread32(__brev(h)) << 1);
        }
        seq[lane] = sq;
        nmk[lane] = nmv;
    }
    __syncthreads();
    PH_ADD(PH_LOADSEG, t_ph);
}
// first base of staged range r
__device__ __forceinline__ u32 range_base(ExactSmem sm, u32 r) { return r * 32u * exact_rangewords(sm.cap); }
// the segment [s, s+L) of a read whose bases are staged as range r: a view, nothing moves
__device__ __forceinline__ ExactSmem view_segment(ExactSmem sm, u32 r, u32 s, const ReadRef &rd) {
    sm.s0 = range_base(sm, r) + s;
    sm.rs = s;
    sm.rnw = rd.nw;
    sm.rw = rd.w;
    return sm;
}
// long mode: stage one slice at base 0 and look at it
__device__ __forceinline__ ExactSmem load_segment(ExactSmem sm, ReadRef rd, u32 s, u32 L) {
    stage_bases(sm, rd, s, L, 0);
    sm.s0 = 0;
    sm.rs = s;
    sm.rnw = rd.nw;
    sm.rw = rd.w;
    return sm;
}


template <typename WT>
__device__ __forceinline__ WT kmask(int k) {
    return 2 * k >= (int) (8 * sizeof(WT)) ? ~(WT) 0 : ((((WT) 1) << (2 * k)) - 1);
}
__device__ __forceinline__ u32 popc_word(u64 w) { return (u32) __popcll(w); }
__device__ __forceinline__ u32 popc_word(u128 w) { return (u32) __popcll((u64) w) + (u32) __popcll((u64) (w >> 64)); }

// value of lane `src` (wave-uniform index) for every lane
__device__ __forceinline__ u64 readlane_word(u64 v, int src) {
    const u32 lo = (u32) __builtin_amdgcn_readlane((int) (u32) v, src), hi = (u32) __builtin_amdgcn_readlane((int) (u32) (v >> 32), src);
    return ((u64) hi << 32) | lo;
}
__device__ __forceinline__ u128 readlane_word(u128 v, int src) {
    return ((u128) readlane_word((u64) (v >> 64), src) << 64) | readlane_word((u64) v, src);
}

// get_rot_seq / get_rot_seq_128, kmer.cpp:1815-1833
template <typename WT>
__device__ __forceinline__ WT min_rotation(WT w, int k) {
    const int sh = 2 * (k - 1);
    if (k <= 16) {  // wave-uniform: the 2k-bit word fits 32 bits
        // rotation i (right by i bases) = bits [2i, 2i+2k) of the word written twice
        const u32 w32 = (u32) w;
        const u64 dup = ((u64) w32 << (2 * k)) | w32;
        const u32 dlo = (u32) dup, dhi = (u32) (dup >> 32);
        const u32 km = low_mask<true>(2 * k);
        u32 ans = w32;
        if (k <= 8) {  // the doubled word fits 32 bits: one bit-field extract per rotation
            for (int i = 1; i < k; i++) ans = min(ans, __builtin_amdgcn_ubfe(dlo, 2u * (u32) i, 2u * (u32) k));
        } else {
            for (int i = 1; i < k; i++) ans = min(ans, alignbit(dhi, dlo, 2u * (u32) i) & km);
        }
        return ans;
    }
    if (sizeof(WT) > 8 && k <= 32) {  // fits 64 bits
        u64 tmp = (u64) w, ans = (u64) w;
        for (int i = 0; i < k - 1; i++) {
            tmp = ((tmp & 3ull) << sh) | (tmp >> 2);
            ans = tmp < ans ? tmp : ans;
        }
        return ans;
    }
    WT tmp = w, ans = w;
    for (int i = 0; i < k - 1; i++) {
        tmp = ((tmp & 3) << sh) | (tmp >> 2);
        ans = tmp < ans ? tmp : ans;
    }
    return ans;
}
// reverse the 32 2-bit groups of a 64-bit word and complement them
// (bit reversal is one v_bfrev per half; it also swaps the two bits of every group, which one more step undoes)
__device__ __forceinline__ u64 revcomp_groups64(u64 x) {
    const u32 lo = __brev((u32) (x >> 32)), hi = __brev((u32) x);  // reversed halves, swapped
    const u32 l2 = ((lo >> 1) & 0x55555555u) | ((lo & 0x55555555u) << 1), h2 = ((hi >> 1) & 0x55555555u) | ((hi & 0x55555555u) << 1);
    return ~(((u64) h2 << 32) | l2);
}
// reverse_complement_64(x) >> 2*(32-k), kmer.cpp:47-54 / 1987
__device__ __forceinline__ u64 revcomp(u64 x, int k) { return revcomp_groups64(x) >> (2 * (32 - k)); }
// reverse_complement_128(x) >> 2*(64-k), kmer.cpp:62-70
__device__ __forceinline__ u128 revcomp(u128 x, int k) {
    const u128 r = ((u128) revcomp_groups64((u64) x) << 64) | revcomp_groups64((u64) (x >> 64));
    return r >> (2 * (64 - k));
}
// get_repeat_check, kmer.cpp:1835-1867: the word uses a single base
template <typename WT>
__device__ __forceinline__ bool is_homopolymer(WT w, int k) {
    WT fives = (WT) 0x5555555555555555ull;
    if (sizeof(WT) > 8) fives |= fives << 64 % (8 * sizeof(WT));
    return w == ((w & 3) * (fives & kmask<WT>(k)));
}

template <typename WT>
struct KStat {
    u32 count;   // K_MER_DATA_COUNT
    u32 maxc;    // K_MER_DATA_MAX
    WT maxseq;   // K_MER_DATA_MAX_SEQ
    u32 n_items; // entries of canon[]/cnt[] left in LDS for emit_k
    bool pruned; // the bucket bound proved MAX/COUNT < need: maxc/maxseq were not computed
};

__device__ __forceinline__ u64 rfl_word(u64 v) { return rfl64(v); }
__device__ __forceinline__ u128 rfl_word(u128 v) { return ((u128) rfl64((u64) (v >> 64)) << 64) | rfl64((u64) v); }
// A KStat / Decision returned by a noinline function arrives in VGPRs; every field is wave-uniform.
// Saying so keeps the drivers' control state (chain counters, thresholds, intent lists) in SGPRs.
template <typename WT>
__device__ __forceinline__ KStat<WT> uni(KStat<WT> st) {
    st.count = rfl(st.count);
    st.maxc = rfl(st.maxc);
    st.maxseq = rfl_word(st.maxseq);
    st.n_items = rfl(st.n_items);
    st.pruned = rfl((u32) st.pruned) != 0;
    return st;
}

__device__ __forceinline__ u32 base_at(ExactSmem sm, u32 p) {
    p += sm.s0;
    return (u32) (sm_seq(sm)[p >> 5] >> (62u - 2u * (p & 31u))) & 3u;
}
template <typename WT>
__device__ __forceinline__ WT window_word(ExactSmem sm, u32 i, int k);
template <>
__device__ __forceinline__ u64 window_word<u64>(ExactSmem sm, u32 i, int k) {
    i += sm.s0;
    const u32 wi = i >> 5, sh = 2u * (i & 31u);
    const u64 a = sm_seq(sm)[wi], b = sm_seq(sm)[wi + 1];
    const u64 x = sh ? ((a << sh) | (b >> (64u - sh))) : a;
    return x >> (64 - 2 * k);
}
template <>
__device__ __forceinline__ u128 window_word<u128>(ExactSmem sm, u32 i, int k) {
    i += sm.s0;
    const u32 wi = i >> 5, sh = 2u * (i & 31u);
    const u64 a = sm_seq(sm)[wi], b = sm_seq(sm)[wi + 1], c = sm_seq(sm)[wi + 2];
    const u128 ab = ((u128) a << 64) | b;
    const u128 x = sh ? ((ab << sh) | (u128) (c >> (64u - sh))) : ab;
    return x >> (128 - 2 * k);
}
__device__ __forceinline__ bool window_valid(ExactSmem sm, u32 i, int k) {  // k <= 64
    i += sm.s0;
    const u32 wi = i >> 5, bi = i & 31u;
    const u64 lo = ((u64) sm_nmask(sm)[wi + 1] << 32) | sm_nmask(sm)[wi];
    const u64 hi = sm_nmask(sm)[wi + 2];
    const u64 nmw = bi ? ((lo >> bi) | (hi << (64u - bi))) : lo;
    const u64 km = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
    return (nmw & km) == 0;  // no N inside the window (kmer.cpp:2190)
}

// wave argmax over per-lane (key, seq): largest class, ties to the class whose
// last window is earliest = the first to reach the maximum in scan order
// (strict '<' at kmer.cpp:2202).  key = (class size << 16) | (0xffff - last window)
template <typename WT>
__device__ __forceinline__ void wave_best(u32 best, WT best_seq, KStat<WT> &st) {
    const u32 m = wave_max_u32(best);
    const u64 who = __ballot(best == m && m != 0);
    if (who) {
        const int src = __ffsll((long long) who) - 1;
        st.maxc = m >> 16;
        st.maxseq = readlane_word(best_seq, src);
    }
}

// Fallback for segments with more than 64 runs: one item per window, class sizes
// by an all-pairs LDS-broadcast compare.  vmask[] must hold the valid-window bits.
template <typename WT>
__attribute__((noinline)) __device__ KStat<WT> eval_k_windows(ExactSmem sm, int W, int k, u32 count) {
    KStat<WT> st;  // returned by value: a reference parameter of a noinline function lives in scratch memory
    PH_T0(t_ph);
    PH_CNT(PH_N_WINDOWS_CALLS, 1);
    sm = uni(sm);
    W = rfl_i(W);
    k = rfl_i(k);
    count = rfl(count);
    st.count = count;
    st.maxc = 0;
    st.maxseq = 0;
    st.pruned = false;
    const u32 lane = lane_id();
    const int rounds = (W + 63) >> 6;
    for (int r = 0; r < rounds; r++) {
        const int i = r * 64 + (int) lane;
        if (i < W) {
            const bool valid = (sm_vmask(sm)[r] >> lane) & 1ull;
            sm_canon<WT>(sm)[i] = valid ? min_rotation<WT>(window_word<WT>(sm, (u32) i, k), k) : (WT) 0;
            sm_cnt(sm)[i] = 0;
        }
    }
    __syncthreads();
    u32 best = 0;
    WT best_seq = 0;
    for (int r = 0; r < rounds; r++) {
        const int i = r * 64 + (int) lane;
        const bool mine = i < W && ((sm_vmask(sm)[r] >> lane) & 1ull);
        const WT my = mine ? sm_canon<WT>(sm)[i] : (WT) 0;
        u32 c = 0, last = 0;
        bool first = true;
        for (int jr = 0; jr < rounds; jr++) {
            u64 vm = rfl64(sm_vmask(sm)[jr]);
            while (vm) {
                const int jb = __ffsll((long long) vm) - 1;
                vm &= vm - 1;
                const int j = jr * 64 + jb;
                const bool eq = sm_canon<WT>(sm)[j] == my;  // LDS broadcast read
                c += eq ? 1u : 0u;
                last = eq ? (u32) j : last;
                first = first && !(eq && j < i);
            }
        }
        if (mine) {
            if (first) sm_cnt(sm)[i] = (unsigned short) c;
            const u32 key = (c << 16) | (0xffffu - last);
            if (key > best) {
                best = key;
                best_seq = my;
            }
        }
    }
    wave_best<WT>(best, best_seq, st);
    st.n_items = (u32) W;
    PH_ADD(PH_WINDOWS, t_ph);
    return st;
}

template <typename WT>
__device__ KStat<WT> eval_runs(ExactSmem sm, int W, int k);

// One k of the counting loop of k_mer_check / k_mer_target (kmer.cpp:2183-2216,
// 1936-1967) on the segment staged in sm.  Lemma A (SURVEY section 7): two
// adjacent valid windows i, i+1 are in the same rotation class iff base i ==
// base i+k, so the windows fall into maximal RUNS and only one canonical
// rotation per run is needed; runs with equal canonical word are then merged.
// Leaves canon[] / cnt[] in LDS for emit_k.  All lanes must call it; the
// result is wave-uniform.
//
// need > 0 asks for an early exit: windows of one class share their base
// composition, so the largest of the 8 (#lo, #hi, #A mod 2) parity buckets
// bounds MAX from above; if even that bound gives a frequency below `need`
// (the smallest threshold this k still has to reach in decide()), the k cannot
// be accepted and the per-run canonicalisation is skipped (st.pruned).
template <typename WT>
__attribute__((noinline)) __device__ KStat<WT> eval_k(ExactSmem sm, int L, int k, double need) {
    KStat<WT> st;
    st.count = 0;
    st.maxc = 0;
    st.maxseq = 0;
    st.n_items = 0;
    st.pruned = false;
    sm = uni(sm);
    L = rfl_i(L);
    k = rfl_i(k);
    need = rfl_f64(need);
    const int W = L - k + 1;
    if (W <= 0) return st;
    PH_T0(t_ph);
    const u32 lane = lane_id();
    const int rounds = (W + 63) >> 6;
    WT m5 = (WT) 0x5555555555555555ull;
    if (sizeof(WT) > 8) m5 |= m5 << 64 % (8 * sizeof(WT));
    m5 &= kmask<WT>(k);
    u32 b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0, b6 = 0, b7 = 0;
    __syncthreads();  // previous users of the LDS arrays are done
    if (need == 0.0 && sm.rw != nullptr && k < 64) {
        // No pruning wanted (record / k_mer_target): the window masks of this one k come straight from
        // the packed planes, lane j building 32 windows at once -- E = bases i and i+k agree, V = the
        // L-k+1 windows of an N-free segment -- instead of a walk over the windows.  A segment with an
        // N keeps the general walk below.
        const u32 segw = ((u32) L + 31u) >> 5;
        ReadRef rr;
        rr.w = sm.rw;
        rr.nw = sm.rnw;
        rr.len = 0;
        u32 lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, nm[3] = {0, 0, 0};
        if (lane < segw) load_planes<3>(rr, sm.rs + 32u * lane, lo, hi, nm);
        if (!__any((nm[0] & low_mask(L - 32 * (int) lane)) != 0u)) {
            const bool big = k >= 32;
            const u32 ks = (u32) k & 31u;
            const u32 slo = alignbit(big ? lo[2] : lo[1], big ? lo[1] : lo[0], ks);
            const u32 shi = alignbit(big ? hi[2] : hi[1], big ? hi[1] : hi[0], ks);
            const u32 e = ~((lo[0] ^ slo) | (hi[0] ^ shi));
            const u32 v = low_mask(W - 32 * (int) lane);
            if (lane < 2u * ((u32) rounds + 1u)) {  // including the terminating zero word
                ((u32 *) sm_vmask(sm))[lane] = v;
                ((u32 *) sm_emask(sm))[lane] = e & v;
            }
            __syncthreads();
            PH_ADD(PH_EVALK_A, t_ph);
            return eval_runs<WT>(sm, W, k);
        }
    }
    for (int r = 0; r < rounds; r++) {
        const u32 i = (u32) r * 64u + lane;
        bool valid = false, eq = false, p1 = false, p2 = false, p3 = false;
        if ((int) i < W) {
            valid = window_valid(sm, i, k);
            const WT w = window_word<WT>(sm, i, k);
            eq = (u32) (w >> (2 * k - 2)) == base_at(sm, i + (u32) k);
            p1 = popc_word(w & m5) & 1;
            p2 = popc_word((w >> 1) & m5) & 1;
            p3 = popc_word(w & (w >> 1) & m5) & 1;
        }
        const u64 bv = __ballot(valid), be = __ballot(eq);
        if (lane == 0) {
            sm_vmask(sm)[r] = bv;
            sm_emask(sm)[r] = be;
        }
        if (need > 0.0) {
            const u64 f1 = __ballot(p1), f2 = __ballot(p2), f3 = __ballot(p3);
            const u64 a1 = bv & f1, a0 = bv ^ a1;
            const u64 a11 = a1 & f2, a10 = a1 ^ a11, a01 = a0 & f2, a00 = a0 ^ a01;
            const u64 c111 = a11 & f3, c101 = a10 & f3, c011 = a01 & f3, c001 = a00 & f3;
            b7 += (u32) __popcll(c111);
            b6 += (u32) __popcll(a11 ^ c111);
            b5 += (u32) __popcll(c101);
            b4 += (u32) __popcll(a10 ^ c101);
            b3 += (u32) __popcll(c011);
            b2 += (u32) __popcll(a01 ^ c011);
            b1 += (u32) __popcll(c001);
            b0 += (u32) __popcll(a00 ^ c001);
        }
    }
    if (lane == 0) {
        sm_vmask(sm)[rounds] = 0;
        sm_emask(sm)[rounds] = 0;
    }
    __syncthreads();
    if (need > 0.0) {
        u32 cnt = 0;
        for (int r = 0; r < rounds; r++) cnt += (u32) __popcll(rfl64(sm_vmask(sm)[r]));
        const u32 mb = max(max(max(b0, b1), max(b2, b3)), max(max(b4, b5), max(b6, b7)));
        // MAX <= mb and IEEE division is monotone in the numerator, so MAX/COUNT <= mb/COUNT < need
        if (cnt == 0 || (double) rfl(mb) / (double) cnt < need) {
            st.count = cnt;
            st.pruned = true;
            __syncthreads();
            return st;
        }
    }
    PH_ADD(PH_EVALK_A, t_ph);
    return eval_runs<WT>(sm, W, k);
}

// Second half of eval_k: vmask[] / emask[] (+ one zero word) are in LDS, visible to the wave.
template <typename WT>
__attribute__((noinline)) __device__ KStat<WT> eval_runs(ExactSmem sm, int W, int k) {
    KStat<WT> st;
    st.maxc = 0;
    st.maxseq = 0;
    st.n_items = 0;
    st.pruned = false;
    sm = uni(sm);
    W = rfl_i(W);
    k = rfl_i(k);
    const u32 lane = lane_id();
    const int rounds = (W + 63) >> 6;
    PH_T0(t_ph);
    PH_CNT(PH_N_RUNS_CALLS, 1);
    PH_CNT(PH_N_K5, k == 5 ? 1 : 0);
    // run starts: valid_i && !(valid_{i-1} && eq_{i-1}); compacted into start[]
    u32 R = 0, count = 0;
    u64 carry = 0;
    for (int r = 0; r < rounds; r++) {
        const u64 vm = rfl64(sm_vmask(sm)[r]), em = rfl64(sm_emask(sm)[r]);
        const u64 ve = vm & em;
        const u64 startmask = vm & ~((ve << 1) | carry);
        carry = ve >> 63;
        count += (u32) __popcll(vm);
        if ((startmask >> lane) & 1ull) sm_start(sm)[R + (u32) __popcll(startmask & ((1ull << lane) - 1ull))] = (unsigned short) (r * 64 + (int) lane);
        R += (u32) __popcll(startmask);
    }
    st.count = count;
    __syncthreads();
    if (R > 64) {
        count_fallback(kFallbackWindows);
        st = eval_k_windows<WT>(sm, W, k, count);
        __syncthreads();
        PH_ADD(PH_RUNS, t_ph);
        return st;
    }
    // one lane per run
    WT canon = ~(WT) 0;
    u32 len = 0, s = 0;
    if (lane < R) {
        s = sm_start(sm)[lane];
        // run length = 1 + number of consecutive j >= s with valid_j && eq_j && valid_{j+1}
        u32 j = s;
        len = 1;
        for (;;) {
            const u32 wi = j >> 6, bi = j & 63u;
            const u64 v0 = sm_vmask(sm)[wi], v1 = sm_vmask(sm)[wi + 1];
            const u64 cw = (v0 & sm_emask(sm)[wi] & ((v0 >> 1) | (v1 << 63))) >> bi;
            const u64 inv = ~cw;
            const u32 ones = inv ? (u32) (__ffsll((long long) inv) - 1) : 64u;
            len += ones;
            if (ones + bi < 64u) break;
            j += ones;
            if (j >= (u32) W) break;
        }
        canon = min_rotation<WT>(window_word<WT>(sm, s, k), k);
    }
    const u32 end = s + len - 1;
    u32 tot = 0, last = 0;
    bool first = false;
    // One iteration per CLASS, not per run: the lowest run without a class is its leader, one ballot
    // finds every member, a DPP sum adds their lengths; runs are in position order, so the member in
    // the highest lane ends last.  (A TTAGGG read probed at k = 5 has ~50 runs in ~8 classes.)
    const u64 act = R >= 64u ? ~0ull : ((1ull << R) - 1ull);
    u64 remaining = act;
    while (remaining) {
        const int rp = __ffsll((long long) remaining) - 1;
        const WT other = readlane_word(canon, rp);
        const u64 eqm = __ballot(other == canon) & act;
        remaining &= ~eqm;
        const bool eq = (eqm >> lane) & 1ull;
        const u32 total = wave_sum_u32(eq ? len : 0u);
        const u32 oend = (u32) __builtin_amdgcn_readlane((int) end, 63 - __clzll((long long) eqm));
        if (eq) {
            tot = total;
            last = oend;
            first = (int) lane == rp;
        }
    }
    u32 key = 0;
    if (lane < R) {
        key = (tot << 16) | (0xffffu - last);
        sm_canon<WT>(sm)[lane] = canon;
        sm_cnt(sm)[lane] = first ? (unsigned short) tot : (unsigned short) 0;
    }
    wave_best<WT>(key, canon, st);
    st.n_items = R;
    __syncthreads();
    PH_CNT(PH_N_RUNS_TOTAL, R);
    PH_ADD(PH_RUNS, t_ph);
    return st;
}

// Wave-private count cache in LDS.  A few keys (the dominant motif's classes) receive an add from
// almost every surviving read; as device atomics on one address they serialise chip-wide
// (0.4 ms of a 1.3 ms launch, measured with TREW_FLAG_DEBUG_NO_EMIT).  Each wave keeps the first
// kCacheSlots distinct keys it meets in LDS (insert-only, no eviction: the hot keys show up in the
// first reads), adds to them with LDS atomics and flushes once when it runs out of work.
// Entry = the 64-bit table key of table_add + the 9 partition bits of the word.
__device__ __forceinline__ void cached_add(ExactSmem sm, const DevTable &T, int table, int k, u64 word, u32 cnt) {
    if (T.log2_part_slots == 0xffffffffu) return;  // TREW_FLAG_DEBUG_NO_EMIT
    const u32 part = (u32) (word & ((1u << kTablePartBits) - 1u));
    const u64 gkey = (1ull << 63) | ((u64) table << 60) | ((u64) (k - 1) << 55) | (word >> kTablePartBits);
    // any function of the key will do for a slot of the wave's cache; hash64 (two 64-bit multiplies, ~20 half-rate
    // instructions) is kept for the device table, where the distribution over a partition matters
    const u32 slot = ((((u32) gkey ^ (u32) (gkey >> 32)) + part * 0x9e3779b1u) * 0x85ebca6bu) >> (32 - 7);
    static_assert(kCacheSlots == 128, "slot = the 7 top bits of the product");
    u64 *ckey = sm_ckey(sm);
    u32 *cpart = sm_cpart(sm), *ccnt = sm_ccnt(sm);
    // Claim and publish in two separated phases.  A lane that wins the CAS stores the partition bits of its key;
    // a lane of the same wave that lost the CAS to an equal gkey then reads them.  The cache is wave-private (one
    // wave per workgroup) and LDS operations of a wave execute in program order, so the only hazard is the
    // compiler moving the load above the store: the workgroup-scope fence + wave barrier between the phases
    // forbid that, and both accesses are atomic, so there is no data race in the formal sense either.
    u64 ek = __hip_atomic_load(&ckey[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    bool won = false;
    if (ek == 0) {
        const u64 prev = atomicCAS((unsigned long long *) &ckey[slot], 0ull, gkey);
        won = prev == 0;
        ek = won ? gkey : prev;
    }
    if (won) __hip_atomic_store(&cpart[slot], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const u32 spart = __hip_atomic_load(&cpart[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (ek == gkey && spart == part)
        atomicAdd(&ccnt[slot], cnt);
    else
        table_add(T, table, k, word, (u64) cnt);
}
__device__ __forceinline__ void cached_add(ExactSmem sm, const DevTable &T, int table, int k, u128 word, u32 cnt) {
    if (k <= 32)
        cached_add(sm, T, table, k, (u64) word, cnt);
    else
        table_add(T, table, k, word, (u64) cnt);
}
__device__ void cache_clear(ExactSmem sm) {
    for (u32 i = lane_id(); i < kCacheSlots; i += 64) {
        sm_ckey(sm)[i] = 0;
        sm_cpart(sm)[i] = 0;
        sm_ccnt(sm)[i] = 0;
    }
    __syncthreads();
}
__device__ void cache_flush(ExactSmem sm, TableRef Tp) {
    const DevTable T = load_table(Tp);
    __syncthreads();
    for (u32 i = lane_id(); i < kCacheSlots; i += 64) {
        const u64 gkey = sm_ckey(sm)[i];
        if (gkey) {
            const u64 word = ((gkey & ((1ull << 55) - 1ull)) << kTablePartBits) | sm_cpart(sm)[i];
            table_add(T, (int) ((gkey >> 60) & 7ull), (int) ((gkey >> 55) & 31ull) + 1, word, (u64) sm_ccnt(sm)[i]);
        }
    }
}

// add every class of the k just evaluated to the tables in table_mask (bit t).
// strand_canon: key = MIN(w, rot(rc(w))) (k_mer_target, kmer.cpp:1979-1988) else the
// rotation-canonical word itself (k_mer_check, kmer.cpp:2264-2313).
// negate (table_mask bit 31): the counts are SUBTRACTED (long reads that chain from end to end: run_long moves what the forward
// walk recorded); table counts are 64-bit sums, so adding the two's complement is exact.
constexpr u32 kEmitNegate = 1u << 31;
// log (table_mask bit 30; TREW_FLAG_COMPAT_G1, pair driver): every (class, table) added here is also appended to the stale-row
// log with the pair index that the driver left in sm_group(sm)[kGroupPairIndex] -- see DevG1.
constexpr u32 kEmitLog = 1u << 30;
// LOG: a second instantiation for the one call that may carry kEmitLog (the pair driver's whole-read flush under
// TREW_FLAG_COMPAT_G1): the logging code stays out of the function every other emission goes through
template <typename WT, bool LOG = false>
__attribute__((noinline)) __device__ void emit_k(ExactSmem sm, TableRef Tp, u32 n_items, int k, u32 table_mask, bool strand_canon) {
    sm = uni(sm);
    const DevTable T = load_table(Tp);
    n_items = rfl(n_items);
    k = rfl_i(k);
    table_mask = rfl(table_mask);
    const bool negate = (table_mask & kEmitNegate) != 0;
    const bool to_log = LOG && (table_mask & kEmitLog) != 0;
    table_mask &= ~(kEmitNegate | kEmitLog);
    strand_canon = rfl((u32) strand_canon) != 0;
    const u32 lane = lane_id();
    PH_T0(t_ph);
    for (u32 base = 0; base < n_items; base += 64) {  // wave-uniform trip count: the de-duplication below is a wave operation
        const u32 i = base + lane;
        u32 c = i < n_items ? sm_cnt(sm)[i] : 0u;
        WT w = 0;
        if (c) {
            w = sm_canon<WT>(sm)[i];
            if (strand_canon) {
                const WT rc = min_rotation<WT>(revcomp(w, k), k);
                w = rc < w ? rc : w;
            }
        }
        if (sizeof(WT) > 8 && k > 32 && strand_canon) {
            // A class and its reverse-complement class reach this point with the SAME strand-canonical key, in
            // two lanes of one wave.  In the wide table the lane that loses the slot claim waits for the winner's
            // ready bit (table_add_wide) -- a sibling lane of a lock-step wave must never be that winner, so equal
            // keys are merged here first (classes are distinct before canonicalisation: at most two lanes per key).
            u64 rem = __ballot(c != 0);
            while (rem) {
                const int src = __ffsll((long long) rem) - 1;
                const WT o = readlane_word(w, src);
                const u64 eqm = __ballot(c != 0 && w == o);
                const bool eq = (eqm >> lane) & 1ull;
                const u32 tot = wave_sum_u32(eq ? c : 0u);
                if (eq) c = (int) lane == src ? tot : 0u;
                rem &= ~eqm;
            }
        }
        if (to_log) {  // wave-uniform; rare (pairs shorter than 4 * MAX_MER under TREW_FLAG_COMPAT_G1)
            typedef const __attribute__((address_space(4))) u64 *c64;
            typedef const __attribute__((address_space(4))) u32 *c32;
            const u64 ga = rfl64((u64) Tp) + offsetof(DevTableG1, g);
            trew_hip_row *log = (trew_hip_row *) *(c64) (ga + offsetof(DevG1, log));
            u32 *counters = (u32 *) *(c64) (ga + offsetof(DevG1, counters));
            const u32 log_cap = *(c32) (ga + offsetof(DevG1, log_cap));
            const u32 pair = rfl(sm_group(sm)[kGroupPairIndex]);
            const u32 per = (u32) __builtin_popcount(table_mask);
            const u64 have = __ballot(c != 0);
            u32 at = 0;
            if (lane == 0 && have) at = atomicAdd(&counters[0], per * (u32) __builtin_popcountll(have));
            at = rfl(at) + per * (u32) __builtin_popcountll(have & ((1ull << lane) - 1ull));
            if (c) {
                for (u32 tm = table_mask; tm; tm &= tm - 1, at++) {
                    if (at < log_cap) {
                        trew_hip_row r;
                        r.k = k;
                        r.table = __ffs((int) tm) - 1;
                        r.word_lo = (u64) w;
                        r.word_hi = pair;
                        r.count = c;
                        log[at] = r;
                    } else {
                        atomicAdd(&T.overflow[kDiagG1Drop], 1u);
                    }
                }
            }
        }
        if (c) {
            if (negate) {  // rare: straight to the table, the wave's LDS cache counts in 32 bits
                for (u32 tm = table_mask; tm; tm &= tm - 1) table_add(T, __ffs((int) tm) - 1, k, w, 0ull - (u64) c);
            } else {
                for (u32 tm = table_mask; tm; tm &= tm - 1) cached_add(sm, T, __ffs((int) tm) - 1, k, w, c);
            }
        }
    }
    PH_ADD(PH_EMIT, t_ph);
}

// Upper bound of MAX/COUNT for EVERY k of one segment at once: lane l handles
// k = gmin + l with the same bit-parallel parity-bucket bound as the prefilter
// (filter_segment), the shift amounts simply differ per lane.  Used by decide()
// to discard a candidate k with one readlane instead of a pass over its windows.
// Returns (double) maxbucket / (double) count, 0 where there is no valid window.
// what lane l knows about k = gmin + l of one segment
template <int NW>
struct LaneMasks {
    u32 V[NW];  // bit i: window i has no N and fits the segment
    u32 E[NW];  // bit i: base i == base i+k (meaningful where windows i and i+1 are both valid)
    double ub;  // maxbucket / COUNT, an upper bound of MAX / COUNT (0 where COUNT == 0)
    u32 runs;   // number of runs of adjacent same-class windows (Lemma A): what counting the classes of this k costs
    u32 m8, cnt;  // the bound as the two integers it is the quotient of (0 / 0 where the k is out of range): decide_group compares exactly, without a division
    bool has_n;   // the segment holds an N (or another non-ACGT byte)
};

template <int NW>
__device__ __forceinline__ void lane_bounds_at(const ReadRef &rd, u32 s, int L, int k, int gmax, LaneMasks<NW> &out);
// lane l <-> k = gmin + l of the segment [s, s+L)
template <int NW>
__device__ __forceinline__ void lane_bounds(const ReadRef &rd, u32 s, int L, int gmin, int gmax, LaneMasks<NW> &out) {
    lane_bounds_at<NW>(rd, s, L, gmin + (int) lane_id(), gmax, out);
}
// Two segments of one read in one pass when the k range fits half a wave (short reads: both
// halves): lanes 0..31 take segment A, lanes 32..63 segment B, k = gmin + (lane & 31).
template <int NW>
__device__ __forceinline__ void lane_bounds_pair(const ReadRef &rd, u32 sA, int LA, u32 sB, int LB, int gmin, int gmax, LaneMasks<NW> &out) {
    const bool hiHalf = lane_id() >= 32u;
    lane_bounds_at<NW>(rd, hiHalf ? sB : sA, hiHalf ? LB : LA, gmin + (int) (lane_id() & 31u), gmax, out);
}
// s, L, k may differ per lane (they do in lane_bounds_pair); everything below is per-lane arithmetic
template <int NW>
__device__ __forceinline__ void lane_bounds_at(const ReadRef &rd, u32 s, int L, int k, int gmax, LaneMasks<NW> &out) {
    PH_T0(t_ph);
    u32 lo[NW], hi[NW], nm[NW];
    load_planes<NW>(rd, s, lo, hi, nm);  // the lanes of one segment read the same (LDS-staged) words
    u32 v1[NW], P1[NW], P2[NW], P3[NW];
    segment_setup<NW, true>(lo, hi, nm, L, v1, P1, P2, P3);
    const u32 ku = (u32) k;
    u32 V[NW];
    const u32 anyn = segment_has_n<NW>(nm, L);
    // V = windows_without_n<NW>(v1, anyn != 0, L, k, gmax) (bound.inc, which bound_at_k calls), written out: through the call --
    // by reference, by value or with a local copy -- the spills of up to twenty exact kernels change
    // (profiles/bound_refactor/README.md).  A change to one of the two is a change to both.
    if (anyn == 0) {
        // no N in the segment (wave-uniform: every lane sees the same segment): V_k = the L-k+1 lowest bits
        const int wbits = L - k + 1;
#pragma unroll
        for (int j = 0; j < NW; j++) {
            V[j] = low_mask(wbits - 32 * j);
        }
    } else {
        // V_k[i] = AND_{t<k} v1[i+t] by binary decomposition of k over A_b = AND of b consecutive bases
        u32 A[NW];
#pragma unroll
        for (int j = 0; j < NW; j++) {
            V[j] = 0xffffffffu;
            A[j] = v1[j];
        }
        u32 off = 0;
#pragma unroll
        for (int b = 1; b <= 64; b <<= 1) {
            if (b > 1) {  // A_b = A_{b/2} & (A_{b/2} >> b/2)
                u32 T2[NW];
#pragma unroll
                for (int j = 0; j < NW; j++) T2[j] = A[j] & shr_var_word<NW>(A, j, (u32) (b / 2));
#pragma unroll
                for (int j = 0; j < NW; j++) A[j] = T2[j];
            }
            if (b <= gmax) {  // wave-uniform
                const bool take = (ku & (u32) b) != 0;
#pragma unroll
                for (int j = 0; j < NW; j++) {
                    const u32 sh = shr_var_word<NW>(A, j, off);
                    V[j] &= take ? sh : 0xffffffffu;
                }
                off += take ? (u32) b : 0u;
            }
        }
    }
    Buckets8<false, false> b8;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const u32 F1 = P1[j] ^ shr_var_word<NW>(P1, j, ku), F2 = P2[j] ^ shr_var_word<NW>(P2, j, ku);
        const u32 F3 = P3[j] ^ shr_var_word<NW>(P3, j, ku);
        const u32 v = V[j];
        out.V[j] = v;
        out.E[j] = ~((lo[j] ^ shr_var_word<NW>(lo, j, ku)) | (hi[j] ^ shr_var_word<NW>(hi, j, ku)));
        b8.add(F1, F2, F3, v);
    }
    const u32 m8 = b8.largest(), count = b8.count;
    // k = 64 is not bounded here (shift amounts stay below 64): never prune it
    out.ub = (k > gmax || k >= 64 || count == 0) ? ((k >= 64 && k <= gmax) ? 2.0 : 0.0) : (double) m8 / (double) count;
    out.m8 = (k > gmax || k >= 64) ? 0u : m8;
    out.cnt = (k > gmax || k >= 64) ? 0u : count;
    out.has_n = anyn != 0u;
    out.runs = count - class_links<NW>(out.V, out.E);
    PH_ADD(PH_BOUNDS, t_ph);
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

template <typename WT>
struct Decision {
    int kh, kl;   // target_k_high / target_k_low
    WT sh, sl;    // MAX_SEQ at those k (repeat_seq, kmer.cpp:2260-2262)
    int ek;       // k of the last class count whose canon[] / cnt[] are still in LDS (0: none)
    u32 en;       // its number of items
    u32 ec;       // its COUNT (windows without N)
};

// bits j-1 for every multiple j <= 64 of k
__device__ __forceinline__ u64 multiples_mask(int k) {  // one scalar load instead of a loop of up to 64 / k iterations
    return load_multiples(k);
}

// selection loops of k_mer_check, kmer.cpp:2221-2258, run online over ascending
// candidate k (non-candidates have frequency < LOW and can never be accepted)
// M: per-lane knowledge of lane_bounds() (lane l <-> k = MIN_MER + l); ignored when NW == 0
template <int NW, typename WT>
__device__ Decision<WT> decide(ExactSmem sm, const DevParams &P, int L, int kmin, int kmax, u64 cand, const LaneMasks<(NW > 0 ? NW : 1)> &M,
                               int lane_base = 0, int lane_span = 64) {
    constexpr bool HAVE_UB = NW > 0;
    constexpr int NWB = NW > 0 ? NW : 1;
    Decision<WT> d;
    PH_T0(t_ph);
    d.kh = d.kl = 0;
    d.sh = d.sl = 0;
    d.ek = 0;
    d.en = 0;
    d.ec = 0;
    double tf_low = 0.0, tf_high = 0.0;
    // closed_*: bit k-1 set <=> k is a multiple of a k already accepted in that loop.  Such a k is
    // never accepted and never moves the running frequency (kmer.cpp:2225-2236).
    u64 closed_low = 0, closed_high = 0;
    u64 todo = cand & all_k_mask(kmin, kmax);
    // Speculative skip (HAVE_UB only).  Counting the classes of a k with many runs is the expensive
    // case, and it is usually a k that cannot matter: a TTAGGG read probed at k = 5 (bound 0.5, ~45 runs)
    // just before k = 6 is accepted at 0.9.  Such a k is passed over; that is exact provided every k
    // accepted later in a selection loop the skipped k was eligible for has a frequency >= the bound of
    // the skipped k and is not a multiple of it (then the skipped k could only have raised the threshold
    // to a value the later k clears and closed multiples nobody took), and at least one such k exists
    // (else the skipped k might be the answer).  If the check fails the segment is decided again with
    // every k counted.
    constexpr u32 kHeavyRuns = 24;
    bool strict = !HAVE_UB;
    int sk_k[2] = {0, 0};
    double sk_ub[2] = {0.0, 0.0};
    u32 sk_el[2] = {0, 0}, sk_ok[2] = {0, 0};
    bool viol = false;
    const u64 todo0 = todo;
    // lane l <-> k = MIN_MER + l (as in lane_bounds); only used when HAVE_UB
    // lanes [lane_base, lane_base + lane_span) hold this segment's bounds (lane_bounds_pair: half a wave)
    const int kl = P.min_mer + (int) lane_id() - lane_base;
    const u32 klb = (u32) (kl - 1) & 63u;
    const bool my_lane = (int) lane_id() >= lane_base && (int) lane_id() < lane_base + lane_span;
again:
    for (;;) {
        const double thr_lo = P.low > tf_low ? P.low : tf_low;     // MAX(LOW_BASELINE, target_frequency_low)
        const double thr_hi = P.high > tf_high ? P.high : tf_high; // MAX(HIGH_BASELINE, target_frequency_high)
        int k;
        if (HAVE_UB) {
            // Next k the scalar loop would evaluate, found for all k at once: k still open in one of
            // the two selection loops and its bound reaches the smallest threshold it has to meet
            // (MAX <= maxbucket and IEEE division is monotone in the numerator: f <= bound < need
            // can never be accepted).  Thresholds only move when a k is accepted, after which the
            // eligibility is recomputed, so skipping is equivalent to the k-by-k walk.
            const bool lo_l = !((closed_low >> klb) & 1ull), hi_l = !((closed_high >> klb) & 1ull);
            const double need_l = lo_l ? (hi_l ? (thr_lo < thr_hi ? thr_lo : thr_hi) : thr_lo) : thr_hi;
            const u64 el = __ballot(my_lane && kl <= 64 && (lo_l || hi_l) && M.ub >= need_l) >> lane_base;
            todo &= P.min_mer > 1 ? (el << (P.min_mer - 1)) : el;
        }
        if (!todo) break;
        k = __ffsll((long long) todo);  // bit k-1 -> k, ascending
        todo &= todo - 1;
        const bool lo_open = !((closed_low >> (k - 1)) & 1ull), hi_open = !((closed_high >> (k - 1)) & 1ull);
        if (!lo_open && !hi_open) continue;
        const double need = lo_open ? (hi_open ? (thr_lo < thr_hi ? thr_lo : thr_hi) : thr_lo) : thr_hi;
        KStat<WT> st;
        // lane_bounds knows nothing about k = 64 (shift amounts stay below 64); only the 128-bit-word kernels can meet it
        constexpr bool kMay64 = sizeof(WT) > 8;
        if (HAVE_UB && !strict && (!kMay64 || k < 64)) {
            const int src = k - P.min_mer + lane_base;
            if ((u32) __builtin_amdgcn_readlane((int) M.runs, src) > kHeavyRuns && (sk_k[0] == 0 || sk_k[1] == 0)) {
                const double ub = readlane_f64(M.ub, src);
                const u32 el = ((lo_open && ub >= thr_lo) ? 1u : 0u) | ((hi_open && ub >= thr_hi) ? 2u : 0u);
                const int s = sk_k[0] == 0 ? 0 : 1;
                sk_k[s] = k;
                sk_ub[s] = ub;
                sk_el[s] = el;
                continue;
            }
        }
        if (HAVE_UB && (!kMay64 || k < 64)) {
            const int src = k - P.min_mer + lane_base;
            // the window masks of this k were computed bit-parallel by lane `src`: fetch them
            // instead of walking the windows (phase A of eval_k)
            st.count = st.maxc = st.n_items = 0;
            st.maxseq = 0;
            st.pruned = false;
            const int W = L - k + 1;
            if (W > 0) {
                __syncthreads();
                u64 *vm = sm_vmask(sm), *em = sm_emask(sm);
                // the LDS mask arrays hold cap/64 + 2 words: never write past them when the
                // instantiation's NW covers more bits than this batch's segments need
                const int nq_all = (NWB + 1) / 2, nq_fit = (int) (sm.cap / 64u) + 1;
                const int nq = nq_all < nq_fit ? nq_all : nq_fit;
                if ((int) lane_id() == src) {  // the lane that owns this k stores its masks itself: no broadcast needed
#pragma unroll
                    for (int q = 0; q < nq_all; q++) {
                        if (q >= nq) break;
                        const u32 v1 = 2 * q + 1 < NWB ? M.V[2 * q + 1 < NWB ? 2 * q + 1 : 0] : 0u;
                        const u32 e1 = 2 * q + 1 < NWB ? M.E[2 * q + 1 < NWB ? 2 * q + 1 : 0] : 0u;
                        vm[q] = ((u64) v1 << 32) | M.V[2 * q];
                        em[q] = ((u64) e1 << 32) | M.E[2 * q];
                    }
                    vm[nq] = 0;
                    em[nq] = 0;
                }
                __syncthreads();
                st = uni(eval_runs<WT>(sm, W, k));
            }
        } else {
            st = uni(eval_k<WT>(sm, L, k, need));
        }
        d.ek = st.pruned ? 0 : k;
        d.en = st.n_items;
        d.ec = st.count;
        if (st.pruned || st.count == 0) continue;  // 0/0 = NaN fails every >=
        const double f = (double) st.maxc / (double) st.count;
        if (is_homopolymer<WT>(st.maxseq, k)) continue;
        u32 acc = 0;
        if (lo_open && f >= thr_lo) {
            d.kl = k;
            tf_low = f;
            closed_low |= multiples_mask(k);
            d.sl = st.maxseq;
            acc |= 1u;
        }
        if (hi_open && f >= thr_hi) {
            d.kh = k;
            tf_high = f;
            closed_high |= multiples_mask(k);
            d.sh = st.maxseq;
            acc |= 2u;
        }
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (sk_k[s] && (acc & sk_el[s])) {
                if (f < sk_ub[s] || k % sk_k[s] == 0) viol = true;
                sk_ok[s] |= acc & sk_el[s];
            }
        }
    }
    if (HAVE_UB && !strict) {
#pragma unroll
        for (int s = 0; s < 2; s++)
            if (sk_k[s] && (sk_el[s] & ~sk_ok[s])) viol = true;
        if (viol) {  // decide again, counting every k
            count_fallback(kFallbackStrictRerun);
            strict = true;
            d.kh = d.kl = 0;
            d.sh = d.sl = 0;
            d.ek = 0;
            d.en = 0;
            tf_low = tf_high = 0.0;
            closed_low = closed_high = 0;
            todo = todo0;
            sk_k[0] = sk_k[1] = 0;
            goto again;
        }
    }
    PH_ADD(PH_DECIDE, t_ph);
    return d;
}

// Keep / reuse the class table a decide() left in LDS (see Decision::ek): slot = where to keep it.
// Returns k | items << 8 | COUNT << 16 when kept, else 0.
template <typename WT>
__device__ __forceinline__ u32 save_classes(ExactSmem sm, const Decision<WT> &d, int slot) {
    if (!(d.ek > 0 && d.en <= kSaveItems && (d.ek == d.kh || d.ek == d.kl))) return 0u;
    if (lane_id() < d.en) {
        sm_save_canon<WT>(sm)[(u32) slot * kSaveItems + lane_id()] = sm_canon<WT>(sm)[lane_id()];
        sm_save_cnt<WT>(sm)[(u32) slot * kSaveItems + lane_id()] = sm_cnt(sm)[lane_id()];
    }
    return (u32) d.ek | (d.en << 8) | (d.ec << 16);  // k <= 64, items <= kSaveItems, COUNT <= 1000
}
// bring a kept table back into canon[] / cnt[] for emit_k; returns its number of items
template <typename WT>
__device__ __forceinline__ u32 restore_classes(ExactSmem sm, u32 saved, int slot) {
    const u32 n_items = (saved >> 8) & 255u;
    __syncthreads();
    if (lane_id() < n_items) {
        sm_canon<WT>(sm)[lane_id()] = sm_save_canon<WT>(sm)[(u32) slot * kSaveItems + lane_id()];
        sm_cnt(sm)[lane_id()] = sm_save_cnt<WT>(sm)[(u32) slot * kSaveItems + lane_id()];
    }
    __syncthreads();
    return n_items;
}

// record the histogram of segment (already staged) at k into tables; `saved` (k | items << 8) names a
// class table of this segment kept by save_classes in `slot`, used when it is the table of this k
template <typename WT>
__device__ void record_kept(ExactSmem sm, TableRef T, int L, int k, u32 table_mask, bool strand_canon, u32 saved, int slot) {
    if (k <= 0 || table_mask == 0) return;
    if ((int) (saved & 255u) == k) {
        const u32 n_items = restore_classes<WT>(sm, saved, slot);
        emit_k<WT>(sm, T, n_items, k, table_mask, strand_canon);
        return;
    }
    const KStat<WT> st = uni(eval_k<WT>(sm, L, k, 0.0));
    emit_k<WT>(sm, T, st.n_items, k, table_mask, strand_canon);
}

// the same right after the decide() of this very segment: its last class count is still in canon[] / cnt[]
template <typename WT>
__device__ void record_live(ExactSmem sm, TableRef T, int L, int k, u32 table_mask, bool strand_canon, const Decision<WT> &d) {
    if (k <= 0 || table_mask == 0) return;
    if (d.ek == k) {
        emit_k<WT>(sm, T, d.en, k, table_mask, strand_canon);
        return;
    }
    const KStat<WT> st = uni(eval_k<WT>(sm, L, k, 0.0));
    emit_k<WT>(sm, T, st.n_items, k, table_mask, strand_canon);
}

// record the histogram of segment (already staged) at k into tables
template <typename WT>
__device__ void record(ExactSmem sm, TableRef T, int L, int k, u32 table_mask, bool strand_canon) {
    if (k <= 0 || table_mask == 0) return;
    PH_T0(t_ph);
    PH_CNT(PH_N_RECORD, 1);
    const KStat<WT> st = uni(eval_k<WT>(sm, L, k, 0.0));
    PH_ADD(PH_RECORD_EVAL, t_ph);
    emit_k<WT>(sm, T, st.n_items, k, table_mask, strand_canon);
}

// the staged slice was recorded at k, as it is, into the tables of from_mask; it belongs strand-canonical into those of to_mask
template <typename WT>
__device__ void move_to_both(ExactSmem sm, TableRef T, int L, int k, u32 from_mask, u32 to_mask) {
    if (k <= 0) return;
    const KStat<WT> st = uni(eval_k<WT>(sm, L, k, 0.0));
    emit_k<WT>(sm, T, st.n_items, k, from_mask | kEmitNegate, false);
    emit_k<WT>(sm, T, st.n_items, k, to_mask, true);
}

// k_mer_target, kmer.cpp:1894-2017, on the staged whole read
template <typename WT>
__device__ void target(ExactSmem sm, const DevParams &P, TableRef T, int L, int k, bool want_high, bool want_low) {
    PH_T0(t_ph);
    PH_CNT(PH_N_RECORD, 1);
    const KStat<WT> st = uni(eval_k<WT>(sm, L, k, 0.0));
    PH_ADD(PH_RECORD_EVAL, t_ph);
    if (st.count == 0) return;
    const double f = is_homopolymer<WT>(st.maxseq, k) ? 0.0 : (double) st.maxc / (double) st.count;
    u32 tm = 0;
    if (want_high && f >= P.high) tm |= 1u << TREW_TABLE_BOTH_HIGH;
    if (want_low && f >= P.low) tm |= 1u << TREW_TABLE_BOTH_LOW;
    if (tm) emit_k<WT>(sm, T, st.n_items, k, tm, true);
}

// k_mer_target on the whole read WITHOUT counting it again, when the class tables both halves were decided with are still
// kept (save_classes, slots slot0 and slot0 + 1, same k): the two halves partition the read, so the whole read's windows are the left
// half's, the right half's and the k-1 windows that span the border -- its rotation classes are the union of the two
// tables plus those few windows, COUNT the sum.  MAX_SEQ is only used for the homopolymer veto (kmer.cpp:1972-1976); which
// of several largest classes reached the maximum first cannot be read off merged tables, so a tie between a homopolymer
// and another class is left to the full recount (returns false; so does any read whose tables are not both at hand).
// LL = length of the left half; sm views the whole read.  (100 k of the 176 k survivors of the bench workload are
// telomeric reads that end here: this replaces their third class count, the longest of the three.)
template <typename WT>
__device__ bool target_from_halves(ExactSmem sm, const DevParams &P, TableRef T, int n, int LL, int k, bool want_high, bool want_low,
                                   u32 keptL, u32 keptR, u32 slot0) {
    if ((int) (keptL & 255u) != k || (int) (keptR & 255u) != k || k < 2) return false;
    PH_T0(t_ph);
    PH_CNT(PH_N_RECORD, 1);
    const u32 nL = (keptL >> 8) & 255u, nR = (keptR >> 8) & 255u;
    const u32 countL = keptL >> 16, countR = keptR >> 16;
    const u32 lane = lane_id();
    __syncthreads();
    WT canon = 0;
    u32 c = 0;
    bool span_valid = false;
    if (lane < nL) {
        canon = sm_save_canon<WT>(sm)[slot0 * kSaveItems + lane];
        c = sm_save_cnt<WT>(sm)[slot0 * kSaveItems + lane];
    } else if (lane >= 16u && lane < 16u + nR) {
        canon = sm_save_canon<WT>(sm)[(slot0 + 1u) * kSaveItems + (lane - 16u)];
        c = sm_save_cnt<WT>(sm)[(slot0 + 1u) * kSaveItems + (lane - 16u)];
    } else if (lane >= 32u && lane < 32u + (u32) (k - 1)) {  // k <= 32 here: see the caller
        const int i = LL - k + 1 + (int) (lane - 32u);  // windows that start in the left half and end in the right
        if (i >= 0 && i + k <= n) {
            span_valid = window_valid(sm, (u32) i, k);
            if (span_valid) {
                canon = min_rotation<WT>(window_word<WT>(sm, (u32) i, k), k);
                c = 1;
            }
        }
    }
    const u32 count = countL + countR + (u32) __popcll(__ballot(span_valid));
    if (count == 0) return true;  // nothing to emit (0/0 fails every >=)
    // merge equal classes: the lowest lane of a class keeps the total
    u64 remaining = __ballot(c != 0);
    while (remaining) {
        const int rp = __ffsll((long long) remaining) - 1;
        const WT other = readlane_word(canon, rp);
        const u64 eqm = __ballot(c != 0 && canon == other);
        remaining &= ~eqm;
        const bool eq = (eqm >> lane) & 1ull;
        const u32 total = wave_sum_u32(eq ? c : 0u);
        if (eq) c = (int) lane == rp ? total : 0u;
    }
    const u32 maxc = wave_max_u32(c);
    const bool top = c != 0 && c == maxc;
    const bool homo = top && is_homopolymer<WT>(canon, k);
    const u64 hb = __ballot(homo), nb = __ballot(top && !homo);
    if (hb && nb) return false;  // which of them is MAX_SEQ depends on the scan order: recount
    const double f = hb ? 0.0 : (double) maxc / (double) count;
    u32 tm = 0;
    if (want_high && f >= P.high) tm |= 1u << TREW_TABLE_BOTH_HIGH;
    if (want_low && f >= P.low) tm |= 1u << TREW_TABLE_BOTH_LOW;
    PH_ADD(PH_RECORD_EVAL, t_ph);
    if (tm) {
        sm_canon<WT>(sm)[lane] = canon;
        sm_cnt(sm)[lane] = (unsigned short) c;
        __syncthreads();
        emit_k<WT>(sm, T, 64u, k, tm, true);
    }
    return true;
}

// buffer_task, kmer.cpp:111-173, from the point where both halves are decided: what is recorded where (kmer.cpp:119-163) and the
// whole-read check (kmer.cpp:165-171).  The read is staged as `range`; keptL / keptR name the class tables kept in save slots
// slot0 / slot0 + 1 (save_classes or the group pass).
// What a decided half hands over through LDS (kGroupRes + 8 slot): decide_halves and the group pass write it, run_short_routed reads it.
template <typename WT>
__device__ __forceinline__ void put_decision(ExactSmem sm, u32 slot, u32 kk, u32 saved, WT sh, WT sl) {  // one lane calls it
    u32 *res = sm_group(sm) + kGroupRes + 8u * slot;
    res[0] = kk;  // target_k_high | target_k_low << 8 | (the row gave the segment back) << 16
    res[1] = saved;
    res[2] = (u32) sh;
    res[3] = (u32) ((u64) sh >> 32);
    res[4] = (u32) sl;
    res[5] = (u32) ((u64) sl >> 32);
}
template <typename WT>
__device__ __forceinline__ Decision<WT> get_decision(ExactSmem sm, u32 slot, u32 &kept, bool &punted) {
    const u32 *res = sm_group(sm) + kGroupRes + 8u * slot;
    const u32 kk = rfl(res[0]);
    Decision<WT> d;
    d.kh = (int) (kk & 255u);
    d.kl = (int) ((kk >> 8) & 255u);
    d.sh = (WT) (((u64) rfl(res[3]) << 32) | rfl(res[2]));  // (64 bits: only the short driver hands decisions over this way, and it ignores MAX_SEQ)
    d.sl = (WT) (((u64) rfl(res[5]) << 32) | rfl(res[4]));
    d.ek = 0;
    d.en = 0;
    d.ec = 0;
    kept = rfl(res[1]);
    punted = (kk >> 16) != 0u;
    return d;
}

template <int NW, typename WT>
__attribute__((noinline)) __device__ void run_short_routed(ExactSmem sm, DevParams P, TableRef T, ReadRef rd, u32 range, u32 slot0, bool halves_valid) {
    constexpr bool UB = NW > 0;
    constexpr int NWB = NW > 0 ? NW : 1;
    sm = uni(sm);
    P = uni(P);
    T = rfl_ptr(T);
    rd = uni(rd);
    range = rfl(range);
    slot0 = rfl(slot0);
    halves_valid = rfl((u32) halves_valid) != 0u;
    Decision<WT> left = {0, 0, 0, 0, 0, 0, 0}, right = {0, 0, 0, 0, 0, 0, 0};
    u32 keptL = 0, keptR = 0;
    if (halves_valid) {
        bool punted;
        left = get_decision<WT>(sm, slot0, keptL, punted);
        right = get_decision<WT>(sm, slot0 + 1u, keptR, punted);
    }
    const int n = (int) rd.len;
    const Segment sL = get_segment(TREW_MODE_SHORT, 0, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    const Segment sR = get_segment(TREW_MODE_SHORT, 1, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    const Segment sW = get_segment(TREW_MODE_SHORT, 2, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    if (halves_valid) {
        sm = view_segment(sm, range, sR.start, rd);
        const bool left_found = left.kh > 0 || left.kl > 0;
        const bool tgt_h = left_found && left.kh == right.kh && left.kh > 0;  // kmer.cpp:128
        const bool tgt_l = left_found && left.kl == right.kl && left.kl > 0;  // kmer.cpp:141
        // right half (staged): recorded only where the map passed was non-null
        //  - left found nothing: result.backward directly (kmer.cpp:157-158)
        //  - left found something: temp_result_right.b only when left.b == 0 (kmer.cpp:125), flushed to backward when no target
        {
            const bool rec_h = right.kh > 0 && (!left_found || (left.kh == 0));
            const bool rec_l = right.kl > 0 && (!left_found || (left.kl == 0));
            if (rec_h && rec_l && right.kh == right.kl) {
                record_kept<WT>(sm, T, (int) sR.len, right.kh, (1u << TREW_TABLE_BACKWARD_HIGH) | (1u << TREW_TABLE_BACKWARD_LOW), false, keptR, (int) slot0 + 1);
            } else {
                if (rec_h) record_kept<WT>(sm, T, (int) sR.len, right.kh, 1u << TREW_TABLE_BACKWARD_HIGH, false, keptR, (int) slot0 + 1);
                if (rec_l) record_kept<WT>(sm, T, (int) sR.len, right.kl, 1u << TREW_TABLE_BACKWARD_LOW, false, keptR, (int) slot0 + 1);
            }
        }
        if (left_found) {
            const bool rec_h = left.kh > 0 && !tgt_h;  // temp_result_left.first -> forward.first (kmer.cpp:132-134)
            const bool rec_l = left.kl > 0 && !tgt_l;
            if (rec_h || rec_l) {
                sm = view_segment(sm, range, sL.start, rd);
                if (rec_h && rec_l && left.kh == left.kl) {
                    record_kept<WT>(sm, T, (int) sL.len, left.kh, (1u << TREW_TABLE_FORWARD_HIGH) | (1u << TREW_TABLE_FORWARD_LOW), false, keptL, (int) slot0);
                } else {
                    if (rec_h) record_kept<WT>(sm, T, (int) sL.len, left.kh, 1u << TREW_TABLE_FORWARD_HIGH, false, keptL, (int) slot0);
                    if (rec_l) record_kept<WT>(sm, T, (int) sL.len, left.kl, 1u << TREW_TABLE_FORWARD_LOW, false, keptL, (int) slot0);
                }
            }
            if (tgt_h || tgt_l) {
                sm = view_segment(sm, range, 0, rd);
                if (tgt_h && tgt_l && left.kh == left.kl) {
                    // (k > 32: 128-bit words and up to 63 spanning windows do not fit the lane layout of the merge)
                    if (!(left.kh <= 32 && target_from_halves<WT>(sm, P, T, n, (int) sL.len, left.kh, true, true, keptL, keptR, slot0)))
                        target<WT>(sm, P, T, n, left.kh, true, true);
                } else {
                    if (tgt_h) target<WT>(sm, P, T, n, left.kh, true, false);
                    if (tgt_l) target<WT>(sm, P, T, n, left.kl, false, true);
                }
            }
        }
    }
    const bool hh = left.kh == 0 && right.kh == 0;  // kmer.cpp:165-166
    const bool lh = left.kl == 0 && right.kl == 0;
    if (sW.valid && (hh || lh)) {  // kmer.cpp:168-171
        sm = view_segment(sm, range, 0, rd);
        LaneMasks<NWB> mW;
        if (UB) lane_bounds<NWB>(rd, 0, n, P.min_mer, P.max_mer, mW);
        const Decision<WT> w = decide<NW, WT>(sm, P, n, sW.kmin, sW.kmax, ~0ull, mW);
        const bool rec_h = hh && w.kh > 0, rec_l = lh && w.kl > 0;
        if (rec_h && rec_l && w.kh == w.kl) {
            record<WT>(sm, T, n, w.kh, (1u << TREW_TABLE_BOTH_HIGH) | (1u << TREW_TABLE_BOTH_LOW), false);
        } else {
            if (rec_h) record<WT>(sm, T, n, w.kh, 1u << TREW_TABLE_BOTH_HIGH, false);
            if (rec_l) record<WT>(sm, T, n, w.kl, 1u << TREW_TABLE_BOTH_LOW, false);
        }
    }
}

// the two halves of a read (staged as `range`) decided one after the other, a wave each: lane bounds + decide(); class tables
// kept in save slots slot0 / slot0 + 1.  which: bit 0 = left, bit 1 = right (the group pass hands back single halves).
template <int NW, typename WT>
__attribute__((noinline)) __device__ void decide_halves(ExactSmem sm, DevParams P, ReadRef rd, u32 range, u32 slot0, u32 which) {
    constexpr bool UB = NW > 0;
    constexpr int NWB = NW > 0 ? NW : 1;
    sm = uni(sm);
    P = uni(P);
    rd = uni(rd);
    range = rfl(range);
    slot0 = rfl(slot0);
    which = rfl(which);
    const Segment sL = get_segment(TREW_MODE_SHORT, 0, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    const Segment sR = get_segment(TREW_MODE_SHORT, 1, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    LaneMasks<NWB> mL, mR;
    const bool both = P.max_mer - P.min_mer < 32;  // the k range fits half a wave: both halves in one pass
    if (UB) {
        if (both) {
            lane_bounds_pair<NWB>(rd, sL.start, (int) sL.len, sR.start, (int) sR.len, P.min_mer, P.max_mer, mL);
        } else {
            if (which & 1u) lane_bounds<NWB>(rd, sL.start, (int) sL.len, P.min_mer, P.max_mer, mL);
            if (which & 2u) lane_bounds<NWB>(rd, sR.start, (int) sR.len, P.min_mer, P.max_mer, mR);
        }
    }
    const bool halves = UB && both;
    if (halves) mR = mL;  // the right half's bounds sit in lanes 32..63 of the same registers
    if (which & 1u) {
        const Decision<WT> left = decide<NW, WT>(view_segment(sm, range, sL.start, rd), P, (int) sL.len, sL.kmin, sL.kmax, ~0ull, mL, 0, halves ? 32 : 64);
        const u32 keptL = save_classes<WT>(sm, left, (int) slot0);  // a junction read records this half as it was counted here
        if (lane_id() == 0) put_decision<WT>(sm, slot0, (u32) left.kh | ((u32) left.kl << 8), keptL, left.sh, left.sl);
    }
    if (which & 2u) {
        const Decision<WT> right = decide<NW, WT>(view_segment(sm, range, sR.start, rd), P, (int) sR.len, sR.kmin, sR.kmax, ~0ull, mR, halves ? 32 : 0, halves ? 32 : 64);
        const u32 keptR = save_classes<WT>(sm, right, (int) slot0 + 1);
        if (lane_id() == 0) put_decision<WT>(sm, slot0 + 1u, (u32) right.kh | ((u32) right.kl << 8), keptR, right.sh, right.sl);
    }
    __syncthreads();
}

// buffer_task, kmer.cpp:111-173: one read, one wave
template <int NW, typename WT>
__device__ void run_short(ExactSmem sm, const DevParams &P, TableRef T, const ReadRef &rd) {
    const Segment sL = get_segment(TREW_MODE_SHORT, 0, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    const Segment sW = get_segment(TREW_MODE_SHORT, 2, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    if (sL.valid || sW.valid) stage_bases(sm, rd, 0, rd.len, 0);  // the whole read, once; segments are views
    if (sL.valid) decide_halves<NW, WT>(sm, P, rd, 0, 0, 3u);
    run_short_routed<NW, WT>(sm, P, T, rd, 0, 0, sL.valid);
}

// TREW_MODE_SEGMENT: k_mer_check on the whole read, high -> table 0, low -> table 1
template <int NW, typename WT>
__device__ void run_segment(ExactSmem sm, const DevParams &P, TableRef T, u32 unit, const ReadRef &rd,
                            const SegResults &R) {
    constexpr bool UB = NW > 0;
    constexpr int NWB = NW > 0 ? NW : 1;
    const Segment s = get_segment(TREW_MODE_SEGMENT, 0, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    if (!s.valid) return;
    sm = load_segment(sm, rd, 0, s.len);
    LaneMasks<NWB> m;
    if (UB) lane_bounds<NWB>(rd, 0, (int) s.len, P.min_mer, P.max_mer, m);
    const Decision<WT> d = decide<NW, WT>(sm, P, (int) s.len, s.kmin, s.kmax, ~0ull, m);
    if (d.kh > 0 && d.kh == d.kl) {
        record<WT>(sm, T, (int) s.len, d.kh, (1u << TREW_TABLE_FORWARD_HIGH) | (1u << TREW_TABLE_FORWARD_LOW), false);
    } else {
        record<WT>(sm, T, (int) s.len, d.kh, 1u << TREW_TABLE_FORWARD_HIGH, false);
        record<WT>(sm, T, (int) s.len, d.kl, 1u << TREW_TABLE_FORWARD_LOW, false);
    }
    if (lane_id() == 0 && R.k_high) {
        R.k_high[unit] = d.kh;
        R.k_low[unit] = d.kl;
        R.seq_high[unit] = (u64) d.sh;
        R.seq_low[unit] = (u64) d.sl;
        if (R.seq_high_hi) {
            R.seq_high_hi[unit] = sizeof(WT) > 8 ? (u64) (d.sh >> (8 * sizeof(WT) - 64)) : 0ull;
            R.seq_low_hi[unit] = sizeof(WT) > 8 ? (u64) (d.sl >> (8 * sizeof(WT) - 64)) : 0ull;
        }
    }
}
