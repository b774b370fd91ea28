// kernels/decide_group.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// decide_group: the selection loops of k_mer_check (kmer.cpp:2183-2258) for FOUR segments in lock step, sixteen lanes each.
//
// decide() (exact_core.inc) gives a whole wave to one segment and spends most of it on three lanes: a class count of a
// telomeric half has 3.2 runs on average, and around it sit a few hundred wave-uniform instructions of selection logic per k
// (profiles/r03/README.md: 36 of 64 lanes active per VALU instruction, decide = 44 % of the short-read kernel).  Here a wave
// takes the four segments of a pass -- both halves of two reads, or the four half-read segments of a pair -- one per DPP
// row: the state of the selection loops (thresholds, closed multiples, the k still to visit) is replicated over the 16 lanes
// of the row in VGPRs, every lane of a row walks the same k, and the class count of that k gives each of its (at most 16) runs
// a lane.  What the rows exchange goes through row-wide DPP reductions and ds_bpermute; nothing is wave-uniform any more, so
// one trip of the loop serves four segments.
//
// The group path only takes what fits it and hands everything else back (GroupOut::punt -> decide() decides the segment as
// before): a k with more than 16 runs when both skip slots are taken, a segment with an N that needs a class count, a failed
// check of a speculative skip.  Results are identical by construction: every comparison of decide() is reproduced exactly --
// frequencies are quotients of integers below 1024, and fl(a/b) >= fl(c/d) <=> a*d >= c*b for such quotients (two different
// ones differ by more than 1e-6, an ulp near 1 is 1.1e-16), so the thresholds an accepted k leaves behind are kept as integer
// pairs and compared by cross-multiplication; only the two baselines (arbitrary doubles) need the IEEE division itself.

// Region markers: a comment in the ISA (tools/isa_regions.py counts the instructions between them, by class) and, in builds with
// -DTREW_REGION_COUNTS, a trip counter per region (lane 0 of each wave, g_region[]) -- static class mix x trips = the DYNAMIC
// instruction mix of the kernel (tools/region_mix.py), instead of one static share applied to the whole instruction count.
#define TREW_REGION_LIST(X) \
    X(chunk) X(stage) X(group_setup) X(bounds) X(group) X(dg_loop) X(dg_pick) X(dg_eval) X(er_gaps) X(er_runs) X(er_canon) X(er_merge) X(er_max) \
    X(dg_decision) X(dg_end) X(routing) X(records) X(target) X(target_rows) X(target_eval) X(target_emit) X(fallback)
#define TREW_REGION_ENUM(n) kRegion_##n,
enum { TREW_REGION_LIST(TREW_REGION_ENUM) kRegionCount };
#ifdef TREW_REGION_COUNTS
__device__ unsigned long long g_region[64];
#define TREW_MARK(n)                                                                   \
    do {                                                                               \
        asm volatile("; MARK " #n);                                                    \
        if (lane_id() == 0) atomicAdd(&g_region[kRegion_##n], 1ull);                   \
    } while (0)
#else
#define TREW_MARK(n) asm volatile("; MARK " #n)
#endif
// Ordering point for LDS traffic of ONE wave (every workgroup of the exact kernel is one wave): the wave's LDS operations
// execute in program order, so all that is needed is that the compiler does not move them across.  __syncthreads() would also
// wait for every vector-memory operation in flight -- the next chunk on its way into LDS (exact_kernel) -- at each call.
__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#define TREW_DPP(v, ctrl) ((u32) __builtin_amdgcn_update_dpp(0, (int) (v), (ctrl), 0xf, 0xf, false))
// reductions over a group of G lanes (16 = a DPP row, 32 = half a wave), every lane gets the result: four rotations inside the
// rows, and for 32 lanes one exchange with the partner row (ds_swizzle: lane ^ 16)
__device__ __forceinline__ u32 swap16(u32 v) { return (u32) __builtin_amdgcn_ds_swizzle((int) v, 0x401F); }  // and 0x1f, or 0, xor 0x10
template <int G = 16>
__device__ __forceinline__ u32 row_or(u32 v) {
    v |= TREW_DPP(v, 0x128);  // row_ror:8
    v |= TREW_DPP(v, 0x124);
    v |= TREW_DPP(v, 0x122);
    v |= TREW_DPP(v, 0x121);
    if (G == 32) v |= swap16(v);
    return v;
}
template <int G = 16>
__device__ __forceinline__ u32 row_add(u32 v) {
    v += TREW_DPP(v, 0x128);
    v += TREW_DPP(v, 0x124);
    v += TREW_DPP(v, 0x122);
    v += TREW_DPP(v, 0x121);
    if (G == 32) v += swap16(v);
    return v;
}
template <int G = 16>
__device__ __forceinline__ u32 row_max(u32 v) {
    v = max(v, TREW_DPP(v, 0x128));
    v = max(v, TREW_DPP(v, 0x124));
    v = max(v, TREW_DPP(v, 0x122));
    v = max(v, TREW_DPP(v, 0x121));
    if (G == 32) v = max(v, swap16(v));
    return v;
}
// value of lane `src` (any lane of the wave, per-lane choice) -- all lanes must call it
__device__ __forceinline__ u32 lane_gather(u32 v, u32 src) { return (u32) __builtin_amdgcn_ds_bpermute((int) (src << 2), (int) v); }
__device__ __forceinline__ u64 lane_gather(u64 v, u32 src) { return ((u64) lane_gather((u32) (v >> 32), src) << 32) | lane_gather((u32) v, src); }

// What lane (half, k) of lane_bounds_pair knows about its k, in one word for the group pass (kGroupBnd):
// bits 0..9 maxbucket, 10..19 COUNT, 20..26 runs (capped), 27 bound >= LOW_BASELINE, 28 bound >= HIGH_BASELINE, 29 the segment holds an N
template <int NW>
__device__ __forceinline__ u32 pack_bound(const LaneMasks<NW> &m, const DevParams &P) {
    static_assert(NW <= 10, "COUNT must fit 10 bits");
    const u32 runs = m.runs < 127u ? m.runs : 127u;
    return m.m8 | (m.cnt << 10) | (runs << 20) | (m.ub >= P.low ? 1u << 27 : 0u) | (m.ub >= P.high ? 1u << 28 : 0u) | (m.has_n ? 1u << 29 : 0u);
}

// kGroupMult[i]: bit t <=> MIN_MER + t is a multiple of MIN_MER + i (t < 32) -- what an accepted k closes (kmer.cpp:2225-2236)
__device__ __forceinline__ void group_fill_multiples(ExactSmem sm, const DevParams &P) {
    const u32 i = lane_id();
    if (i < 32u) {
        const int k = P.min_mer + (int) i;
        u32 m = 0;
        for (int t = k; t <= P.min_mer + 31; t += k) m |= 1u << (t - P.min_mer);
        sm_group(sm)[kGroupMult + i] = m;
    }
}

// position of the r-th (0-based) set bit of an NW-word mask; r < popcount
template <int NW>
__device__ __forceinline__ u32 select_bit(const u32 (&m)[NW], u32 r) {
    u32 word = m[0], sub = 0, base = 0, cum = 0;
#pragma unroll
    for (int w = 0; w + 1 < NW; w++) {
        cum += __popc(m[w]);
        const bool ge = r >= cum;  // monotone in w: the last word that still says so is the one
        word = ge ? m[w + 1] : word;
        sub = ge ? cum : sub;
        base = ge ? 32u * (u32) (w + 1) : base;
    }
    r -= sub;
#pragma unroll
    for (u32 sh = 16; sh >= 1; sh >>= 1) {
        const u32 c = __popc(word & ((1u << sh) - 1u));
        const bool ge = r >= c;
        r -= ge ? c : 0u;
        word = ge ? word >> sh : word;
        base += ge ? sh : 0u;
    }
    return base;
}

// window starting at staged base p (per lane), k bases (k <= 32), first base most significant
__device__ __forceinline__ u64 window_word_at(ExactSmem sm, u32 p, int k) {
    const u32 wi = p >> 5, sh = 2u * (p & 31u);
    const u64 a = sm_seq(sm)[wi], b = sm_seq(sm)[wi + 1];
    const u64 x = sh ? ((a << sh) | (b >> (64u - sh))) : a;
    return x >> (64 - 2 * k);
}

// One class count of a row (the body of eval_runs, kmer.cpp:2183-2216, for 16 lanes): the windows of a segment at k, a lane per
// run.  lo / hi / v1: the segment's planes and valid-base mask from bit 0 (same in every lane of the row), has_n: it holds an N,
// s0: its first base in the staged seq[], k and W = L - k + 1: per row, ev: the row takes part.  All 64 lanes call it together.
template <typename WT>
struct RowCount {
    u32 R;      // runs of the row (more than 16, or more than 4 N in the segment: nothing was counted, `over`)
    u32 over;
    u32 count;  // K_MER_DATA_COUNT: windows without an N
    WT canon;   // canonical word of the lane's run (all ones in lanes without one)
    u32 cnt;    // class size in the lane of the class's first run, else 0: (canon, cnt) is the row's class table
    u32 maxc;   // K_MER_DATA_MAX
    u32 homo;   // K_MER_DATA_MAX_SEQ uses a single base (get_repeat_check)
    WT mseq;    // K_MER_DATA_MAX_SEQ (WANT_SEQ)
};
template <int NW, typename WT, bool WANT_SEQ, int G = 16>
__device__ __forceinline__ RowCount<WT> eval_row(ExactSmem sm, const u32 (&lo)[NW], const u32 (&hi)[NW], const u32 (&v1)[NW], u32 has_n, u32 s0, int k,
                                                 int W, u32 ev) {
    static_assert(G == 16 || G == 32, "a group is a DPP row or half a wave");
    constexpr u32 kGM = G == 32 ? 0xffffffffu : 0xffffu;  // the group's lanes as a mask
    const u32 lane = lane_id(), j = lane & (u32) (G - 1), gbase = lane & (u32) (64 - G);
    RowCount<WT> rc;
    // V = the W windows ...
    u32 V[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) {
        V[w] = low_mask(W - 32 * w);
    }
    // ... without those that hold an N (kmer.cpp:2190): an N at base p spoils the windows p-k+1 .. p.  Segments with an N are one
    // in five of those that reach this point and carry one N as a rule, so the N are taken one at a time (more than four: the
    // row gives up) instead of the AND over k shifted masks that lane_bounds builds for every k.
    u32 many_n = 0;
    const bool gaps = __any((ev & has_n) != 0u);
    if (gaps) {
        TREW_MARK(er_gaps);
        u32 nn[NW], left = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            nn[w] = (ev & has_n) ? (~v1[w] & low_mask(W + k - 1 - 32 * w)) : 0u;
            left += __popc(nn[w]);
        }
        many_n = left > 4u ? 1u : 0u;
        left = many_n ? 0u : left;
        while (__any(left != 0u)) {
            // lowest N of the row
            u32 p = 0, found = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const u32 here = (found == 0u && nn[w] != 0u) ? 1u : 0u;
                p = here ? 32u * (u32) w + (u32) __builtin_ctz(nn[w] | (here ^ 1u)) : p;
                nn[w] = here ? (nn[w] & (nn[w] - 1u)) : nn[w];
                found |= here;
            }
            const int a = left ? ((int) p - k + 1 > 0 ? (int) p - k + 1 : 0) : 0, b = left ? (int) p + 1 : 0;  // windows [a, b) go
#pragma unroll
            for (int w = 0; w < NW; w++) {
                V[w] &= ~(low_mask(b - 32 * w) & ~low_mask(a - 32 * w));
            }
            left = left ? left - 1u : 0u;
        }
    }
    // Lemma A from the planes: E = bases i and i+k agree; a run starts where a window does not continue its predecessor and ends
    // where its successor does not continue it
    TREW_MARK(er_runs);
    u32 st[NW], E[NW], R = 0, count = 0;
    {
        u32 prev = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            E[w] = ~((lo[w] ^ shr_var_word<NW>(lo, w, (u32) k)) | (hi[w] ^ shr_var_word<NW>(hi, w, (u32) k)));
            const u32 ve = V[w] & E[w];
            st[w] = V[w] & ~((ve << 1) | (prev >> 31));
            prev = ve;
            R += __popc(st[w]);
            count += __popc(V[w]);
        }
    }
    rc.R = R;
    rc.count = count;
    rc.over = ev & ((R > (u32) G ? 1u : 0u) | many_n);
    ev &= rc.over ^ 1u;
    const bool runlane = ev != 0u && j < R;
    const u32 s = runlane ? select_bit<NW>(st, j) : 0u;
    u32 e;
    if (gaps) {  // wave-uniform: some row's windows have holes
        u32 en[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const u32 vn = w + 1 < NW ? V[w + 1 < NW ? w + 1 : 0] : 0u;
            en[w] = V[w] & ~(E[w] & alignbit(vn, V[w], 1u));
        }
        e = runlane ? select_bit<NW>(en, j) : 0u;
    } else {  // an N-free segment's runs tile its windows: a run ends where the next begins
        // lane j gets lane j + 1: row_shl:1 inside a row, wave_shl:1 across the two rows of a 32-lane group (what the last lane of
        // the group receives is not used: j + 1 < R fails there)
        const u32 nxt = G == 32 ? (u32) __builtin_amdgcn_update_dpp(0, (int) s, 0x130, 0xf, 0xf, true) : (u32) __builtin_amdgcn_update_dpp(0, (int) s, 0x101, 0xf, 0xf, true);
        e = (j + 1u < R) ? nxt - 1u : (u32) (W - 1);
    }
    const u32 len = e - s + 1u;
    WT canon = ~(WT) 0;
    TREW_MARK(er_canon);
    if (runlane) canon = min_rotation<WT>(window_word_at(sm, s0 + s, k), k);
    // classes: the lowest run without one leads, one gather + compare finds its members; runs are in position order, so the
    // member in the highest lane ends last
    u32 rem = ev ? (R >= (u32) G ? kGM : ((1u << (R & 31u)) - 1u)) : 0u;
    u32 tot = 0, last = 0, first = 0;
    // Classes: the lowest run that has none yet leads, one gather + compare finds its members (runs are in position order, so the
    // member in the highest lane ends last).  The loop ends for a row as soon
    // as the largest class found so far is larger than all the windows still without a class: it is K_MER_DATA_MAX whatever the
    // rest adds up to, and nothing else needs the rest merged -- counts add up in the count table, so every remaining run stands
    // as a class of its own (the same key may then sit in several lanes of the row's table).  A telomeric slice of a long read
    // has ~15 runs in a dozen classes, one per sequencing error: a dozen trips, two LDS round trips each, become one.
    u32 covered = 0, best = 0;
    while (__any(rem != 0u)) {
        TREW_MARK(er_merge);
        const bool open = ((rem >> j) & 1u) != 0u;  // (rem has bits of run lanes only)
        const u32 lead = rem ? (u32) __builtin_ctz(rem) : 0u;
        const WT other = lane_gather(canon, gbase + lead);
        const bool eq = open && other == canon;
        const u32 bal = (u32) (__ballot(eq) >> gbase) & kGM;
        const u32 total = row_add<G>(eq ? len : 0u);
        const u32 lend = lane_gather(e, gbase + (bal ? 31u - (u32) __builtin_clz(bal) : 0u));
        covered += total;
        best = total > best ? total : best;
        const bool settled = rem != 0u && best > count - covered;
        const bool alone = settled && open && !eq;  // a run left without a class when its row is settled: a class of its own
        tot = eq ? total : (alone ? len : tot);
        last = eq ? lend : (alone ? e : last);
        first = eq ? (j == lead ? 1u : 0u) : (alone ? 1u : first);
        rem = settled ? 0u : (rem & ~bal);
    }
    // MAX and MAX_SEQ: the largest class, ties to the one whose last window comes first (strict '<' at kmer.cpp:2202)
    TREW_MARK(er_max);
    const u32 key = runlane ? ((tot << 16) | (0xffffu - last)) : 0u;
    const u32 mkey = row_max<G>(key);
    const u32 win = (runlane && key == mkey) ? 1u : 0u;
    rc.maxc = mkey >> 16;
    rc.homo = row_or<G>(win & (is_homopolymer<WT>(canon, k) ? 1u : 0u));
    rc.mseq = 0;
    if (WANT_SEQ) {
        const u32 wb = (u32) (__ballot(win != 0u) >> gbase) & kGM;
        rc.mseq = lane_gather(canon, gbase + (wb ? (u32) __builtin_ctz(wb) : 0u));
    }
    rc.canon = canon;
    rc.cnt = first ? tot : 0u;
    return rc;
}

// ---- bounds in row layout ----
// lane_bounds_pair gives a (half, k) to every lane, and every lane repeats what does not depend on k: the segment's planes
// (12 LDS reads, 9 funnel shifts), its masks and three prefix parities (~190 of ~380 instructions, tools/attribute_insts.sh).
// Here 3 NW lanes of a row prepare the segment once -- a lane per (feature, word) -- and leave planes, valid mask and prefix
// parities in LDS (kGroupBnd, 6 NW words per row); then every lane of the row reads them back and bounds its two k (MIN_MER + j
// and MIN_MER + 16 + j).  The bound of a k is the one of lane_bounds_at, word for word.
template <int NW, int G = 16, bool IN_LDS = true>
__device__ __forceinline__ void row_prepare(ExactSmem sm, const ReadRef &rd, const Segment &sg, bool rowvalid) {
    static_assert((64 / G) * 6 * NW <= 128, "the groups' 6 NW words each must fit kGroupBnd's 128 words");
    static_assert(3 * NW <= G, "a lane per (feature, word)");
    // Lane j = p NW + w of a group takes word w of feature p (lo, hi, lo & hi): its word of the three planes, the parity prefix
    // inside the word (five shift + xor steps), and the parity of the feature's lower words from the lanes that hold them --
    // instead of three lanes walking all NW words one after the other (100 instructions for 3 words, 160 for 5, on 3 lanes).
    const u32 lane = lane_id(), g = lane / (u32) G, j = lane & (u32) (G - 1);
    u32 *prep = sm_group(sm) + kGroupBnd + g * (6u * NW);
    const u32 p = j / (u32) NW, w = j - p * (u32) NW;
    const bool mine = j < 3u * NW && rowvalid;
    u32 lo1[1] = {0}, hi1[1] = {0}, nm1[1] = {0};
    if (mine) {
        if (IN_LDS)
            load_planes_lds<1>(rd, sg.start + 32u * w, lo1, hi1, nm1);  // (the rows' reads are staged in LDS)
        else
            load_planes<1>(rd, sg.start + 32u * w, lo1, hi1, nm1);  // (long reads stay in global memory)
    }
    const u32 v1 = ~nm1[0] & low_mask((int) sg.len - 32 * (int) w);  // base is A/C/G/T and inside the segment
    const u32 f1 = lo1[0] & v1, f2 = hi1[0] & v1;
    const u32 x = word_parity(p == 0u ? f1 : (p == 1u ? f2 : (f1 & f2)));  // bit i = parity of the word's bits 0..i
    const u32 top = mine ? x >> 31 : 0u;  // parity of the whole word
    u32 carry = 0;   // parity of the feature's words below w
#pragma unroll
    for (int u = 0; u + 1 < NW; u++) {
        const u32 t = lane_gather(top, g * (u32) G + p * (u32) NW + (u32) u);
        carry ^= (u32) u < w ? t : 0u;
    }
    if (mine) {
        prep[j] = p == 0u ? lo1[0] : (p == 1u ? hi1[0] : v1);  // planes and valid mask: word p NW + w
        prep[3 * NW + j] = ((x ^ (0u - carry)) << 1) | carry;   // exclusive prefix parity: P[i] = XOR of f below i
    }
}

// what a row's lanes read back: planes, valid-base mask, the three prefix parities
template <int NW>
struct RowSeg {
    u32 lo[NW], hi[NW], v1[NW], P1[NW], P2[NW], P3[NW];
    u32 has_n;
};
template <int NW, int G = 16>
__device__ __forceinline__ void row_load(ExactSmem sm, int L, RowSeg<NW> &r) {
    const u32 g = lane_id() / (u32) G;
    const u32 *prep = sm_group(sm) + kGroupBnd + g * (6u * NW);
    u32 anyn = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        r.lo[w] = prep[0 * NW + w];
        r.hi[w] = prep[1 * NW + w];
        r.v1[w] = prep[2 * NW + w];
        r.P1[w] = prep[3 * NW + w];
        r.P2[w] = prep[4 * NW + w];
        r.P3[w] = prep[5 * NW + w];
        anyn |= ~r.v1[w] & low_mask(L - 32 * w);
    }
    r.has_n = anyn != 0u ? 1u : 0u;
}

// frequency bound of one k of the row's segment, packed as pack_bound does (lane_bounds_at from "V" on); k > gmax or outside the
// k range the instantiation handles: the empty bound (nothing passes)
// SMALLK: the caller knows k < 32 (the first k of a lane when MIN_MER + 15 < 32): a funnel shift by k needs no choice of words
template <int NW, bool SMALLK>
__device__ __forceinline__ u32 shr_k_word(const u32 (&x)[NW], int w, u32 k) {
    if (SMALLK) return alignbit(w + 1 < NW ? x[w + 1 < NW ? w + 1 : 0] : 0u, x[w], k);
    return shr_var_word<NW>(x, w, k);
}
template <int NW, bool SMALLK = false>
__device__ __forceinline__ u32 bound_at_k(const RowSeg<NW> &r, int L, int k, int gmax, const DevParams &P) {
    const u32 ku = (u32) k;
    u32 V[NW];
    windows_without_n<NW>(r.v1, r.has_n != 0u /* row-uniform */, L, k, 32, V);
    Buckets8<false, false> b8;
    u32 Ew[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const u32 F1 = r.P1[w] ^ shr_k_word<NW, SMALLK>(r.P1, w, ku), F2 = r.P2[w] ^ shr_k_word<NW, SMALLK>(r.P2, w, ku);
        const u32 F3 = r.P3[w] ^ shr_k_word<NW, SMALLK>(r.P3, w, ku);
        Ew[w] = ~((r.lo[w] ^ shr_k_word<NW, SMALLK>(r.lo, w, ku)) | (r.hi[w] ^ shr_k_word<NW, SMALLK>(r.hi, w, ku)));
        b8.add(F1, F2, F3, V[w]);
    }
    const u32 m8 = b8.largest(), count = b8.count, links = class_links<NW>(V, Ew);
    const u32 runs = count - links < 127u ? count - links : 127u;
    // m8 / COUNT >= baseline as the reference's doubles say it (MAX <= m8 and IEEE division is monotone in the numerator).  The
    // division itself is only needed within rounding distance of the threshold: baseline * COUNT lies within 2e-13 of its double.
    const double dm = (double) m8, dc = (double) count;
    const double tl = P.low * dc, th = P.high * dc;
    u32 pass_lo = dm > tl ? 1u : 0u, pass_hi = dm > th ? 1u : 0u;
    const bool amb = fabs(dm - tl) <= 1e-9 || fabs(dm - th) <= 1e-9;
    if (__any(amb)) {
        const double ub = count ? dm / dc : 0.0;
        pass_lo = ub >= P.low ? 1u : 0u;
        pass_hi = ub >= P.high ? 1u : 0u;
    }
    const bool inr = k <= gmax && count != 0u;
    return inr ? (m8 | (count << 10) | (runs << 20) | (pass_lo << 27) | (pass_hi << 28) | (r.has_n << 29)) : (r.has_n << 29);
}

template <typename WT>
struct GroupOut {  // per lane; everything but the class table entry is the same in the 16 lanes of a row
    u32 kk;         // target_k_high | target_k_low << 8
    WT sh, sl;      // MAX_SEQ at those k
    u32 saved;      // k | items << 8 | COUNT << 16 of the class table of the last accepted k (0: none), as save_classes packs it
    WT kept_canon;  // entry (lane & 15) of that table
    u32 kept_cnt;
    bool punt;      // the row gave the segment back: decide() takes it
};

// One pass: the row of a lane decides segment sg (staged as `range`) of read rd; valid = the row has a segment at all.
// The packed bounds of the four segments are in kGroupBnd (lane_bounds_pair + pack_bound, row g at [32 g, 32 g + 32)).
// All 64 lanes call it together.  WANT_SEQ: MAX_SEQ of the accepted k is reported (the pair driver compares them; the short
// driver does not look at them).
// Written branch-free on purpose: conditions are 0 / 1 words combined with & and |, updates are selects.  With `&&` and `if`
// the compiler turns every condition into an exec-mask region (s_and_saveexec + s_cbranch + s_or) -- the first version of this
// loop had 530 instructions a trip, a third of them scalar mask bookkeeping.
// G = 16: four segments a wave, a lane bounds two k (index j and 16 + j: bnd0, bnd1); G = 32: two segments a wave (long-read
// slices: up to 32 runs a class count), a lane bounds one k (index j: bnd0).
template <int NW, typename WT, bool WANT_SEQ, int G = 16>
__device__ __forceinline__ GroupOut<WT> decide_group(ExactSmem sm, const DevParams &P, const RowSeg<NW> &rs, u32 bnd0, u32 bnd1, u32 range, const Segment &sg,
                                                     bool valid) {
    static_assert(sizeof(WT) == 8, "k <= 32: the k range must fit a 32-bit index mask");
    PH_T0(t_ph);
    const u32 lane = lane_id(), j = lane & (u32) (G - 1), gbase = lane & (u32) (64 - G);
    const u32 *grp = sm_group(sm);
    const u32 (&lo)[NW] = rs.lo;
    const u32 (&hi)[NW] = rs.hi;
    const int L = (int) sg.len;
    const u32 s0 = range_base(sm, range) + sg.start;
    const u32 has_n = rs.has_n;
    GroupOut<WT> o;
    o.kk = 0;
    o.sh = o.sl = 0;
    o.saved = 0;
    o.kept_canon = 0;
    o.kept_cnt = 0;
    // k index i <-> k = MIN_MER + i; the segment's own range
    u32 todo = 0;
    {
        const u32 a = (u32) (sg.kmin - P.min_mer) & 31u, b = (u32) (sg.kmax - P.min_mer);
        const u32 m = (b >= 31u ? 0xffffffffu : ((2u << (b & 31u)) - 1u)) & ~((1u << a) - 1u);
        todo = (valid && sg.kmax >= sg.kmin) ? m : 0u;
    }
    // thresholds of the two selection loops as fractions num / den: 0 / 0 = nothing accepted yet (every bound reaches it; the
    // baseline is in the pass bits of the packed bound); after an acceptance the accepted MAX / COUNT
    u32 lo_num = 0, lo_den = 0, hi_num = 0, hi_den = 0, closed_lo = 0, closed_hi = 0;
    // speculative skips (see decide()): k index | eligible loops << 8 | loops that later accepted << 10 | taken << 12; the bound
    // as m8 | COUNT << 16; the multiples of the k
    u32 sk0 = 0, sk1 = 0, skb0 = 0, skb1 = 0, skm0 = 0, skm1 = 0;
    u32 viol = 0, punt = 0;
    const u32 m8_0 = bnd0 & 1023u, cn_0 = (bnd0 >> 10) & 1023u, m8_1 = bnd1 & 1023u, cn_1 = (bnd1 >> 10) & 1023u;
    const u32 bit0 = 1u << j, bit1 = G == 16 ? 1u << ((16u + j) & 31u) : 0u;
    // k still worth a visit: open in a loop whose threshold the bound reaches (fractions compared by cross-multiplication)
    auto eligible = [&]() __attribute__((always_inline)) -> u32 {
        const u32 l0 = (bnd0 >> 27) & ~(closed_lo >> j) & (__umul24(m8_0, lo_den) >= __umul24(lo_num, cn_0) ? 1u : 0u);
        const u32 h0 = (bnd0 >> 28) & ~(closed_hi >> j) & (__umul24(m8_0, hi_den) >= __umul24(hi_num, cn_0) ? 1u : 0u);
        if (G == 32) return row_or<G>(((l0 | h0) & 1u) ? bit0 : 0u);
        const u32 l1 = (bnd1 >> 27) & ~(closed_lo >> ((16u + j) & 31u)) & (__umul24(m8_1, lo_den) >= __umul24(lo_num, cn_1) ? 1u : 0u);
        const u32 h1 = (bnd1 >> 28) & ~(closed_hi >> ((16u + j) & 31u)) & (__umul24(m8_1, hi_den) >= __umul24(hi_num, cn_1) ? 1u : 0u);
        return row_or<G>((((l0 | h0) & 1u) ? bit0 : 0u) | (((l1 | h1) & 1u) ? bit1 : 0u));
    };
    TREW_MARK(dg_loop);
    todo &= eligible();
    for (;;) {
        // ---- the next k of every row; a k with more runs than the row has lanes is passed over on the spot (skip slot) ----
        u32 act, kidx, bk;
        for (;;) {
            TREW_MARK(dg_pick);
            act = (todo != 0u && punt == 0u) ? 1u : 0u;
            kidx = act ? (u32) __builtin_ctz(todo) : 0u;
            bk = G == 32 ? lane_gather(bnd0, gbase + kidx) : lane_gather(kidx >= 16u ? bnd1 : bnd0, gbase + (kidx & 15u));
            const u32 heavy = act & (((bk >> 20) & 127u) > (u32) G ? 1u : 0u);
            if (!__any(heavy)) break;
            const u32 m8k = bk & 1023u, cntk = (bk >> 10) & 1023u;
            const u32 el = ((bk >> 27) & ~(closed_lo >> kidx) & (__umul24(m8k, lo_den) >= __umul24(lo_num, cntk) ? 1u : 0u) & 1u) |
                           (((bk >> 28) & ~(closed_hi >> kidx) & (__umul24(m8k, hi_den) >= __umul24(hi_num, cntk) ? 1u : 0u) & 1u) << 1);
            const u32 mk = grp[kGroupMult + kidx];
            const u32 take0 = heavy & (sk0 == 0u ? 1u : 0u), take1 = heavy & (take0 ^ 1u) & (sk1 == 0u ? 1u : 0u);
            sk0 = take0 ? (kidx | (el << 8) | (1u << 12)) : sk0;
            skb0 = take0 ? (m8k | (cntk << 16)) : skb0;
            skm0 = take0 ? mk : skm0;
            sk1 = take1 ? (kidx | (el << 8) | (1u << 12)) : sk1;
            skb1 = take1 ? (m8k | (cntk << 16)) : skb1;
            skm1 = take1 ? mk : skm1;
            punt |= heavy & ((take0 | take1) ^ 1u);  // no slot left
            todo = heavy ? (todo & (todo - 1u)) : todo;
        }
        if (!__any(act)) break;
        TREW_MARK(dg_eval);
        todo &= todo - 1u;  // (0 stays 0)
        const int k = P.min_mer + (int) kidx;
        const u32 lo_open = ~(closed_lo >> kidx) & 1u, hi_open = ~(closed_hi >> kidx) & 1u;
        u32 ev = act;
        const int W = ev ? L - k + 1 : 1;
        // ---- class count of k, a lane per run ----
        PH_T0(t_runs);
        const RowCount<WT> rc = eval_row<NW, WT, WANT_SEQ, G>(sm, lo, hi, rs.v1, has_n, s0, k, W, ev);
        punt |= rc.over;  // more than four N (more than 16 runs cannot happen: the bound pass counted the same runs)
        ev &= rc.over ^ 1u;
        const u32 R = rc.R, maxc = rc.maxc, count = rc.count, homo = rc.homo;
        const WT mseq = rc.mseq, canon = rc.canon;
        PH_ADD(PH_RUNS, t_runs);
        TREW_MARK(dg_decision);
        // ---- f >= MAX(baseline, running frequency), kmer.cpp:2221-2258: the running frequency, once there is one, is at least
        // the baseline; before that the baseline itself decides (IEEE division, as the reference) ----
        // (MAX / COUNT >= baseline by one multiplication; the division only within rounding distance of the threshold, as in bound_at_k)
        const double dm = (double) maxc, dc = (double) count;
        const double tl = P.low * dc, th = P.high * dc;
        u32 base_lo = dm > tl ? 1u : 0u, base_hi = dm > th ? 1u : 0u;
        if (__any(ev != 0u && (fabs(dm - tl) <= 1e-9 || fabs(dm - th) <= 1e-9))) {
            const double f = dm / dc;
            base_lo = f >= P.low ? 1u : 0u;
            base_hi = f >= P.high ? 1u : 0u;
        }
        const u32 ge_lo = lo_den ? (__umul24(maxc, lo_den) >= __umul24(lo_num, count) ? 1u : 0u) : base_lo;
        const u32 ge_hi = hi_den ? (__umul24(maxc, hi_den) >= __umul24(hi_num, count) ? 1u : 0u) : base_hi;
        const u32 okv = ev & (homo ^ 1u) & (maxc != 0u ? 1u : 0u);
        const u32 acc_lo = okv & lo_open & ge_lo, acc_hi = okv & hi_open & ge_hi, acc = acc_lo | (acc_hi << 1);
        const u32 mk = grp[kGroupMult + kidx];
        o.kk = acc_lo ? ((o.kk & 0xffu) | ((u32) k << 8)) : o.kk;
        o.kk = acc_hi ? ((o.kk & 0xff00u) | (u32) k) : o.kk;
        lo_num = acc_lo ? maxc : lo_num;
        lo_den = acc_lo ? count : lo_den;
        hi_num = acc_hi ? maxc : hi_num;
        hi_den = acc_hi ? count : hi_den;
        closed_lo |= acc_lo ? mk : 0u;
        closed_hi |= acc_hi ? mk : 0u;
        if (WANT_SEQ) {
            o.sl = acc_lo ? mseq : o.sl;
            o.sh = acc_hi ? mseq : o.sh;
        }
        o.saved = acc ? ((u32) k | (R << 8) | (count << 16)) : o.saved;
        o.kept_canon = acc ? canon : o.kept_canon;
        o.kept_cnt = acc ? rc.cnt : o.kept_cnt;
        // a k passed over earlier stays harmless only if every later acceptance in a loop it was eligible for clears its bound
        // and is not one of its multiples (decide())
        {
            const u32 hit0 = acc & (sk0 >> 8) & 3u, hit1 = acc & (sk1 >> 8) & 3u;
            const u32 bad0 = (__umul24(maxc, skb0 >> 16) < __umul24(skb0 & 0xffffu, count) ? 1u : 0u) | ((skm0 >> kidx) & 1u);
            const u32 bad1 = (__umul24(maxc, skb1 >> 16) < __umul24(skb1 & 0xffffu, count) ? 1u : 0u) | ((skm1 >> kidx) & 1u);
            viol |= (hit0 ? bad0 : 0u) | (hit1 ? bad1 : 0u);
            sk0 |= hit0 << 10;
            sk1 |= hit1 << 10;
        }
        if (__any(acc)) {
            todo &= eligible();
            if (!__any(todo != 0u && punt == 0u)) break;  // nothing left anywhere: spare the pick that would find that out
        }
    }
    TREW_MARK(dg_end);
    // ... and at least one such acceptance exists in each of those loops; otherwise the skipped k might have been the answer
    viol |= ((sk0 >> 8) & 3u & ~((sk0 >> 10) & 3u)) | ((sk1 >> 8) & 3u & ~((sk1 >> 10) & 3u));
    o.punt = (punt | viol) != 0u;
    PH_ADD(PH_DECIDE, t_ph);
    return o;
}

// Both reads' bases (triples staged in LDS) into seq[] / nmask[] of ranges 0 and 1, read A in lanes 0..31, read B in lanes
// 32..63 -- what two stage_bases calls do, inline: stage_bases is a call, and a call waits for everything in flight, including
// the next chunk on its way into LDS (exact_kernel).
__device__ __forceinline__ void stage_two(ExactSmem sm, const ReadRef &rdA, const ReadRef &rdB, bool haveB) {
    const u32 lane = lane_id();
    lds_sync();
    const u32 r = lane >> 5, segwords = exact_rangewords(sm.cap);
    ReadRef rr;
    rr.w = r ? rdB.w : rdA.w;
    rr.len = r ? rdB.len : rdA.len;
    rr.nw = r ? rdB.nw : rdA.nw;
    const u32 L = rr.len;
    u64 *seq = sm_seq(sm) + r * segwords;
    u32 *nmk = sm_nmask(sm) + r * segwords;
    const u32 nwords = (L + 31u) >> 5;
    if (r == 0u || haveB) {
        for (u32 l = lane & 31u; l < segwords; l += 32u) {
            u64 sq = 0;
            u32 nmv = 0xffffffffu;
            if (l < nwords) {
                u32 lo1[1], hi1[1], nm1[1];
                load_planes_lds<1>(rr, 32u * l, lo1, hi1, nm1);
                nmv = nm1[0] | ~low_mask<true>((int) L - 32 * (int) l);
                const u32 lq = lo1[0] & ~nmv, hq = hi1[0] & ~nmv;
                sq = spread32(__brev(lq)) | (spread32(__brev(hq)) << 1);
            }
            seq[l] = sq;
            nmk[l] = nmv;
        }
    }
    lds_sync();
}

// strand-canonical key of k_mer_target, kmer.cpp:1979-1988
template <typename WT>
__device__ __forceinline__ WT strand_canon(WT w, int k) {
    const WT rc = min_rotation<WT>(revcomp(w, k), k);
    return rc < w ? rc : w;
}

// MAX_SEQ as the other strand's chain sees it (get_dir_seq, kmer.cpp:307-313)
template <typename WT>
__device__ __forceinline__ WT strand_flip(WT w, int k) {
    return min_rotation<WT>(revcomp(w, k), k);
}

// buffer_task (kmer.cpp:111-173) for TWO reads in one pass: the four halves decided together by decide_group, then routed and
// recorded in ROW SPACE -- the class tables are still in the rows' registers, so a record (kmer.cpp:119-163) is one pass of
// count-cache adds straight from them, and k_mer_target (kmer.cpp:1894-2017) of a read whose halves agree is one more class count
// of the same kind over the whole read (eval_row on the read's planes, both reads at once).  A read that needs anything else --
// a half the rows gave back, records at two different k, the whole-read check of reads shorter than 4 MAX_MER, a whole read with
// more than 16 runs -- goes through decide_halves / run_short_routed / target as before.
// rdA / rdB: reads whose triples are staged in LDS, both with valid halves (n >= 4 MIN_MER); haveB = false: rdA alone (rows 2
// and 3 idle).  Only instantiated where the k range fits 32 indices.
// SB: the positions of the two reads in the kernel's list, by which the packed bounds the bounds pass (bounds_pass.inc) left for them are
// found -- StoredBounds (positions at or beyond the stored prefix have none), or NoStoredBounds in the instantiations that
// never have any.  Where both reads have stored bounds, lane (row g, j) loads word j and word 16 + j of its half and the row needs
// no parities; otherwise the rows bound their k themselves (row_prepare, bound_at_k).
constexpr u32 kBoundWords = 32;                   // packed words per half, index k - MIN_MER: every k of a run the group pass takes
constexpr u32 kBoundItemWords = 2 * kBoundWords;  // per worklist entry: left half, right half
struct NoStoredBounds {
    static constexpr bool kAny = false;
};
struct StoredBounds {
    static constexpr bool kAny = true;
    u32 posA, posB;  // worklist positions of rdA and rdB (wave-uniform)
};
// The argument list of exact_kernel as the kernarg ABI lays it out (natural alignment, in order).  The kernel hands a pointer into
// the segment down as its table descriptor (TableRef), and run_short_group reads the last two arguments from it where it wants
// them: scalar loads, cached, instead of SGPRs held across every pass (see fetch_words in exact_kernel.inc).
struct ExactKernArgs {
    DevParams P;
    DevBatch B;
    DevTableG1 TG;
    const u32 *wl;
    u32 *wl_count, *wl_count_next;
    u32 wl_cap;
    SegResults R;
    u32 cap, rawwords;
    const u32 *bnd;  // the packed bounds of the first bnd_cap worklist entries (bounds_pass.inc), bnd_cap = 0: none
    u32 bnd_cap;
    const u32 *live;  // the leading entries of the list exact_kernel<3, short, u64> works on (exact_kernel.inc)
};
template <int NW, typename WT, typename SB>
__device__ void run_short_group(ExactSmem sm, const DevParams &P, TableRef T, const ReadRef rdA, const ReadRef rdB, bool haveB, const SB sb) {
    const u32 lane = lane_id();
#if defined(TREW_AB_SKIP) && TREW_AB_SKIP >= 5  // A/B builds (instruction attribution, profiles/r04): 5 = chunk fetch only
    return;
#endif
    // the stored bounds start travelling before the bases are staged: they are wanted behind that
    u32 st0 = 0, st1 = 0;
    bool stored = false;
    if constexpr (SB::kAny) {
        typedef const __attribute__((address_space(4))) u64 *c64;
        typedef const __attribute__((address_space(4))) u32 *c32;
        const u64 ka = (u64) __builtin_amdgcn_kernarg_segment_ptr();
        // the positions with stored bounds: the leading wl_count[kStoredPrefixWord] of the kernel's list (bounds_pass.inc)
        const u32 bcap = *(c32) (*(c64) (ka + offsetof(ExactKernArgs, wl_count)) + 4u * kStoredPrefixWord);
        const u32 posA = rfl(sb.posA), posB = rfl(sb.posB);  // (wave-uniform, see rfl_i)
        stored = posA < bcap && posB < bcap;  // both reads of the pass have stored bounds
        if (stored && (lane < 32u || haveB)) {
            const u32 *const base = (const u32 *) *(c64) (ka + offsetof(ExactKernArgs, bnd));
            const u32 *src = base + ((u64) (lane < 32u ? posA : posB) * 2u + ((lane >> 4) & 1u)) * kBoundWords + (lane & 15u);
            st0 = src[0];
            st1 = src[16];
        }
    }
    TREW_MARK(stage);
    PH_T0(t_stage);
    stage_two(sm, rdA, rdB, haveB);
    PH_ADD(PH_STAGE, t_stage);
#if defined(TREW_AB_SKIP) && TREW_AB_SKIP >= 4  // 4 = + staging
    return;
#endif
    TREW_MARK(group_setup);
    const u32 g = lane >> 4, j = lane & 15u;
    const bool second = g >= 2u;
    const u32 is_right = g & 1u;
    ReadRef rd;
    rd.w = second ? rdB.w : rdA.w;
    rd.len = second ? rdB.len : rdA.len;
    rd.nw = second ? rdB.nw : rdA.nw;
    const Segment sg = get_segment(TREW_MODE_SHORT, (int) is_right, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
    const bool rowvalid = sg.valid && (!second || haveB);
    TREW_MARK(bounds);
    PH_T0(t_bounds);
    RowSeg<NW> rs;
    u32 bnd0, bnd1;
    if (stored) {  // wave-uniform
        // what decide_group reads of the segment besides its bounds: the planes, the valid bases (eval_row, segments with an N) and has_n
        u32 nm[NW];
        ReadRef r = rd;
        if (!rowvalid) r.nw = 0;
        load_planes_lds<NW>(r, sg.start, rs.lo, rs.hi, nm);
        u32 anyn = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            rs.v1[w] = ~nm[w] & low_mask((int) sg.len - 32 * w);
            rs.P1[w] = rs.P2[w] = rs.P3[w] = 0;
            anyn |= ~rs.v1[w] & low_mask((int) sg.len - 32 * w);
        }
        rs.has_n = anyn != 0u ? 1u : 0u;
        bnd0 = rowvalid ? st0 : 0u;
        bnd1 = rowvalid ? st1 : 0u;
    } else {
        lds_sync();
        row_prepare<NW>(sm, rd, sg, rowvalid);
        lds_sync();
        row_load<NW>(sm, (int) sg.len, rs);
        if (P.min_mer + 15 < 32)  // wave-uniform
            bnd0 = rowvalid ? bound_at_k<NW, true>(rs, (int) sg.len, P.min_mer + (int) j, P.max_mer, P) : 0u;
        else
            bnd0 = rowvalid ? bound_at_k<NW, false>(rs, (int) sg.len, P.min_mer + (int) j, P.max_mer, P) : 0u;
        bnd1 = rowvalid ? bound_at_k<NW>(rs, (int) sg.len, P.min_mer + 16 + (int) j, P.max_mer, P) : 0u;
    }
#if defined(TREW_AB_SKIP) && TREW_AB_SKIP >= 3  // 3 = + bounds (kept alive: results nobody reads are not computed)
    asm volatile("" ::"v"(bnd0), "v"(bnd1));
    return;
#endif
    PH_ADD(PH_BOUNDS, t_bounds);
    TREW_MARK(group);
    const GroupOut<WT> o = decide_group<NW, WT, false>(sm, P, rs, bnd0, bnd1, second ? 1u : 0u, sg, rowvalid);
#if defined(TREW_AB_SKIP) && TREW_AB_SKIP >= 2  // 2 = + the group pass; 1 = everything but table adds (run with TREW_FLAG_DEBUG_NO_EMIT)
    asm volatile("" ::"v"(o.kk), "v"(o.saved), "v"(o.kept_cnt), "v"((u32) o.kept_canon), "v"((u32) (o.kept_canon >> 32)), "v"((u32) o.punt));
    return;
#endif
    TREW_MARK(routing);
    PH_T0(t_route);
    // ---- routing, kmer.cpp:119-163, per row: my verdict and my partner's (the other half of my read) ----
    const u32 mine = rowvalid ? (o.kk | (o.punt ? 1u << 16 : 0u)) : 0u;
    const u32 other = lane_gather(mine, lane ^ 16u);
    const u32 kkL = is_right ? other : mine, kkR = is_right ? mine : other;
    const u32 lkh = kkL & 255u, lkl = (kkL >> 8) & 255u, rkh = kkR & 255u, rkl = (kkR >> 8) & 255u;
    const u32 left_found = (lkh | lkl) != 0u ? 1u : 0u;
    const u32 tgt_h = left_found & (lkh == rkh ? 1u : 0u) & (lkh != 0u ? 1u : 0u);  // kmer.cpp:128
    const u32 tgt_l = left_found & (lkl == rkl ? 1u : 0u) & (lkl != 0u ? 1u : 0u);  // kmer.cpp:141
    const u32 myk = o.saved & 255u, items = (o.saved >> 8) & 255u;
    u32 need_old = ((kkL | kkR) >> 16) & 1u;  // a half was given back
    u32 rec_mask = 0;
    {
        // left half: temp_result_left.b -> forward.b unless the halves agree (kmer.cpp:132-134, 145-147);
        // right half: recorded only where the left half found nothing for that baseline (kmer.cpp:125, 157-158)
        const u32 kh = is_right ? rkh : lkh, kl = is_right ? rkl : lkl;
        const u32 rec_h = (kh != 0u ? 1u : 0u) & (is_right ? ((left_found ^ 1u) | (lkh == 0u ? 1u : 0u)) : (tgt_h ^ 1u));
        const u32 rec_l = (kl != 0u ? 1u : 0u) & (is_right ? ((left_found ^ 1u) | (lkl == 0u ? 1u : 0u)) : (tgt_l ^ 1u));
        const u32 th = is_right ? (1u << TREW_TABLE_BACKWARD_HIGH) : (1u << TREW_TABLE_FORWARD_HIGH);
        const u32 tl = is_right ? (1u << TREW_TABLE_BACKWARD_LOW) : (1u << TREW_TABLE_FORWARD_LOW);
        rec_mask = ((rec_h & (kh == myk ? 1u : 0u)) ? th : 0u) | ((rec_l & (kl == myk ? 1u : 0u)) ? tl : 0u);
        need_old |= (rec_h & (kh != myk ? 1u : 0u)) | (rec_l & (kl != myk ? 1u : 0u));  // a record at a k whose table the row did not keep
    }
    need_old |= tgt_h & tgt_l & (lkh != lkl ? 1u : 0u);  // two whole-read counts at different k
    {  // the whole-read check of reads shorter than 4 MAX_MER (kmer.cpp:165-171)
        const u32 hh = (lkh == 0u && rkh == 0u) ? 1u : 0u, lh = (lkl == 0u && rkl == 0u) ? 1u : 0u;
        const Segment sW = get_segment(TREW_MODE_SHORT, 2, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
        need_old |= (sW.valid ? 1u : 0u) & (hh | lh);
    }
    need_old |= lane_gather(need_old, lane ^ 16u);  // per read
    need_old &= rowvalid ? 1u : 0u;
    const DevTable Tv = load_table(T);
    TREW_MARK(records);
    // ---- records straight from the rows' class tables (rotation-canonical keys, kmer.cpp:2264-2313) ----
    if (need_old == 0u && rec_mask != 0u && j < items && o.kept_cnt != 0u) {
        for (u32 tm = rec_mask; tm; tm &= tm - 1u) cached_add(sm, Tv, __ffs((int) tm) - 1, (int) myk, o.kept_canon, o.kept_cnt);
    }
    PH_ADD(PH_EMIT, t_route);
    TREW_MARK(target);
    PH_T0(t_target);
    // ---- k_mer_target of reads whose halves agree (kmer.cpp:1894-2017: a class count of the whole read at that k) ----
    u32 want_t = (need_old ^ 1u) & (tgt_h | tgt_l) & (rowvalid ? 1u : 0u);
    // The windows of the read are those of its left half, those of its right half and the k - 1 that span the middle, and both
    // halves' class tables at that k are still in their rows' registers.  The whole read's table is their sum (counts add up in the
    // count table, so nothing has to be merged before it is added) -- what is needed first is its MAX and MAX_SEQ.  When both halves
    // have the same largest class x and it leads by more than the spanning windows could close (any other class has at most the
    // windows of the two halves that are not in x, plus k - 1), x is the whole read's unique largest class and MAX = the halves' counts of x + the
    // spanning windows in x.  One canonical rotation for each spanning window (the 32 lanes of the read take one each) replaces the
    // class count of 145 windows.  Anything else -- a table kept at another k, different or tied leaders -- is counted as before.
    {
        const int tk = (int) (tgt_h ? lkh : lkl);
        const u32 rowbase = lane & 48u;
        const u32 cnt = (j < items) ? o.kept_cnt : 0u;
        const u32 c1 = row_max<16>(cnt);
        const u32 topb = (u32) (__ballot(cnt != 0u && cnt == c1) >> rowbase) & 0xffffu;
        const u32 tl = topb ? (u32) __builtin_ctz(topb) : 0u;
        const u32 c2 = (o.saved >> 16) - c1;  // what any other class of the half can hold at most (the table may list a class in several lanes, eval_row)
        const WT xkey = lane_gather(o.kept_canon, rowbase + tl);
        const u32 okrow = want_t & (myk == (u32) tk ? 1u : 0u) & (c1 != 0u ? 1u : 0u) & (o.punt ? 0u : 1u);
        const u32 pc1 = lane_gather(c1, lane ^ 16u), pc2 = lane_gather(c2, lane ^ 16u), pok = lane_gather(okrow, lane ^ 16u);
        const u32 pcount = lane_gather(o.saved >> 16, lane ^ 16u);
        const WT pkey = lane_gather(xkey, lane ^ 16u);
        const u32 fast = okrow & pok & (xkey == pkey ? 1u : 0u) & (c1 + pc1 > c2 + pc2 + (u32) (tk - 1) ? 1u : 0u);
        if (__any(fast != 0u)) {
            TREW_MARK(target_rows);
            const u32 q = lane & 31u, r = second ? 1u : 0u, segwords = exact_rangewords(sm.cap);
            const int i = (int) (rd.len >> 1) - tk + 1 + (int) q;  // spanning window q of the read: starts in the left half, ends in the right
            u32 sv = 0;
            WT cs = 0;
            if (fast != 0u && q + 1u < (u32) tk) {
                const u32 *nmk = sm_nmask(sm) + r * segwords;
                const u32 wi = (u32) i >> 5;
                const u32 nb = alignbit(wi + 1u < segwords ? nmk[wi + 1u] : 0xffffffffu, nmk[wi], (u32) i & 31u);  // N flags of bases i .. i + 31
                if ((nb & low_mask<true>(tk)) == 0u) {
                    sv = 1u;
                    cs = min_rotation<WT>(window_word_at(sm, range_base(sm, r) + (u32) i, tk), tk);
                }
            }
            const u32 halfbase = lane & 32u;
            const u32 nspan = (u32) __popc((u32) (__ballot(sv != 0u) >> halfbase));
            const u32 sx = (u32) __popc((u32) (__ballot(sv != 0u && cs == xkey) >> halfbase));
            const u32 maxc = c1 + pc1 + sx, count = (o.saved >> 16) + pcount + nspan;
            const double f = is_homopolymer<WT>(xkey, tk) ? 0.0 : (double) maxc / (double) count;  // kmer.cpp:1972-1976
            const u32 tm = fast ? (((tgt_h && f >= P.high) ? 1u << TREW_TABLE_BOTH_HIGH : 0u) | ((tgt_l && f >= P.low) ? 1u << TREW_TABLE_BOTH_LOW : 0u)) : 0u;
            // the leading class is added once, by the left row's lane that holds it, with the whole read's count; every other class
            // of the two tables and every spanning window outside the leading class adds itself
            const bool lead = is_right == 0u && j == tl;
            const u32 add = (cnt != 0u && o.kept_canon == xkey) ? (lead ? maxc : 0u) : cnt;
            if (tm != 0u && add != 0u) {  // strand-canonical keys (kmer.cpp:1979-1988)
                const WT w = strand_canon<WT>(o.kept_canon, tk);
                for (u32 t2 = tm; t2; t2 &= t2 - 1u) cached_add(sm, Tv, __ffs((int) t2) - 1, tk, w, add);
            }
            if (tm != 0u && sv != 0u && cs != xkey) {
                const WT w = strand_canon<WT>(cs, tk);
                for (u32 t2 = tm; t2; t2 &= t2 - 1u) cached_add(sm, Tv, __ffs((int) t2) - 1, tk, w, 1u);
            }
        }
        want_t &= fast ^ 1u;
    }
    u32 tgt_old = 0;
    if (__any(want_t != 0u)) {
        constexpr int NWW = 2 * NW;
        const u32 ev = want_t & (is_right ^ 1u);
        const int tk = (int) (tgt_h ? lkh : lkl);
        u32 wlo[NWW], whi[NWW], wv1[NWW], w_n = 0;
        {
            u32 nm[NWW];
            ReadRef r = rd;
            if (!ev) r.nw = 0;
            load_planes_lds<NWW>(r, 0, wlo, whi, nm);
#pragma unroll
            for (int w = 0; w < NWW; w++) {
                const u32 lm = low_mask((int) rd.len - 32 * w);
                wv1[w] = ~nm[w] & lm;
                w_n |= nm[w] & lm;
            }
        }
        const int W = ev ? (int) rd.len - tk + 1 : 1;
        TREW_MARK(target_eval);
        const RowCount<WT> rc = eval_row<NWW, WT, false>(sm, wlo, whi, wv1, w_n != 0u ? 1u : 0u, range_base(sm, second ? 1u : 0u), ev ? tk : P.min_mer, W, ev);
        TREW_MARK(target_emit);
        tgt_old = rc.over;  // more runs than a row has lanes: target() counts it with a wave
        const u32 okc = ev & (rc.over ^ 1u);
        const double f = rc.homo ? 0.0 : (double) rc.maxc / (double) rc.count;  // kmer.cpp:1972-1976 (COUNT == 0: nothing passes, and no class exists)
        const u32 tm = ((tgt_h && f >= P.high) ? 1u << TREW_TABLE_BOTH_HIGH : 0u) | ((tgt_l && f >= P.low) ? 1u << TREW_TABLE_BOTH_LOW : 0u);
        if (okc != 0u && tm != 0u && rc.cnt != 0u) {
            const WT w = strand_canon<WT>(rc.canon, tk);
            for (u32 t2 = tm; t2; t2 &= t2 - 1u) cached_add(sm, Tv, __ffs((int) t2) - 1, tk, w, rc.cnt);
        }
    }
    PH_ADD(PH_RECORD_EVAL, t_target);
    TREW_MARK(fallback);
    // ---- reads that need the wave-per-segment code ----
    const u64 ob = __ballot(need_old != 0u), tb = __ballot(tgt_old != 0u);
    if ((ob | tb) == 0ull) return;
    // hand over: the class table of row g goes to save slot g (what save_classes would have kept), the verdict to gres[g]
    __syncthreads();
    if (!o.punt && j < items) {
        sm_save_canon<WT>(sm)[g * kSaveItems + j] = o.kept_canon;
        sm_save_cnt<WT>(sm)[g * kSaveItems + j] = (unsigned short) o.kept_cnt;
    }
    if (j == 0u) put_decision<WT>(sm, g, o.kk | (o.punt ? 1u << 16 : 0u), o.saved, o.sh, o.sl);
    const u64 pb = __ballot(o.punt && rowvalid);  // rows that gave their segment back
    const u64 thb = __ballot(tgt_h != 0u), tlb = __ballot(tgt_l != 0u);
    const u32 tkA = (u32) __builtin_amdgcn_readlane((int) (tgt_h ? lkh : lkl), 0), tkB = (u32) __builtin_amdgcn_readlane((int) (tgt_h ? lkh : lkl), 32);
    __syncthreads();
    for (u32 r = 0; r < (haveB ? 2u : 1u); r++) {
        const ReadRef &rr = r ? rdB : rdA;
        if ((ob >> (32u * r)) & 1ull) {
            const u32 punted = ((pb >> (32u * r)) & 1ull ? 1u : 0u) | ((pb >> (32u * r + 16u)) & 1ull ? 2u : 0u);
            if (punted) {  // the halves the rows gave back, a wave each
                count_fallback(kFallbackGroupPunt);
                decide_halves<NW, WT>(sm, P, rr, r, 2u * r, punted);
            }
            count_fallback(kFallbackGroupRouted);
            run_short_routed<NW, WT>(sm, P, T, rr, r, 2u * r, true);
            __syncthreads();
        } else if ((tb >> (32u * r)) & 1ull) {
            count_fallback(kFallbackGroupTarget);
            target<WT>(view_segment(sm, r, 0, rr), P, T, (int) rr.len, (int) (r ? tkB : tkA), ((thb >> (32u * r)) & 1ull) != 0ull, ((tlb >> (32u * r)) & 1ull) != 0ull);
            __syncthreads();
        }
    }
}
