// kernels/prefilter.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// filter_kernel<NW>: one lane per read, bit-parallel parity-bucket bound for every (segment, k); general path, uniform-geometry fast path
// and the two drains of what the fast path sets aside (whole units, single halves).  The fast path and its drains derive no
// geometry: they read the block the host filled for the batch's read length (FilterGeom, trew_common.hpp).

// ------------------------------------------------------------------ prefilter

// '; MARK name' comments in the ISA around the joint branch's set-up (tools/isa_regions.py), with -DTREW_MARK_READ_SETUP only
#ifdef TREW_MARK_READ_SETUP
#define TREW_SETUP_MARK(n) asm volatile("; MARK " #n)
#else
#define TREW_SETUP_MARK(n)
#endif

// (x ^ y) & m as ONE instruction (v_bitop3_b32, truth table 0x28 = (0xF0 ^ 0xCC) & 0xAA)
__device__ __forceinline__ u32 xor_and(u32 x, u32 y, u32 m) { return __builtin_amdgcn_bitop3_b32(x, y, m, 0x28); }

__device__ __forceinline__ u64 all_k_mask(int kmin, int kmax) {
    if (kmax < kmin) return 0;
    u64 hi = kmax >= 64 ? ~0ull : ((1ull << kmax) - 1ull);
    u64 lo = (1ull << (kmin - 1)) - 1ull;
    return hi & ~lo;
}

// word j of (x >> k), k = 32*WS + bs, zero-extended above word NW-1
template <int NW, int WS>
__device__ __forceinline__ u32 shr_word(const u32 (&x)[NW], int j, u32 bs) {
    const u32 lo = (j + WS < NW) ? x[j + WS < NW ? j + WS : 0] : 0u;
    const u32 hi = (j + WS + 1 < NW) ? x[j + WS + 1 < NW ? j + WS + 1 : 0] : 0u;
    return alignbit(hi, lo, bs);
}

// One k of the prefilter.  V holds V_k (windows with no N) on entry and V_{k+1} on exit.
// NWW = number of mask words that can still hold a window at this k (compile-time, so the
// per-word work has no scalar branches).
// Stage 1 uses two parities (4 buckets); the third parity (8 buckets) is evaluated only
// when some lane of the wave would otherwise get its FIRST candidate from the 4-bucket
// bound.  Lanes that already own a candidate keep the looser -- still sound -- verdict:
// the exact kernel prunes their extra candidates itself (lane_bounds).  The result of
// a lane never depends on its neighbours: 8-bucket max <= 4-bucket max.
// Measured on MI355X (tools/valu_rate.hip): v_alignbit / v_bcnt occupy a SIMD for ~4.2 cycles
// per wave-instruction, simple logic / add / v_bitop3 for ~2.3-2.7; the slow ones are what is
// minimised here (e.g. bucket 00 is COUNT minus the other three instead of a fourth popcount).
template <int NW, int WS, int NWW>
__device__ __forceinline__ void filter_k(const u32 (&P1)[NW], const u32 (&P2)[NW], const u32 (&P3)[NW],
                                         const u32 (&v1)[NW], u32 (&V)[NW], int k, float lowf, u32 &cand_lo, u32 &cand_hi) {
    const u32 bs = (u32) k & 31u;
    u32 c01 = 0, c10 = 0, c11 = 0, count = 0;
#pragma unroll
    for (int j = 0; j < NWW; j++) {
        const u32 F1 = P1[j] ^ shr_word<NW, WS>(P1, j, bs), F2 = P2[j] ^ shr_word<NW, WS>(P2, j, bs);
        const u32 v = V[j];
        const u32 a1 = v & F1;
        const u32 a11 = a1 & F2;
        count += __popc(v);
        c11 += __popc(a11);
        c10 += __popc(a1 ^ a11);
        c01 += __popc((v ^ a1) & F2);
    }
    const u32 c00 = count - c01 - c10 - c11;
    const u32 m4 = max(max(c00, c01), max(c10, c11));
    // MAX <= m4; MAX/COUNT >= LOW needs m4 >= LOW*COUNT > lowf*COUNT (lowf < LOW*(1-1e-6), COUNT > 0);
    // the strict '>' also rejects COUNT == 0 (m4 == 0)
    const float thr = (float) count * lowf;
    const bool pass4 = (float) m4 > thr;
    bool pass = pass4;
    const bool first = (cand_lo | cand_hi) == 0;
#ifdef TREW_AB_SKIP_DRAIN8  // A/B builds (instruction attribution, profiles/r05): the 8-bucket block left out
    if (false) {
#else
    if (__any(pass4 && first)) {
#endif
        Buckets8<false, true> b8;
#pragma unroll
        for (int j = 0; j < NWW; j++) {
            const u32 F1 = P1[j] ^ shr_word<NW, WS>(P1, j, bs), F2 = P2[j] ^ shr_word<NW, WS>(P2, j, bs);
            const u32 F3 = P3[j] ^ shr_word<NW, WS>(P3, j, bs);
            b8.add(F1, F2, F3, V[j]);
        }
        const u32 m8 = b8.largest(count);
        pass = first ? ((float) m8 > thr) : pass4;
    }
    if (k <= 32)
        cand_lo |= pass ? (1u << ((k - 1) & 31)) : 0u;
    else
        cand_hi |= pass ? (1u << ((k - 33) & 31)) : 0u;
    // V_{k+1} = V_k & (v1 >> k)
#pragma unroll
    for (int j = 0; j < NWW; j++) V[j] &= shr_word<NW, WS>(v1, j, bs);
}

// k range [klo, khi] split by the number of window words: windows i <= max_seg - k need
// ceil((max_seg - k + 1) / 32) words.  Recursion over NWW keeps every trip count static.
template <int NW, int WS, int NWW>
struct FilterRange {
    static __device__ __forceinline__ void run(const u32 (&P1)[NW], const u32 (&P2)[NW], const u32 (&P3)[NW], const u32 (&v1)[NW],
                                               u32 (&V)[NW], int klo, int khi, int max_seg, float lowf, u32 &clo, u32 &chi) {
        // k values whose windows need exactly NWW words (or more than NW: clamp) : max_seg+1-32*NWW < k <= max_seg+1-32*(NWW-1)
        int a = max_seg + 2 - 32 * NWW, b = max_seg + 1 - 32 * (NWW - 1);
        if (NWW == NW) a = klo;  // segments are never longer than the instantiation allows
        a = a < klo ? klo : a;
        b = b > khi ? khi : b;
        for (int k = a; k <= b; k++) filter_k<NW, WS, NWW>(P1, P2, P3, v1, V, k, lowf, clo, chi);
        FilterRange<NW, WS, NWW - 1>::run(P1, P2, P3, v1, V, klo, khi, max_seg, lowf, clo, chi);
    }
};
template <int NW, int WS>
struct FilterRange<NW, WS, 0> {
    static __device__ __forceinline__ void run(const u32 (&)[NW], const u32 (&)[NW], const u32 (&)[NW], const u32 (&)[NW], u32 (&)[NW],
                                               int, int, int, float, u32 &, u32 &) {}
};

// Candidate-k mask of one segment (bit k-1).  lo/hi/nm hold the segment's
// planes from bit 0; L <= 32*NW-1 bases.  gmin..gmax is the wave-uniform k
// loop (MIN_MER..MAX_MER); only k in [kmin,kmax] can become candidates.
// max_seg (wave-uniform) bounds L over the whole batch.
//
// Soundness: windows of one rotation class (kmer.cpp:1815-1823) have the same
// base composition, hence the same (#lo-bit, #hi-bit, #A) parities.  With
// P_b the exclusive prefix parity of feature b, the parity of window i is
// P_b[i] ^ P_b[i+k]; so the size of every parity bucket is one popcount and the
// largest bucket is an upper bound of K_MER_DATA_MAX (kmer.cpp:2202).
template <int NW>
__device__ __forceinline__ u64 filter_segment(const u32 (&lo)[NW], const u32 (&hi)[NW], const u32 (&nm)[NW], int L,
                                              int kmin, int kmax, int gmin, int gmax, int max_seg, float lowf) {
    u32 v1[NW], P1[NW], P2[NW], P3[NW], V[NW];
    {
        // segment_setup<NW, true> (bound.inc) written out, with V = v1 in the same loop: calling it here changes the register
        // allocation of filter_kernel<32> (profiles/bound_refactor/README.md)
        u32 f1[NW], f2[NW], f3[NW];
#pragma unroll
        for (int j = 0; j < NW; j++) {
            int bits = L - 32 * j;
            u32 lm = low_mask(bits);
            v1[j] = ~nm[j] & lm;  // base is A/C/G/T and inside the segment
            f1[j] = lo[j] & v1[j];
            f2[j] = hi[j] & v1[j];
            f3[j] = f1[j] & f2[j];
            V[j] = v1[j];
        }
        prefix_parity<NW>(f1, P1);
        prefix_parity<NW>(f2, P2);
        prefix_parity<NW>(f3, P3);
    }
    // V = V_gmin: windows of length gmin with no N (kmer.cpp:2190)
    for (int t = 1; t < gmin && t < 32; t++) {
#pragma unroll
        for (int j = 0; j < NW; j++) V[j] &= shr_word<NW, 0>(v1, j, (u32) t);
    }
    for (int t = 32; t < gmin && t < 64; t++) {
#pragma unroll
        for (int j = 0; j < NW; j++) V[j] &= shr_word<NW, 1>(v1, j, (u32) t & 31u);
    }
    u32 clo = 0, chi = 0;
    const int g31 = gmax < 31 ? gmax : 31;
    if (NW <= 5) {
        FilterRange<NW, 0, NW>::run(P1, P2, P3, v1, V, gmin, g31, max_seg, lowf, clo, chi);
        FilterRange<NW, 1, NW>::run(P1, P2, P3, v1, V, gmin > 32 ? gmin : 32, gmax < 63 ? gmax : 63, max_seg, lowf, clo, chi);
        FilterRange<NW, 2, NW>::run(P1, P2, P3, v1, V, gmin > 64 ? gmin : 64, gmax, max_seg, lowf, clo, chi);
    } else {
        // long segments: all words every k (static trip counts would multiply the code size)
        for (int k = gmin; k <= g31; k++) filter_k<NW, 0, NW>(P1, P2, P3, v1, V, k, lowf, clo, chi);
        for (int k = gmin > 32 ? gmin : 32; k <= (gmax < 63 ? gmax : 63); k++) filter_k<NW, 1, NW>(P1, P2, P3, v1, V, k, lowf, clo, chi);
        for (int k = gmin > 64 ? gmin : 64; k <= gmax; k++) filter_k<NW, 2, NW>(P1, P2, P3, v1, V, k, lowf, clo, chi);
    }
    // only k inside the segment's own range can be candidates
    return ((((u64) chi) << 32) | clo) & all_k_mask(kmin, kmax);
}


// ------------------------------------------------------------------ prefilter, uniform-geometry fast path
// Batches of equal-length reads (trew_hip_batch.uniform_length, the usual Illumina case) have the same
// segment geometry for every unit, so everything that depends only on (segment length, k) is wave-uniform:
// COUNT = L-k+1, the window mask of the last word and the pass threshold live in SGPRs / an LDS table
// instead of being recomputed per lane.  Reads with an N inside a segment do not fit that model (their
// COUNT differs); they are set aside in LDS and go through the general filter_segment, 256 at a time.
// Per k and word this leaves 2 alignbit + 2 xor + 1 and + 3 bcnt -- the kernel is VALU-issue bound
// (every wave64 VALU instruction occupies its SIMD16 for 4 cycles), so instruction count is time.
// The verdicts of the 64 lanes are kept as wave masks in SGPRs (hasm: lanes that already own a
// candidate, the return value: lanes passing at this k), so the bookkeeping per k is scalar work.
// thr_row[k-1] = {ithr, jthr} (kThrRow entries per slot, computed by fill_thresholds): (float) m > (float) COUNT * lowf  <=>  m >= ithr = floor((float) COUNT * lowf) + 1,
// and bucket 00 = COUNT - t reaches ithr  <=>  t <= jthr = COUNT - ithr.
// SUBSET (3-word kernels, 64 < COUNT <= 72): only the first 64 windows are looked at, NWW = 2 full words.  Sound: a class with
// MAX members among all COUNT windows has at least MAX - (COUNT - 64) among the first 64, so the pass threshold drops by the
// windows left out (uni_windows / fill_thresholds bake that into th) -- a third mask word for 1..8 windows would cost a third
// more instructions per k.
template <int NW, int WS, int NWW, bool SUBSET = false>
__device__ __forceinline__ u64 filter_k_uni(const u32 (&P1)[NW], const u32 (&P2)[NW], const u32 (&P3)[NW], int L, int k,
                                            const int2 th, u64 hasm) {
    const u32 bs = (u32) k & 31u;
    const int W = SUBSET ? 32 * NWW : L - k + 1;  // COUNT (or the windows looked at), wave-uniform
    const int lastbits = W - 32 * (NWW - 1);  // windows in word NWW-1: [0, 32) by construction of FilterRangeUni
    const u32 wm = SUBSET ? 0xffffffffu : (1u << (lastbits & 31)) - 1u;
    u32 F1[NWW], F2[NWW];
    u32 c1x = 0, cx1 = 0, c11 = 0;
#pragma unroll
    for (int j = 0; j < NWW; j++) {
        F1[j] = P1[j] ^ shr_word<NW, WS>(P1, j, bs);
        F2[j] = P2[j] ^ shr_word<NW, WS>(P2, j, bs);
        if (j == NWW - 1 && !SUBSET) {
            F1[j] &= wm;
            F2[j] &= wm;
            // keep the masked words as values: otherwise the compiler re-derives them inside every
            // 3-input bit op below and spends two extra xors per k
            asm volatile("" : "+v"(F1[j]), "+v"(F2[j]));
        }
        // v_bcnt_u32_b32 adds its second operand: chaining the words' popcounts costs no separate add (left to itself
        // the compiler counts three words independently and spends a v_add3 per bucket)
        c1x = bcnt_acc(F1[j], c1x);
        cx1 = bcnt_acc(F2[j], cx1);
        c11 = bcnt_acc(F1[j] & F2[j], c11);
    }
    const u32 c10 = c1x - c11, c01 = cx1 - c11;
    const u32 m3 = max(max(c10, c01), c11);
    const int t = (int) (c1x + c01);  // COUNT - c00
    const u64 p4 = __ballot(m3 >= (u32) th.x) | __ballot(t <= th.y);  // two compares straight into SGPR masks
    u64 pm = p4;
    if (p4 & ~hasm) {  // third parity, as in filter_k: only for a lane's first candidate
        u32 F3[NWW], Vw[NWW];
#pragma unroll
        for (int j = 0; j < NWW; j++) {
            F3[j] = P3[j] ^ shr_word<NW, WS>(P3, j, bs);
            Vw[j] = j == NWW - 1 ? wm : 0xffffffffu;
        }
        const u32 m8 = max_bucket8<NWW>(F1, F2, F3, Vw, (u32) W);
        const u64 p8 = __ballot(m8 >= (u32) th.x);
        pm = (p4 & hasm) | (p8 & ~hasm);
    }
    return pm;
}

// 64-bit container of a 3-word mask: bits [s, s + 64), s in [0, 32] (wave-uniform)
__device__ __forceinline__ u64 container64(const u32 (&P)[3], int s) {
    const bool big = s >= 32;
    const u32 lo = alignbit(big ? P[2] : P[1], big ? P[1] : P[0], (u32) s & 31u);
    const u32 hi = alignbit(big ? 0u : P[2], big ? P[2] : P[1], (u32) s & 31u);
    return ((u64) hi << 32) | lo;
}

// 32 <= COUNT <= 64 in a 3-word kernel: the two words of P >> k come from ONE 64-bit shift of the container
// Q = P[s .. s+64), s = max(0, L - 63):  (P >> k)[0 .. 64) = Q >> (k - s) for every k >= s, because prefix positions past L
// belong to no window of this k.  v_lshrrev_b64 occupies the SIMD for less time than one v_alignbit_b32 and replaces two
// (tools/valu_rate.hip: 1.96 against 2 x 2.62 cycles per wave at 8 waves per SIMD).
__device__ __forceinline__ u64 filter_k_uni_q(const u32 (&P1)[3], const u32 (&P2)[3], const u32 (&P3)[3], u64 Q1, u64 Q2, int s, int L, int k,
                                              const int2 th, u64 hasm) {
    const int W = L - k + 1;  // COUNT: 32..64
    const u32 sh = (u32) (k - s);
    const u64 S1 = Q1 >> sh, S2 = Q2 >> sh;
    const u32 wm = W >= 64 ? 0xffffffffu : ((1u << ((W - 32) & 31)) - 1u);  // scalar: windows 32 .. COUNT-1
    const u32 F1a = P1[0] ^ (u32) S1, F2a = P2[0] ^ (u32) S2;
    const u32 F1b = xor_and(P1[1], (u32) (S1 >> 32), wm), F2b = xor_and(P2[1], (u32) (S2 >> 32), wm);  // one v_bitop3_b32 each
    u32 c1x = 0, cx1 = 0, c11 = 0;
    c1x = bcnt_acc(F1a, c1x);
    cx1 = bcnt_acc(F2a, cx1);
    c11 = bcnt_acc(F1a & F2a, c11);
    c1x = bcnt_acc(F1b, c1x);
    cx1 = bcnt_acc(F2b, cx1);
    c11 = bcnt_acc(F1b & F2b, c11);
    const u32 c10 = c1x - c11, c01 = cx1 - c11;
    const u32 m3 = max(max(c10, c01), c11);
    const int t = (int) (c1x + c01);  // COUNT - c00
    const u64 p4 = __ballot(m3 >= (u32) th.x) | __ballot(t <= th.y);
    u64 pm = p4;
    if (p4 & ~hasm) {  // third parity, only for a lane's first candidate (rare: its shifted words are rebuilt here)
        const u64 S3 = container64(P3, s) >> sh;
        const u32 F1[2] = {F1a, F1b}, F2[2] = {F2a, F2b}, F3[2] = {P3[0] ^ (u32) S3, P3[1] ^ (u32) (S3 >> 32)}, Vw[2] = {0xffffffffu, wm};
        const u32 m8 = max_bucket8<2>(F1, F2, F3, Vw, (u32) W);
        const u64 p8 = __ballot(m8 >= (u32) th.x);
        pm = (p4 & hasm) | (p8 & ~hasm);
    }
    return pm;
}

// what one segment's k loop accumulates
struct UniVerdict {
    u64 hasm;   // wave mask: lanes with a candidate at any k of the loop so far
    u64 flagm;  // wave mask: lanes with a candidate inside the segment's own [kmin, kmax]
    u32 clo, chi;  // this lane's candidate mask (only maintained when `dbg`)
};

// the verdict mask pm of one k goes into the segment's.  slow: see FilterRangeUni
__device__ __forceinline__ void uni_note(UniVerdict &vd, u64 pm, int k, bool slow, int kmin, int kmax, bool dbg) {
    vd.hasm |= pm;
    if (slow) {
        if (k >= kmin && k <= kmax) vd.flagm |= pm;
        if (dbg) {  // wave-uniform
            const bool mine = (pm >> lane_id()) & 1ull;
            if (k <= 32)
                vd.clo |= mine ? (1u << ((k - 1) & 31)) : 0u;
            else
                vd.chi |= mine ? (1u << ((k - 33) & 31)) : 0u;
        }
    }
}

// as FilterRange, with the word count taken from the segment's own (uniform) length.
// SLOW: some k of the loop lie outside the segment's [kmin, kmax], or the per-lane masks are wanted
// (trew_hip_filter_masks); otherwise flagm is simply hasm after the loop and the per-k bookkeeping
// is one scalar OR.  The thresholds of the next k are fetched from LDS one iteration ahead.
template <int NW, int WS, int NWW, bool SLOW>
struct FilterRangeUni {
    static __device__ __forceinline__ void run(const u32 (&P1)[NW], const u32 (&P2)[NW], const u32 (&P3)[NW], int klo, int khi, int L,
                                               int kmin, int kmax, const int2 *__restrict__ thr_row, bool dbg, UniVerdict &vd) {
        int a = L + 2 - 32 * NWW, b = L + 1 - 32 * (NWW - 1);
        if (NWW == NW) a = klo;
        a = a < klo ? klo : a;
        b = b > khi ? khi : b;
        if (a <= b) {
            int2 th_next = thr_row[a - 1];
            for (int k = a; k <= b; k++) {
                const int2 th = th_next;
                th_next = thr_row[k];  // entry 64 exists (padding)
                uni_note(vd, filter_k_uni<NW, WS, NWW>(P1, P2, P3, L, k, th, vd.hasm), k, SLOW, kmin, kmax, dbg);
            }
        }
        FilterRangeUni<NW, WS, NWW - 1, SLOW>::run(P1, P2, P3, klo, khi, L, kmin, kmax, thr_row, dbg, vd);
    }
};
template <int NW, int WS, bool SLOW>
struct FilterRangeUni<NW, WS, 0, SLOW> {
    static __device__ __forceinline__ void run(const u32 (&)[NW], const u32 (&)[NW], const u32 (&)[NW], int, int, int, int, int, const int2 *,
                                               bool, UniVerdict &) {}
};

// N-free segment of wave-uniform length L (same verdicts as filter_segment): vd.flagm = lanes with a
// candidate k, vd.clo/chi = the lane's candidate mask when dbg
template <int NW>
__device__ __forceinline__ void filter_segment_uni(const u32 (&lo)[NW], const u32 (&hi)[NW], int L, int kmin, int kmax, int gmin, int gmax,
                                                   const int2 *__restrict__ thr_row, bool dbg, UniVerdict &vd) {
    u32 P1[NW], P2[NW], P3[NW], none[NW];
    segment_setup<NW, false>(lo, hi, /* N plane: not read */ lo, L, /* v1: not written */ none, P1, P2, P3);
    vd.hasm = vd.flagm = 0;
    vd.clo = vd.chi = 0;
    const int g31 = gmax < 31 ? gmax : 31;
    const bool slow = dbg || kmin > gmin || kmax < gmax;  // wave-uniform
    if constexpr (NW == 3) {
        // The 3-word kernel (segments of up to 95 bases: the halves of 150-bp reads) splits the k range by COUNT = L-k+1:
        //   COUNT >= 73         three mask words, funnel shifts                  (FilterRangeUni, NWW = 3)
        //   65 <= COUNT <= 72   the first 64 windows only, two full words        (filter_k_uni<.., SUBSET>)
        //   32 <= COUNT <= 64   two words from one 64-bit container shift        (filter_k_uni_q)
        //   COUNT <= 31         one word                                         (FilterRangeUni, NWW = 1)
        // kUniSubsetMax (trew_common.hpp) is shared with fill_thresholds: both sides must agree on the windows counted.
        // (a) COUNT >= 73: k <= L - 72 (always below 32 since L <= 95)
        {
            const int hi = (L - kUniSubsetMax) < g31 ? (L - kUniSubsetMax) : g31;
            if (slow)
                FilterRangeUni<NW, 0, NW, true>::run(P1, P2, P3, gmin, hi, L, kmin, kmax, thr_row, dbg, vd);
            else
                FilterRangeUni<NW, 0, NW, false>::run(P1, P2, P3, gmin, hi, L, kmin, kmax, thr_row, dbg, vd);
        }
        // (b) 65 <= COUNT <= 72: k in [L-71, L-64] (k <= 31)
        {
            int a = L + 1 - kUniSubsetMax, b = L - 64;
            a = a < gmin ? gmin : a;
            b = b > g31 ? g31 : b;
            if (a <= b) {
                int2 th_next = thr_row[a - 1];
                for (int k = a; k <= b; k++) {
                    const int2 th = th_next;
                    th_next = thr_row[k];
                    uni_note(vd, filter_k_uni<NW, 0, 2, true>(P1, P2, P3, L, k, th, vd.hasm), k, slow, kmin, kmax, dbg);
                }
            }
        }
        // (c) 32 <= COUNT <= 64: k in [L-63, L-31]
        {
            const int s = L > 63 ? L - 63 : 0;
            int a = L - 63, b = L - 31;
            a = a < gmin ? gmin : a;
            b = b > gmax ? gmax : b;
            if (a <= b) {
                const u64 Q1 = container64(P1, s), Q2 = container64(P2, s);
                int2 th_next = thr_row[a - 1];
                for (int k = a; k <= b; k++) {
                    const int2 th = th_next;
                    th_next = thr_row[k];
                    uni_note(vd, filter_k_uni_q(P1, P2, P3, Q1, Q2, s, L, k, th, vd.hasm), k, slow, kmin, kmax, dbg);
                }
            }
        }
        // (d) COUNT <= 31: one word, k >= L - 30
        // (the three word offsets of a range are spelled out here and below: a helper that runs them costs filter_kernel<5>
        // fourteen instructions, profiles/bound_refactor/README.md)
        if (slow) {
            FilterRangeUni<NW, 0, 1, true>::run(P1, P2, P3, gmin, g31, L, kmin, kmax, thr_row, dbg, vd);
            FilterRangeUni<NW, 1, 1, true>::run(P1, P2, P3, gmin > 32 ? gmin : 32, gmax < 63 ? gmax : 63, L, kmin, kmax, thr_row, dbg, vd);
            FilterRangeUni<NW, 2, 1, true>::run(P1, P2, P3, gmin > 64 ? gmin : 64, gmax, L, kmin, kmax, thr_row, dbg, vd);
        } else {
            FilterRangeUni<NW, 0, 1, false>::run(P1, P2, P3, gmin, g31, L, kmin, kmax, thr_row, false, vd);
            FilterRangeUni<NW, 1, 1, false>::run(P1, P2, P3, gmin > 32 ? gmin : 32, gmax < 63 ? gmax : 63, L, kmin, kmax, thr_row, false, vd);
            FilterRangeUni<NW, 2, 1, false>::run(P1, P2, P3, gmin > 64 ? gmin : 64, gmax, L, kmin, kmax, thr_row, false, vd);
        }
        if (!slow) vd.flagm = vd.hasm;
    } else {
        if (slow) {
            FilterRangeUni<NW, 0, NW, true>::run(P1, P2, P3, gmin, g31, L, kmin, kmax, thr_row, dbg, vd);
            FilterRangeUni<NW, 1, NW, true>::run(P1, P2, P3, gmin > 32 ? gmin : 32, gmax < 63 ? gmax : 63, L, kmin, kmax, thr_row, dbg, vd);
            FilterRangeUni<NW, 2, NW, true>::run(P1, P2, P3, gmin > 64 ? gmin : 64, gmax, L, kmin, kmax, thr_row, dbg, vd);
        } else {
            FilterRangeUni<NW, 0, NW, false>::run(P1, P2, P3, gmin, g31, L, kmin, kmax, thr_row, false, vd);
            FilterRangeUni<NW, 1, NW, false>::run(P1, P2, P3, gmin > 32 ? gmin : 32, gmax < 63 ? gmax : 63, L, kmin, kmax, thr_row, false, vd);
            FilterRangeUni<NW, 2, NW, false>::run(P1, P2, P3, gmin > 64 ? gmin : 64, gmax, L, kmin, kmax, thr_row, false, vd);
            vd.flagm = vd.hasm;
        }
    }
}

// ---- the two halves of a read in one k loop (3-word kernel, N-free lanes, equal half lengths L <= 95) ----
// What the prefilter decides per read is one bit, and what this loop decides is less: whether some k passes the 4-bucket test
// of either half (filter_halves_uni).  It carries no per-k state but the shift amount and the address of the window mask, and
// takes the constants of two k from one scalar load.
// Measured on MI355X (profiles/r03/README.md): scalar instructions are not free beside the VALU stream -- the round-2 loop
// spent 18 SALU on 22 VALU per (k, half) and trading 23 M VALU for 61 M SALU instructions per launch changed nothing -- so the
// loop is written to keep them down: both halves share the loop control, the thresholds and the masks.
// The threshold table is read-only for the kernel's lifetime (filled by the host before the launch), which the compiler cannot
// see through the kernel's other stores: the constant address space says so, and a wave-uniform load from it is an s_load
// straight into SGPRs (load_thr8 / load_thr4 below).
struct HalvesP {
    u32 P1[3], P2[3];  // prefix parities of the lo plane and the hi plane of one half
};
__device__ __forceinline__ void halves_prefix(const u32 (&lo)[3], const u32 (&hi)[3], int L, HalvesP &o) {
    u32 none[3];
    segment_setup<3, false, false>(lo, hi, /* N plane: not read */ lo, L, /* v1, P3: not written */ none, o.P1, o.P2, none);
}
// ---- both halves of a read from ONE load and ONE prefix parity per plane (load_read5, helpers.inc) ----
// The left half starts at base 0 and the right half at base h, 64 <= h < 96 (wave-uniform), of a read of at most 159 bases.
// three words of a 5-word plane (or prefix parity) from base h on; bs = h & 31
__device__ __forceinline__ void read5_from64(const u32 (&x)[5], u32 bs, u32 (&o)[3]) {
    o[0] = alignbit(x[3], x[2], bs);
    o[1] = alignbit(x[4], x[3], bs);
    o[2] = alignbit(0u, x[4], bs);
}
// an N among bases [0, len) (left: words 0..2, len <= 95) / among bases [h, h + len) (right: words 2..4, h >= 64, h + len <= 159)
// of the raw N plane: the masks are wave-uniform, the plane is not shifted for them
__device__ __forceinline__ u32 read5_left_has_n(const u32 (&nm)[5], int len) {
    return (nm[0] & low_mask(len)) | (nm[1] & low_mask(len - 32)) | (nm[2] & low_mask(len - 64));
}
__device__ __forceinline__ u32 read5_right_has_n(const u32 (&nm)[5], int h, int len) {
    u32 anyn = 0;
#pragma unroll
    for (int j = 2; j < 5; j++) anyn |= nm[j] & low_mask(h + len - 32 * j) & ~low_mask(h - 32 * j);
    return anyn;
}
// The prefix parities of both halves from one prefix parity of the whole read per plane.  P of the read at bit i is the parity of
// bases 0 .. i-1, whatever lies behind them: the left half's words are words 0..2 as they stand, with no mask at all.  From base
// h on the words hold the right half's own prefix parity XOR the constant P[h], which drops out of every window parity
// P[i] ^ P[i + k].  filter_halves_uni reads a half's P at bits 0 .. L, bit L included (the last window of a k): range (b) takes
// bits 0 .. 63 + k with k <= L - 64, range (c) the container's bits s .. s + 63 = L (s = L - 63; a shorter half: s = 0 and the second word masked to COUNT - 32 windows,
// all below L), and what the 64-bit shift fills with zeros lies at windows >= COUNT, which wm masks -- so neither the bases
// behind a half (the right half's, for the left one; the extra base of an odd-length read) nor the bits behind the read in its
// last word are ever looked at, and nothing is masked to a length here.
// Bit L of the right half is bit h + L of the read, and five words hold the read's P at bits 0 .. 159 only: P[160], the parity
// of all 160 bases, has no place in them (read5_from64 would hand the loop a zero for it).  So the read has at most 159 bases
// -- h + L <= 159, the caller's condition; a batch of 160-base reads keeps a prefix parity per half, whose third word has room.
__device__ __forceinline__ void halves_prefix_read5(const ReadPlanes5 &r, u32 bs, HalvesP &left, HalvesP &right) {
    u32 P1[5], P2[5];
    prefix_parity_read5(r.lo, P1);
    prefix_parity_read5(r.hi, P2);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        left.P1[j] = P1[j];
        left.P2[j] = P2[j];
    }
    read5_from64(P1, bs, right.P1);
    read5_from64(P2, bs, right.P2);
}

// 4-bucket statistics of one half at one k from its two window-parity words (second word already masked to the windows that
// exist), as SIGNS: with the popcount chains started at -2 ithr (c1x, cx1) and -ithr (c11),
// p = c10 - ithr, q = c01 - ithr, c = c11 - ithr and t = (COUNT - c00) - jthr - 1 come out of the same two subtractions and one
// three-operand add, and "some bucket reaches ithr" is a sign test: x = p & q & c is negative iff none of the three does, t is
// negative iff bucket 00 does.  v_max / v_min / v_cmp / v_add3 occupy the SIMD for 4.2 cycles, v_sub / v_bitop3 for 2.3
// (tools/valu_rate.hip): three max, a min and two compares per k become three v_bitop3 per half -- the third (halves_note) keeps
// the half's verdict over all k as the sign of an accumulator, so the loop has no compare at all.
__device__ __forceinline__ u32 bcnt_acc_s(u32 x, int acc) {
    u32 d;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "s"(acc));
    return d;
}
__device__ __forceinline__ void halves_signs(u32 F1a, u32 F2a, u32 F1b, u32 F2b, int n2, int n1, int K, u32 &x, u32 &t) {
    u32 a = bcnt_acc_s(F1a, n2);
    u32 b = bcnt_acc_s(F2a, n2);
    u32 c = bcnt_acc_s(F1a & F2a, n1);
    a = bcnt_acc(F1b, a);
    b = bcnt_acc(F2b, b);
    c = bcnt_acc(F1b & F2b, c);
    const u32 p = a - c, q = b - c;
    x = __builtin_amdgcn_bitop3_b32(p, q, c, 0x80);  // p & q & c
    t = a + q + (u32) K;
}
// acc & x & ~t: acc (all ones before the first k) stays negative as long as no bucket of the half has reached its threshold
__device__ __forceinline__ u32 halves_note(u32 acc, u32 x, u32 t) { return __builtin_amdgcn_bitop3_b32(acc, x, t, 0x40); }
// {-2 ithr, -ithr, 3 ithr - jthr - 1, ithr} of two consecutive k in one scalar load (the joint rows' table, fill_thresholds)
struct Thr8 {
    int4 a, b;
};
__device__ __forceinline__ Thr8 load_thr8(const int4 *p) {
    typedef int v8i __attribute__((ext_vector_type(8)));
    typedef const __attribute__((address_space(4))) v8i *cptr;
    const v8i v = *(cptr) (unsigned long long) p;
    Thr8 o;
    o.a = make_int4(v[0], v[1], v[2], v[3]);
    o.b = make_int4(v[4], v[5], v[6], v[7]);
    return o;
}
__device__ __forceinline__ int4 load_thr4(const int4 *p) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(4))) v4i *cptr;
    const v4i v = *(cptr) (unsigned long long) p;
    return make_int4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ const int4 *joint_thresholds(const int2 *thr_tab) { return (const int4 *) (thr_tab + kThrRows * kThrRow); }

// The batch geometry behind the thresholds (FilterGeom, filled by the host with them).  One 32- or 64-byte struct of it from a
// wave-uniform address in the constant address space: one s_load_dwordx8 / x16 that the scalar cache serves, its fields SGPRs.
// (two of them: [1] is the block of a launch that writes the per-slot candidate masks, with nothing for the joint loop)
__device__ __forceinline__ const FilterGeom *filter_geom(const int2 *thr_tab, bool masks) {
    return (const FilterGeom *) ((const char *) thr_tab + kThrGeomOffset) + (masks ? 1 : 0);
}
template <typename T>
__device__ __forceinline__ T load_geom(const T *p) {
    constexpr int N = (int) (sizeof(T) / 4);
    static_assert(N == 8 || N == 16, "one scalar load");
    typedef u32 vNu __attribute__((ext_vector_type(N)));
    typedef const __attribute__((address_space(4))) vNu *cptr;
    // a cast between address spaces, not through an integer: that would let the table's pointer escape, and with it the promise
    // (__restrict__) that no store of the kernel reaches the table -- the k loops' threshold loads then stop being scalar loads
    const vNu v = *(cptr) p;
    T o;
    __builtin_memcpy(&o, &v, sizeof(T));
    return o;
}
// The block's address as a value the compiler cannot follow, taken where a round (or a drain) starts: the loads behind it stay at
// their point of use.  Left alone the compiler hoists them out of the persistent loop, runs out of SGPRs and parks the fields in
// VGPR lanes, a v_readlane for every use -- what became of the geometry when the kernel derived it (profiles/round_geometry).
// tick: the round's number, an input of the statement, so that it belongs to its round without being volatile.
__device__ __forceinline__ const FilterGeom *geom_here(const FilterGeom *g, u32 tick) {
    asm("" : "+s"(g) : "s"(tick));
    return g;
}
// the read `mate` of a unit of a batch of equal-length reads (no offsets, no lengths: stage_thresholds); an inactive lane gets an
// empty descriptor
__device__ __forceinline__ ReadRef uniform_read(const DevBatch &B, u32 reads_per_unit, u64 unit, u32 mate, bool active, u32 read_words) {
    ReadRef r;
    r.w = B.words + (active ? (unit * reads_per_unit + mate) * (u64) B.uniform_stride : 0ull);
    r.len = active ? B.uniform_length : 0u;
    r.nw = active ? read_words : 0u;
    return r;
}
__device__ __forceinline__ ReadRef uniform_read(const DevBatch &B, u32 reads_per_unit, u64 unit, u32 mate, bool active) {
    return uniform_read(B, reads_per_unit, unit, mate, active, (B.uniform_length + 31u) >> 5);
}
// prefix parities of one half from its planes and the (wave-uniform) masks of its L bases: halves_prefix with the masks given
__device__ __forceinline__ void halves_prefix_masked(const u32 (&lo)[3], const u32 (&hi)[3], const u32 (&lm)[3], HalvesP &o) {
    u32 f1[3], f2[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        f1[j] = lo[j] & lm[j];
        f2[j] = hi[j] & lm[j];
    }
    prefix_parity<3>(f1, o.P1);
    prefix_parity<3>(f2, o.P2);
}

// Both halves of a read in ONE k loop.  passA / passB: this lane's half passes the 4-bucket test at some k of [klo, khi].
// That is all the loop decides: such a half (3 % of the reads have one: the telomeric ones and a few near misses) is set aside and
// judged by the drain with the other set-aside halves, a lane each -- the 8-bucket verdict used to be taken here, by the whole
// wave for the one lane that needed it (two verdicts per 64 reads: 12 % of the kernel's instructions, plus the third prefix
// parity of every read).  The loop carries no state but one sign accumulator per half: no compare, no branch on a trigger, no
// thresholds kept.  The verdict of a half is valid whatever the other half holds (an N there spoils only its own).
// Preconditions (checked by the caller): L <= 95, klo <= 31 and every k of the range has 33..kUniSubsetMax windows, so that
// only the first 64 windows are ever looked at (uni_windows) and a parity mask is two words.
// (Tried and dropped, profiles/r03/README.md: carrying the window parities from k to k+1, F_{k+1} = F_k ^ (f >> k), which
// needs no prefix parities at all but rebuilds the third parity for every verdict.)
// wm_tab: LDS, wm_tab[i] = all ones >> i (i = 0..31; two words of read-ahead behind them).  The window mask of the second word
// comes from there as a VECTOR register: a VALU instruction with a scalar source operand occupies the SIMD for 4.1 cycles instead
// of 2.3 (tools/valu_rate.hip: v_and / v_xor / v_bitop3 with an SGPR source), four of them per k; an LDS load costs no VALU issue.
__device__ __forceinline__ void filter_halves_uni(const HalvesP &A, const HalvesP &Bh, int L, int klo, int khi, const int4 *__restrict__ thr_row,
                                                  const u32 *wm_tab, bool &passA, bool &passB) {
    u32 accA = 0xffffffffu, accB = 0xffffffffu;
    int k = klo;
    const int4 *tp = thr_row + (klo - 1);  // {-2 ithr, -ithr, 3 ithr - jthr - 1, ithr} per k
    // (b) 65 <= COUNT <= kUniSubsetMax: the first 64 windows (thresholds lowered accordingly by fill_thresholds), funnel shifts
    {
        int b = L - 64;
        b = b > khi ? khi : b;
        auto probe = [&](u32 bs, const int4 t) __attribute__((always_inline)) {
            u32 xA, tA, xB, tB;
            halves_signs(A.P1[0] ^ alignbit(A.P1[1], A.P1[0], bs), A.P2[0] ^ alignbit(A.P2[1], A.P2[0], bs), A.P1[1] ^ alignbit(A.P1[2], A.P1[1], bs),
                         A.P2[1] ^ alignbit(A.P2[2], A.P2[1], bs), t.x, t.y, t.z, xA, tA);
            halves_signs(Bh.P1[0] ^ alignbit(Bh.P1[1], Bh.P1[0], bs), Bh.P2[0] ^ alignbit(Bh.P2[1], Bh.P2[0], bs), Bh.P1[1] ^ alignbit(Bh.P1[2], Bh.P1[1], bs),
                         Bh.P2[1] ^ alignbit(Bh.P2[2], Bh.P2[1], bs), t.x, t.y, t.z, xB, tB);
            accA = halves_note(accA, xA, tA);
            accB = halves_note(accB, xB, tB);
        };
        for (; k + 1 <= b; k += 2, tp += 2) {  // two k per trip, thresholds of both from one scalar load
            const Thr8 t8 = load_thr8(tp);
            probe((u32) k, t8.a);
            probe((u32) k + 1u, t8.b);
        }
        if (k <= b) {
            probe((u32) k, load_thr4(tp));
            k++, tp++;
        }
    }
    // (c) 33 <= COUNT <= 64: one 64-bit container shift per parity and half
    if (k <= khi) {
        const int b = khi;
        const int s = L > 63 ? L - 63 : 0;
        const u64 QA1 = container64(A.P1, s), QA2 = container64(A.P2, s), QB1 = container64(Bh.P1, s), QB2 = container64(Bh.P2, s);
        u32 sh = (u32) (k - s);  // running scalar instead of a function of k
        typedef const __attribute__((address_space(3))) u32 *lds_u32;
        u32 wa = (u32) (unsigned long long) (lds_u32) wm_tab + 4u * (u32) (63 - (L - k));  // LDS address of this k's mask: COUNT - 32 low bits = all ones >> (64 - COUNT)
        asm volatile("" : "+v"(wa));  // a vector register from here on: advancing it is a v_add of an inline constant
        auto probe = [&](u32 shk, u32 wmk, const int4 t) __attribute__((always_inline)) {
            const u64 SA1 = QA1 >> shk, SA2 = QA2 >> shk, SB1 = QB1 >> shk, SB2 = QB2 >> shk;
            // (x ^ y) & m in one v_bitop3_b32: the compiler splits it into a xor and an and when left to choose
            const u32 gA1 = xor_and(A.P1[1], (u32) (SA1 >> 32), wmk), gA2 = xor_and(A.P2[1], (u32) (SA2 >> 32), wmk);
            const u32 gB1 = xor_and(Bh.P1[1], (u32) (SB1 >> 32), wmk), gB2 = xor_and(Bh.P2[1], (u32) (SB2 >> 32), wmk);
            u32 xA, tA, xB, tB;
            halves_signs(A.P1[0] ^ (u32) SA1, A.P2[0] ^ (u32) SA2, gA1, gA2, t.x, t.y, t.z, xA, tA);
            halves_signs(Bh.P1[0] ^ (u32) SB1, Bh.P2[0] ^ (u32) SB2, gB1, gB2, t.x, t.y, t.z, xB, tB);
            accA = halves_note(accA, xA, tA);
            accB = halves_note(accB, xB, tB);
        };
        for (; k + 1 <= b; k += 2, sh += 2u, wa += 8u, tp += 2) {
            const Thr8 t8 = load_thr8(tp);
            const u32 wm0 = *(lds_u32) (unsigned long long) wa, wm1 = *(lds_u32) (unsigned long long) (wa + 4u);
            probe(sh, wm0, t8.a);
            probe(sh + 1u, wm1, t8.b);
        }
        if (k <= b) probe(sh, *(lds_u32) (unsigned long long) wa, load_thr4(tp));
    }
    passA = (int) accA >= 0;
    passB = (int) accB >= 0;
}

// ---- the reads the uniform path set aside, judged in one joint k loop (3-word kernel) ----
// The fast path sets aside every read with an N in a half (7 % of the synthetic reads) and every read some k of which passes
// its 4-bucket test (3 %: the telomeric ones and a few near misses).  Most of them need the drain for ONE half (a single N; a
// junction read): those go to filter_deferred_half, a lane per half, the rest to filter_deferred_uni, a lane per unit; both run
// the probes below (drain_probe3 / drain_probe2).  filter_deferred_uni gives a unit the verdict the general
// path (filter_segment, a call per half) gives when the k loop is the halves' own [kmin, kmax]: a read is flagged exactly when
// some half has some k whose 8-bucket maximum over the windows without an N reaches ithr(COUNT) -- the general path's first
// candidate of a segment is always an 8-bucket pass, and m8 <= m4.  Written like the fast loop, with per-lane window masks:
//   - both halves in one k loop, wave-uniform loop control;
//   - V_k (windows of length k with no N, bit i = window i) per lane: V_{k+1} = V_k & (V_k >> 1) from V_1 = the valid bases, for
//     any number of Ns; it goes into the xor_and that builds each parity word, so masking a word costs nothing;
//   - COUNT = popc(V_k) per lane, its thresholds from an LDS table indexed by COUNT (cnt_thr, the general path's float
//     expression, so exact by construction): the popcount chains start from them and the 4-bucket test is a sign test;
//   - the 8-bucket stage runs per half only when some lane not flagged yet passes that half's 4-bucket test, and a lane once
//     flagged is done (the loop ends when every lane is);
//   - k with more than 64 windows in some half: three words and funnel shifts; the rest: one 64-bit container shift per parity.
constexpr int kCntThr = 97;  // COUNT = 0 .. 96: segments of at most 95 bases
// cnt_thr[c] = {-2 ithr, -ithr, 4 ithr - c - 1, ithr}, ithr = floor((float) c * lowf) + 1: (float) m > (float) c * lowf  <=>  m >= ithr
__device__ __forceinline__ int4 count_thresholds(int c, float lowf) {
    const float prod = __fmul_rn((float) c, lowf);  // the general path's (float) count * lowf
    const int ithr = (int) floorf(prod) + 1;
    return make_int4(-2 * ithr, -ithr, 4 * ithr - c - 1, ithr);
}

struct DrainHalf {
    u32 P1[3], P2[3], P3[3];  // prefix parities of the lo, hi and lo & hi planes
    u32 V[3];                 // V_k
};
__device__ __forceinline__ void drain_half_init(const u32 (&lo)[3], const u32 (&hi)[3], const u32 (&nm)[3], int L, bool active, DrainHalf &h) {
    segment_setup<3, false, true, true>(lo, hi, nm, L, h.V, h.P1, h.P2, h.P3);  // V_1: bases inside the half that are A/C/G/T
#pragma unroll
    for (int j = 0; j < 3; j++) h.V[j] = active ? h.V[j] : 0u;  // an inactive lane has no window
}
__device__ __forceinline__ void drain_v_step3(u32 (&V)[3]) {  // V_{k+1} = V_k & (V_k >> 1)
    V[0] &= alignbit(V[1], V[0], 1u);
    V[1] &= alignbit(V[2], V[1], 1u);
    V[2] &= V[2] >> 1;
}
// 4-bucket test of one half from its N window-parity words (already masked by V_k), thresholds th = cnt_thr[COUNT]:
// the result is >= 0 (as int) iff some bucket reaches ithr (halves_signs with per-lane constants)
template <int N>
__device__ __forceinline__ int drain_signs(const u32 (&F1)[N], const u32 (&F2)[N], const int4 th) {
    u32 a = (u32) th.x, b = (u32) th.x, c = (u32) th.y;
#pragma unroll
    for (int j = 0; j < N; j++) {
        a = bcnt_acc(F1[j], a);
        b = bcnt_acc(F2[j], b);
        c = bcnt_acc(F1[j] & F2[j], c);
    }
    const u32 p = a - c, q = b - c;
    const u32 t = a + q + (u32) th.z;
    return (int) __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(p, q, c, 0x80), t, t, 0x30);  // p & q & c & ~t
}
// 8-bucket maximum of one half reaches ithr (the rare stage: only for lanes not flagged yet that pass the 4-bucket test)
template <int N>
__device__ __forceinline__ bool drain_pass8(const u32 (&F1)[N], const u32 (&F2)[N], const u32 (&F3)[N], const u32 (&V)[N], u32 count, int ithr) {
    const u32 m8 = max_bucket8<N>(F1, F2, F3, V, count);
    return (int) m8 >= ithr;
}

// One half at one k of the drain: the lanes whose 8-bucket maximum over the windows of V_k reaches ithr(COUNT).  The 8-bucket
// stage runs only when some lane not in `flag` (the lanes decided already) passes the 4-bucket test.  cnt_thr: LDS, kCntThr entries.
// k with more than 64 windows in some lane (k <= 31): three words, funnel shifts
__device__ __forceinline__ u64 drain_probe3(const DrainHalf &h, u32 bs, u64 flag, const int4 *cnt_thr) {
    const u32 cnt = bcnt_acc(h.V[2], bcnt_acc(h.V[1], __popc(h.V[0])));
    const int4 th = cnt_thr[cnt];
    u32 F1[3], F2[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        F1[j] = xor_and(h.P1[j], alignbit(j < 2 ? h.P1[j < 2 ? j + 1 : 0] : 0u, h.P1[j], bs), h.V[j]);
        F2[j] = xor_and(h.P2[j], alignbit(j < 2 ? h.P2[j < 2 ? j + 1 : 0] : 0u, h.P2[j], bs), h.V[j]);
    }
    const u64 p4 = __ballot(drain_signs<3>(F1, F2, th) >= 0);
    u64 p8 = 0;
    if (p4 & ~flag) {
        u32 F3[3];
#pragma unroll
        for (int j = 0; j < 3; j++) F3[j] = h.P3[j] ^ alignbit(j < 2 ? h.P3[j < 2 ? j + 1 : 0] : 0u, h.P3[j], bs);
        p8 = __ballot(drain_pass8<3>(F1, F2, F3, h.V, cnt, th.w));
    }
    return p8;
}
// at most 64 windows: windows 0..63 of P >> k from one 64-bit shift of the container Q = P[s .. s + 64); V = V_k (V[2] is empty)
__device__ __forceinline__ u64 drain_probe2(const DrainHalf &h, u64 Q1, u64 Q2, u64 V, int s, int k, u64 flag, const int4 *cnt_thr) {
    const u32 v0 = (u32) V, v1 = (u32) (V >> 32);
    const u32 cnt = bcnt_acc(v1, __popc(v0));
    const int4 th = cnt_thr[cnt];
    const u32 sh = (u32) (k - s);
    const u64 S1 = Q1 >> sh, S2 = Q2 >> sh;
    const u32 F1[2] = {xor_and(h.P1[0], (u32) S1, v0), xor_and(h.P1[1], (u32) (S1 >> 32), v1)};
    const u32 F2[2] = {xor_and(h.P2[0], (u32) S2, v0), xor_and(h.P2[1], (u32) (S2 >> 32), v1)};
    const u64 p4 = __ballot(drain_signs<2>(F1, F2, th) >= 0);
    u64 p8 = 0;
    if (p4 & ~flag) {
        const u64 S3 = container64(h.P3, s) >> sh;
        const u32 F3[2] = {h.P3[0] ^ (u32) S3, h.P3[1] ^ (u32) (S3 >> 32)};
        const u32 Vw[2] = {v0, v1};
        p8 = __ballot(drain_pass8<2>(F1, F2, F3, Vw, cnt, th.w));
    }
    return p8;
}

// Verdict of one unit (short: a read, pair: two mates) set aside by the uniform path with two or more halves to judge.
__device__ __forceinline__ bool filter_deferred_uni(const DevParams &P, const DevBatch &B, u64 unit, bool active, const FilterGeom *geom, u32 tick,
                                                    const int4 *cnt_thr) {
    // the geometry of the halves from the batch's block (drain_ok: slot[i] is half i, and every half has the drain's k range)
    const FilterGeom *g = geom_here(geom, tick);
    const GeomHead hd = load_geom(&g->head);
    const u32 rpu = P.mode == TREW_MODE_PAIR ? 2u : 1u;
    const u64 actm = __ballot(active);
    u64 flag = 0;
    const int n_halves = (int) hd.n_halves;
    for (int p = 0; p < n_halves && flag != actm; p += 2) {
        const SlotGeom sA = load_geom(&g->slot[p]), sB = load_geom(&g->slot[p + 1]);
        const int LA = (int) sA.len, LB = (int) sB.len, Lmax = LA < LB ? LB : LA;
        const int klo = hd.drain_klo, khi = hd.drain_khi;
        DrainHalf A, Bh;
        {
            u32 lo[3], hi[3], nm[3];
            load_planes<3>(uniform_read(B, rpu, unit, sA.mate, active), sA.start, lo, hi, nm);
            drain_half_init(lo, hi, nm, LA, active, A);
            load_planes<3>(uniform_read(B, rpu, unit, sB.mate, active), sB.start, lo, hi, nm);
            drain_half_init(lo, hi, nm, LB, active, Bh);
        }
        for (int t = 1; t < klo; t++) {  // V_klo
            drain_v_step3(A.V);
            drain_v_step3(Bh.V);
        }
        int k = klo;
        // (b) k with more than 64 windows in some half (k <= Lmax - 64 <= 31)
        for (const int b = khi < Lmax - 64 ? khi : Lmax - 64; k <= b && flag != actm; k++) {
            flag |= drain_probe3(A, (u32) k, flag, cnt_thr);
            flag |= drain_probe3(Bh, (u32) k, flag, cnt_thr);
            drain_v_step3(A.V);
            drain_v_step3(Bh.V);
        }
        // (c) at most 64 windows in either half
        if (k <= khi && flag != actm) {
            const int oA = LA > 63 ? LA - 63 : 0, oB = LB > 63 ? LB - 63 : 0;  // container offsets
            const u64 QA1 = container64(A.P1, oA), QA2 = container64(A.P2, oA), QB1 = container64(Bh.P1, oB), QB2 = container64(Bh.P2, oB);
            u64 VA = ((u64) A.V[1] << 32) | A.V[0], VB = ((u64) Bh.V[1] << 32) | Bh.V[0];  // V[2] is empty from here on
            for (; k <= khi && flag != actm; k++) {
                flag |= drain_probe2(A, QA1, QA2, VA, oA, k, flag, cnt_thr);
                flag |= drain_probe2(Bh, QB1, QB2, VB, oB, k, flag, cnt_thr);
                VA &= VA >> 1;
                VB &= VB >> 1;
            }
        }
    }
    return (flag >> lane_id()) & 1ull;
}

// Verdict of a unit of which only half `half` (its slot: 0..1 short, 0..3 pair) has to be judged, a lane per half: the other
// halves hold no N and passed no 4-bucket test in the fast loop, and m8 <= m4 over the windows that loop looks at, against the
// thresholds it uses (fill_thresholds), so they cannot flag the unit.  The k loop is filter_deferred_uni's, once per k instead
// of twice; every half has the same [kmin, kmax] (drain_uni_applies).  Length, start and container offset are per lane: the
// halves of an odd-length read differ by one base, and the probes take their window masks from V_k, not from the length.
__device__ __forceinline__ bool filter_deferred_half(const DevParams &P, const DevBatch &B, u64 unit, u32 half, bool active, const FilterGeom *geom, u32 tick,
                                                     const int4 *cnt_thr) {
    const FilterGeom *g = geom_here(geom, tick);
    const GeomHead hd = load_geom(&g->head);
    const u32 rpu = P.mode == TREW_MODE_PAIR ? 2u : 1u;
    // the lane's own half out of the block (drain_ok: slot[i] is half i; half < n_halves, 0 for an idle lane): a load per lane
    const SlotGeom *mine = &g->slot[half < hd.n_halves ? half : 0u];
    const u32 mate = mine->mate, start = mine->start;
    const int L = (int) mine->len;
    const int Lmax = hd.drain_lmax, klo = hd.drain_klo, khi = hd.drain_khi;
    DrainHalf h;
    {
        u32 lo[3], hi[3], nm[3];
        load_planes<3>(uniform_read(B, rpu, unit, mate, active), start, lo, hi, nm);
        drain_half_init(lo, hi, nm, L, active, h);
    }
    for (int t = 1; t < klo; t++) drain_v_step3(h.V);  // V_klo
    const u64 actm = __ballot(active);
    u64 flag = 0;
    int k = klo;
    for (const int b = khi < Lmax - 64 ? khi : Lmax - 64; k <= b && flag != actm; k++) {
        flag |= drain_probe3(h, (u32) k, flag, cnt_thr);
        drain_v_step3(h.V);
    }
    if (k <= khi && flag != actm) {
        const int o = L > 63 ? L - 63 : 0;
        const u64 Q1 = container64(h.P1, o), Q2 = container64(h.P2, o);
        u64 V = ((u64) h.V[1] << 32) | h.V[0];
        for (; k <= khi && flag != actm; k++) {
            flag |= drain_probe2(h, Q1, Q2, V, o, k, flag, cnt_thr);
            V &= V >> 1;
        }
    }
    return (flag >> lane_id()) & 1ull;
}

// Block size of the prefilter.  Measured on MI355X (tools/filter_grid_ab.sh, profiles/r02/README.md): 64-thread blocks
// (no block-level barrier at all) and 256-thread blocks run the same 0.70-0.72 ms on 10 M reads, and a variant with
// wave-private staging lists was slower (95 VGPRs, 5 waves per SIMD) -- the kernel is bound by VALU issue, not by
// its barriers.  Twice as many blocks as are resident is worth 5 % (the dispatcher back-fills the uneven tail).
constexpr u32 kFilterThreads = TREW_FILTER_THREADS;
constexpr u32 kStage = kFilterThreads == 256 ? 1024 : 192;  // unit indices a block stages in LDS before one global append
constexpr u32 kDefer = 2 * kFilterThreads;                   // units set aside by the fast path (drained one block-full at a time)

// Persistent blocks that pull chunks of kFilterThreads reads from device counters (word kChunkCounterWord of each of the
// eight queue-head lines of the slot's counter block; chunk blockIdx.x is the block's first, the counters hand out the rest).  A static grid-stride share left the chip 79 % occupied
// on average (SQ_WAVE_CYCLES / kernel time, profiles/r03): 12.7 rounds per block means some blocks do 13 and most do 12, the
// deferred N reads and the 8-bucket stage land unevenly, and whoever finishes last sets the kernel's time.  With chunks
// handed out on demand every block ends within one round (~25 us) of the others.  The atomic for the NEXT chunk is issued
// ahead of the loads of the current one and read after its k loops, so its round trip never shows.
// Survivors are staged in LDS and appended to the worklist with ONE global atomic per flush: a per-wave atomic on the single
// worklist counter caps at ~88 appends/us on MI355X (MI355X_MICROARCH.md "dequeue"), which was as long as the whole k loop.
template <int NW>
#ifndef TREW_FILTER3_WAVES
#define TREW_FILTER3_WAVES 6
#endif
#ifndef TREW_FILTER5_WAVES
#define TREW_FILTER5_WAVES 6  // 250-bp reads: 80 VGPRs with 46 spilled beat 117 unspilled at 4 waves per SIMD (profiles/r03/README.md)
#endif
__global__ __launch_bounds__(kFilterThreads, (NW <= 3 ? TREW_FILTER3_WAVES : (NW == 5 ? TREW_FILTER5_WAVES : 1))) void filter_kernel(DevParams P, DevBatch B, u32 *wl, u32 *wl_count, u32 wl_cap,
                                                                u64 *dbg_masks, int dbg_slots, int max_seg, u32 *diag,
                                                                const int2 *__restrict__ thr_tab) {
#ifdef TREW_AB_FILTER_PRIO
    __builtin_amdgcn_s_setprio(TREW_AB_FILTER_PRIO);  // A/B builds
#endif
    __shared__ u32 stage[kStage];
    __shared__ u32 stage_n, flush_base;
    __shared__ u32 defer_n, half_n;       // units and single halves set aside by the fast path (the lists themselves are declared with the loop below)
    u32 defer_seen = 0, half_seen = 0;    // defer_n and half_n as of the last append(): block-uniform, see there
    if (threadIdx.x == 0) stage_n = 0;
    __syncthreads();
    auto flush = [&]() __attribute__((always_inline)) {  // block-uniform
        const u32 n = stage_n;
        if (n) {
            if (threadIdx.x == 0) flush_base = atomicAdd(wl_count, n);
            __syncthreads();
            const u32 fb = flush_base;
            for (u32 i = threadIdx.x; i < n; i += blockDim.x) {
                if (fb + i < wl_cap)
                    wl[fb + i] = stage[i];
                else
                    atomicAdd(&diag[kDiagWorklistDrop], 1u);  // surfaced by trew_hip_collect: never silent
            }
            __syncthreads();
            if (threadIdx.x == 0) stage_n = 0;
        }
        __syncthreads();
    };
    // wave-aggregated append of the flagged units to the block's LDS stage (block-uniform call)
    auto append = [&](bool flag, u32 unit) __attribute__((always_inline)) {
        wave_append(&stage_n, flag, [&](u32 at) __attribute__((always_inline)) { stage[at] = unit; });  // < kStage: flushed below when > kStage - block size
        __syncthreads();
        // Every thread reads the fill level before any thread goes on: a wave that ran ahead into the NEXT append (the general path
        // makes two in a row) would add to stage_n while a slower wave still looked at it, and the block would disagree about
        // flushing -- barriers inside flush() then pair up wrongly (seen as a few units twice and a few missing in the worklist,
        // about one pass in five hundred; tools/flag_diff.py).
        const bool full = stage_n > kStage - kFilterThreads;
        defer_seen = defer_n;  // the same holds for the two lists of reads set aside: their lengths are read here, between the barriers
        if constexpr (NW == 3) half_seen = half_n;
        __syncthreads();
        if (full) flush();
    };
    const int nslots = mode_slots(P.mode);
    const int gmax_run = filter_gmax_run(P);
    // general path: any read length, N anywhere
    auto general = [&](u64 unit, bool active) __attribute__((always_inline)) -> u64 {
        ReadRef rd[2];
        unit_reads(P, B, unit, active, rd);
        u64 any = 0;
#pragma unroll
        for (int slot = 0; slot < kMaxSlots; slot++) {
            if (slot < nslots) {
                u64 mask = 0;
                Segment sg = get_segment(P.mode, slot, rd[0].len, rd[1].len, P.min_mer, P.max_mer, P.slice_len);
                const bool ok = active && sg.valid && sg.len <= (u32) (32 * NW - 1);
                if (__any(ok)) {
                    u32 lo[NW], hi[NW], nm[NW];
                    const ReadRef &r = sg.mate ? rd[1] : rd[0];
                    if (ok) {
                        load_planes<NW>(r, sg.start, lo, hi, nm);
                    } else {
#pragma unroll
                        for (int j = 0; j < NW; j++) {
                            lo[j] = hi[j] = 0;
                            nm[j] = 0xffffffffu;
                        }
                    }
                    u64 m;
                    if (P.flags & TREW_FLAG_NO_FILTER)
                        m = all_k_mask(sg.kmin, sg.kmax);
                    else
                        m = filter_segment<NW>(lo, hi, nm, ok ? (int) sg.len : 0, sg.kmin, sg.kmax, P.min_mer, gmax_run, max_seg, P.lowf);
                    mask = ok ? m : 0ull;
                }
                // a segment too long for this instantiation must never be dropped silently
                if (active && sg.valid && sg.len > (u32) (32 * NW - 1)) mask = all_k_mask(sg.kmin, sg.kmax);
                any |= mask;
                if (dbg_masks && active && slot < dbg_slots) dbg_masks[unit * (u64) dbg_slots + slot] = mask;
            }
        }
        return any;
    };

    // One loop for both kinds of batch, so that the (large) general path is instantiated once:
    // every round the block takes one fresh unit per thread; the fast path judges the N-free ones on the spot
    // and sets the others aside, a batch without uniform geometry sets all of them aside; whenever
    // a block-full of units is waiting (or the input is exhausted) the general path drains them.
    __shared__ u32 defer[kDefer];
    __shared__ unsigned char defer_kind[kDefer];  // 1: set aside because of an N
    constexpr u32 kHalfDefer = NW == 3 ? kDefer : 1;  // only the 3-word kernel has the joint loop that fills this list
    __shared__ u32 hdefer[kHalfDefer];                // units of which one half is set aside (filter_deferred_half), drained like defer[]
    __shared__ unsigned char hdefer_kind[kHalfDefer];  // bit 0: because of an N; bits 1..2: the half (its slot)
    __shared__ u32 wm_tab[34];  // all ones >> i: the joint loop's window masks (filter_halves_uni)
    if (threadIdx.x < 34) wm_tab[threadIdx.x] = threadIdx.x < 32 ? 0xffffffffu >> threadIdx.x : 0u;
    __shared__ int4 cnt_thr[kCntThr];  // thresholds by window count (filter_deferred_uni)
    for (u32 i = threadIdx.x; i < (u32) kCntThr; i += blockDim.x) cnt_thr[i] = count_thresholds((int) i, P.lowf);
    // thr_tab[slot * kThrRow + k - 1] = pass thresholds of (slot, k) for this batch's uniform geometry (fill_thresholds, below): read-only
    // global memory at a wave-uniform address, i.e. scalar loads into SGPRs -- the k loops spend no vector instruction on them
    const u32 UL = B.uniform_length;
    // The batch geometry (FilterGeom: which slots are valid and where they lie, what the joint loop and the drains need) stands
    // behind the thresholds, filled by the host for this read length, this instantiation and P.flags.  The rounds read it at the
    // point of use (geom_here / load_geom); what is read here, once, is only what decides the path of the whole launch.
    const FilterGeom *geom = thr_tab ? filter_geom(thr_tab, dbg_masks != nullptr) : nullptr;
    // head.nw == NW always holds: launch_filter picks NW from the longest valid segment of the uniform length (batch_geometry,
    // trew_capi.cpp) and fill_thresholds fills the block for pick_nw of the same maximum over the same get_segment calls.  Were they
    // ever to differ, the thresholds (uni_windows) would be another instantiation's as well, so the launch takes the general path.
    const bool uni = NW <= 5 && UL != 0 && thr_tab != nullptr && P.mode != TREW_MODE_LONG && !(P.flags & TREW_FLAG_NO_FILTER) &&
                     load_geom(&geom->head).nw == (u32) NW;
    // the reads set aside by the uniform path are judged by filter_deferred_uni, or by the general path (any NW, dbg_masks, A/B)
    const bool uni_drain = NW == 3 && uni && !dbg_masks && !(P.flags & TREW_FLAG_DEBUG_NO_UNI_DRAIN) && load_geom(&geom->head).drain_ok != 0u;
#ifdef TREW_AB_PIN_GEOM  // A/B builds (profiles/round_geometry, step 0): the round's geometry read ONCE, here, and pinned in scalar
                         // registers across the persistent loop (single-end batches: the first pair of halves serves every round)
    GeomHead hd_pin = {};
    HalvesRound hr_pin = {};
    if (uni) {
        hd_pin = load_geom(&geom->head);
        hr_pin = load_geom(&geom->round[0]);
    }
    asm volatile("" : "+s"(hd_pin.n_halves), "+s"(hd_pin.n_joint), "+s"(hd_pin.n_slots));
    asm volatile("" : "+s"(hr_pin.L), "+s"(hr_pin.klo), "+s"(hr_pin.khi), "+s"(hr_pin.row), "+s"(hr_pin.one_load), "+s"(hr_pin.mate), "+s"(hr_pin.bs),
                 "+s"(hr_pin.slot_p), "+s"(hr_pin.slot_q), "+s"(hr_pin.read_words));
    asm volatile("" : "+s"(hr_pin.nl[0]), "+s"(hr_pin.nl[1]), "+s"(hr_pin.nl[2]), "+s"(hr_pin.nr[0]), "+s"(hr_pin.nr[1]), "+s"(hr_pin.nr[2]));
#endif
    if (threadIdx.x == 0) defer_n = 0;
    if constexpr (NW == 3) {  // the half list is unused, and so not allocated, in the other instantiations
        if (threadIdx.x == 0) half_n = 0;
    }
    __syncthreads();
    __shared__ u32 next_chunk[2];  // written by thread 0 in round r (slot r & 1), read by all after that round's barrier
    // Eight counters on separate 128-B lines (a single word serves ~88 atomics a microsecond on MI355X -- 39 k chunks would keep
    // it busy for two thirds of the kernel): shard s hands out chunks gridDim.x + 8 c + s; a block whose shard has run dry
    // walks the others.
    constexpr u32 kChunkShards = 8;
    const u32 my_shard = blockIdx.x & (kChunkShards - 1u);
    auto shard_ctr = [&](u32 sh) __attribute__((always_inline)) { return wl_count + 32u + 32u * sh + kChunkCounterWord; };
    u64 chunk = blockIdx.x;
    u32 round = 0;
    for (;;) {
        const bool more = chunk * kFilterThreads < B.n_units;  // block-uniform
        if (more) {
            const u64 unit = chunk * kFilterThreads + threadIdx.x;
            const bool active = unit < B.n_units;
            // thread 0 asks for the next chunk FIRST: memory operations complete in order, so the round trip of this atomic
            // (L2, ~1-2 us) lies under the HBM latency of the read loads below, which have to be waited for anyway
            u32 nxt = 0;
            if (threadIdx.x == 0) nxt = gridDim.x + kChunkShards * atomicAdd(shard_ctr(my_shard), 1u) + my_shard;
            u64 any = 0;
            bool dfr = active, dfr_n = false;  // dfr_n: set aside because of an N
            bool dfr_half = false;             // set aside for one half only: half `hsel`
            u32 hsel = 0;
            if constexpr (NW <= 5) {
                if (uni) {
                    TREW_SETUP_MARK(read_setup);
                    // nothing below derives geometry: no get_segment, no branch on the mode or the slot, no mask of a length
                    const FilterGeom *g = geom_here(geom, round);
#ifndef TREW_AB_PIN_GEOM
                    const GeomHead hd = load_geom(&g->head);
#else
                    const GeomHead hd = hd_pin;
#endif
                    const u32 rpu = P.mode == TREW_MODE_PAIR ? 2u : 1u;  // reads of a unit
                    dfr = false;
                    u32 first = 0;  // valid slots the joint loop has taken: slot[first ..] go through the per-segment loops
                    if constexpr (NW == 3) {
                        // halves of equal length (or a right half one base longer) whose whole k range has 32..72 windows (150-bp
                        // reads at 5..32: 44..71): both halves of a read in one k loop (filter_halves_uni); anything else takes the
                        // per-segment loops below.  Which pairs of halves: the host decided (joint_loop_admits, build_filter_geom).
                        const u32 n_joint = hd.n_joint;  // none where the candidate masks are wanted: that launch has a block of its own
                        u32 nneed = 0;  // halves of this unit the drain has to judge
                        for (u32 pr = 0; pr < n_joint; pr++) {
#ifndef TREW_AB_PIN_GEOM
                            const HalvesRound hr = load_geom(&g->round[pr]);
#else
                            const HalvesRound hr = hr_pin;
#endif
                            // The two halves as the loop sees them: p and q, of slots slot_p and slot_q (scalars).  The loop treats both
                            // alike (one length L, one row of thresholds), so which is which matters only for the slot handed to the drain.
                            HalvesP hp, hq;
                            u32 np, nq;
                            // one_load: both halves lie in one read of at most five triples, one from base 0 and the other from a base in
                            // [64, 96), whatever the k range (reads of 128 .. 159 bases; at 5 .. 32 the joint loop takes 128 .. 153): the
                            // read is loaded once, and p is its left half.  Pair mode's second mate has its right half in the first
                            // slot.  Not 160: bit L of the right half's prefix parity would be bit 160 of the read's (halves_prefix_read5).
                            if (hr.one_load) {
                                TREW_SETUP_MARK(one_load);
                                ReadPlanes5 r;
                                load_read5(uniform_read(B, rpu, unit, hr.mate, active, hr.read_words), r);
                                np = (r.nm[0] & hr.nl[0]) | (r.nm[1] & hr.nl[1]) | (r.nm[2] & hr.nl[2]);
                                nq = (r.nm[2] & hr.nr[0]) | (r.nm[3] & hr.nr[1]) | (r.nm[4] & hr.nr[2]);  // an N in the right half's extra base counts
#ifndef TREW_AB_NO_READ_PREFIX
                                halves_prefix_read5(r, hr.bs, hp, hq);
#else  // A/B builds (profiles/read_setup): the one load alone, a prefix parity per half as before
                                u32 loq[3], hiq[3];
                                read5_from64(r.lo, hr.bs, loq);
                                read5_from64(r.hi, hr.bs, hiq);
                                const u32 lop[3] = {r.lo[0], r.lo[1], r.lo[2]}, hip[3] = {r.hi[0], r.hi[1], r.hi[2]};
                                halves_prefix(lop, hip, hr.L, hp);
                                halves_prefix(loq, hiq, hr.L, hq);
#endif
                            } else {
                                TREW_SETUP_MARK(two_loads);
                                const HalvesLoads hl = load_geom(&g->loads[pr]);
                                u32 loA[3], hiA[3], nmA[3], loB[3], hiB[3], nmB[3];
                                load_planes<3>(uniform_read(B, rpu, unit, hl.mate_a, active, hr.read_words), hl.start_a, loA, hiA, nmA);
                                load_planes<3>(uniform_read(B, rpu, unit, hl.mate_b, active, hr.read_words), hl.start_b, loB, hiB, nmB);
                                np = (nmA[0] & hr.nl[0]) | (nmA[1] & hr.nl[1]) | (nmA[2] & hr.nl[2]);
                                nq = (nmB[0] & hr.nr[0]) | (nmB[1] & hr.nr[1]) | (nmB[2] & hr.nr[2]);  // an N in the right half's extra base counts
                                halves_prefix_masked(loA, hiA, hr.nl, hp);
                                halves_prefix_masked(loB, hiB, hr.nl, hq);
                            }
                            dfr_n = dfr_n || (active && (np | nq) != 0);
                            // thresholds: halves of the same length share the row of the first; unequal ones have a joint row
                            bool passp, passq;
                            TREW_SETUP_MARK(joint_loop);
                            filter_halves_uni(hp, hq, hr.L, hr.klo, hr.khi, joint_thresholds(thr_tab) + hr.row * (u32) kThrRow, wm_tab, passp, passq);
                            // A half with an N does not fit the model, and a half some k of which passes the 4-bucket test needs its
                            // 8-bucket verdicts: the drain takes them, a lane per read or half (the verdict of a read never depends on
                            // its neighbours, so the flagged reads are the same).  A half that is neither cannot flag the read.
                            const bool needp = active && (np != 0 || passp), needq = active && (nq != 0 || passq);
                            nneed += (u32) needp + (u32) needq;
                            hsel = needq ? hr.slot_q : (needp ? hr.slot_p : hsel);  // read only when exactly one half of the unit is needed
                            dfr = dfr || needp || needq;
                        }
                        first = 2u * n_joint;  // admitted halves are valid: their place in slot[] is their slot
                        // one half to judge, every half went through the joint loop and the drain knows this geometry: the half list
                        dfr_half = uni_drain && first == hd.n_halves && nneed == 1u;
                    }
                    for (u32 i = first; i < hd.n_slots; i++) {  // the valid slots left, wave-uniform geometry: no need to unroll
                        const SlotGeom sg = load_geom(&g->slot[i < (u32) kMaxSlots ? i : 0u]);
                        if (sg.too_long) {  // too long for this instantiation: the general path keeps every k
                            dfr = dfr || active;
                            continue;
                        }
                        u32 lo[NW], hi[NW], nm[NW];
                        load_planes<NW>(uniform_read(B, rpu, unit, sg.mate, active), sg.start, lo, hi, nm);
                        u32 anyn = 0;  // segment_has_n<NW> written out: the call costs filter_kernel<5> two instructions (profiles/bound_refactor/README.md)
#pragma unroll
                        for (int j = 0; j < NW; j++) {
                            const int bits = (int) sg.len - 32 * j;
                            const u32 lm = low_mask(bits);
                            anyn |= nm[j] & lm;
                        }
                        UniVerdict vd;
                        filter_segment_uni<NW>(lo, hi, (int) sg.len, sg.kmin, sg.kmax, P.min_mer, gmax_run, thr_tab + sg.slot * (u32) kThrRow, dbg_masks != nullptr, vd);
                        dfr = dfr || (active && anyn != 0);
                        dfr_n = dfr_n || (active && anyn != 0);
                        any |= (vd.flagm >> lane_id()) & 1ull;
                        if (dbg_masks && active && anyn == 0 && (int) sg.slot < dbg_slots)
                            dbg_masks[unit * (u64) dbg_slots + sg.slot] = ((((u64) vd.chi) << 32) | vd.clo) & all_k_mask(sg.kmin, sg.kmax);
                    }
                }
            }
            {
                wave_append(&defer_n, dfr && !dfr_half, [=](u32 at) __attribute__((always_inline)) {  // < kDefer: drained below at one block-full
                    defer[at] = (u32) unit;
                    defer_kind[at] = dfr_n ? 1 : 0;
                });
                if constexpr (NW == 3) wave_append(&half_n, dfr_half, [=](u32 at) __attribute__((always_inline)) {  // a unit is in one list or the other; < kDefer likewise
                    hdefer[at] = (u32) unit;
                    hdefer_kind[at] = (unsigned char) ((hsel << 1) | (dfr_n ? 1u : 0u));
                });
            }
            if (threadIdx.x == 0) next_chunk[round & 1u] = nxt;
            append(active && !dfr && any != 0, (u32) unit);  // syncs the block
            chunk = next_chunk[round & 1u];
            if (chunk * kFilterThreads >= B.n_units) {  // block-uniform; end of the input only: look at the other shards, synchronously
                __syncthreads();  // every thread has read the dry id above before thread 0 replaces it (else a late wave would skip this branch and its barriers)
                if (threadIdx.x == 0) {
                    u64 c = chunk;
                    for (u32 att = 1; att < kChunkShards && c * kFilterThreads >= B.n_units; att++) {
                        const u32 sh = (my_shard + att) & (kChunkShards - 1u);
                        c = (u64) gridDim.x + (u64) kChunkShards * atomicAdd(shard_ctr(sh), 1u) + sh;
                    }
                    next_chunk[round & 1u] = (u32) (c < 0xffffffffull ? c : 0xffffffffull);
                }
                __syncthreads();
                chunk = next_chunk[round & 1u];
                __syncthreads();  // the next round may write this slot's twin only after everybody has read this one
            }
            round++;
        }
        // block-uniform: the lengths as every thread read them inside the last append() -- every add of this round happened before
        // that barrier, and no thread can have started the next round's adds.  (Reading defer_n here let a wave that ran a whole
        // round ahead change it under a slower wave's eyes: the block then disagreed about draining, once in ten million rounds,
        // and a block-full of the list was judged twice while another was lost -- tools/flag_diff.py.  half_n is handled the same
        // way: written by wave_append and, in drain(), by thread 0 behind a barrier; read only into half_seen inside append().)
        const u32 dn = defer_seen, hn = half_seen;
        // one block-full (or, at the end of the input, the rest) of a list: whole units, or single halves
        auto drain = [&](const u32 *list, const unsigned char *kind, u32 *list_n, u32 n, bool halves) __attribute__((always_inline)) {
            const u32 take = n < kFilterThreads ? n : kFilterThreads;
            const u32 at = n - take;
            const bool active2 = threadIdx.x < take;
            const u32 unit2 = active2 ? list[at + threadIdx.x] : 0u;
            const u32 kind2 = active2 ? kind[at + threadIdx.x] : 0u;
            const bool n2 = (kind2 & 1u) != 0;
            __syncthreads();
            if (threadIdx.x == 0) {
                *list_n = at;
                if (halves || uni_drain) atomicAdd(&g_fallback[halves ? kFallbackHalfDrain : kFallbackUnitDrain], take);
            }
#if !defined(TREW_AB_SKIP_DRAIN) && !defined(TREW_AB_SKIP_UNIT_DRAIN)
            const u64 any2 = halves      ? (u64) filter_deferred_half(P, B, unit2, kind2 >> 1, active2, geom, round, cnt_thr)
                             : uni_drain ? (u64) filter_deferred_uni(P, B, unit2, active2, geom, round, cnt_thr)
                                         : general(unit2, active2);
#else  // A/B builds (instruction attribution): the drain computes nothing and its inputs are kept alive -- both drains with
       // TREW_AB_SKIP_DRAIN (profiles/r05), the whole-unit drain alone with TREW_AB_SKIP_UNIT_DRAIN (profiles/read_setup)
#ifdef TREW_AB_SKIP_DRAIN
            constexpr bool kSkipHalves = true;
#else
            constexpr bool kSkipHalves = false;
#endif
            u64 any2 = 0;
            if (halves && !kSkipHalves) {
                any2 = (u64) filter_deferred_half(P, B, unit2, kind2 >> 1, active2, geom, round, cnt_thr);
            } else {
                u32 keep = unit2 + kind2;
                asm volatile("" : "+v"(keep), "+v"(any2));
                (void) keep;
            }
#endif
            // The reads with an N go to the worklist behind the others of this block-full, next to each other: the exact kernel
            // decides two consecutive reads of the worklist in one pass and runs the N variant of its bounds when either holds
            // an N (mixed at random, 12 % of its passes did; exact kernel 0.408 against 0.399 ms with the same reads).
            append(active2 && any2 != 0 && !n2, unit2);
            append(active2 && any2 != 0 && n2, unit2);
        };
        const bool drain_units = dn >= kFilterThreads || (!more && dn > 0u), drain_halves = NW == 3 && (hn >= kFilterThreads || (!more && hn > 0u));
        if (drain_units || drain_halves) {
            if (drain_units) drain(defer, defer_kind, &defer_n, dn, false);
            if constexpr (NW == 3) {
                if (drain_halves) drain(hdefer, hdefer_kind, &half_n, hn, true);
            }
        } else if (!more) {
            break;
        }
    }
    flush();
}
