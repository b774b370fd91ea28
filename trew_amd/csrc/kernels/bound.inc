// kernels/bound.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// The parity-bucket bound, written once: the prefilter flags reads with it (prefilter.inc) and the exact kernel prunes k with it
// (lane_bounds_at in exact_core.inc, bound_at_k in decide_group.inc).  The prefilter never drops a k only as long as every user
// computes the same thing, so the building blocks live here and nowhere else.
//
// Soundness: windows of one rotation class (kmer.cpp:1815-1823) have the same base composition, hence the same (#lo-bit, #hi-bit,
// #A) parities.  With P_b the exclusive prefix parity of feature b, the parity of window i at length k is P_b[i] ^ P_b[i+k]; so the
// size of every parity bucket is one popcount and the largest bucket is an upper bound of K_MER_DATA_MAX (kmer.cpp:2202).

// ------------------------------------------------------------------ parity-bucket bound

// the `bits` lowest bits of a word.  POS: the caller knows bits > 0 (the word holds a base of its segment)
template <bool POS = false>
__device__ __forceinline__ u32 low_mask(int bits) {
    return bits >= 32 ? 0xffffffffu : ((!POS && bits <= 0) ? 0u : ((1u << bits) - 1u));
}

// inclusive prefix parity inside one word: bit i = parity of x's bits 0..i
__device__ __forceinline__ u32 word_parity(u32 x) {
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    return x;
}

// exclusive prefix parity of f over bits 0..32*NW-1: P[i] = XOR_{t<i} f[t]
template <int NW>
__device__ __forceinline__ void prefix_parity(const u32 (&f)[NW], u32 (&P)[NW]) {
    u32 carry = 0, prev_top = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const u32 x = word_parity(f[j]) ^ carry;  // carry = all-ones when the parity of all lower words is odd
        P[j] = (x << 1) | prev_top;
        prev_top = x >> 31;
        carry = 0u - prev_top;
    }
}

// the same for 3 words with the first two as one 64-bit value: six 64-bit shift + xor steps instead of ten 32-bit ones
// (v_lshlrev_b64 costs what a 32-bit shift costs, tools/valu_rate.hip)
template <>
__device__ __forceinline__ void prefix_parity<3>(const u32 (&f)[3], u32 (&P)[3]) {
    u64 x = ((u64) f[1] << 32) | f[0];
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    x ^= x << 32;  // bit i = parity of f bits 0..i
    u32 y = word_parity(f[2]);
    const u32 top = (u32) (x >> 63);
    y ^= 0u - top;  // the parity of the 64 lower bits carries into every bit of the third word
    const u64 e = x << 1;  // exclusive prefix of the first two words
    P[0] = (u32) e;
    P[1] = (u32) (e >> 32);
    P[2] = (y << 1) | top;
}

// and for 5 words (a whole read of up to 160 bases; P at bits 0 .. 159 -- the parity of all 160 bases has no bit here) as two
// 64-bit pairs and one word, the carry chained from each into the next.
// A function of its own, not the specialisation prefix_parity<5>: that one would also be picked up by the 5-word kernels
// (segment_setup<5>, filter_segment<5>), which are to stay as they are.
__device__ __forceinline__ void prefix_parity_read5(const u32 (&f)[5], u32 (&P)[5]) {
    u64 x = ((u64) f[1] << 32) | f[0], y = ((u64) f[3] << 32) | f[2];
    x ^= x << 1, y ^= y << 1;
    x ^= x << 2, y ^= y << 2;
    x ^= x << 4, y ^= y << 4;
    x ^= x << 8, y ^= y << 8;
    x ^= x << 16, y ^= y << 16;
    x ^= x << 32, y ^= y << 32;  // bit i = parity of the pair's own bits 0..i
    u32 z = word_parity(f[4]);
    const u32 topx = (u32) (x >> 63);
    y ^= 0ull - (u64) topx;  // the parity of words 0..1 carries into every bit of words 2..3
    const u32 topy = (u32) (y >> 63);
    z ^= 0u - topy;  // and that of words 0..3 into word 4
    const u64 ex = x << 1, ey = (y << 1) | topx;
    P[0] = (u32) ex;
    P[1] = (u32) (ex >> 32);
    P[2] = (u32) ey;
    P[3] = (u32) (ey >> 32);
    P[4] = (z << 1) | topy;
}

// the segment [0, L) of the planes holds an N (or another non-ACGT byte): non-zero if so
template <int NW>
__device__ __forceinline__ u32 segment_has_n(const u32 (&nm)[NW], int L) {
    u32 anyn = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) anyn |= nm[j] & low_mask(L - 32 * j);
    return anyn;
}

// Set-up of one segment: lo/hi/nm hold its planes from bit 0, L <= 32*NW-1 bases.  The features are lo, hi and lo & hi (A) inside
// the segment; P1, P2, P3 are their exclusive prefix parities.
//   MASK_N   the features are cleared where the base is an N, and v1 = valid bases (A/C/G/T and inside the segment) is written.
//            Users that never look at a window with an N (the uniform path sets such reads aside, the drain masks every parity
//            word by V_k) leave it out: one AND per word less.
//   WANT_V1  v1 is written although the features are not masked (the drain's V_1)
//   WANT_P3  the third parity (the halves loop decides on four buckets and wants none)
// Outputs that are not wanted are left untouched: pass any array.
template <int NW, bool MASK_N, bool WANT_P3 = true, bool WANT_V1 = MASK_N>
__device__ __forceinline__ void segment_setup(const u32 (&lo)[NW], const u32 (&hi)[NW], const u32 (&nm)[NW], int L, u32 (&v1)[NW],
                                              u32 (&P1)[NW], u32 (&P2)[NW], u32 (&P3)[NW]) {
    static_assert(WANT_V1 || !MASK_N, "masked features come with their mask");
    u32 f1[NW], f2[NW], f3[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const u32 lm = low_mask(L - 32 * j);
        const u32 v = ~nm[j] & lm;  // base is A/C/G/T and inside the segment
        if (WANT_V1) v1[j] = v;
        f1[j] = lo[j] & (MASK_N ? v : lm);
        f2[j] = hi[j] & (MASK_N ? v : lm);
        f3[j] = f1[j] & f2[j];
    }
    prefix_parity<NW>(f1, P1);
    prefix_parity<NW>(f2, P2);
    if (WANT_P3) prefix_parity<NW>(f3, P3);
}

// per-lane variable right shift of a multiword mask by off in [0, 63]
template <int NW>
__device__ __forceinline__ u32 shr_var_word(const u32 (&x)[NW], int j, u32 off) {
    const bool big = off >= 32u;
    const u32 x0 = x[j], x1 = j + 1 < NW ? x[j + 1 < NW ? j + 1 : 0] : 0u, x2 = j + 2 < NW ? x[j + 2 < NW ? j + 2 : 0] : 0u;
    return alignbit(big ? x2 : x1, big ? x1 : x0, off & 31u);
}

// V_k of a segment of L bases, k < 64: bit i = window i has no N and fits the segment (kmer.cpp:2190), from v1 = its valid bases.
// has_n must be uniform over the lanes that share the segment.  bmax: the powers of two above it are known not to occur in k.
template <int NW>
__device__ __forceinline__ void windows_without_n(const u32 (&v1)[NW], bool has_n, int L, int k, int bmax, u32 (&V)[NW]) {
    if (!has_n) {
        // no N in the segment: V_k = the L-k+1 lowest bits
        const int wbits = L - k + 1;
#pragma unroll
        for (int j = 0; j < NW; j++) V[j] = low_mask(wbits - 32 * j);
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
            if (b <= bmax) {  // wave-uniform
                const bool take = ((u32) k & (u32) b) != 0;
#pragma unroll
                for (int j = 0; j < NW; j++) {
                    const u32 sh = shr_var_word<NW>(A, j, off);
                    V[j] &= take ? sh : 0xffffffffu;
                }
                off += take ? (u32) b : 0u;
            }
        }
    }
}

// The 8-bucket split of one k, a word of windows at a time: F1, F2, F3 = window parities of the three features
// (P_b ^ (P_b >> k)), v = the windows that count; the largest bucket is an upper bound of MAX.  One body, so that every user
// splits alike; the flags only say what the caller already has:
//   MASKED   F1 and F2 hold no bit outside v (the uniform loops and the drain mask them while building them), so the four
//            two-parity classes need no v; otherwise they are peeled off v one parity at a time
//   COUNTED  the caller knows COUNT = popc(V), and bucket 000 is what the other seven leave of it (v_bcnt is a slow instruction,
//            tools/valu_rate.hip); otherwise bucket 000 is counted like the others and so is COUNT
template <bool MASKED, bool COUNTED>
struct Buckets8 {
    u32 c000 = 0, c001 = 0, c010 = 0, c011 = 0, c100 = 0, c101 = 0, c110 = 0, c111 = 0, count = 0;
    __device__ __forceinline__ void add(u32 F1, u32 F2, u32 F3, u32 v) {
        u32 a11, a10, a01, a00;
        if (MASKED) {
            a11 = F1 & F2, a10 = F1 & ~F2, a01 = ~F1 & F2, a00 = v & ~(F1 | F2);
        } else {
            const u32 a1 = v & F1, a0 = v ^ a1;
            a11 = a1 & F2, a10 = a1 ^ a11, a01 = a0 & F2, a00 = a0 ^ a01;
        }
        const u32 b111 = a11 & F3, b101 = a10 & F3, b011 = a01 & F3, b001 = a00 & F3;
        if (!COUNTED) count += __popc(v);
        c111 += __popc(b111);
        c110 += __popc(a11 ^ b111);
        c101 += __popc(b101);
        c100 += __popc(a10 ^ b101);
        c011 += __popc(b011);
        c010 += __popc(a01 ^ b011);
        c001 += __popc(b001);
        if (!COUNTED) c000 += __popc(a00 ^ b001);
    }
    // the largest bucket; COUNTED: of `known` = COUNT windows
    __device__ __forceinline__ u32 largest(u32 known = 0) {
        if (COUNTED) c000 = known - c001 - c010 - c011 - c100 - c101 - c110 - c111;
        return max(max(max(c000, c001), max(c010, c011)), max(max(c100, c101), max(c110, c111)));
    }
};
// the masked form over whole word arrays: F1 and F2 masked, V = the windows, count = COUNT
template <int N>
__device__ __forceinline__ u32 max_bucket8(const u32 (&F1)[N], const u32 (&F2)[N], const u32 (&F3)[N], const u32 (&V)[N], u32 count) {
    Buckets8<true, true> b;
#pragma unroll
    for (int j = 0; j < N; j++) b.add(F1[j], F2[j], F3[j], V[j]);
    return b.largest(count);
}

// valid windows i, i+1 that share a class (E: bases i and i+k agree): COUNT minus this is the number of runs of adjacent
// same-class windows (Lemma A)
template <int NW>
__device__ __forceinline__ u32 class_links(const u32 (&V)[NW], const u32 (&E)[NW]) {
    u32 links = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const u32 vn = j + 1 < NW ? V[j + 1 < NW ? j + 1 : 0] : 0u;
        links += __popc(V[j] & E[j] & alignbit(vn, V[j], 1u));
    }
    return links;
}

// ------------------------------------------------------------------ the fourth invariant: adjacent equal bases
// The number of cyclically adjacent equal bases of a k-mer (base t == base t+1, and base k-1 == base 0) is the same for every
// rotation of it, so its parity is one more feature that is constant on a rotation class: it splits each of the eight parity
// buckets in two.  For window i at length k the parity is PD[i] ^ PD[i+k-1] ^ [base i == base i+k-1], with PD the exclusive prefix
// parity of D[t] = [base t == base t+1] over valid neighbours.  A window that counts has no N, so every adjacent pair inside it
// is a valid one and D says the truth about it; windows with an N are in no bucket, as in the 8-bucket split.
// Only the bounds pass uses it (bounds_pass.inc): inline in the prefilter it cost the fast loop its registers.

// PD of a segment: lo / hi = its planes from bit 0, v1 = its valid bases (segment_setup)
template <int NW>
__device__ __forceinline__ void adjacency_parity(const u32 (&lo)[NW], const u32 (&hi)[NW], const u32 (&v1)[NW], u32 (&PD)[NW]) {
    u32 D[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const int jn = j + 1 < NW ? j + 1 : 0;
        const u32 nlo = alignbit(j + 1 < NW ? lo[jn] : 0u, lo[j], 1u), nhi = alignbit(j + 1 < NW ? hi[jn] : 0u, hi[j], 1u);
        const u32 nv = alignbit(j + 1 < NW ? v1[jn] : 0u, v1[j], 1u);
        D[j] = ~((lo[j] ^ nlo) | (hi[j] ^ nhi)) & v1[j] & nv;
    }
    prefix_parity<NW>(D, PD);
}

// word j of the feature at length k, s = k - 1 in [0, 31] (wave-uniform); bits outside the windows that count are not defined
template <int NW>
__device__ __forceinline__ u32 adjacency_feature_word(const u32 (&PD)[NW], const u32 (&lo)[NW], const u32 (&hi)[NW], int j, u32 s) {
    const int jn = j + 1 < NW ? j + 1 : 0;
    const u32 pd = alignbit(j + 1 < NW ? PD[jn] : 0u, PD[j], s);
    const u32 sl = alignbit(j + 1 < NW ? lo[jn] : 0u, lo[j], s), sh = alignbit(j + 1 < NW ? hi[jn] : 0u, hi[j], s);
    return PD[j] ^ pd ^ ~((lo[j] ^ sl) | (hi[j] ^ sh));
}

// The 16-bucket split of one k: Buckets8's masked form (F1, F2 hold no bit outside V) with every bucket split once more by F4.
// The largest of the sixteen is at most the largest of the eight, and still an upper bound of MAX.  Written plainly, a popcount
// a bucket: its only caller runs it where a half with an N passed on eight buckets, which is rare.
template <int N>
__device__ __forceinline__ u32 max_bucket16(const u32 (&F1)[N], const u32 (&F2)[N], const u32 (&F3)[N], const u32 (&F4)[N], const u32 (&V)[N]) {
    u32 c[16];
#pragma unroll
    for (int b = 0; b < 16; b++) c[b] = 0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const u32 a[4] = {V[j] & ~(F1[j] | F2[j]), ~F1[j] & F2[j], F1[j] & ~F2[j], F1[j] & F2[j]};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const u32 b1 = a[q] & F3[j], b0 = a[q] ^ b1;
            const u32 d11 = b1 & F4[j], d01 = b0 & F4[j];
            c[4 * q + 0] += __popc(b0 ^ d01);
            c[4 * q + 1] += __popc(d01);
            c[4 * q + 2] += __popc(b1 ^ d11);
            c[4 * q + 3] += __popc(d11);
        }
    }
    u32 m = 0;
#pragma unroll
    for (int b = 0; b < 16; b++) m = max(m, c[b]);
    return m;
}
