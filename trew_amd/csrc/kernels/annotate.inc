// kernels/annotate.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Per-read annotation against given motifs (trew_hip_annotate): for every read and motif, on each strand, the number of
// windows of k bases that are a rotation of the motif and the longest uninterrupted run of such windows.  A kernel beside
// the scan: it reads the same bit planes, writes only its own result buffer, touches neither tables nor worklists.
//
// Formulation (both kernels).  Let T be the strand's target (the motif, or its reverse complement) and P_q the endless
// string of period k with P_q[i] = T[(i + q) mod k].  Window i is a rotation of T exactly when its k bases agree with P_q for
// some q, i.e. when the mismatch mask (lo ^ Plo_q) | (hi ^ Phi_q) | nmask has k zero bits from bit i on.  The first 32 bits
// of P_q are one {lo, hi} pair of words per q (AnnotMotifDev, built on the host); the words of P_q that follow are those of
// P_(q + 32) mod k, so every pattern word is a wave-uniform table entry (scalar loads).  OR over the k phases gives `match`.
// Bits at and past the end of the read count as mismatches, so no window reaches over the end.
// The longest run of ones in `match` comes from eroding by doubling: E_L = starts of runs of at least L ones,
// E_2L = E_L & (E_L >> L), then the length is put together from its binary digits, highest first:
// E_(S + L) = E_S & (E_L >> S).  The first set bit of the last non-empty E is the earliest longest run.

// `a >> S` for a mask of NW words, word j of the result; S is a compile-time constant
template <int S, int NW>
__device__ __forceinline__ u32 annot_shr(const u32 (&a)[NW], int j) {
    constexpr int ws = S >> 5, bs = S & 31;
    const u32 l = j + ws < NW ? a[j + ws] : 0u;
    const u32 h = j + ws + 1 < NW ? a[j + ws + 1] : 0u;
    return bs ? alignbit(h, l, (u32) bs) : l;
}

// one level of the refinement: is there a run of len + S windows?
template <int S, int NW>
__device__ __forceinline__ void annot_refine(const u32 (&lev)[NW], u32 (&cur)[NW], u32 &len) {
    u32 t[NW], any = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        t[j] = lev[j] & annot_shr<S, NW>(cur, j);
        any |= t[j];
    }
    if (any) {
#pragma unroll
        for (int j = 0; j < NW; j++) cur[j] = t[j];
        len += (u32) S;
    }
}

// match mask of one strand of one motif: windows whose k bases are a rotation of the target
template <int NW>
__device__ __forceinline__ void annot_match(const u32 (&lo)[NW], const u32 (&hi)[NW], const u32 (&nm)[NW], const AnnotMotifDev *mt, int strand, u32 k,
                                            u32 (&match)[NW]) {
#pragma unroll
    for (int j = 0; j < NW; j++) match[j] = 0;
    const u32 step = 32u % k;
    for (u32 q = 0; q < k; q++) {
        u32 z[NW];
        u32 qi = q;  // phase of word j: (q + 32 j) mod k
#pragma unroll
        for (int j = 0; j < NW; j++) {
            z[j] = ~((lo[j] ^ mt->plo[strand][qi]) | (hi[j] ^ mt->phi[strand][qi]) | nm[j]);
            qi += step;
            qi = qi >= k ? qi - k : qi;
        }
        // starts of k ones in a row: double the run length while it fits, then one last step of k - L <= L
        u32 L = 1;
        for (; 2 * L <= k; L *= 2) {
#pragma unroll
            for (int j = 0; j < NW; j++) z[j] &= alignbit(j + 1 < NW ? z[j + 1] : 0u, z[j], L);  // L <= 16
        }
        if (L < k) {
            const u32 sh = k - L;  // 1 .. 15
#pragma unroll
            for (int j = 0; j < NW; j++) z[j] &= alignbit(j + 1 < NW ? z[j + 1] : 0u, z[j], sh);
        }
#pragma unroll
        for (int j = 0; j < NW; j++) match[j] |= z[j];
    }
}

// windows, start and length (in windows) of the earliest longest run of a match mask of at most 32 NW - 2 bits
template <int NW>
__device__ __forceinline__ void annot_longest(const u32 (&match)[NW], u32 &windows, u32 &start, u32 &len) {
    static_assert(NW <= 8, "eight levels cover runs of up to 255 windows");
    windows = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) windows = bcnt_acc(match[j], windows);
    u32 cur[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) cur[j] = match[j];
    len = windows ? 1u : 0u;
    // most waves hold no read with two matching windows: their answer is already there
    if (__builtin_amdgcn_ballot_w64(windows >= 2u)) {
        u32 l1[NW], l2[NW], l3[NW], l4[NW], l5[NW], l6[NW], l7[NW];
#pragma unroll
        for (int j = 0; j < NW; j++) l1[j] = match[j] & annot_shr<1, NW>(match, j);
#pragma unroll
        for (int j = 0; j < NW; j++) l2[j] = l1[j] & annot_shr<2, NW>(l1, j);
#pragma unroll
        for (int j = 0; j < NW; j++) l3[j] = l2[j] & annot_shr<4, NW>(l2, j);
#pragma unroll
        for (int j = 0; j < NW; j++) l4[j] = l3[j] & annot_shr<8, NW>(l3, j);
#pragma unroll
        for (int j = 0; j < NW; j++) l5[j] = l4[j] & annot_shr<16, NW>(l4, j);
#pragma unroll
        for (int j = 0; j < NW; j++) l6[j] = l5[j] & annot_shr<32, NW>(l5, j);
#pragma unroll
        for (int j = 0; j < NW; j++) l7[j] = l6[j] & annot_shr<64, NW>(l6, j);
        // E_0 = every position.  Starting from all ones loses nothing although the shift moves zeros in at the top: a run of S
        // windows starts at or below bit 32 NW - 2 - S, because the last two bits of a match mask are never set (k >= 3).
#pragma unroll
        for (int j = 0; j < NW; j++) cur[j] = 0xffffffffu;
        len = 0;
        annot_refine<128, NW>(l7, cur, len);
        annot_refine<64, NW>(l6, cur, len);
        annot_refine<32, NW>(l5, cur, len);
        annot_refine<16, NW>(l4, cur, len);
        annot_refine<8, NW>(l3, cur, len);
        annot_refine<4, NW>(l2, cur, len);
        annot_refine<2, NW>(l1, cur, len);
        annot_refine<1, NW>(match, cur, len);
    }
    start = 0;
#pragma unroll
    for (int j = NW - 1; j >= 0; j--)
        if (cur[j]) start = 32u * (u32) j + (u32) __builtin_ctz(cur[j]);
    if (len == 0) start = 0;
}

// ---- lane per read: reads of at most 32 NW bases, planes in registers, no LDS, no cross-lane traffic
template <int NW>
__global__ void __launch_bounds__(256) annotate_lane_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, uint2 *__restrict__ out) {
    const u64 r = (u64) blockIdx.x * 256ull + threadIdx.x;
    const bool live = r < B.n_reads;
    ReadRef rd;
    rd.w = B.words;
    rd.len = 0;
    rd.nw = 0;
    if (live) rd = get_read(B, r);
    // the host picks NW from the longest read; a read longer than that (a wrong max_length hint) is cut, never read past
    rd.len = min(rd.len, 32u * (u32) NW);
    rd.nw = min(rd.nw, (u32) NW);
    u32 lo[NW], hi[NW], nm[NW];
    load_planes<NW>(rd, 0, lo, hi, nm);
#pragma unroll
    for (int j = 0; j < NW; j++) {  // bits at and past the end of the read never match
        const int left = (int) rd.len - 32 * j;
        nm[j] |= left <= 0 ? 0xffffffffu : left >= 32 ? 0u : 0xffffffffu << left;
    }
    for (int m = 0; m < n_motifs; m++) {
        const AnnotMotifDev *mm = mt + m;
        const u32 k = mm->k;
        u32 match[NW], wf, sf, lf, wr, sr, lr;
        annot_match<NW>(lo, hi, nm, mm, 0, k, match);
        annot_longest<NW>(match, wf, sf, lf);
        annot_match<NW>(lo, hi, nm, mm, 1, k, match);
        annot_longest<NW>(match, wr, sr, lr);
        if (live) {
            uint2 *o = out + (r * (u64) n_motifs + (u64) m) * 3ull;  // trew_hip_annot: six u32
            o[0] = make_uint2(wf, wr);
            o[1] = make_uint2(sf, lf ? lf + k - 1u : 0u);
            o[2] = make_uint2(sr, lr ? lr + k - 1u : 0u);
        }
    }
}

// ---- wave per read: any length.  Lane l takes 32-base word 64 t + l in iteration t, with the next word as look-ahead
// (k - 1 <= 31 bases).  Runs are joined across lanes from {ones at the low end, ones at the high end, all ones} of every
// lane's match word; the run still open at the end of an iteration is carried into the next.
struct AnnotRun {
    u32 len, start;
};
// earliest longest run of ones inside one 32-bit word
__device__ __forceinline__ AnnotRun annot_word_run(u32 m) {
    const u32 e1 = m & (m >> 1), e2 = e1 & (e1 >> 2), e3 = e2 & (e2 >> 4), e4 = e3 & (e3 >> 8), e5 = e4 & (e4 >> 16);
    u32 cur = m, len = m ? 1u : 0u;
    if (e1) {
        len = 0;
        u32 t;
        if (e5) { cur = e5; len = 32; }
        t = len ? e4 & (cur >> 16) : e4; if (t) { cur = t; len += 16; }
        t = len ? e3 & (cur >> 8) : e3; if (t) { cur = t; len += 8; }
        t = len ? e2 & (cur >> 4) : e2; if (t) { cur = t; len += 4; }
        t = len ? e1 & (cur >> 2) : e1; if (t) { cur = t; len += 2; }
        t = len ? m & (cur >> 1) : m; if (t) { cur = t; len += 1; }
    }
    AnnotRun r;
    r.len = len;
    r.start = len ? (u32) __builtin_ctz(cur) : 0u;
    return r;
}
// longer run first, earlier start on a tie: one u64 whose maximum is the answer
__device__ __forceinline__ u64 annot_key(u32 len, u32 start) { return ((u64) len << 32) | (u64) (0xffffffffu - start); }

// match word of 32-base word w of a read, one strand of one motif: bit i = window 32 w + i is a rotation of the target.  The
// next word is the look-ahead (k - 1 <= 31 bases); a word at or past the end of the read has no match.  Shared with
// kernels/tracts.inc, so the k-phase match exists once.
__device__ __forceinline__ u32 annot_wave_match(const ReadRef &rd, const AnnotMotifDev *mm, int strand, u32 k, u32 w) {
    const u32 step = 32u % k;
    u32 c0 = 0, c1 = 0, c2 = 0xffffffffu, n0 = 0, n1 = 0, n2 = 0xffffffffu;
    if (w < rd.nw) {
        c0 = rd.w[3ull * w + 0];
        c1 = rd.w[3ull * w + 1];
        c2 = rd.w[3ull * w + 2];
        const long long left = (long long) rd.len - 32ll * (long long) w;  // >= 1
        if (left < 32) c2 |= 0xffffffffu << (u32) left;
    }
    if (w + 1u < rd.nw) {
        n0 = rd.w[3ull * (w + 1u) + 0];
        n1 = rd.w[3ull * (w + 1u) + 1];
        n2 = rd.w[3ull * (w + 1u) + 2];
        const long long left = (long long) rd.len - 32ll * (long long) (w + 1u);
        if (left < 32) n2 |= 0xffffffffu << (u32) left;
    }
    u32 m = 0;
    for (u32 q = 0; q < k; q++) {
        u32 q1 = q + step;
        q1 = q1 >= k ? q1 - k : q1;
        const u32 z0 = ~((c0 ^ mm->plo[strand][q]) | (c1 ^ mm->phi[strand][q]) | c2);
        const u32 z1 = ~((n0 ^ mm->plo[strand][q1]) | (n1 ^ mm->phi[strand][q1]) | n2);
        u64 z = ((u64) z1 << 32) | z0;  // window i <= 31 needs bits i .. i + k - 1 <= 62
        u32 L = 1;
        for (; 2 * L <= k; L *= 2) z &= z >> L;
        if (L < k) z &= z >> (k - L);
        m |= (u32) z;
    }
    return m;
}

__device__ __forceinline__ void annot_wave_strand(const ReadRef &rd, const AnnotMotifDev *mm, int strand, u32 k, u32 &windows, u32 &start, u32 &len) {
    const u32 lane = lane_id();
    u32 wsum = 0;
    u64 best = 0;
    u32 carry_len = 0, carry_start = 0;  // wave-uniform: the run of ones that ends with the previous iteration's last bit
    for (u32 t0 = 0; t0 < rd.nw; t0 += 64u) {
        const u32 w = t0 + lane;
        const u32 m = annot_wave_match(rd, mm, strand, k, w);
        wsum = bcnt_acc(m, wsum);
        // this lane's word: ones at its low end, ones at its high end, the best run inside
        const bool full = m == 0xffffffffu;
        const u32 pre = full ? 32u : (u32) __builtin_ctz(~m);
        const u32 suf = full ? 32u : (u32) __builtin_clz(~m);
        const u32 base = w << 5;
        const AnnotRun in = annot_word_run(m);
        if (in.len) best = max(best, annot_key(in.len, base + in.start));
        // the run that ends with the last bit of lane - 1: c full lanes below this one, under them the high end of lane a
        // (or, with a = -1, what the previous iteration left open)
        const u64 fm = __builtin_amdgcn_ballot_w64(full);
        u32 c = 0;
        if (lane) {
            const u64 nb = ~(fm << (64u - lane));  // bit 63 = lane - 1; the low 64 - lane bits are ones
            c = (u32) __builtin_clzll(nb);
        }
        const int a = (int) lane - 1 - (int) c;
        const u32 suf_a = (u32) __shfl((int) suf, a < 0 ? 0 : a, 64);
        const u32 in_len = 32u * c + (a >= 0 ? suf_a : carry_len);
        const u32 in_start = a >= 0 ? ((t0 + (u32) a + 1u) << 5) - suf_a : (carry_len ? carry_start : t0 << 5);
        if (!full && in_len + pre) best = max(best, annot_key(in_len + pre, in_len ? in_start : base));
        // what lane 63 leaves open
        const u32 out_len = full ? in_len + 32u : suf;
        const u32 out_start = full ? (in_len ? in_start : base) : base + 32u - suf;
        carry_len = (u32) __builtin_amdgcn_readlane((int) out_len, 63);
        carry_start = (u32) __builtin_amdgcn_readlane((int) out_start, 63);
    }
    // the last word of a read ends in at least one zero bit (window n - 1 does not exist), so no run is left open here
    windows = wave_sum_u32(wsum);
    const u32 blen = wave_max_u32((u32) (best >> 32));
    const u32 inv = wave_max_u32((u32) (best >> 32) == blen ? (u32) best : 0u);
    len = blen;
    start = blen ? 0xffffffffu - inv : 0u;
}

__global__ void __launch_bounds__(256) annotate_wave_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, u32 *__restrict__ out) {
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_motifs; m++) {
            const AnnotMotifDev *mm = mt + m;
            const u32 k = mm->k;
            u32 wf, sf, lf, wr, sr, lr;
            annot_wave_strand(rd, mm, 0, k, wf, sf, lf);
            annot_wave_strand(rd, mm, 1, k, wr, sr, lr);
            // six lanes write the record's six words: one vector store
            const u32 lane = lane_id();
            const u32 tf = lf ? lf + k - 1u : 0u, tr = lr ? lr + k - 1u : 0u;
            const u32 v = lane == 0 ? wf : lane == 1 ? wr : lane == 2 ? sf : lane == 3 ? tf : lane == 4 ? sr : tr;
            if (lane < 6) out[(r * (u64) n_motifs + (u64) m) * 6ull + lane] = v;
        }
    }
}
