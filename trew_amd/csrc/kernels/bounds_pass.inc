// kernels/bounds_pass.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// bounds_kernel<3>: the packed bounds of every (half, k) of the flagged short reads, a LANE per half and a wave-uniform k loop,
// between the prefilter and the exact kernel.
//
// The group pass of the exact kernel wants, per half and per k of the run, the word bound_at_k (decide_group.inc) packs: maxbucket,
// COUNT, runs, the two pass bits, has_n.  In its row layout every lane bounds a k of its own: shift amounts per lane, V_k rebuilt
// by binary decomposition, eight popcounts of their own, three words carried through every k -- about 5.4 wave-instructions per
// (segment, k).  The prefilter's drains (drain_probe3 / drain_probe2, prefilter.inc) compute the same 8-bucket split in the other
// layout, where a wave bounds 64 halves at one k: shifts by a scalar, V_{k+1} = V_k & (V_k >> 1), one 64-bit container shift per
// mask once at most 64 windows are left.  This kernel is that loop with the full bound at its end, over the first bnd_cap entries
// of the worklist (the host never learns its length: the lanes stride over wl_count[0]); the exact kernel reads the words back
// where they exist (run_short_group) and bounds in row layout where they do not.
//
// Every quantity is built from bound.inc's blocks (segment_setup, Buckets8, class_links), so the bound is still written once;
// only the tail that turns (m8, COUNT, links) into the packed word is repeated here (pack_bound_word), see there.
//
// Output: bnd[(worklist position * 2 + half) * 32 + k - MIN_MER].  The 64 lanes of a wave own 64 consecutive rows of 32 words; they
// are transposed through LDS so that the wave writes whole 256-byte lines.

// (kBoundWords, kBoundItemWords: decide_group.inc, beside the code that reads the words back)
constexpr u32 kBoundsTileStride = kBoundWords + 1;  // LDS row stride of the transposition (odd: no bank conflicts either way)

// The tail of bound_at_k (decide_group.inc), from "m8 / COUNT >= baseline" on, word for word: the reference's doubles decide the
// pass bits (a multiplication, and the IEEE division itself within rounding distance of a threshold).  Repeated and not shared
// because bound_at_k compiles into every exact kernel and those keep their registers only as long as its source is untouched
// (profiles/bound_refactor/README.md).  A change of either copy is a change of both.
__device__ __forceinline__ u32 pack_bound_word(u32 m8, u32 count, u32 links, u32 has_n, int k, int gmax, const DevParams &P) {
    const u32 runs = count - links < 127u ? count - links : 127u;
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
    return inr ? (m8 | (count << 10) | (runs << 20) | (pass_lo << 27) | (pass_hi << 28) | (has_n << 29)) : (has_n << 29);
}

template <int NW>
__global__ __launch_bounds__(64) void bounds_kernel(DevParams P, DevBatch B, const u32 *__restrict__ wl, const u32 *__restrict__ wl_count, u32 wl_cap,
                                                    u32 *__restrict__ bnd, u32 bnd_cap) {
    static_assert(NW == 3, "the k loop is written for three words: halves of at most 95 bases");
    __shared__ u32 tile[64 * kBoundsTileStride];
    const u32 lane = lane_id();
    u32 n = wl_count[0];
    n = n < wl_cap ? n : wl_cap;
    n = n < bnd_cap ? n : bnd_cap;
    const u64 total = 2ull * n;  // halves
    const int klo = P.min_mer, khi = P.max_mer < P.min_mer + (int) kBoundWords - 1 ? P.max_mer : P.min_mer + (int) kBoundWords - 1;
    for (u64 base = (u64) blockIdx.x * 64u; base < total; base += (u64) gridDim.x * 64u) {
        const u64 idx = base + lane;
        const bool active = idx < total;
        const u32 half = (u32) idx & 1u;
        ReadRef rd;
        rd.w = B.words;
        rd.len = rd.nw = 0;
        if (active) rd = get_read(B, wl[idx >> 1]);
        const Segment sg = get_segment(TREW_MODE_SHORT, (int) half, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
        // a read the group pass does not take (too short for halves) or a half the three words cannot hold: the lane has no
        // window at any k and its words are never read
        const bool can = active && sg.valid && sg.len <= 32u * NW - 1u;
        if (!can) rd.nw = 0;  // (no plane is loaded)
        const int L = can ? (int) sg.len : 0;
        u32 lo[3], hi[3], nm[3], V[3], P1[3], P2[3], P3[3];
        load_planes<3>(rd, sg.start, lo, hi, nm);
        segment_setup<3, false, true, true>(lo, hi, nm, L, V, P1, P2, P3);  // V_1 and the three prefix parities, as drain_half_init
        const u32 has_n = segment_has_n<3>(nm, L) != 0u ? 1u : 0u;
        for (int t = 1; t < klo; t++) drain_v_step3(V);  // V_klo
        const int Lmax = (int) wave_max_u32((u32) L);
        u32 *const row = tile + lane * kBoundsTileStride;
        int k = klo;
        // (b) k with more than 64 windows in some half of the wave (k <= Lmax - 64 <= 31): three words, funnel shifts by a scalar
        for (const int b = khi < Lmax - 64 ? khi : Lmax - 64; k <= b; k++) {
            const u32 bs = (u32) k;
            u32 F1[3], F2[3], F3[3], E[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int jn = j < 2 ? j + 1 : 0;
                F1[j] = xor_and(P1[j], alignbit(j < 2 ? P1[jn] : 0u, P1[j], bs), V[j]);
                F2[j] = xor_and(P2[j], alignbit(j < 2 ? P2[jn] : 0u, P2[j], bs), V[j]);
                F3[j] = P3[j] ^ alignbit(j < 2 ? P3[jn] : 0u, P3[j], bs);
                E[j] = ~((lo[j] ^ alignbit(j < 2 ? lo[jn] : 0u, lo[j], bs)) | (hi[j] ^ alignbit(j < 2 ? hi[jn] : 0u, hi[j], bs)));
            }
            const u32 count = bcnt_acc(V[2], bcnt_acc(V[1], __popc(V[0])));
            const u32 m8 = max_bucket8<3>(F1, F2, F3, V, count);
            row[k - klo] = pack_bound_word(m8, count, class_links<3>(V, E), has_n, k, P.max_mer, P);
            drain_v_step3(V);
        }
        // (c) at most 64 windows in every half: windows 0..63 of a mask shifted by k come from ONE 64-bit shift of its container
        // [o, o + 64), o = max(0, L - 63) per lane (k >= Lmax - 63 >= o; positions past L belong to no window of this k)
        if (k <= khi) {
            const int o = L > 63 ? L - 63 : 0;
            const u64 Q1 = container64(P1, o), Q2 = container64(P2, o), Q3 = container64(P3, o), Ql = container64(lo, o), Qh = container64(hi, o);
            u64 Vq = ((u64) V[1] << 32) | V[0];  // V[2] is empty from here on
            for (; k <= khi; k++) {
                const u32 sh = (u32) (k - o);
                const u64 S1 = Q1 >> sh, S2 = Q2 >> sh, S3 = Q3 >> sh, Sl = Ql >> sh, Sh = Qh >> sh;
                const u32 Vw[2] = {(u32) Vq, (u32) (Vq >> 32)};
                const u32 F1[2] = {xor_and(P1[0], (u32) S1, Vw[0]), xor_and(P1[1], (u32) (S1 >> 32), Vw[1])};
                const u32 F2[2] = {xor_and(P2[0], (u32) S2, Vw[0]), xor_and(P2[1], (u32) (S2 >> 32), Vw[1])};
                const u32 F3[2] = {P3[0] ^ (u32) S3, P3[1] ^ (u32) (S3 >> 32)};
                const u32 E[2] = {~((lo[0] ^ (u32) Sl) | (hi[0] ^ (u32) Sh)), ~((lo[1] ^ (u32) (Sl >> 32)) | (hi[1] ^ (u32) (Sh >> 32)))};
                const u32 count = bcnt_acc(Vw[1], __popc(Vw[0]));
                const u32 m8 = max_bucket8<2>(F1, F2, F3, Vw, count);
                row[k - klo] = pack_bound_word(m8, count, class_links<2>(Vw, E), has_n, k, P.max_mer, P);
                Vq &= Vq >> 1;
            }
        }
        for (int ki = khi >= klo ? khi - klo + 1 : 0; ki < (int) kBoundWords; ki++) row[ki] = has_n << 29;  // k above MAX_MER: the empty bound
        // the wave's rows, transposed: 32 words a lane -> consecutive words in consecutive lanes
        lds_sync();
        const u64 left = total - base;
        const u32 words = (left < 64u ? (u32) left : 64u) * kBoundWords;
        u32 *const dst = bnd + base * kBoundWords;
#pragma unroll 4
        for (u32 r = 0; r < kBoundWords; r++) {
            const u32 w = r * 64u + lane;
            if (w < words) dst[w] = tile[(w >> 5) * kBoundsTileStride + (w & 31u)];
        }
        lds_sync();
    }
}
