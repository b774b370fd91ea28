// kernels/variants.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Telomere variant repeats (trew_hip_variants): what a repeat is made of.  Per read, motif and strand the number of exact
// units of the motif as typed, the number of in-phase units with exactly one substituted base, and which base at which
// position of the motif was substituted; the per-read histograms are added into one per batch on the device.  A kernel
// beside the scan, the annotation, the tracts and the intervals: it reads the same bit planes and pattern tables and writes
// only buffers of its own (the records and the two batch histograms).  512 bytes of LDS per wave, no worklist, no table.
//
// Definition (DESIGN 4.7).  T_s is the strand's target in the typed rotation (bit j of plo/phi[s][0] is base j of T_s).
// exact_s[i]: window i is valid and equals T_s; var_s[i]: it is valid and differs in exactly one position j, where the read
// has base c; a variant window is anchored when exact_s[i - k] or exact_s[i + k]; its bin is 4 j + c on the forward strand
// and 4 (k - 1 - j) + (3 - c) on the reverse strand, i.e. in motif coordinates on both.
//
// Wave per read, for every length.  A lane takes one 32-base word with the next word as look-ahead (k - 1 <= 31 bases) and
// counts, per window of its word, the mismatches against T_s saturated at two: k funnel-shift steps, step j comparing
// every base with T_s[j] and moving the result down by j (about ten instructions per step, against a log k erosion of a
// 64-bit mask for each of the k phases of annotate.inc's match, whose phases have no use here: the rotation is given).  A window with an N, or one that
// reaches over the end of the read, is neither exact nor a variant.  exact at i - k lies in the word in front (one DPP read;
// at the same bit of it for k = 32), exact at i + k in the word behind (one DPP read the other way).
//
// Seams.  An iteration covers 63 words, not 64: lane l takes word 63 t + l, lanes 0 .. 62 own their words and lane 63 only
// supplies the exact word behind lane 62 (its own look-ahead reaches one word further, so a k = 32 anchor two words past
// an owned word is seen).  Word 63 t + 63 is computed again as lane 0 of the next iteration.  The exact word in front of
// lane 0 is the one wave-uniform value carried between iterations (lane 62's).  One word in 64 is computed twice; in
// exchange no lane ever waits for a word that only the next iteration has.
//
// The only loop over bits is the one over a word's anchored variant bits: j from the XOR of the window with T_s, c from
// the planes, one LDS atomic on the wave's 128 bins.  At the end of a (read, motif, strand) lane l holds bins l and l + 64:
// distinct by a wave sum, top by a wave maximum of the counts and a second one over the bins that reach it (the smallest
// bin wins), then the non-zero bins go to the batch histograms with 64-bit vector-memory atomics (integer sums: the result
// does not depend on scheduling) and are cleared for the wave's next user.  A (read, motif, strand) without an anchored
// variant, which is nearly all of them outside telomeres, touches neither LDS nor the histograms.

constexpr u32 kVariantBins = TREW_VARIANT_BINS;

// exact word E and variant word V of 32-base word w: bit i = window 32 w + i equals T_s / differs from it in one base.
// c0, c1 / n0, n1: the lo and hi planes of the word and of the one behind it (for the bit loop).
__device__ __forceinline__ void variant_words(const ReadRef &rd, u32 tlo, u32 thi, u32 k, u32 w, u32 &c0, u32 &c1, u32 &n0, u32 &n1, u32 &E, u32 &V) {
    u32 c2 = 0xffffffffu, n2 = 0xffffffffu;
    c0 = c1 = n0 = n1 = 0;
    if (w < rd.nw) {
        c0 = rd.w[3ull * w + 0];
        c1 = rd.w[3ull * w + 1];
        c2 = rd.w[3ull * w + 2];
        const long long left = (long long) rd.len - 32ll * (long long) w;  // >= 1
        if (left < 32) c2 |= 0xffffffffu << (u32) left;
    }
    if (w < rd.nw && w + 1u < rd.nw) {
        n0 = rd.w[3ull * (w + 1u) + 0];
        n1 = rd.w[3ull * (w + 1u) + 1];
        n2 = rd.w[3ull * (w + 1u) + 2];
        const long long left = (long long) rd.len - 32ll * (long long) (w + 1u);
        if (left < 32) n2 |= 0xffffffffu << (u32) left;
    }
    // windows with an N or a base past the end: nmask dilated downwards by k (window i needs bits i .. i + k - 1 <= 62)
    u64 bad = ((u64) n2 << 32) | c2;
    u32 L = 1;
    for (; 2 * L <= k; L *= 2) bad |= bad >> L;
    if (L < k) bad |= bad >> (k - L);
    u32 one = 0, two = 0;  // at least one / at least two mismatches
    for (u32 j = 0; j < k; j++) {
        const u32 bl = 0u - ((tlo >> j) & 1u), bh = 0u - ((thi >> j) & 1u);  // base j of T_s, wave-uniform
        const u32 d = alignbit((n0 ^ bl) | (n1 ^ bh), (c0 ^ bl) | (c1 ^ bh), j);  // bit i: base i + j differs from T_s[j]
        two |= one & d;
        one |= d;
    }
    E = ~(one | (u32) bad);
    V = one & ~(two | (u32) bad);
}

// one strand of one motif: o = {units, variants, distinct, top, top_count}; h = the wave's 128 bins, all zero on entry and on exit
__device__ __forceinline__ void variant_wave_strand(const ReadRef &rd, const AnnotMotifDev *mm, int strand, u32 k, u32 *h, unsigned long long *hist,
                                                    unsigned long long *reads_with, u32 (&o)[5]) {
    const u32 lane = lane_id();
    const u32 tlo = mm->plo[strand][0], thi = mm->phi[strand][0];
    const u32 kmask = k >= 32u ? 0xffffffffu : (1u << k) - 1u;
    const bool own = lane < 63u;
    u32 carry_e = 0;  // exact word of the word in front of this iteration
    u32 units = 0, nvar = 0;
    for (u32 t0 = 0; t0 < rd.nw; t0 += 63u) {
        const u32 w = t0 + lane;
        u32 c0, c1, n0, n1, E, V;
        variant_words(rd, tlo, thi, k, w, c0, c1, n0, n1, E, V);
        const u32 Ep = (u32) __builtin_amdgcn_update_dpp((int) carry_e, (int) E, 0x138, 0xf, 0xf, false);  // wave_shr:1; lane 0 keeps carry_e
        const u32 En = (u32) __builtin_amdgcn_update_dpp(0, (int) E, 0x130, 0xf, 0xf, false);              // wave_shl:1; lane 63 gets 0
        carry_e = (u32) __builtin_amdgcn_readlane((int) E, 62);
        const u32 back = alignbit(E, Ep, 32u - k);                // exact at i - k; k = 32: the same bit of the word in front
        const u32 fwd = k >= 32u ? En : alignbit(En, E, k);       // exact at i + k
        const u32 A = own ? V & (back | fwd) : 0u;
        units = bcnt_acc(own ? E : 0u, units);
        nvar = bcnt_acc(A, nvar);
        for (u32 a = A; a; a &= a - 1u) {
            const u32 i = (u32) __builtin_ctz(a);
            const u32 wl = alignbit(n0, c0, i), wh = alignbit(n1, c1, i);  // the window's k bases (and what follows)
            const u32 j = (u32) __builtin_ctz(((wl ^ tlo) | (wh ^ thi)) & kmask);
            const u32 c = ((wl >> j) & 1u) | (((wh >> j) & 1u) << 1);
            atomicAdd(&h[(strand ? 4u * (k - 1u - j) + (3u - c) : 4u * j + c) & (kVariantBins - 1u)], 1u);  // j < k: the mask never bites
        }
    }
    o[0] = wave_sum_u32(units);
    o[1] = wave_sum_u32(nvar);
    o[2] = 0;
    o[3] = TREW_VARIANT_NONE;
    o[4] = 0;
    if (o[1] == 0) return;  // wave-uniform
    // the wave's own LDS operations complete in program order; the fences keep the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const u32 b0 = h[lane], b1 = h[lane + 64u];
    h[lane] = 0;
    h[lane + 64u] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    o[2] = wave_sum_u32((b0 ? 1u : 0u) + (b1 ? 1u : 0u));
    const u32 mx = wave_max_u32(max(b0, b1));
    const u32 key = b0 == mx ? 255u - lane : b1 == mx ? 191u - lane : 0u;  // the smallest bin has the largest key
    o[3] = 255u - wave_max_u32(key);
    o[4] = mx;
    if (b0) {
        atomicAdd(hist + lane, (unsigned long long) b0);
        atomicAdd(reads_with + lane, 1ull);
    }
    if (b1) {
        atomicAdd(hist + lane + 64u, (unsigned long long) b1);
        atomicAdd(reads_with + lane + 64u, 1ull);
    }
}

// hist / reads_with: [motif][strand][bin] u64, zero when the kernel starts (the caller's memset on the same stream)
__global__ void __launch_bounds__(256) variants_wave_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, u32 *__restrict__ out,
                                                            unsigned long long *__restrict__ hist, unsigned long long *__restrict__ reads_with) {
    __shared__ u32 bins[4][kVariantBins];
    const u32 lane = lane_id();
    u32 *h = bins[threadIdx.x >> 6];
    h[lane] = 0;
    h[lane + 64u] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_motifs; m++) {
            const AnnotMotifDev *mm = mt + m;
            const u32 k = mm->k;
            u32 f[5], v[5];
            variant_wave_strand(rd, mm, 0, k, h, hist + (u64) (2 * m) * kVariantBins, reads_with + (u64) (2 * m) * kVariantBins, f);
            variant_wave_strand(rd, mm, 1, k, h, hist + (u64) (2 * m + 1) * kVariantBins, reads_with + (u64) (2 * m + 1) * kVariantBins, v);
            // ten lanes write the record's ten words (trew_hip_variant): one vector store
            u32 x = v[4];
#pragma unroll
            for (int i = 3; i >= 0; i--) x = lane == 5u + (u32) i ? v[i] : x;
#pragma unroll
            for (int i = 4; i >= 0; i--) x = lane == (u32) i ? f[i] : x;
            if (lane < 10) out[(r * (u64) n_motifs + (u64) m) * 10ull + lane] = x;
        }
    }
}
