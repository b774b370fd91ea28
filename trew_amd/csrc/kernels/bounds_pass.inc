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
// where they exist (run_short_group) and bounds in row layout where they do not.  Knowing every (half, k) of an entry, the kernel
// also drops the entries no k of which can still count and hands the exact kernel the rest (the live worklist, see bounds_kernel).
//
// Every quantity is built from bound.inc's blocks (segment_setup, Buckets8, class_links), so the bound is still written once;
// only the tail that turns (m8, COUNT, links) into the packed word is repeated here (pack_bound_word), see there.
//
// Output: bnd[(position in the exact kernel's list * 2 + half) * 32 + k - MIN_MER].  The 64 lanes of a wave own 64 rows of 32
// words; those of its live entries are transposed through LDS so that the wave writes whole 256-byte lines.

// (kBoundWords, kBoundItemWords: decide_group.inc, beside the code that reads the words back)
constexpr u32 kBoundsTileStride = kBoundWords + 1;  // LDS row stride of the transposition (odd: no bank conflicts either way)

// The tail of bound_at_k (decide_group.inc), from "m8 / COUNT >= baseline" on, word for word: the reference's doubles decide the
// pass bits (a multiplication, and the IEEE division itself within rounding distance of a threshold).  Repeated and not shared
// because bound_at_k compiles into every exact kernel and those keep their registers only as long as its source is untouched
// (profiles/bound_refactor/README.md).  A change of either copy is a change of both.
// need: the same two decisions as integers, or nullptr.  need[COUNT] = the smallest m8 that passes LOW | the smallest that passes
// HIGH << 16, which the host worked out with these very doubles for every (m8, COUNT) and hands over only where it is sure of them
// (fill_bound_needs, trew_kernels.hip); the doubles took about a quarter of a k's instructions to decide two bits.
__device__ __forceinline__ u32 pack_bound_word(u32 m8, u32 count, u32 links, u32 has_n, int k, int gmax, const DevParams &P, const u32 *need) {
    const u32 runs = count - links < 127u ? count - links : 127u;
    u32 pass_lo, pass_hi;
    if (need) {  // (uniform over the launch)
        const u32 nd = need[count];
        pass_lo = m8 >= (nd & 0xffffu) ? 1u : 0u;
        pass_hi = m8 >= (nd >> 16) ? 1u : 0u;
    } else {
        const double dm = (double) m8, dc = (double) count;
        const double tl = P.low * dc, th = P.high * dc;
        pass_lo = dm > tl ? 1u : 0u, pass_hi = dm > th ? 1u : 0u;
        const bool amb = fabs(dm - tl) <= 1e-9 || fabs(dm - th) <= 1e-9;
        if (__any(amb)) {
            const double ub = count ? dm / dc : 0.0;
            pass_lo = ub >= P.low ? 1u : 0u;
            pass_hi = ub >= P.high ? 1u : 0u;
        }
    }
    const bool inr = k <= gmax && count != 0u;
    return inr ? (m8 | (count << 10) | (runs << 20) | (pass_lo << 27) | (pass_hi << 28) | (has_n << 29)) : (has_n << 29);
}

// Sixteen buckets where eight passed by chance.  A half with an N in its middle has few windows at the large k (75 bases, k = 30:
// about 16 of 46), and the largest of eight buckets of so few windows reaches half of them often enough that 15 % of the flagged
// reads of a WGS-like batch are random reads with one N (profiles/r02/README.md).  Where some lane of the wave has an N and a pass
// bit at this k, its buckets are split once more by the parity of adjacent equal bases (bound.inc) and the word is packed again,
// by the same tail, from min(m8, m16).  Sound for the reason the eight are: the windows of a rotation class agree in every
// rotation invariant, so they lie in one of the sixteen, and windows with an N are in none.  COUNT and the runs do not change, and
// a lane without an N keeps its word bit for bit.  F4: the feature's words, built by the caller for its layout.
template <int N>
__device__ __forceinline__ u32 sharpen_bound_word(u32 word, const u32 (&F1)[N], const u32 (&F2)[N], const u32 (&F3)[N], const u32 (&F4)[N],
                                                  const u32 (&V)[N], u32 links, u32 has_n, int k, int gmax, const DevParams &P, const u32 *need) {
    const u32 m8 = word & 1023u, count = (word >> 10) & 1023u;
    const u32 m16 = max_bucket16<N>(F1, F2, F3, F4, V);
    const u32 sharp = pack_bound_word(m16 < m8 ? m16 : m8, count, links, has_n, k, gmax, P, need);
    return (has_n != 0u && (word & (3u << 27)) != 0u) ? sharp : word;
}

// The live worklist.  An entry of the worklist is DEAD when both halves were bounded here, no k of either half kept a pass bit
// and the read has no whole-read segment: the exact kernel could record nothing for it (every k of a half is pruned by these very
// words, and with no half found and no whole-read check run_short_group adds no row).  The live entries of the first bnd_cap
// worklist positions are written to `live`, in the order the worklist has inside a block-full (the reads with an N stay next to
// each other at its end, DESIGN 5), their rows to bnd at the COMPACTED positions, and wl_count[kStoredPrefixWord] counts them:
// one returning atomic a block of four waves (a wave each would be 5 500 of them on one word, more than the kernel lasts).
// Worklist entries at or beyond bnd_cap are not copied: the exact kernel reads them behind the live ones from the worklist
// itself (exact_kernel.inc).  live == nullptr (TREW_FLAG_DEBUG_NO_LIVE_LIST): nothing is sharpened and nothing dropped, the rows
// stay at their worklist positions and the word says how many of those have rows.
constexpr u32 kBoundsWaves = 4;
template <int NW>
__global__ __launch_bounds__(64 * kBoundsWaves) void bounds_kernel(DevParams P, DevBatch B, const u32 *__restrict__ wl, u32 *__restrict__ wl_count,
                                                                     u32 wl_cap, u32 *__restrict__ bnd, u32 bnd_cap, u32 *__restrict__ live,
                                                                     const u32 *__restrict__ need_table) {
    static_assert(NW == 3, "the k loop is written for three words: halves of at most 95 bases");
    __shared__ u32 tile_all[kBoundsWaves * 64 * kBoundsTileStride];
    __shared__ u32 src_row_all[kBoundsWaves * 64];  // compacted row of the wave -> the lane that holds it
    __shared__ u32 wave_live[kBoundsWaves + 1];     // live entries of every wave; [kBoundsWaves]: the block's first compacted position
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    u32 *const tile = tile_all + wave * 64u * kBoundsTileStride;
    u32 *const src_row = src_row_all + wave * 64u;
    const bool sharpen = live != nullptr;
    __shared__ u32 need_lds[kBoundNeedWords];
    const u32 *const need = need_table ? need_lds : nullptr;
    if (need_table) {
        for (u32 i = threadIdx.x; i < (u32) kBoundNeedWords; i += 64u * kBoundsWaves) need_lds[i] = need_table[i];
        __syncthreads();
    }
    u32 n = wl_count[0];
    n = n < wl_cap ? n : wl_cap;
    n = n < bnd_cap ? n : bnd_cap;
    if (!live && blockIdx.x == 0 && threadIdx.x == 0) wl_count[kStoredPrefixWord] = n;
    const u64 total = 2ull * n;  // halves
    const int klo = P.min_mer, khi = P.max_mer < P.min_mer + (int) kBoundWords - 1 ? P.max_mer : P.min_mer + (int) kBoundWords - 1;
    constexpr u32 kBlockHalves = 64u * kBoundsWaves;
    for (u64 bbase = (u64) blockIdx.x * kBlockHalves; bbase < total; bbase += (u64) gridDim.x * kBlockHalves) {
        const u64 idx = bbase + threadIdx.x;
        const bool active = idx < total;
        const u32 half = (u32) idx & 1u;
        ReadRef rd;
        rd.w = B.words;
        rd.len = rd.nw = 0;
        u32 unit = 0;
        if (active) {
            unit = wl[idx >> 1];
            rd = get_read(B, unit);
        }
        const Segment sg = get_segment(TREW_MODE_SHORT, (int) half, rd.len, 0, P.min_mer, P.max_mer, P.slice_len);
        // a read the group pass does not take (too short for halves) or a half the three words cannot hold: the lane has no
        // window at any k and its words are never read
        const bool can = active && sg.valid && sg.len <= 32u * NW - 1u;
        const bool whole = get_segment(TREW_MODE_SHORT, 2, rd.len, 0, P.min_mer, P.max_mer, P.slice_len).valid;
        if (!can) rd.nw = 0;  // (no plane is loaded)
        const int L = can ? (int) sg.len : 0;
        u32 lo[3], hi[3], nm[3], V[3], P1[3], P2[3], P3[3], PD[3];
        load_planes<3>(rd, sg.start, lo, hi, nm);
        segment_setup<3, false, true, true>(lo, hi, nm, L, V, P1, P2, P3);  // V_1 and the three prefix parities, as drain_half_init
        adjacency_parity<3>(lo, hi, V, PD);
        const u32 has_n = segment_has_n<3>(nm, L) != 0u ? 1u : 0u;
        for (int t = 1; t < klo; t++) drain_v_step3(V);  // V_klo
        const int Lmax = (int) wave_max_u32((u32) L);
        u32 *const row = tile + lane * kBoundsTileStride;
        u32 seen = 0;  // every word of the half, or-ed: its pass bits
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
            const u32 links = class_links<3>(V, E);
            u32 word = pack_bound_word(m8, count, links, has_n, k, P.max_mer, P, need);
            if (sharpen && __any(has_n != 0u && (word & (3u << 27)) != 0u)) {
                u32 F4[3];
#pragma unroll
                for (int j = 0; j < 3; j++) F4[j] = adjacency_feature_word<3>(PD, lo, hi, j, bs - 1u);
                word = sharpen_bound_word<3>(word, F1, F2, F3, F4, V, links, has_n, k, P.max_mer, P, need);
            }
            row[k - klo] = word;
            seen |= word;
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
                const u32 links = class_links<2>(Vw, E);
                u32 word = pack_bound_word(m8, count, links, has_n, k, P.max_mer, P, need);
                if (sharpen && __any(has_n != 0u && (word & (3u << 27)) != 0u)) {
                    // the shift by k - 1 can start one base in front of the container (k = o): the rare stage takes the funnel
                    // shifts of (b) on the two words that hold windows (k - 1 <= 31: 64-bit keys end at MAX_MER = 32)
                    const u32 F4[2] = {adjacency_feature_word<3>(PD, lo, hi, 0, (u32) k - 1u), adjacency_feature_word<3>(PD, lo, hi, 1, (u32) k - 1u)};
                    word = sharpen_bound_word<2>(word, F1, F2, F3, F4, Vw, links, has_n, k, P.max_mer, P, need);
                }
                row[k - klo] = word;
                seen |= word;
                Vq &= Vq >> 1;
            }
        }
        for (int ki = khi >= klo ? khi - klo + 1 : 0; ki < (int) kBoundWords; ki++) row[ki] = has_n << 29;  // k above MAX_MER: the empty bound
        // which entries of the wave go on: lanes 2 e and 2 e + 1 hold entry e
        const u64 even = 0x5555555555555555ull;
        const u64 activeb = __ballot(active);
        const u64 dropb = __ballot(sharpen && can && !whole && (seen & (3u << 27)) == 0u);
        const u64 liveb = activeb & ~(dropb & (dropb >> 1)) & even;
        const u32 nlive = (u32) __popcll(liveb), nent = (u32) __popcll(activeb & even);
        if (lane == 0) wave_live[wave] = nlive | (nent << 16);
        __syncthreads();
        if (live && threadIdx.x == 0) {
            u32 tl = 0, te = 0;
            for (u32 w = 0; w < kBoundsWaves; w++) tl += wave_live[w] & 0xffffu, te += wave_live[w] >> 16;
            wave_live[kBoundsWaves] = atomicAdd(&wl_count[kStoredPrefixWord], tl);
            if (te != tl) atomicAdd(&wl_count[kDeadEntriesWord], te - tl);
        }
        if (live) __syncthreads();
        u32 pos0 = live ? wave_live[kBoundsWaves] : (u32) (bbase >> 1);
        for (u32 w = 0; w < wave; w++) pos0 += wave_live[w] & 0xffffu;
        const u32 mine = lane & ~1u;
        if ((liveb >> mine) & 1ull) {
            const u32 rank = (u32) __popcll(liveb & ((1ull << mine) - 1ull));
            src_row[rank * 2u + half] = lane;
            if (live && half == 0u) live[pos0 + rank] = unit;
        }
        // the wave's live rows, transposed: 32 words a lane -> consecutive words in consecutive lanes
        lds_sync();
        const u32 words = nlive * 2u * kBoundWords;
        u32 *const dst = bnd + (u64) pos0 * kBoundItemWords;
#pragma unroll 4
        for (u32 r = 0; r < kBoundWords; r++) {
            const u32 w = r * 64u + lane;
            if (w < words) dst[w] = tile[src_row[w >> 5] * kBoundsTileStride + (w & 31u)];
        }
        __syncthreads();
    }
}

