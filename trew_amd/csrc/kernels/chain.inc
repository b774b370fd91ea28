// kernels/chain.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Ordered unit chain per read (trew_hip_chain): the maximal in-phase runs of exact units and every anchored variant unit at
// its position -- what variants.inc counts, kept in order.  A kernel beside the scan and the other five measures: it reads the
// same bit planes and pattern tables and writes only buffers of its own (an append log of events with its counter, two counts
// per (read, motif, strand)).  No LDS, no worklist, no table.
//
// Definition (DESIGN 4.7b).  exact_s[i], var_s[i], "anchored" and the bin are those of DESIGN 4.7 (variant_words is called,
// not copied).  A run starts at an exact window i whose window i - k is not exact and ends at an exact window e whose window
// e + k is not exact (a window outside the read is not exact); an item is a run {start, count of units} or an anchored
// variant {start, 1, bin}.
//
// Wave per read, for every length, with the iteration of variants_wave_kernel: lane l takes word 63 t + l, lanes 0 .. 62 own
// their words, lane 63 only supplies the exact word behind lane 62, and the exact word in front of lane 0 travels wave-uniform
// from one iteration to the next.  With back (exact at i - k) and fwd (exact at i + k) formed as there, everything is local:
//   S = E & ~back  run starts     T = E & ~fwd  run ends     A = V & (back | fwd)  anchored variants
//
// Events, not runs.  A run may span any number of words and iterations, and k residue classes may each have one open; the
// kernel keeps none of that: it appends a start event and an end event (one event with both kinds for a one-unit run) and the
// host pairs them -- within a (read, motif, strand, start mod k), ordered by start, starts and ends alternate.  Nothing is
// carried between iterations beyond what variants carries.
//
// Append.  S | T | A of a lane has one bit per event.  An iteration with events takes one 64-bit vector-memory atomic on the
// log's counter for the whole wave (a ballot, then offsets from wave_scan_u32 of the lanes' event counts); the events go out
// as 16-byte vector stores, those at or beyond the capacity not at all while the counter keeps counting.  An iteration without
// events -- nearly every one outside tracts -- touches no memory beyond its loads.

// one strand of one motif; runs / nvar: the key's two counts (wave-uniform on return)
__device__ __forceinline__ void chain_wave_strand(const ReadRef &rd, const AnnotMotifDev *mm, int strand, u32 k, u32 r, u32 m, const ChainLog &lg, u32 &runs,
                                                  u32 &nvar) {
    const u32 lane = lane_id();
    const u32 tlo = mm->plo[strand][0], thi = mm->phi[strand][0];
    const u32 kmask = k >= 32u ? 0xffffffffu : (1u << k) - 1u;
    const u32 meta = m | ((u32) strand << 4);
    const bool own = lane < 63u;
    u32 carry_e = 0;  // exact word of the word in front of this iteration
    u32 ns = 0, nv = 0;
    for (u32 t0 = 0; t0 < rd.nw; t0 += 63u) {
        const u32 w = t0 + lane;
        u32 c0, c1, n0, n1, E, V;
        variant_words(rd, tlo, thi, k, w, c0, c1, n0, n1, E, V);
        const u32 Ep = (u32) __builtin_amdgcn_update_dpp((int) carry_e, (int) E, 0x138, 0xf, 0xf, false);  // wave_shr:1; lane 0 keeps carry_e
        const u32 En = (u32) __builtin_amdgcn_update_dpp(0, (int) E, 0x130, 0xf, 0xf, false);              // wave_shl:1; lane 63 gets 0
        carry_e = (u32) __builtin_amdgcn_readlane((int) E, 62);
        const u32 back = alignbit(E, Ep, 32u - k);           // exact at i - k; k = 32: the same bit of the word in front
        const u32 fwd = k >= 32u ? En : alignbit(En, E, k);  // exact at i + k
        const u32 S = own ? E & ~back : 0u;
        const u32 T = own ? E & ~fwd : 0u;
        const u32 A = own ? V & (back | fwd) : 0u;
        ns = bcnt_acc(S, ns);
        nv = bcnt_acc(A, nv);
        const u32 X = S | T | A;  // one bit per event: S and T lie in E, A in V, and a window is exact or variant, never both
        if (__ballot(X != 0u)) {  // wave-uniform
            const u32 cnt = (u32) __builtin_popcount(X);
            const u32 incl = wave_scan_u32(cnt);
            const u32 total = (u32) __builtin_amdgcn_readlane((int) incl, 63);
            u64 base = 0;
            if (lane == 0) base = atomicAdd(lg.counter, (unsigned long long) total);
            base = rfl64(base);
            u64 idx = base + (u64) (incl - cnt);
            for (u32 x = X; x; x &= x - 1u, idx++) {
                const u32 i = (u32) __builtin_ctz(x);
                const u32 kind = ((S >> i) & 1u) * kChainStart | ((T >> i) & 1u) * kChainEnd | ((A >> i) & 1u) * kChainVariant;
                u32 bin = TREW_VARIANT_NONE;
                if (kind & kChainVariant) {  // j and c as in variants' bit loop
                    const u32 wl = alignbit(n0, c0, i), wh = alignbit(n1, c1, i);
                    const u32 j = (u32) __builtin_ctz(((wl ^ tlo) | (wh ^ thi)) & kmask);
                    const u32 c = ((wl >> j) & 1u) | (((wh >> j) & 1u) << 1);
                    bin = strand ? 4u * (k - 1u - j) + (3u - c) : 4u * j + c;
                }
                if (idx < lg.cap) lg.events[idx] = make_uint4(r, meta | (kind << 8), (w << 5) + i, bin);
            }
        }
    }
    runs = wave_sum_u32(ns);
    nvar = wave_sum_u32(nv);
}

// counts: [read][motif][strand]{runs, variants} u32; the counter of lg is zero when the kernel starts (the caller's memset on the same stream)
__global__ void __launch_bounds__(256) chain_wave_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, ChainLog lg, u32 *__restrict__ counts) {
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const u32 lane = lane_id();
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_motifs; m++) {
            const AnnotMotifDev *mm = mt + m;
            const u32 k = mm->k;
            u32 rf, vf, rr, vr;
            chain_wave_strand(rd, mm, 0, k, (u32) r, (u32) m, lg, rf, vf);
            chain_wave_strand(rd, mm, 1, k, (u32) r, (u32) m, lg, rr, vr);
            // four lanes write the key pair's four counts: one vector store
            const u32 x = lane == 0 ? rf : lane == 1 ? vf : lane == 2 ? rr : vr;
            if (lane < 4) counts[(r * (u64) n_motifs + (u64) m) * 4ull + lane] = x;
        }
    }
}
