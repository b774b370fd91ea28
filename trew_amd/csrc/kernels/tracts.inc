// kernels/tracts.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Error-tolerant terminal motif tracts per read (trew_hip_tracts): how far a repeat reaches in from either end of a read
// when single wrong bases are forgiven.  A kernel beside the scan and beside the annotation: it reads the same bit planes
// and pattern tables, writes only its own result buffer, uses no LDS, no worklist, no counter and no table.
//
// Definition (DESIGN 4.5).  match[i] is annotate's match mask; cov[p] = some matching window contains base p (the match
// mask dilated by k); score(p) = +1 when covered, else -penalty; S(e) = sum of score(p) over p < e.  The head tract is the
// shortest prefix with the largest S (length 0 when that is 0), the tail tract the shortest suffix with the largest sum, i.e.
// it starts at the largest b with the smallest S(b).  One pass over S gives both: arg-max for the head, arg-min for the tail.
// With c covered bases among len, score = c - penalty (len - c), so c = (score + penalty len) / (1 + penalty): no second pass.
//
// Wave per read, for every length: lane l takes 32-base word 64 t + l in iteration t (annot_wave_match).  Its coverage word
// is its match word dilated by k together with the top k - 1 bits of the word before it (wave_cov_word, shared with
// kernels/intervals.inc).  Every lane walks its word for the word's total, its best prefix (earliest position) and its lowest prefix (latest position); a DPP prefix sum of the totals places
// the words, two DPP maxima over packed {value, position} keys give the iteration's arg-max and arg-min, and those are
// compared with the wave-uniform best so far.  The running sum travels between iterations in 64 bits; inside an iteration
// |S| <= 64 words * 32 bases * 64 = 2^17.

// numerator / (1 + penalty), both wave-uniform; the 64-bit division only where a read is long enough to need it
__device__ __forceinline__ u32 tract_div(u64 num, u32 p1) { return (num >> 32) ? (u32) (num / (u64) p1) : (u32) num / p1; }

// coverage word of 32-base word w of a read, one strand of one motif, every lane of the wave calling it for w = 64 t + lane:
// bit i = some matching window contains base 32 w + i.  Base p is covered by the windows p - k + 1 .. p, up to k - 1 of
// which start in the word before: the match word dilated by k together with the top bits of the previous lane's match word
// (one DPP read), lane 63's match word carried (wave-uniform, carry_m; 0 in front of the first iteration) into lane 0 of the
// next iteration.  nv = bases of the read inside the word; bits at and past the end of the read are not covered (no window
// reaches there).  Shared with kernels/intervals.inc, so the dilation exists once.
__device__ __forceinline__ u32 wave_cov_word(const ReadRef &rd, const AnnotMotifDev *mm, int strand, u32 k, u32 w, u32 &carry_m, u32 &nv) {
    const u32 m = annot_wave_match(rd, mm, strand, k, w);
    const u32 pm = (u32) __builtin_amdgcn_update_dpp((int) carry_m, (int) m, 0x138, 0xf, 0xf, false);  // wave_shr:1; lane 0 keeps carry_m
    carry_m = (u32) __builtin_amdgcn_readlane((int) m, 63);
    u64 y = ((u64) m << 32) | pm;
    u32 L = 1;
    for (; 2 * L <= k; L *= 2) y |= y << L;
    if (L < k) y |= y << (k - L);
    const long long left = (long long) rd.len - 32ll * (long long) w;
    nv = left >= 32 ? 32u : left > 0 ? (u32) left : 0u;
    const u32 valid = nv >= 32u ? 0xffffffffu : (1u << nv) - 1u;
    return (u32) (y >> 32) & valid;
}

// one strand of one motif: o = {covered, head_len, head_cov, tail_len, tail_cov}
__device__ __forceinline__ void tract_wave_strand(const ReadRef &rd, const AnnotMotifDev *mm, int strand, u32 k, int P, u32 (&o)[5]) {
    const u32 lane = lane_id();
    constexpr int kBias = 1 << 18;  // above every |S| inside an iteration
    long long run = 0;              // S at the start of the iteration
    long long best_hi = 0, best_lo = 0;  // largest and smallest S so far: S(0) = 0 at position 0
    u32 pos_hi = 0, pos_lo = 0;          // earliest position of the largest, latest position of the smallest
    u32 carry_m = 0;                     // match word of the word in front of this iteration
    for (u32 t0 = 0; t0 < rd.nw; t0 += 64u) {
        const u32 w = t0 + lane;
        u32 nv;
        const u32 cov = wave_cov_word(rd, mm, strand, k, w, carry_m, nv);
        const u32 valid = nv >= 32u ? 0xffffffffu : (1u << nv) - 1u;
        const u32 unc = valid & ~cov;
        // in-word walk over the prefixes e = 1 .. 32 (e = 0: value 0).  Keys: the largest value with the smallest e, the
        // smallest value with the largest e.  A bit past the end scores 0, which can only tie: towards the smaller e in kmx,
        // and in kmn the position is clamped to nv afterwards (the value there is the same).
        int s = 0, kmx = 63, kmn = 0;
#pragma unroll
        for (int i = 0; i < 32; i++) {
            s += (int) ((cov >> i) & 1u) - P * (int) ((unc >> i) & 1u);
            kmx = max(kmx, s * 64 + (62 - i));
            kmn = max(kmn, -s * 64 + (i + 1));
        }
        const int mx = kmx >> 6, mn = -(kmn >> 6);
        const u32 emx = 63u - (u32) (kmx & 63), emn = min((u32) (kmn & 63), nv);
        // place the words: exclusive prefix sum of the totals, then the wave's arg-max and arg-min
        const u32 incl = wave_scan_u32((u32) s);
        const int off = (int) (incl - (u32) s);
        const int total = __builtin_amdgcn_readlane((int) incl, 63);
        const bool live = w < rd.nw;  // an idle lane would add positions past the end of the read
        const u32 key_hi = live ? ((u32) (off + mx + kBias) << 12) | (4095u - (lane * 32u + emx)) : 0u;
        const u32 key_lo = live ? ((u32) (kBias - (off + mn)) << 12) | (lane * 32u + emn) : 0u;
        const u32 kh = wave_max_u32(key_hi), kl = wave_max_u32(key_lo);
        const long long cand_hi = run + (long long) ((int) (kh >> 12) - kBias);
        const long long cand_lo = run + (long long) (kBias - (int) (kl >> 12));
        if (cand_hi > best_hi) {  // strictly: an earlier iteration keeps a tie
            best_hi = cand_hi;
            pos_hi = (t0 << 5) + (4095u - (kh & 4095u));
        }
        if (cand_lo <= best_lo) {  // a later iteration takes a tie
            best_lo = cand_lo;
            pos_lo = (t0 << 5) + (kl & 4095u);
        }
        run += (long long) total;
    }
    const u32 p1 = (u32) P + 1u;
    const u64 pen = (u64) (u32) P;
    const u32 tail_len = rd.len - pos_lo;
    o[0] = tract_div((u64) (run + (long long) (pen * (u64) rd.len)), p1);
    o[1] = pos_hi;
    o[2] = tract_div((u64) best_hi + pen * (u64) pos_hi, p1);
    o[3] = tail_len;
    o[4] = tract_div((u64) (run - best_lo) + pen * (u64) tail_len, p1);
}

__global__ void __launch_bounds__(256) tracts_wave_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, int penalty,
                                                          u32 *__restrict__ out) {
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    const int P = rfl_i(penalty);
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_motifs; m++) {
            const AnnotMotifDev *mm = mt + m;
            const u32 k = mm->k;
            u32 f[5], v[5];
            tract_wave_strand(rd, mm, 0, k, P, f);
            tract_wave_strand(rd, mm, 1, k, P, v);
            // ten lanes write the record's ten words (trew_hip_tract): one vector store
            const u32 lane = lane_id();
            u32 x = v[4];
#pragma unroll
            for (int i = 3; i >= 0; i--) x = lane == 5u + (u32) i ? v[i] : x;
#pragma unroll
            for (int i = 4; i >= 0; i--) x = lane == (u32) i ? f[i] : x;
            if (lane < 10) out[(r * (u64) n_motifs + (u64) m) * 10ull + lane] = x;
        }
    }
}
