// kernels/intervals.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Gap-tolerant motif intervals anywhere in a read (trew_hip_intervals): where in a read a repeat lies, however many tracts
// the read carries.  A kernel beside the scan, the annotation and the tracts: it reads the same bit planes and pattern
// tables and writes only buffers of its own (an append log with its counter, one count per (read, motif, strand)); no LDS,
// no worklist, no table.
//
// Definition (DESIGN 4.6).  cov[p] is tracts' coverage (wave_cov_word).  With the covered positions p1 < p2 < ..., an interval
// is a maximal group of consecutive covered positions whose neighbours are at most max_gap uncovered bases apart; its record
// is {start = first covered position, end = last covered position + 1, covered = covered bases in between}; it is kept when
// end - start >= min_len.
//
// Wave per read, for every length: lane l takes 32-base word 64 t + l in iteration t.  A covered base is a *start* when the
// covered base in front of it is absent or more than max_gap + 1 positions back.  Inside a word that is the coverage word
// without its own dilation by max_gap + 1; for a word's lowest covered bit the covered base in front comes from an exclusive
// prefix maximum (DPP) over every word's highest covered position, whose running value travels wave-uniform from one
// iteration to the next, so a gap may span any number of uncovered words or iterations.  A start at q closes the interval
// in front of it: {the last start before q, the last covered position before q + 1, the covered bases between the two},
// the covered-count from a DPP prefix sum of the words' popcounts plus the popcount below the bit.  The last start before a
// word and the covered-count at it come from a second exclusive prefix maximum, over {position + 1, count} of every word's
// highest start packed into one u32 (both relative to the iteration: 12 bits each).  The interval still open at the end of
// the read is closed there.  The only loop over bits is the one over a word's own start bits: none in almost every word.
//
// Between iterations (wave-uniform): the last covered position + 1 (0: none yet), the last start, the covered-count at that
// start, the running covered-count; all u32, since a read has fewer than 2^32 bases.

// one kept interval: one atomic on the counter; the record only where the log has room for it
__device__ __forceinline__ void interval_put(const IntervalLog &lg, u32 r, u32 m, u32 strand, u32 start, u32 end, u32 covered) {
    const u64 idx = atomicAdd(lg.counter, 1ull);
    if (idx < lg.cap) {
        uint2 *o = (uint2 *) (lg.recs + idx * 6ull);  // 24 bytes: 8-byte aligned
        o[0] = make_uint2(r, m);
        o[1] = make_uint2(strand, start);
        o[2] = make_uint2(end, covered);
    }
}

// one strand of one motif; returns the number of kept intervals (wave-uniform)
__device__ __forceinline__ u32 interval_wave_strand(const ReadRef &rd, const AnnotMotifDev *mm, int strand, u32 k, u32 G, u32 min_len, u32 r, u32 m,
                                                    const IntervalLog &lg) {
    const u32 lane = lane_id();
    const u32 g1 = min(G, 30u) + 1u;  // in-word reach of a covered base: the max_gap + 1 positions behind it, at most 31
    u32 carry_m = 0;                  // match word of the word in front of this iteration
    u32 last_end = 0;                 // last covered position + 1 in front of this iteration; 0: none yet
    u32 open_start = 0, open_cnt = 0; // the last start in front of this iteration and the covered-count in front of it
    u32 run = 0;                      // covered bases in front of this iteration
    u32 kept = 0;                     // per lane
    for (u32 t0 = 0; t0 < rd.nw; t0 += 64u) {
        const u32 w = t0 + lane;
        u32 nv;
        const u32 cov = wave_cov_word(rd, mm, strand, k, w, carry_m, nv);
        const u32 it0 = t0 << 5, rel = lane << 5;  // first base of the iteration; of this word inside it
        const u32 pc = (u32) __builtin_popcount(cov);
        const u32 incl = wave_scan_u32(pc);
        const u32 excl = incl - pc;  // covered bases of the iteration in front of this word
        // the covered base in front of this word: position + 1 relative to the iteration, 0 for none
        const u32 hp = cov ? rel + 32u - (u32) __builtin_clz(cov) : 0u;
        const u32 hpi = wave_scan_max_u32(hp);
        const u32 hpe = wave_prev_lane_u32(hpi);
        const u32 prev_end = hpe ? it0 + hpe : last_end;
        // starts: covered bits with no covered bit among the g1 bits below them ...
        u32 y = cov << 1, L = 1;
        for (; 2 * L <= g1; L *= 2) y |= y << L;
        if (L < g1) y |= y << (g1 - L);
        u32 starts = cov & ~y;
        // ... of which the word's lowest covered bit has to look at the words in front
        if (cov && prev_end && it0 + rel + (u32) __builtin_ctz(cov) - prev_end <= G) starts &= starts - 1u;
        // the last start in front of this word and the covered-count in front of it
        u32 key = 0;
        if (starts) {
            const u32 ts = 31u - (u32) __builtin_clz(starts);
            key = ((rel + ts + 1u) << 12) | (excl + (u32) __builtin_popcount(cov & ((1u << ts) - 1u)));
        }
        const u32 ki = wave_scan_max_u32(key);
        const u32 ke = wave_prev_lane_u32(ki);
        u32 cur_start = ke ? it0 + (ke >> 12) - 1u : open_start;
        u32 cur_cnt = ke ? run + (ke & 4095u) : open_cnt;
        // every start of this word closes the interval in front of it
        for (u32 s = starts; s; s &= s - 1u) {
            const u32 i = (u32) __builtin_ctz(s);
            const u32 below = cov & ((1u << i) - 1u);
            const u32 pe = below ? it0 + rel + 32u - (u32) __builtin_clz(below) : prev_end;
            const u32 c = run + excl + (u32) __builtin_popcount(below);
            if (pe && pe - cur_start >= min_len) {
                interval_put(lg, r, m, (u32) strand, cur_start, pe, c - cur_cnt);
                kept++;
            }
            cur_start = it0 + rel + i;
            cur_cnt = c;
        }
        // what the iteration leaves behind
        const u32 kl = (u32) __builtin_amdgcn_readlane((int) ki, 63);
        if (kl) {
            open_start = it0 + (kl >> 12) - 1u;
            open_cnt = run + (kl & 4095u);
        }
        const u32 hl = (u32) __builtin_amdgcn_readlane((int) hpi, 63);
        if (hl) last_end = it0 + hl;
        run += (u32) __builtin_amdgcn_readlane((int) incl, 63);
    }
    kept = wave_sum_u32(kept);
    if (last_end && last_end - open_start >= min_len) {  // the interval still open at the end of the read
        if (lane == 0) interval_put(lg, r, m, (u32) strand, open_start, last_end, run - open_cnt);
        kept++;
    }
    return kept;
}

__global__ void __launch_bounds__(256) intervals_wave_kernel(DevBatch B, const AnnotMotifDev *__restrict__ mt, int n_motifs, IntervalRulesDev rules,
                                                             IntervalLog lg, u32 *__restrict__ counts) {
    const u64 wave = ((u64) blockIdx.x * 256ull + threadIdx.x) >> 6;
    const u64 n_waves = (u64) gridDim.x * 4ull;
    for (u64 r = wave; r < B.n_reads; r += n_waves) {
        const ReadRef rd = uni(get_read(B, r));
        for (int m = 0; m < n_motifs; m++) {
            const AnnotMotifDev *mm = mt + m;
            const u32 k = mm->k;
            const u32 G = rfl(rules.max_gap[m]), min_len = rfl(rules.min_len[m]);
            const u32 nf = interval_wave_strand(rd, mm, 0, k, G, min_len, (u32) r, (u32) m, lg);
            const u32 nr = interval_wave_strand(rd, mm, 1, k, G, min_len, (u32) r, (u32) m, lg);
            // two lanes write the pair of counts: one vector store
            const u32 lane = lane_id();
            if (lane < 2) counts[(r * (u64) n_motifs + (u64) m) * 2ull + lane] = lane ? nr : nf;
        }
    }
}
