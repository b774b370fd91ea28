// kernels/driver_long.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// buffer_task_long (kmer.cpp:747-985): the slice walker.

// ------------------------------------------------------------------ long reads
// slice t (1-based) of buffer_task_long, kmer.cpp:790-798: SLICE_LENGTH bases each, the
// remainder len % SLICE_LENGTH goes to slice mid = (snum+1)/2
__device__ __forceinline__ void long_slice(int t, int mid, int bonus, int SL, u32 &start, u32 &len) {
    start = (u32) ((t - 1) * SL + (t > mid ? bonus : 0));
    len = (u32) (SL + (t == mid ? bonus : 0));
}

// buffer_task_long, kmer.cpp:785-871.  The forward walk accumulates into temp_result_left, whose destination (both,
// strand-canonical / forward) is only known when the walk ends; it records into forward at once and corrects the rare
// read that chains from end to end afterwards (see below).  The backward walk records straight into result.backward
// (kmer.cpp:840).
template <int NW, typename WT>
__device__ void run_long(ExactSmem sm, const DevParams &P, const DevBatch &B, TableRef T, u32 unit) {
    constexpr bool UB = NW > 0;
    constexpr int NWB = NW > 0 ? NW : 1;
    const ReadRef rd = uni(get_read(B, rfl(unit)));
    const int SL = P.slice_len;
    const int len = (int) rd.len;
    const int snum = len / SL;
    if (snum <= 0) return;  // read_fastq_long_thread drops reads shorter than SLICE_LENGTH (kmer.cpp:1184)
    const int mid = (snum + 1) / 2, bonus = len % SL;
    const u64 allk = all_k_mask(P.min_mer, P.max_mer);
    // The kernel is instantiated for the REGULAR slice (SLICE_LENGTH bases: NW mask words, 5 for the default 150); the one
    // middle slice that carries the remainder (up to 2 SLICE_LENGTH - 1 bases) is decided without lane bounds -- decide<0>
    // prunes inside eval_k, a walk over its windows -- so that its 10-word masks do not set the register budget of every
    // wave (round 2: 128 VGPRs, 64 of them spilled, 4 waves per SIMD; a walk reaches the middle slice of few reads).
    // Bounds of two neighbouring slices share one lane pass (lanes 0..31 / 32..63) when the k range fits half a wave: a walk
    // that continues finds the next slice's bounds already there.
    constexpr int NS = NWB;
    LaneMasks<NS> mp;
    int mp_lo = 0, mp_hi = 0;  // slices whose bounds sit in the low / high half of mp (0: none)
#ifdef TREW_PHASE_PROFILE
    u32 dbg_steps = 0;
#endif
    auto slice_decide = [&](int t, u64 cand, int dir) {
#ifdef TREW_PHASE_PROFILE
        dbg_steps++;
#endif
        u32 st, sl;
        long_slice(t, mid, bonus, SL, st, sl);
        sm = load_segment(sm, rd, st, sl);
        if (UB && sl <= (u32) (32 * NS - 1)) {
            if (P.max_mer - P.min_mer < 32) {
                if (t != mp_lo && t != mp_hi) {
                    const int tn = t + dir;
                    u32 stn = st, sln = sl;
                    int other = 0;
                    if (tn >= 1 && tn <= snum) {
                        long_slice(tn, mid, bonus, SL, stn, sln);
                        if (sln <= (u32) (32 * NS - 1)) other = tn;
                    }
                    if (!other) {
                        stn = st;
                        sln = sl;
                    }
                    lane_bounds_pair<NS>(rd, st, (int) sl, stn, (int) sln, P.min_mer, P.max_mer, mp);
                    mp_lo = t;
                    mp_hi = other;
                }
                return decide<NW, WT>(sm, P, (int) sl, P.min_mer, P.max_mer, cand, mp, t == mp_lo ? 0 : 32, 32);
            }
            LaneMasks<NS> m5;
            lane_bounds<NS>(rd, st, (int) sl, P.min_mer, P.max_mer, m5);
            return decide<NW, WT>(sm, P, (int) sl, P.min_mer, P.max_mer, cand, m5);
        }
        LaneMasks<1> none;
        none.V[0] = none.E[0] = 0;
        none.ub = 0.0;
        none.runs = 0;
        return decide<0, WT>(sm, P, (int) sl, P.min_mer, P.max_mer, cand, none);
    };
    auto slice_len = [&](int t) { return (int) (SL + (t == mid ? bonus : 0)); };
    // forward chain (kmer.cpp:797-817).  The reference collects the slices of the walk in temp_result_left and only knows at the
    // end where they go: as they are into `forward` (kmer.cpp:858-867) or, if EVERY slice of the read chained, strand-canonical
    // into `both` (kmer.cpp:819-830).  Counts are sums, so the walk records straight into `forward` while it decides -- the
    // class table of the slice is still in LDS (record_live) -- and the rare read that chains from end to end is corrected
    // afterwards: its slices are counted once more, subtracted from `forward` and added to `both`.  (Round 2 walked twice,
    // decide then re-stage and record, for every read whose tail lies at the 5' end: half of all tailed reads.)
    int si[2] = {1, 1}, kmer[2] = {0, 0};
    bool rend[2] = {false, false};
    for (int ti = 1; ti <= snum && (!rend[0] || !rend[1]); ti++) {
        const Decision<WT> d = slice_decide(ti, ti == 1 ? ~0ull : (ti == snum ? ~0ull : allk), 1);
        const bool rh = !rend[0] && d.kh > 0, rl = !rend[1] && d.kl > 0;  // this slice is part of temp_result_left[b]
        if (rh && rl && d.kh == d.kl) {
            record_live<WT>(sm, T, slice_len(ti), d.kh, (1u << TREW_TABLE_FORWARD_HIGH) | (1u << TREW_TABLE_FORWARD_LOW), false, d);
        } else {  // two different k: the first record may count again and overwrite the live table
            Decision<WT> d2 = d;
            if (rh) {
                record_live<WT>(sm, T, slice_len(ti), d.kh, 1u << TREW_TABLE_FORWARD_HIGH, false, d2);
                if (d2.ek != d.kh) d2.ek = 0;
            }
            if (rl) record_live<WT>(sm, T, slice_len(ti), d.kl, 1u << TREW_TABLE_FORWARD_LOW, false, d2);
        }
        const int tk[2] = {d.kh, d.kl};
#pragma unroll
        for (int b = 0; b < 2; b++) {
            if (!rend[b] && tk[b] > 0 && (kmer[b] == tk[b] || ti == 1)) {
                si[b] += 1;
                kmer[b] = tk[b];
            } else {
                rend[b] = true;
            }
        }
    }
    // every slice chained (kmer.cpp:819-830): all of them were recorded at k = kmer[b]; move them from forward to both
    {
        const bool canon_h = si[0] == snum + 1, canon_l = si[1] == snum + 1;
        if (canon_h || canon_l) {
            for (int ti = 1; ti <= snum; ti++) {
#ifdef TREW_PHASE_PROFILE
                dbg_steps++;
#endif
                u32 st, sl;
                long_slice(ti, mid, bonus, SL, st, sl);
                sm = load_segment(sm, rd, st, sl);
                if (canon_h && canon_l && kmer[0] == kmer[1]) {
                    move_to_both<WT>(sm, T, (int) sl, kmer[0], (1u << TREW_TABLE_FORWARD_HIGH) | (1u << TREW_TABLE_FORWARD_LOW),
                                     (1u << TREW_TABLE_BOTH_HIGH) | (1u << TREW_TABLE_BOTH_LOW));
                } else {
                    if (canon_h) move_to_both<WT>(sm, T, (int) sl, kmer[0], 1u << TREW_TABLE_FORWARD_HIGH, 1u << TREW_TABLE_BOTH_HIGH);
                    if (canon_l) move_to_both<WT>(sm, T, (int) sl, kmer[1], 1u << TREW_TABLE_FORWARD_LOW, 1u << TREW_TABLE_BOTH_LOW);
                }
            }
        }
    }
    // backward chain (kmer.cpp:832-856)
    if (si[0] <= snum || si[1] <= snum) {
        int sj[2] = {snum, snum};
        kmer[0] = kmer[1] = 0;
        rend[0] = rend[1] = false;
        for (int tj = snum; (!rend[0] || !rend[1]) && tj >= 1; tj--) {
            const Decision<WT> d = slice_decide(tj, tj == snum ? ~0ull : (tj == 1 ? ~0ull : allk), -1);
            const bool rh = !rend[0] && d.kh > 0, rl = !rend[1] && d.kl > 0;
            if (rh && rl && d.kh == d.kl) {
                record_live<WT>(sm, T, slice_len(tj), d.kh, (1u << TREW_TABLE_BACKWARD_HIGH) | (1u << TREW_TABLE_BACKWARD_LOW), false, d);
            } else {  // two different k: the first record may count again and overwrite the live table
                Decision<WT> d2 = d;
                if (rh) {
                    record_live<WT>(sm, T, slice_len(tj), d.kh, 1u << TREW_TABLE_BACKWARD_HIGH, false, d2);
                    if (d2.ek != d.kh) d2.ek = 0;
                }
                if (rl) record_live<WT>(sm, T, slice_len(tj), d.kl, 1u << TREW_TABLE_BACKWARD_LOW, false, d2);
            }
            const int tk[2] = {d.kh, d.kl};
#pragma unroll
            for (int b = 0; b < 2; b++) {
                if (sj[b] >= si[b] && !rend[b] && tk[b] > 0 && (kmer[b] == tk[b] || tj == snum)) {
                    sj[b] -= 1;
                    kmer[b] = tk[b];
                } else {
                    rend[b] = true;
                }
            }
        }
    }
#ifdef TREW_PHASE_PROFILE
    if (lane_id() == 0) {
        atomicMax(&g_phase[24], (unsigned long long) dbg_steps);
        const int bucket = dbg_steps <= 4 ? 25 : dbg_steps <= 16 ? 26 : dbg_steps <= 64 ? 27 : dbg_steps <= 128 ? 28 : dbg_steps <= 256 ? 29 : 30;
        atomicAdd(&g_phase[bucket], 1ull);
        atomicAdd(&g_phase[31], (unsigned long long) dbg_steps);
    }
#endif
}

// ------------------------------------------------------------------ long reads, two at a time
// buffer_task_long (kmer.cpp:785-871) for TWO reads per wave, one per half-wave (decide_group with 32-lane groups: a slice of a
// long read has ~15 runs of adjacent same-class windows at the k that matters, more than a DPP row has lanes).  Each half walks
// its own read -- forward chain, then backward chain -- one slice per trip of the loop, and pulls its next read from the
// worklist when its walks end, so the two halves never wait for each other's reads.  A slice is decided, recorded from the
// group's registers and chained in row space; what does not fit goes, for that one slice, through the wave-per-slice code of
// run_long (slice_old below): the middle slice that carries the remainder (10-word masks), a slice the group gave back, a record
// at a k whose class table the group did not keep, and the rare read whose forward chain runs to the end (its slices are moved
// from `forward` to `both` afterwards, as run_long does).
// Only instantiated for 64-bit words and 5-word masks (SLICE_LENGTH <= 159), with a k range of at most 32 values.
template <int NW, typename WT>
__device__ void run_long_groups(ExactSmem sm, const DevParams &P, const DevBatch &B, TableRef T, const u32 *wl, u32 *heads, u32 n) {
    constexpr u32 kShards = 8, kHeadStride = 32;
    constexpr int G = 32;
    const u32 lane = lane_id(), gi = lane >> 5, j = lane & 31u;
    const int SL = P.slice_len;
    // ---- the worklist (one read per claim; shards as in exact_kernel) ----
    u32 sh = blockIdx.x & (kShards - 1u), shards_tried = 0;
    bool dry = false;
    auto claim = [&]() -> u32 {  // worklist position, or ~0 when every shard has run dry
        for (;;) {
            u32 c = 0;
            if (lane == 0) c = atomicAdd(&heads[sh * kHeadStride], 1u);
            c = rfl(c);
            const u64 pos = (u64) c * kShards + sh;
            if (pos < n) return (u32) pos;
            u32 seen = 0;
            do {  // a shard that a plain load already shows dry is not asked atomically
                if (++shards_tried >= kShards) return ~0u;
                sh = (sh + 1u) & (kShards - 1u);
                seen = rfl(__hip_atomic_load(&heads[sh * kHeadStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            } while ((u64) seen * kShards + sh >= n);
        }
    };
    // ---- per-group state, the same in the 32 lanes of a group ----
    u32 phase = 0;  // 0 idle (wants a read), 1 forward chain, 2 backward chain
    u64 rw = 0;     // the read's triples (global memory)
    u32 rlen = 0, rnw = 0;
    int snum = 0, mid = 0, bonus = 0, t = 0;
    u32 si0 = 1, si1 = 1, sj0 = 0, sj1 = 0, kmer0 = 0, kmer1 = 0, rend = 0;
    const u32 tab_fh = 1u << TREW_TABLE_FORWARD_HIGH, tab_fl = 1u << TREW_TABLE_FORWARD_LOW;
    const u32 tab_bh = 1u << TREW_TABLE_BACKWARD_HIGH, tab_bl = 1u << TREW_TABLE_BACKWARD_LOW;
    const DevTable Tv = load_table(T);
    for (;;) {
        // ---- 1. a read for every idle group ----
        for (u32 gs = 0; gs < 2u && !dry; gs++) {
            if ((u32) __builtin_amdgcn_readlane((int) phase, (int) (32u * gs)) != 0u) continue;
            for (;;) {
                const u32 pos = claim();
                if (pos == ~0u) {
                    dry = true;
                    break;
                }
                const ReadRef rd = uni(get_read(B, (u64) rfl(wl[pos])));
                const int sn = (int) rd.len / SL;
                if (sn <= 0) continue;  // read_fastq_long_thread drops reads shorter than SLICE_LENGTH (kmer.cpp:1184)
                const bool mine = gi == gs;
                phase = mine ? 1u : phase;
                rw = mine ? (u64) rd.w : rw;
                rlen = mine ? rd.len : rlen;
                rnw = mine ? rd.nw : rnw;
                snum = mine ? sn : snum;
                mid = mine ? (sn + 1) / 2 : mid;
                bonus = mine ? (int) rd.len % SL : bonus;
                t = mine ? 1 : t;
                si0 = mine ? 1u : si0;
                si1 = mine ? 1u : si1;
                kmer0 = mine ? 0u : kmer0;
                kmer1 = mine ? 0u : kmer1;
                rend = mine ? 0u : rend;
                break;
            }
        }
        if (!__any(phase != 0u)) break;
        // ---- 2. the slice of every active group ----
        const bool active = phase != 0u;
        u32 st = 0, sl = (u32) SL;
        if (active) long_slice(t, mid, bonus, SL, st, sl);
        const bool fits = active && sl <= (u32) (32 * NW - 1);
        // The slice's triples travel from global memory ONCE per trip, coalesced, into 32 words of LDS per group (the upper half
        // of kGroupBnd: the groups' prepared planes take 2 x 6 NW = 60 of its 128 words); staging and row_prepare read them from
        // there.  (Each used to load them itself: six dependent global loads per staging lane and eighteen per preparing lane.)
        static_assert(2 * 6 * NW <= 64 && 3 * (NW + 2) <= 32, "slice triples + prepared planes must fit kGroupBnd");
        u32 *const slice_raw = sm_group(sm) + kGroupBnd + 64u + 32u * gi;
        const u32 w_lo = st >> 5;                                                  // first triple of the slice
        const u32 w_hi = fits ? min(rnw, ((st + sl + 31u) >> 5) + 1u) : w_lo;        // one past its last (+ the funnel shift's look-ahead)
        lds_sync();
        if (j < 3u * (w_hi - w_lo)) slice_raw[j] = ((const u32 *) rw)[3u * w_lo + j];
        lds_sync();
        ReadRef rd;  // the slice as a read of its own, staged in LDS
        rd.w = (const u32 *) slice_raw;
        rd.len = rlen;
        rd.nw = w_hi - w_lo;  // (0 for a group that sits this trip out: nothing is read)
        const u32 sst = st - 32u * w_lo;  // the slice's first base inside those triples
        // bases of the slice into seq[] / nmask[] of range gi (as stage_bases)
        {
            const u32 segwords = exact_rangewords(sm.cap), nwords = (sl + 31u) >> 5;
            u64 *seq = sm_seq(sm) + gi * segwords;
            u32 *nmk = sm_nmask(sm) + gi * segwords;
            if (fits) {
                for (u32 l = j; l < segwords; l += 32u) {
                    u64 sq = 0;
                    u32 nmv = 0xffffffffu;
                    if (l < nwords) {
                        u32 lo1[1], hi1[1], nm1[1];
                        load_planes_lds<1>(rd, sst + 32u * l, lo1, hi1, nm1);
                        nmv = nm1[0] | ~low_mask<true>((int) sl - 32 * (int) l);
                        const u32 lq = lo1[0] & ~nmv, hq = hi1[0] & ~nmv;
                        sq = spread32(__brev(lq)) | (spread32(__brev(hq)) << 1);
                    }
                    seq[l] = sq;
                    nmk[l] = nmv;
                }
            }
        }
        Segment sg;
        sg.mate = 0;
        sg.start = sst;
        sg.len = sl;
        sg.kmin = P.min_mer;
        sg.kmax = P.max_mer;
        sg.valid = fits;
        row_prepare<NW, G, true>(sm, rd, sg, fits);
        lds_sync();
        RowSeg<NW> rs;
        row_load<NW, G>(sm, (int) sl, rs);
        const u32 bnd0 = fits ? bound_at_k<NW>(rs, (int) sl, P.min_mer + (int) j, P.max_mer, P) : 0u;
        // (the staged slice starts at base 0 of its range: s0 = range_base + 0)
        Segment sv = sg;
        sv.start = 0;
        const GroupOut<WT> o = decide_group<NW, WT, false, G>(sm, P, rs, bnd0, 0u, gi, sv, fits);
        u32 kh = o.kk & 255u, kl = (o.kk >> 8) & 255u;
        const u32 myk = o.saved & 255u, items = (o.saved >> 8) & 255u;
        // what of it this trip records: forward chain -> temp_result_left -> forward (kmer.cpp:800-817, 858-867), backward chain ->
        // backward (kmer.cpp:840)
        u32 rh = ((rend & 1u) ^ 1u) & (kh != 0u ? 1u : 0u), rl = (((rend >> 1) & 1u) ^ 1u) & (kl != 0u ? 1u : 0u);
        // ---- 3. the wave-per-slice code for what the groups cannot take ----
        u32 old = active && (!fits || o.punt || (rh && kh != myk) || (rl && kl != myk)) ? 1u : 0u;
        if (__any(old != 0u)) {
            for (u32 gs = 0; gs < 2u; gs++) {
                const int src = (int) (32u * gs);
                if ((u32) __builtin_amdgcn_readlane((int) old, src) == 0u) continue;
                ReadRef r1;
                r1.w = (const u32 *) readlane_word(rw, src);
                r1.len = (u32) __builtin_amdgcn_readlane((int) rlen, src);
                r1.nw = (u32) __builtin_amdgcn_readlane((int) rnw, src);
                const u32 st1 = (u32) __builtin_amdgcn_readlane((int) st, src), sl1 = (u32) __builtin_amdgcn_readlane((int) sl, src);
                const u32 ph1 = (u32) __builtin_amdgcn_readlane((int) phase, src), re1 = (u32) __builtin_amdgcn_readlane((int) rend, src);
                count_fallback(kFallbackGroupPunt);
                __syncthreads();
                const ExactSmem s1 = load_segment(sm, r1, st1, sl1);
                Decision<WT> d;
                if (sl1 <= (u32) (32 * NW - 1)) {
                    LaneMasks<NW> m5;
                    lane_bounds<NW>(r1, st1, (int) sl1, P.min_mer, P.max_mer, m5);
                    d = decide<NW, WT>(s1, P, (int) sl1, P.min_mer, P.max_mer, ~0ull, m5);
                } else {
                    LaneMasks<1> none;
                    none.V[0] = none.E[0] = 0;
                    none.ub = 0.0;
                    none.runs = 0;
                    d = decide<0, WT>(s1, P, (int) sl1, P.min_mer, P.max_mer, ~0ull, none);
                }
                const bool r_h = !(re1 & 1u) && d.kh > 0, r_l = !(re1 & 2u) && d.kl > 0;
                const u32 th = ph1 == 1u ? tab_fh : tab_bh, tl = ph1 == 1u ? tab_fl : tab_bl;
                if (r_h && r_l && d.kh == d.kl) {
                    record_live<WT>(s1, T, (int) sl1, d.kh, th | tl, false, d);
                } else {  // two different k: the first record may count again and overwrite the live table
                    Decision<WT> d2 = d;
                    if (r_h) {
                        record_live<WT>(s1, T, (int) sl1, d.kh, th, false, d2);
                        if (d2.ek != d.kh) d2.ek = 0;
                    }
                    if (r_l) record_live<WT>(s1, T, (int) sl1, d.kl, tl, false, d2);
                }
                __syncthreads();
                const bool mine = gi == gs;
                kh = mine ? (u32) d.kh : kh;
                kl = mine ? (u32) d.kl : kl;
            }
        }
        // ---- 4. records straight from the groups' class tables ----
        if (active && old == 0u && j < items && o.kept_cnt != 0u) {
            const u32 th = phase == 1u ? tab_fh : tab_bh, tl = phase == 1u ? tab_fl : tab_bl;
            const u32 mask = (rh ? th : 0u) | (rl ? tl : 0u);
            for (u32 tm = mask; tm; tm &= tm - 1u) cached_add(sm, Tv, __ffs((int) tm) - 1, (int) myk, o.kept_canon, o.kept_cnt);
        }
        // ---- 5. the chains (kmer.cpp:806-817, 845-856) and the next slice ----
        u32 corr = 0, fk0 = 0, fk1 = 0;  // the forward chain ran to the end for baseline bit b, with these k
        if (active) {
            const u32 first = phase == 1u ? (t == 1 ? 1u : 0u) : (t == snum ? 1u : 0u);
            const u32 ok0 = ((rend & 1u) ^ 1u) & (kh != 0u ? 1u : 0u) & ((kmer0 == kh ? 1u : 0u) | first) & (phase == 1u ? 1u : (sj0 >= si0 ? 1u : 0u));
            const u32 ok1 = (((rend >> 1) & 1u) ^ 1u) & (kl != 0u ? 1u : 0u) & ((kmer1 == kl ? 1u : 0u) | first) & (phase == 1u ? 1u : (sj1 >= si1 ? 1u : 0u));
            if (phase == 1u) {
                si0 += ok0;
                si1 += ok1;
            } else {
                sj0 -= ok0;
                sj1 -= ok1;
            }
            kmer0 = ok0 ? kh : kmer0;
            kmer1 = ok1 ? kl : kmer1;
            rend |= (ok0 ^ 1u) | ((ok1 ^ 1u) << 1);
            const bool more = rend != 3u;
            if (phase == 1u) {
                if (more && t + 1 <= snum) {
                    t++;
                } else {  // forward chain over
                    corr = (si0 == (u32) snum + 1u ? 1u : 0u) | (si1 == (u32) snum + 1u ? 2u : 0u);
                    fk0 = kmer0;
                    fk1 = kmer1;
                    if (si0 <= (u32) snum || si1 <= (u32) snum) {  // backward chain, kmer.cpp:832-835: its own chain state starts empty
                        phase = 2u;
                        t = snum;
                        sj0 = sj1 = (u32) snum;
                        kmer0 = kmer1 = 0u;
                        rend = 0u;
                    } else {
                        phase = 0u;
                    }
                }
            } else {
                if (more && t - 1 >= 1) {
                    t--;
                } else {
                    phase = 0u;
                }
            }
        }
        // every slice chained (kmer.cpp:819-830): all of them were recorded into `forward` at k = kmer[b]; move them to `both`
        if (__any(corr != 0u)) {
            for (u32 gs = 0; gs < 2u; gs++) {
                const int src = (int) (32u * gs);
                const u32 c1 = (u32) __builtin_amdgcn_readlane((int) corr, src);
                if (c1 == 0u) continue;
                ReadRef r1;
                r1.w = (const u32 *) readlane_word(rw, src);
                r1.len = (u32) __builtin_amdgcn_readlane((int) rlen, src);
                r1.nw = (u32) __builtin_amdgcn_readlane((int) rnw, src);
                const int sn1 = __builtin_amdgcn_readlane(snum, src), mid1 = __builtin_amdgcn_readlane(mid, src), bo1 = __builtin_amdgcn_readlane(bonus, src);
                const int k0 = __builtin_amdgcn_readlane((int) fk0, src), k1 = __builtin_amdgcn_readlane((int) fk1, src);
                const bool canon_h = (c1 & 1u) != 0u, canon_l = (c1 & 2u) != 0u;
                for (int ti = 1; ti <= sn1; ti++) {
                    u32 st1, sl1;
                    long_slice(ti, mid1, bo1, SL, st1, sl1);
                    __syncthreads();
                    const ExactSmem s1 = load_segment(sm, r1, st1, sl1);
                    if (canon_h && canon_l && k0 == k1) {
                        move_to_both<WT>(s1, T, (int) sl1, k0, tab_fh | tab_fl, (1u << TREW_TABLE_BOTH_HIGH) | (1u << TREW_TABLE_BOTH_LOW));
                    } else {
                        if (canon_h) move_to_both<WT>(s1, T, (int) sl1, k0, tab_fh, 1u << TREW_TABLE_BOTH_HIGH);
                        if (canon_l) move_to_both<WT>(s1, T, (int) sl1, k1, tab_fl, 1u << TREW_TABLE_BOTH_LOW);
                    }
                }
                __syncthreads();
            }
        }
    }
}
