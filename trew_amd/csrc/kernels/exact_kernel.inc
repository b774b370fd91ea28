// kernels/exact_kernel.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// exact_kernel<NW, MODE, WT>: persistent single-wave workgroups, self-scheduled from the worklist.

// NW > 0: every staged segment fits 32*NW-1 bases and decide() prunes with lane_bounds<NW>;
// NW == 0: long segments, pruning happens inside eval_k instead.
#ifndef TREW_EXACT_SHORT_WAVES
#define TREW_EXACT_SHORT_WAVES 5  // waves per SIMD the short-read kernel (group pass) is compiled for: 96 VGPRs; 4 (128, no spills) and 6 (80) lose 2-4 % on the two-slot step (profiles/r04)
#endif
#ifndef TREW_EXACT_PAIR_WAVES
#define TREW_EXACT_PAIR_WAVES 4  // the pair kernel: 128 VGPRs (12 spilled), 3.4 ms against 3.65 at 5 waves (44 spilled: 1.5 GB of scratch writes a launch) and 4.1 at 6
#endif
#ifndef TREW_EXACT_LONG_WAVES
#define TREW_EXACT_LONG_WAVES 4  // the long-read kernel with two reads a wave (run_long_groups, 5-word masks)
#endif
template <int NW, int MODE>
constexpr int exact_waves(bool narrow) {
    return NW >= 10 ? 4
                    : (narrow && NW > 0 && MODE == TREW_MODE_SHORT
                           ? TREW_EXACT_SHORT_WAVES
                           : (narrow && NW > 0 && MODE == TREW_MODE_PAIR ? TREW_EXACT_PAIR_WAVES : (narrow && NW == 5 && MODE == TREW_MODE_LONG ? TREW_EXACT_LONG_WAVES : 6)));
}
template <int NW, int MODE, typename WT>
__global__ __launch_bounds__(64, (exact_waves<NW, MODE>(sizeof(WT) == 8))) void exact_kernel(DevParams P, DevBatch B, DevTableG1 TG, const u32 *wl,
                                                   u32 *wl_count, u32 *wl_count_next, u32 wl_cap, SegResults R, u32 cap, u32 rawwords,
                                                   const u32 *bnd, u32 bnd_cap, const u32 *live) {
    // bnd / bnd_cap: the packed bounds the bounds pass left for the first bnd_cap worklist entries (kernels/bounds_pass.inc; 0: none --
    // only the short-read kernel on 3-word masks is ever given any)
    // live: the list that kernel reads in front of the worklist (kLive below); everywhere else it is not looked at
    // The table descriptor is a by-value kernel argument that the kernel never touches as such: it hands a POINTER to it --
    // into the kernarg segment of this very dispatch -- down to the functions that add rows (TableRef, exact_core.inc), which
    // read its fields with scalar loads when they need them.  (A device-resident copy of the descriptor, written once at
    // init, was the first form of this: the kernarg segment is the one piece of memory whose visibility to a dispatch the
    // launch itself guarantees, whatever other contexts left in the caches at the address of a freed and re-used copy.)
    typedef ExactKernArgs KernArgs;  // the argument list as the kernarg ABI lays it out (decide_group.inc)
    // the kernarg ABI lays arguments out in order at their natural alignment: all three are 8-byte aligned structs of 8-byte
    // multiples, so TG sits right behind P and B.  A change of either struct that breaks this fails here, not at run time.
    static_assert(alignof(DevParams) == 8 && alignof(DevBatch) == 8 && alignof(DevTableG1) == 8, "kernarg layout: 8-byte aligned argument structs");
    static_assert(sizeof(DevParams) % 8 == 0 && sizeof(DevBatch) % 8 == 0, "kernarg layout: no padding between the argument structs");
    static_assert(offsetof(KernArgs, TG) == sizeof(DevParams) + sizeof(DevBatch), "kernarg layout: TG follows P and B");
    static_assert(offsetof(DevTableG1, t) == 0, "TableRef points at DevTableG1::t");
    const TableRef T = (TableRef) ((const char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(KernArgs, TG));
    // A slot owns two counter blocks and alternates between them: while this launch consumes one, its first wave
    // clears the other for the slot's next submit (stream order puts that submit's prefilter after this kernel), so
    // a submit needs no memset call.
#ifdef TREW_AB_EXACT_PRIO
    __builtin_amdgcn_s_setprio(TREW_AB_EXACT_PRIO);  // A/B builds: issue priority of the exact kernel's waves beside the prefilter's
#endif
    if (blockIdx.x == 0 && wl_count_next) {
        for (u32 i = lane_id(); i < (1u + 8u) * 32u; i += 64u) wl_count_next[i] = 0u;
    }
    ExactSmem sm;
    sm.lds = lds_offset_in_kernel();
    sm.cap = cap;
    sm.rawwords = rawwords;
    sm.s0 = 0;
    sm.rs = sm.rnw = 0;
    sm.rw = nullptr;
    u32 n = wl_count[0];
    n = n < wl_cap ? n : wl_cap;
    // The short-read kernel on 3-word masks works on the list the bounds pass left (bounds_pass.inc): `live`, whose
    // wl_count[kStoredPrefixWord] entries have their packed bounds stored at their positions, and behind them the worklist's
    // entries from bnd_cap on, which have none.  Where that pass dropped nothing (TREW_FLAG_DEBUG_NO_LIVE_LIST: live = wl, the word =
    // min(n, bnd_cap)) or did not run (the word and bnd_cap are zero) this is the worklist itself.
    constexpr bool kLive = MODE == TREW_MODE_SHORT && NW == 3 && sizeof(WT) == 8;
    if constexpr (kLive) n = wl_count[kStoredPrefixWord] + (n > bnd_cap ? n - bnd_cap : 0u);
#ifdef TREW_PHASE_PROFILE
    if (lane_id() < 32) ph_lds()[lane_id()] = 0;
    __syncthreads();
#endif
    PH_T0(t_total);
    if (P.flags & TREW_FLAG_DEBUG_POISON_LDS) {  // tests
        // the descriptor read through the kernarg pointer must be the by-value argument, dword for dword (a layout assumption
        // the static_asserts above cannot see -- e.g. a toolchain that reorders kernel arguments -- raises kDiagKernarg)
        if (blockIdx.x == 0 && lane_id() == 0) {
            const u32 *through = (const u32 *) T, *byval = (const u32 *) &TG;
            bool same = true;
            for (u32 i = 0; i < sizeof(DevTableG1) / 4; i++) same = same && through[i] == byval[i];
            if (!same) atomicAdd(&TG.t.overflow[kDiagKernarg], 1u);
        }
        // nothing may depend on what a previous kernel left in LDS
        const u32 nb = exact_lds_bytes(cap, rawwords, sizeof(WT));
        for (u32 i = lane_id() * 4u; i < nb; i += 256u) *(u32 *) (lds0() + i) = 0xA5C3F00Du ^ (i * 2654435761u);
        __syncthreads();
    }
    cache_clear(sm);
    const bool use_group = P.max_mer - P.min_mer < 32 && !(P.flags & TREW_FLAG_DEBUG_NO_GROUP);
    if (use_group) group_fill_multiples(sm, P);  // (visible to the wave by the barriers every pass crosses before it reads them)
    // dynamic self-scheduling: reads differ 10x in cost, so waves pull work from device counters
    // instead of a static stride.  One returning atomic on a single word saturates at ~88
    // dequeues/us on MI355X (MI355X_MICROARCH.md, row "dequeue") -- 2 ms for 176 k reads -- so the
    // queue head is sharded 8 ways (own cache line each; chunk c of shard s = global chunk 8c+s)
    // and a wave whose shard runs dry steals from the next one.
    // A chunk is kChunk consecutive worklist items: their reads are fetched together so that the
    // dependent global round trips (queue head -> worklist entry -> read words) are paid once
    // per chunk, not once per read (measured: 0.40 ms of a 1.3 ms launch was this latency chain).
    // Long reads cost 2 to 40 slice evaluations each: one read per dequeue keeps the waves level at the end of the queue
    // (exact kernel on 1 M ONT-like reads 4.82 -> 4.10 ms).
    constexpr u32 kChunk = MODE == TREW_MODE_LONG ? 1 : 4, kShards = 8, kHeadStride = 32;
    u32 *heads = wl_count + kHeadStride;
    const u32 my = blockIdx.x & (kShards - 1);
    const u32 lane = lane_id();
    if constexpr (MODE == TREW_MODE_SHORT || MODE == TREW_MODE_SEGMENT || MODE == TREW_MODE_PAIR) {
        // ---- short reads and pairs: a software pipeline over the chunks (a chunk = four reads: four units, or two pairs) ----
        // The dependent round trips of a chunk (queue head -> worklist entries -> read words) used to be paid in front of every
        // chunk, ~13 us of a wave's ~35 us per chunk (tools/attribute_insts.sh: the kernel with everything but the fetch removed
        // still took 38 % of its time).  Now the NEXT chunk travels while the current one is computed: its worklist entries and
        // then its read words are written straight into a second LDS buffer by the load unit (global_load_lds: no destination
        // registers, so nothing is held across the passes and no call inside a pass has to wait for them), and the queue head for
        // the chunk after it is asked for one pass ahead.  Three hook points per chunk: P0 in front of its first pass (entries
        // of the next chunk), P1 between its passes (words of the next chunk, head of the one after), P2 behind it (wait, swap).
        // Lane t holds the descriptor of item t; per buffer, struct-of-arrays in LDS: unit[4] len[4] off_lo[4] off_hi[4] staged[4].
        constexpr u32 kMetaWords = 32;
        constexpr u32 kPer = MODE == TREW_MODE_PAIR ? 2u : 1u;  // reads per unit
        constexpr u32 kUnits = kChunk / kPer;                   // units per chunk
        u32 *const meta_base = sm_intent(sm);
        u32 *const raw_base = sm_raw(sm);
        u32 sh = my, shards_tried = 0, cpend = 0;
        auto issue_claim = [&]() __attribute__((always_inline)) {
            if (lane == 0) cpend = atomicAdd(&heads[sh * kHeadStride], 1u);
        };
        // first item of the claimed chunk, or ~0 when every shard has run dry (then and only then the wave is done)
        auto resolve_claim = [&]() __attribute__((always_inline)) -> u64 {
            u32 c = rfl(cpend);
            for (;;) {
                const u64 w0l = ((u64) c * kShards + sh) * kUnits;
                if (w0l < n) return w0l;
                // This shard is dry: the next one, synchronously (end of the queue only).  A shard that a plain load already shows
                // dry is not asked atomically -- heads only grow, and at the end of the queue every wave of the grid walks all eight:
                // 40 k returning atomics on eight words are ~50 us of the launch's tail at ~88 a microsecond and word.
                u32 seen = 0;
                do {
                    if (++shards_tried >= kShards) return ~0ull;
                    sh = (sh + 1u) & (kShards - 1u);
                    seen = rfl(__hip_atomic_load(&heads[sh * kHeadStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                } while (((u64) seen * kShards + sh) * kUnits >= n);
                u32 c2 = 0;
                if (lane == 0) c2 = atomicAdd(&heads[sh * kHeadStride], 1u);
                c = rfl(c2);
            }
        };
        auto chunk_items = [&](u64 w0l) __attribute__((always_inline)) -> u32 { return (u32) ((w0l + kUnits < n ? w0l + kUnits : n) - w0l); };
        // step A: the chunk's worklist entries -> unit[] of buffer bf
        auto fetch_units = [&](u32 bf, u64 w0l, u32 nit) __attribute__((always_inline)) {
            const u32 *src = wl + w0l + lane;
            if constexpr (kLive) {  // (all three from memory: scalar loads a chunk, no register held across the passes)
                typedef const __attribute__((address_space(4))) u64 *c64;
                typedef const __attribute__((address_space(4))) u32 *c32;
                const u64 ka = (u64) __builtin_amdgcn_kernarg_segment_ptr();
                const u32 pre = *(c32) (*(c64) (ka + offsetof(KernArgs, wl_count)) + 4u * kStoredPrefixWord);
                const u32 p = (u32) w0l + lane;  // (positions fit 32 bits: n <= wl_cap)
                src = p < pre ? (const u32 *) *(c64) (ka + offsetof(KernArgs, live)) + p : wl + (p - pre) + *(c32) (ka + offsetof(KernArgs, bnd_cap));
            }
            if (lane < nit) __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) u32 *) (meta_base + bf * kMetaWords), 4, 0, 0);
        };
        // step B (unit[] has landed): descriptors, then the reads' words -> raw[] of buffer bf
        auto fetch_words = [&](u32 bf, u32 nit) __attribute__((always_inline)) {
            // The batch descriptor is re-read from the kernel-argument segment here, where it is needed (scalar loads, cached), instead
            // of living in ten SGPRs across the passes: those were spilled into VGPR lanes, and the VGPRs that held them to scratch
            // (15 dword stores a chunk -- 107 MB of the launch's HBM writes, profiles/r04/README.md).
            typedef const __attribute__((address_space(4))) u64 *c64;
            typedef const __attribute__((address_space(4))) u32 *c32;
            const u64 ka = (u64) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(KernArgs, B);
            DevBatch Bk;
            Bk.words = (const u32 *) *(c64) (ka + offsetof(DevBatch, words));
            Bk.offsets = (const u32 *) *(c64) (ka + offsetof(DevBatch, offsets));
            Bk.lengths = (const u32 *) *(c64) (ka + offsetof(DevBatch, lengths));
            Bk.uniform_length = *(c32) (ka + offsetof(DevBatch, uniform_length));
            Bk.uniform_stride = *(c32) (ka + offsetof(DevBatch, uniform_stride));
            u32 *meta = meta_base + bf * kMetaWords;
            const bool mine = lane < nit * kPer;  // lane t: read t of the chunk = mate (t % kPer) of its unit
            const u64 read_l = mine ? (u64) meta[lane / kPer] * kPer + lane % kPer : 0ull;
            u64 off_l = 0;
            u32 len_l = 0;
            if (mine) {
                off_l = Bk.offsets ? (u64) Bk.offsets[read_l] : read_l * (u64) Bk.uniform_stride;
                len_l = Bk.lengths ? Bk.lengths[read_l] : Bk.uniform_length;
            }
            if (lane < kChunk) {
                meta[4 + lane] = len_l;
                meta[8 + lane] = (u32) off_l;
                meta[12 + lane] = (u32) (off_l >> 32);
                meta[16 + lane] = 3u * ((len_l + 31u) >> 5) <= sm.rawwords ? 1u : 0u;
            }
#pragma unroll
            for (u32 t = 0; t < kChunk; t++) {
                const u64 off = readlane_word(off_l, (int) t);
                const u32 nwords = 3u * (((u32) __builtin_amdgcn_readlane((int) len_l, (int) t) + 31u) >> 5);
                if (nwords <= sm.rawwords) {
                    u32 *dst = raw_base + (bf * kChunk + t) * sm.rawwords;
                    for (u32 j0 = 0; j0 < nwords; j0 += 64u)
                        if (j0 + lane < nwords) __builtin_amdgcn_global_load_lds(Bk.words + off + j0 + lane, (__attribute__((address_space(3))) u32 *) (dst + j0), 4, 0, 0);
                }
            }
        };
        auto landed = [&]() __attribute__((always_inline)) {
            __builtin_amdgcn_s_waitcnt(0);  // every counter: the LDS writes of the load unit count as vector-memory operations
            __syncthreads();
        };
        u32 bf = 0;
        PH_T0(t_stage0);
        issue_claim();
        u64 cur = resolve_claim();
        if (cur != ~0ull) {  // prologue: the first chunk is fetched in the open
            fetch_units(0, cur, chunk_items(cur));
            landed();
            fetch_words(0, chunk_items(cur));
            issue_claim();
            landed();
        }
        PH_ADD(PH_STAGE, t_stage0);
        constexpr bool kGroup = MODE == TREW_MODE_SHORT && sizeof(WT) == 8 && (NW == 3 || NW == 5);
        bool grouped = false;
        if constexpr (kGroup) grouped = use_group;
        while (cur != ~0ull) {
            TREW_MARK(chunk);
            const u32 nit = chunk_items(cur);
            u32 *const meta = meta_base + bf * kMetaWords;
            // P0: the next chunk's worklist entries start travelling
            PH_T0(t_p0);
            const u64 nxt = resolve_claim();
            PH_ADD(PH_STAGE, t_p0);  // PH_STAGE = what the wave still waits for its input: the queue head here, the two landings below
            const u32 nxt_nit = nxt != ~0ull ? chunk_items(nxt) : 0u;
            if (nxt_nit) fetch_units(bf ^ 1u, nxt, nxt_nit);
            const u32 hook = nit < kUnits / 2u ? nit : kUnits / 2u;  // between the chunk's two passes (two reads each / one pair each)
            PH_CNT(PH_N_READS, nit);
            auto item = [&](u32 t, ReadRef &rd, u32 &unit, bool &staged) __attribute__((always_inline)) {
                rd.len = rfl(meta[4 + t]);
                rd.nw = (rd.len + 31u) >> 5;
                unit = rfl(meta[t / kPer]);
                const u64 off = ((u64) rfl(meta[12 + t]) << 32) | rfl(meta[8 + t]);
                staged = rfl(meta[16 + t]) != 0u;
                rd.w = staged ? (const u32 *) (raw_base + (bf * kChunk + t) * sm.rawwords) : B.words + off;
            };
            // Reads whose halves fit the group pass go two at a time: the four halves are decided in lock step, one per DPP
            // row (decide_group.inc).  Anything else -- too short for halves, not staged in LDS, a k range wider than 32,
            // 128-bit words -- keeps a wave per segment.
            ReadRef held;  // a group-able read waiting for a partner
            held.w = nullptr;
            held.len = held.nw = 0;
            bool have_held = false;
            u32 held_pos = 0;  // its worklist position (run_short_group: the stored bounds of an item are found by it)
            for (u32 t = 0; t <= nit; t++) {  // not unrolled: one copy of each driver; trip nit flushes a read left waiting
                if (t == hook && nxt_nit) {  // P1: the entries are there; the next chunk's words start travelling, and the head after it
                    PH_T0(t_p1);
                    landed();
                    PH_ADD(PH_STAGE, t_p1);
                    fetch_words(bf ^ 1u, nxt_nit);
                    issue_claim();
                }
                if constexpr (MODE == TREW_MODE_PAIR) {  // unit t = reads 2 t and 2 t + 1 of the chunk
                    if (t < nit) {
                        ReadRef r0, r1;
                        u32 unit = 0, unit1 = 0;
                        bool st0, st1;
                        item(2u * t, r0, unit, st0);
                        item(2u * t + 1u, r1, unit1, st1);
                        run_pair<NW, WT>(sm, P, T, unit, r0, r1);
                        __syncthreads();
                    }
                    continue;
                }
                ReadRef rd;
                rd.w = nullptr;
                rd.len = rd.nw = 0;
                u32 unit = 0;
                bool ok = false;
                if (t < nit) {
                    bool staged;
                    item(t, rd, unit, staged);
                    ok = grouped && staged && 4 * P.min_mer <= (int) rd.len;
                    if (!ok) {
                        if (MODE == TREW_MODE_SHORT)
                            run_short<NW, WT>(sm, P, T, rd);
                        else
                            run_segment<NW, WT>(sm, P, T, unit, rd, R);
                        __syncthreads();
                        continue;
                    }
                }
                if constexpr (kGroup) {
                    const u32 pos = (u32) cur + t;  // (worklist positions fit 32 bits: n <= wl_cap)
                    if (ok && !have_held) {
                        held = rd;
                        held_pos = pos;
                        have_held = true;
                    } else if (have_held) {
                        ReadRef second = held;  // (by value: a reference to one of two structs would put both in scratch memory)
                        if (ok) second = rd;
                        if constexpr (NW == 3) {
                            StoredBounds sb;
                            sb.posA = held_pos;
                            sb.posB = ok ? pos : held_pos;
                            // (the triples of a read follow from its length: held.nw is not kept across the trips, held_pos takes its register)
                            ReadRef first = held;
                            first.nw = (first.len + 31u) >> 5;
                            second.nw = (second.len + 31u) >> 5;
                            run_short_group<NW, WT>(sm, P, T, first, second, ok, sb);
                        } else {
                            run_short_group<NW, WT>(sm, P, T, held, second, ok, NoStoredBounds());
                        }
                        have_held = false;
                    }
                }
            }
            // P2: the next chunk is (or soon will be) in the other buffer
            PH_T0(t_p2);
            if (nxt_nit) landed();
            PH_ADD(PH_STAGE, t_p2);
            cur = nxt;
            bf ^= 1u;
        }
    } else if (MODE == TREW_MODE_LONG && sizeof(WT) == 8 && NW == 5 && use_group) {
        if constexpr (MODE == TREW_MODE_LONG && sizeof(WT) == 8 && NW == 5) run_long_groups<NW, WT>(sm, P, B, T, wl, heads, n);
    } else {
        for (u32 attempt = 0; attempt < kShards; attempt++) {
            const u32 sh = (my + attempt) & (kShards - 1);
            for (;;) {
                u32 c = 0;
                if (lane == 0) c = atomicAdd(&heads[sh * kHeadStride], 1u);
                c = rfl(c);
                const u64 w0l = ((u64) c * kShards + sh) * kChunk;
                if (w0l >= n) break;
                const u32 w0 = (u32) w0l;
                const u32 nit = (w0 + kChunk < n ? w0 + kChunk : n) - w0;
                u32 units[kChunk];
#pragma unroll
                for (u32 t = 0; t < kChunk; t++) units[t] = t < nit ? wl[w0 + t] : 0u;
#pragma unroll
                for (u32 t = 0; t < kChunk; t++) {
                    if (t < nit) {
                        if constexpr (MODE == TREW_MODE_LONG) run_long<NW, WT>(sm, P, B, T, units[t]);
                        __syncthreads();
                    }
                }
            }
        }
    }
    {
        PH_T0(t_flush);
        cache_flush(sm, T);
        PH_ADD(PH_FLUSH, t_flush);
    }
    PH_ADD(PH_TOTAL, t_total);
#ifdef TREW_PHASE_PROFILE
    __syncthreads();
    if (lane_id() < 32) atomicAdd(&g_phase[lane_id()], ph_lds()[lane_id()]);
#endif
}

#ifdef TREW_REGION_COUNTS
// trips of every TREW_MARK region since the last reset, in TREW_REGION_LIST order (tools/region_mix.py)
extern "C" int trew_debug_regions(unsigned long long *out, int n, int reset) {
    unsigned long long v[64];
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_region), sizeof(v)) != hipSuccess) return 1;
    for (int i = 0; i < n && i < 64; i++) out[i] = v[i];
    if (reset) {
        unsigned long long z[64] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_region), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
extern "C" const char *trew_debug_region_names() {
#define TREW_REGION_NAME(n) #n " "
    return TREW_REGION_LIST(TREW_REGION_NAME);
}
#endif
#ifdef TREW_PHASE_PROFILE
extern "C" int trew_debug_phases(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 32) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif
