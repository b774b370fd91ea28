// kernels/helpers.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Small device helpers shared by both kernels: funnel shifts, wave reductions (DPP), read descriptors, plane loads, LDS list append.

// ------------------------------------------------------------------ helpers
__device__ u32 g_fallback[kFallbackWords];  // see kFallback* (trew_common.hpp); read by fallback_counters_read()
__device__ __forceinline__ void count_fallback(int which) {  // wave-uniform call sites: one add per wave
    if ((threadIdx.x & 63u) == 0) atomicAdd(&g_fallback[which], 1u);
}
__device__ __forceinline__ u32 alignbit(u32 hi, u32 lo, u32 sh) {
    return __builtin_amdgcn_alignbit(hi, lo, sh);  // ((hi:lo) >> (sh & 31)) & 0xffffffff
}
__device__ __forceinline__ u32 lane_id() { return threadIdx.x & 63u; }
// popc(x) + acc in one instruction
__device__ __forceinline__ u32 bcnt_acc(u32 x, u32 acc) {
    u32 d;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(acc));
    return d;
}
// kMultiples[k] = bits j-1 of every multiple j <= 64 of k (k = 1..64; entry 0 unused): the k values an accepted k closes in a
// selection loop of k_mer_check (kmer.cpp:2225-2236)
struct MultiplesTable {
    u64 v[65];
    constexpr MultiplesTable() : v() {
        for (int k = 1; k <= 64; k++) {
            u64 m = 0;
            for (int j = k; j <= 64; j += k) m |= 1ull << (j - 1);
            v[k] = m;
        }
    }
};
__constant__ MultiplesTable kMultiples = MultiplesTable();
__device__ __forceinline__ u64 load_multiples(int k) { return kMultiples.v[k & 127 ? (k <= 64 ? k : 0) : 0]; }
__device__ __forceinline__ u32 rfl(u32 v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u64 rfl64(u64 v) {
    u32 lo = __builtin_amdgcn_readfirstlane((u32) v);
    u32 hi = __builtin_amdgcn_readfirstlane((u32) (v >> 32));
    return ((u64) hi << 32) | lo;
}

// Arguments of a noinline device function arrive in VGPRs, so the compiler has to treat them as
// divergent: loops run on exec masks and address arithmetic on the VALU.  The values below are
// wave-uniform by construction; re-reading them through readfirstlane moves them (and everything
// derived from them) to the scalar unit.
__device__ __forceinline__ int rfl_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename Tp>
__device__ __forceinline__ Tp *rfl_ptr(Tp *p) {
    return (Tp *) rfl64((u64) p);
}
__device__ __forceinline__ double rfl_f64(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// wave max of a u32 (0 for idle lanes), every lane gets the result.  DPP row shifts and row
// broadcasts: 6 VALU instructions instead of 6 LDS-crossbar round trips (ds_bpermute).
__device__ __forceinline__ u32 wave_max_u32(u32 v) {
    // max is idempotent, so overlapping shifts are fine: after row_shr 1,2,4,8 lane 15 of each row holds the row's max
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, true));  // row_shr:1
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, true));  // row_shr:2
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, true));  // row_shr:4
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, true));  // row_shr:8
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false)); // row_bcast:15 into rows 1 and 3
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false)); // row_bcast:31 into rows 2 and 3
    return (u32) __builtin_amdgcn_readlane((int) v, 63);
}

// wave sum of a u32, every lane gets the result: Hillis-Steele inside each row of 16 lanes (row_shr
// 1, 2, 4, 8), then the row totals are passed on with the two row broadcasts; lane 63 holds the sum
__device__ __forceinline__ u32 wave_sum_u32(u32 v) {
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, true);
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, true);
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, true);
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, true);
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    return (u32) __builtin_amdgcn_readlane((int) v, 63);
}

// inclusive prefix sum of a u32 across the wave (the same steps as wave_sum_u32, whose lane 63 is the last prefix): lane l
// gets v[0] + ... + v[l]; two's complement, so signed values sum as well
__device__ __forceinline__ u32 wave_scan_u32(u32 v) {
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, true);
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, true);
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, true);
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, true);
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    v += (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    return v;
}

// inclusive prefix maximum of a u32 across the wave (0 for idle lanes), the steps of wave_scan_u32: lane l gets
// max(v[0], ..., v[l])
__device__ __forceinline__ u32 wave_scan_max_u32(u32 v) {
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, true));
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, true));
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, true));
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, true));
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1 and 3
    v = max(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2 and 3
    return v;
}
// the value of the lane below (wave_shr:1); lane 0 gets 0: turns an inclusive scan into an exclusive one
__device__ __forceinline__ u32 wave_prev_lane_u32(u32 v) {
    return (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x138, 0xf, 0xf, false);
}

struct ReadRef {
    const u32 *w;  // first triple
    u32 len;       // bases
    u32 nw;        // triples
};
// one wave works on one read: its descriptor is wave-uniform
__device__ __forceinline__ ReadRef uni(ReadRef r) {
    r.w = rfl_ptr(r.w);
    r.len = rfl(r.len);
    r.nw = rfl(r.nw);
    return r;
}

__device__ __forceinline__ ReadRef get_read(const DevBatch &b, u64 r) {
    ReadRef x;
    u64 off = b.offsets ? (u64) b.offsets[r] : r * (u64) b.uniform_stride;
    x.len = b.lengths ? b.lengths[r] : b.uniform_length;
    x.w = b.words + off;
    x.nw = (x.len + 31u) >> 5;
    return x;
}

// the one or two reads of a unit (pair mode: the two mates); an inactive lane gets empty descriptors
__device__ __forceinline__ void unit_reads(const DevParams &P, const DevBatch &B, u64 unit, bool active, ReadRef (&rd)[2]) {
    rd[0].w = B.words;
    rd[0].len = 0;
    rd[0].nw = 0;
    rd[1] = rd[0];
    if (active) {
        if (P.mode == TREW_MODE_PAIR) {
            rd[0] = get_read(B, 2 * unit);
            rd[1] = get_read(B, 2 * unit + 1);
        } else {
            rd[0] = get_read(B, unit);
        }
    }
}

// 32*NW plane bits starting at base s of a read of nw triples at w: lo/hi/nmask, bit i = base s+i.  Ptr: the pointer's address
// space decides the load instruction (load_planes / load_planes_lds below).
template <int NW, typename Ptr>
__device__ __forceinline__ void load_planes_from(const Ptr w, u32 nw, u32 s, u32 (&lo)[NW], u32 (&hi)[NW], u32 (&nm)[NW]) {
    const u32 ws = s >> 5, bs = s & 31u;
    u32 c0 = 0, c1 = 0, c2 = 0;
    if (ws < nw) {
        c0 = w[3 * ws + 0];
        c1 = w[3 * ws + 1];
        c2 = w[3 * ws + 2];
    }
#pragma unroll
    for (int j = 0; j < NW; j++) {
        u32 n0 = 0, n1 = 0, n2 = 0;
        const u32 idx = ws + (u32) j + 1u;
        if (idx < nw) {
            n0 = w[3 * idx + 0];
            n1 = w[3 * idx + 1];
            n2 = w[3 * idx + 2];
        }
        lo[j] = alignbit(n0, c0, bs);
        hi[j] = alignbit(n1, c1, bs);
        nm[j] = alignbit(n2, c2, bs);
        c0 = n0;
        c1 = n1;
        c2 = n2;
    }
}
template <int NW>
__device__ __forceinline__ void load_planes(const ReadRef &rd, u32 s, u32 (&lo)[NW], u32 (&hi)[NW], u32 (&nm)[NW]) {
    load_planes_from<NW>(rd.w, rd.nw, s, lo, hi, nm);
}

// the same for a read whose triples are staged in LDS: ds_read instead of flat loads (a flat load counts as a vector-memory
// operation, and waiting for one waits for everything the load unit was given before it -- the exact kernel's chunk prefetch)
typedef const __attribute__((address_space(3))) u32 *lds_u32;
template <int NW>
__device__ __forceinline__ void load_planes_lds(const ReadRef &rd, u32 s, u32 (&lo)[NW], u32 (&hi)[NW], u32 (&nm)[NW]) {
    load_planes_from<NW>((lds_u32) rd.w, rd.nw, s, lo, hi, nm);
}

// A whole read of at most five triples (160 bases; the prefilter's caller stops at 159, see halves_prefix_read5), loaded once: word j of a plane holds bases 32 j .. 32 j + 31 as they lie in
// memory, no funnel shift.  For callers that cut several segments out of the same read (the prefilter's joint loop: both halves).
// The caller knows the read has four or five triples; a lane with fewer (an inactive one: nw = 0) loads nothing and gets zeros,
// so no address past the read's own triples is ever formed.  The loads of a branch are adjacent: the compiler may merge them.
struct ReadPlanes5 {
    u32 lo[5], hi[5], nm[5];
};
__device__ __forceinline__ void load_read5(const ReadRef &rd, ReadPlanes5 &r) {
#pragma unroll
    for (int j = 0; j < 5; j++) r.lo[j] = r.hi[j] = r.nm[j] = 0u;
    if (rd.nw >= 4u) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            r.lo[j] = rd.w[3 * j + 0];
            r.hi[j] = rd.w[3 * j + 1];
            r.nm[j] = rd.w[3 * j + 2];
        }
    }
    if (rd.nw >= 5u) {
        r.lo[4] = rd.w[12];
        r.hi[4] = rd.w[13];
        r.nm[4] = rd.w[14];
    }
}

// Wave-aggregated append to a list in LDS: one atomic on its counter per wave (the first flagged lane's); every flagged lane then
// calls put(index of its entry).  (A callback, not a return value: the store stays inside the two conditions, as the generated
// code has it; a capture by value where the callback reads variables the caller goes on using.)
template <typename Put>
__device__ __forceinline__ void wave_append(u32 *counter, bool flag, Put put) {
    const u64 bal = __ballot(flag);
    if (bal) {
        const u32 lane = lane_id();
        const int leader = __ffsll((long long) bal) - 1;
        u32 sb = 0;
        if ((int) lane == leader) sb = atomicAdd(counter, (u32) __popcll(bal));
        sb = __shfl(sb, leader);
        if (flag) put(sb + (u32) __popcll(bal & ((1ull << lane) - 1ull)));
    }
}
