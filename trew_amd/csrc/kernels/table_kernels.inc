// kernels/table_kernels.inc -- part of trew_kernels.hip (included there, inside namespace trew; not a translation unit of its own).
// Table maintenance kernels: add rows, compact occupied slots into rows.

// ------------------------------------------------------------------ table maintenance
// Rows handed in by a caller are validated in a pass of their own BEFORE anything is added, so that an add is all
// or nothing: a bad row (k / table out of range, a high word on a narrow key) raises flags[kRowFlagBad] and the add
// kernel queued behind the check on the same stream returns at once.  flags is a 4-word device scratch of the context (kRowFlag*, trew_common.hpp).
__device__ __forceinline__ bool row_ok(const trew_hip_row &r) {
    return !(r.k < 1 || r.k > 64 || r.table < 0 || r.table >= TREW_NUM_TABLES || (r.k <= 32 && r.word_hi));
}
__global__ void table_check_rows_kernel(const trew_hip_row *rows, u64 n, u32 *flags) {
    const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !row_ok(rows[i])) atomicAdd(&flags[kRowFlagBad], 1u);
}
__global__ void table_add_rows_kernel(DevTable T, const trew_hip_row *rows, u64 n, const u32 *flags) {
    const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flags && flags[kRowFlagBad]) return;  // written by the check kernel that ran before this one
    const trew_hip_row r = rows[i];
    if (r.count) table_add(T, r.table, r.k, ((u128) r.word_hi << 64) | r.word_lo, r.count);
}

// The gather buffer of the cross-GPU table exchange (trew_hip_add_gathered_device): n_slices slices of 1 + slice_rows
// rows, one per rank; row 0 of a slice is its header (count = rows the rank has -- possibly more than fit).  One
// thread per (slice, row); the caller's own slice is skipped by index.
__global__ void table_check_gathered_kernel(const trew_hip_row *buf, u32 n_slices, u32 own, u64 slice_rows, u32 *flags) {
    const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    const u64 per = slice_rows + 1ull;
    if (i >= (u64) n_slices * per) return;
    const u32 s = (u32) (i / per);
    const u64 r = i - (u64) s * per;
    const u64 cnt = buf[(u64) s * per].count;
    if (r == 0) {  // header: every rank sees every count, so every rank takes the same decision to retry
        atomicMax((unsigned long long *) &flags[kRowFlagMaxLo], (unsigned long long) cnt);
        if (cnt > slice_rows) atomicAdd(&flags[kRowFlagOverflow], 1u);
        return;
    }
    if (s == own || r > cnt) return;
    if (!row_ok(buf[i])) atomicAdd(&flags[kRowFlagBad], 1u);
}
__global__ void table_add_gathered_kernel(DevTable T, const trew_hip_row *buf, u32 n_slices, u32 own, u64 slice_rows, const u32 *flags) {
    const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    const u64 per = slice_rows + 1ull;
    if (i >= (u64) n_slices * per) return;
    if (flags[kRowFlagBad] | flags[kRowFlagOverflow]) return;  // all or nothing
    const u32 s = (u32) (i / per);
    const u64 r = i - (u64) s * per;
    if (r == 0 || s == own || r > buf[(u64) s * per].count) return;
    const trew_hip_row row = buf[i];
    if (row.count) table_add(T, row.table, row.k, ((u128) row.word_hi << 64) | row.word_lo, row.count);
}

// compaction of the sparse table into rows (collect): one atomic per occupied slot
__global__ void table_compact_kernel(DevTable T, u64 n_slots, int table, trew_hip_row *rows, u64 cap, unsigned long long *n_rows) {
    const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) {  // wide slots follow the narrow ones
        const u64 j = i - n_slots;
        const DevWide Wd = *T.wide;
        if (j >= (1ull << Wd.wide_log2_slots)) return;
        const u64 tag = Wd.wtag[j];
        if (!(tag >> 63)) return;
        if (Wd.wcount[j] == 0) return;  // counts moved elsewhere (run_long): not a row
        const int t = (int) ((tag >> 59) & 7ull);
        if (table >= 0 && t != table) return;
        const u64 at = atomicAdd(n_rows, 1ull);
        if (at < cap) {
            trew_hip_row r;
            r.k = (int32_t) ((tag >> 52) & 127ull);
            r.table = t;
            r.word_lo = Wd.wlo[j];
            r.word_hi = Wd.whi[j];
            r.count = Wd.wcount[j];
            rows[at] = r;
        }
        return;
    }
    const u64 key = T.keys[i];
    if (!key) return;
    if (T.counts[i] == 0) return;  // a key whose counts were moved elsewhere (run_long: forward -> both): not a row
    const int t = (int) ((key >> 60) & 7ull);
    if (table >= 0 && t != table) return;
    const u64 at = atomicAdd(n_rows, 1ull);
    if (at < cap) {
        trew_hip_row r;
        r.k = (int32_t) ((key >> 55) & 31ull) + 1;
        r.table = t;
        r.word_lo = ((key & ((1ull << 55) - 1ull)) << kTablePartBits) | (i >> T.log2_part_slots);
        r.word_hi = 0;
        r.count = T.counts[i];
        rows[at] = r;
    }
}

// Finishes a rank's slice of the cross-GPU exchange behind table_compact_kernel, on the device: appends the spill log after
// the n compacted rows (rows 1 + n ..) and writes the slice's header (row 0: count = n + spilled rows, everything else 0).
// The host never learns the count before the collective: the header IS the count (trew_hip_collect_slice_device).
__global__ void table_slice_finish_kernel(trew_hip_row *slice, u64 slice_rows, const unsigned long long *n_rows, const trew_hip_row *spill_rows,
                                          const u32 *spill_n, u32 spill_cap) {
    const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    const u64 n = *n_rows;
    const u32 ns = *spill_n < spill_cap ? *spill_n : spill_cap;
    if (i < ns && n + i < slice_rows) slice[1 + n + i] = spill_rows[i];
    if (i == 0) {
        trew_hip_row h;
        h.k = 0;
        h.table = 0;
        h.word_lo = 0;
        h.word_hi = 0;
        h.count = n + ns;
        slice[0] = h;
    }
}

// ------------------------------------------------------------------ text -> bit planes
// codes[] of kmer.cpp:14-31 on the device: T=0 G=1 C=2 A=3 in either case, every other byte is "N".  One thread per
// packed triple (32 bases): eight aligned dwords of text (+ one when the read does not start on a dword), byte-wise
// equality by SWAR (exact per byte: no borrow crosses a byte), the four flag bits of a dword gathered with one multiply.
// Output identical to trew_pack_reads (trew_capi.cpp): bits past the end of the read are 0 in all three planes.
__device__ __forceinline__ u32 zero_bytes(u32 v) {  // 0x80 in every byte of v that is 0, exact
    return ~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v | 0x7f7f7f7fu);
}
__device__ __forceinline__ u32 gather4(u32 flags80) {  // bits 7, 15, 23, 31 -> bits 0..3
    return (((flags80 >> 7) * 0x01020408u) >> 24) & 0xfu;
}
__global__ void pack_ascii_kernel(const unsigned char *__restrict__ bases, const u32 *__restrict__ byte_offsets, const u32 *__restrict__ lengths,
                                  const u32 *__restrict__ word_offsets, u32 uniform_length, u64 n_reads, u64 n_triples, u32 *__restrict__ words) {
    const u64 t = (u64) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_triples) return;
    u64 r, j, src;
    u32 len;
    if (!word_offsets) {
        const u32 tpr = (uniform_length + 31u) >> 5;
        r = t / tpr;
        j = t - r * tpr;
        len = uniform_length;
        src = r * (u64) uniform_length;
    } else {  // the read whose triples hold triple t: last r with word_offsets[r] <= 3 t
        u64 lo = 0, hi = n_reads - 1;
        const u64 want = 3ull * t;
        while (lo < hi) {
            const u64 mid = (lo + hi + 1) >> 1;
            if ((u64) word_offsets[mid] <= want)
                lo = mid;
            else
                hi = mid - 1;
        }
        r = lo;
        j = t - (u64) word_offsets[r] / 3ull;
        len = lengths[r];
        src = byte_offsets[r];
    }
    const u64 first = src + 32ull * j;
    const u32 m = len - (u32) (32ull * j) < 32u ? len - (u32) (32ull * j) : 32u;  // bases in this triple (>= 1: empty reads have no triple)
    const u32 *aligned = (const u32 *) (bases + (first & ~3ull));
    const u32 sh = (u32) (first & 3ull);
    u32 lo = 0, hi = 0, nm = 0;
    u32 prev = aligned[0];
#pragma unroll
    for (int d = 0; d < 8; d++) {
        // the triple occupies bytes [sh, sh + m) of the aligned dwords; dword d + 1 is fetched only if it holds one of them
        // (nothing is read past the dword of the read's last base)
        const u32 next = (4u * (u32) (d + 1) < sh + m) ? aligned[d + 1] : 0u;
        const u32 x = sh ? __builtin_amdgcn_alignbyte(next, prev, sh) : prev;
        prev = next;
        const u32 y = x & 0xdfdfdfdfu;  // upper case; non-letters cannot become A/C/G/T this way (their twins 0x61.. are the lower-case letters)
        const u32 a = zero_bytes(y ^ 0x41414141u), c = zero_bytes(y ^ 0x43434343u), g = zero_bytes(y ^ 0x47474747u), tt = zero_bytes(y ^ 0x54545454u);
        lo |= gather4(g | a) << (4 * d);
        hi |= gather4(c | a) << (4 * d);
        nm |= gather4(~(a | c | g | tt) & 0x80808080u) << (4 * d);
    }
    const u32 keep = low_mask<true>((int) m);
    const u64 w = word_offsets ? (u64) word_offsets[r] + 3ull * j : 3ull * t;
    words[w + 0] = lo & keep;
    words[w + 1] = hi & keep;
    words[w + 2] = nm & keep;
}
