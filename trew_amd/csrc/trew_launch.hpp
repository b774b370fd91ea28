// trew_launch.hpp -- host-callable launchers implemented in trew_kernels.hip
#pragma once
#include <hip/hip_runtime.h>

#include "trew_common.hpp"

namespace trew {

int pick_nw(u32 max_seg_len);

hipError_t launch_filter(hipStream_t st, u32 n_cu, u32 max_seg_len, const DevParams &P, const DevBatch &B, u32 *wl, u32 *wl_count,
                         u32 wl_cap, u64 *dbg_masks, int dbg_slots, u32 *diag, const int2 *d_thr);
void fill_thresholds(const DevParams &P, u32 uniform_length, int2 *table);  // kThrTableBytes: the thresholds and, at kThrGeomOffset, the batch geometry (build_filter_geom)
hipError_t launch_exact(hipStream_t st, u32 n_cu, u64 n_units, const DevParams &P, const DevBatch &B, const DevTableG1 &T,
                        const u32 *wl, u32 *wl_count, u32 *wl_count_next, u32 wl_cap, const SegResults &R, u32 cap, u32 rawwords,
                        u32 max_seg_len, bool share, const u32 *bnd, u32 bnd_cap, const u32 *live);  // share: leave half of the wave slots to a prefilter on another stream
// the bounds pass (kernels/bounds_pass.inc): bnd = what launch_bounds left for the first bnd_cap worklist entries, or nullptr;
// live = the live worklist it wrote (the exact kernel reads it in front of the worklist entries from bnd_cap on), or nullptr
bool bounds_pass_applies(const DevParams &P, u32 max_seg_len);  // this batch's exact kernel reads stored bounds
size_t bounds_entry_bytes();                                    // of one worklist entry in bnd
hipError_t launch_bounds(hipStream_t st, u32 n_cu, u64 n_units, const DevParams &P, const DevBatch &B, const u32 *wl, u32 *wl_count, u32 wl_cap,
                         u32 *bnd, u32 bnd_cap, u32 *live, const u32 *need);
// need: the device copy of what fill_bound_needs wrote (kBoundNeedWords words), or nullptr where it returned false
bool fill_bound_needs(const DevParams &P, u32 *table);
u32 exact_lds_bytes_host(u32 cap, u32 rawwords, u32 wordbytes);
hipError_t launch_g1_apply(hipStream_t st, const DevTable &T, const DevG1 &G, const DevBatch &B, int min_mer, const trew_hip_row *carry_in,
                           trew_hip_row *carry_out, u32 carry_cap);
hipError_t fallback_counters_read(u32 *out);  // kFallbackWords words of the current device
hipError_t fallback_counters_clear(hipStream_t st);  // queued on st
hipError_t launch_add_rows(hipStream_t st, const DevTable &T, const trew_hip_row *d_rows, u64 n, u32 *d_flags);
hipError_t launch_add_gathered(hipStream_t st, const DevTable &T, const trew_hip_row *d_buf, u32 n_slices, u32 own, u64 slice_rows, u32 *d_flags);
hipError_t launch_pack_ascii(hipStream_t st, const unsigned char *d_bases, const u32 *d_byte_offsets, const u32 *d_lengths, const u32 *d_word_offsets,
                             u32 uniform_length, u64 n_reads, u64 n_triples, u32 *d_words);
hipError_t launch_compact(hipStream_t st, const DevTable &T, u64 n_slots, u32 wide_log2_slots, int table, trew_hip_row *d_rows, u64 cap,
                          unsigned long long *d_n);
hipError_t launch_slice_finish(hipStream_t st, trew_hip_row *d_slice, u64 slice_rows, const unsigned long long *d_n, const trew_hip_row *d_spill_rows,
                               const u32 *d_spill_n, u32 spill_cap);
// the blocks of every wave-per-read launch below for a batch of n_reads (trew_hip_debug_measure_grid reports them)
u32 wave_per_read_blocks(u32 n_cu, u64 n_reads);
// trew_hip_annotate: general = the wave-per-read kernel, else the lane-per-read one (max_len <= 256)
hipError_t launch_annotate(hipStream_t st, u32 n_cu, const DevBatch &B, const AnnotMotifDev *d_motifs, int n_motifs, u32 max_len, bool general,
                           trew_hip_annot *d_out);
// trew_hip_tracts: the wave-per-read kernel of kernels/tracts.inc, whatever the read lengths
hipError_t launch_tracts(hipStream_t st, u32 n_cu, const DevBatch &B, const AnnotMotifDev *d_motifs, int n_motifs, int penalty, trew_hip_tract *d_out);
// trew_hip_intervals: the wave-per-read kernel of kernels/intervals.inc on the grid of launch_tracts; the counter of `lg` is zero
// when the kernel starts (the caller's memset on the same stream)
hipError_t launch_intervals(hipStream_t st, u32 n_cu, const DevBatch &B, const AnnotMotifDev *d_motifs, int n_motifs, const IntervalRulesDev &rules,
                            const IntervalLog &lg, u32 *d_counts);
// trew_hip_variants: the wave-per-read kernel of kernels/variants.inc on the grid of launch_tracts; hist and reads_with are zero
// when the kernel starts (the caller's memsets on the same stream)
hipError_t launch_variants(hipStream_t st, u32 n_cu, const DevBatch &B, const AnnotMotifDev *d_motifs, int n_motifs, trew_hip_variant *d_out,
                           unsigned long long *d_hist, unsigned long long *d_reads_with);
// trew_hip_periods: the wave-per-read kernel of kernels/periods.inc on the grid of launch_tracts; no motifs
hipError_t launch_periods(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, trew_hip_period *d_out);
// trew_hip_chain: the wave-per-read kernel of kernels/chain.inc on the grid of launch_tracts; the counter of `lg` is zero when
// the kernel starts (the caller's memset on the same stream)
hipError_t launch_chain(hipStream_t st, u32 n_cu, const DevBatch &B, const AnnotMotifDev *d_motifs, int n_motifs, const ChainLog &lg, u32 *d_counts);
// trew_hip_repeats: the wave-per-read kernel of kernels/repeats.inc on the grid of launch_tracts; no motifs; the counter of `lg`
// is zero when the kernel starts (the caller's memset on the same stream)
hipError_t launch_repeats(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, const RepeatLog &lg,
                          u32 *d_counts);
// trew_hip_satellites: the wave-per-read kernel of kernels/satellites.inc on the grid of launch_tracts; no motifs; `lg` holds
// records of 26 u32, its counter is zero when the kernel starts (the caller's memset on the same stream)
hipError_t launch_satellites(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score,
                             const RepeatLog &lg, u32 *d_counts);
// trew_hip_align: the wave-per-read kernel of kernels/align.inc on the grid of launch_tracts
hipError_t launch_align(hipStream_t st, u32 n_cu, const DevBatch &B, const AnnotMotifDev *d_motifs, int n_motifs, int penalty, trew_hip_alignment *d_out);
// trew_hip_monomers: the wave-per-read kernel of kernels/monomers.inc on the grid of launch_tracts; max_k (3 .. 256): the
// largest k of d_monomers, which picks the phases a lane holds (1, 2 or 4)
hipError_t launch_monomers(hipStream_t st, u32 n_cu, const DevBatch &B, const trew_hip_monomer *d_monomers, int n_monomers, u32 max_k, int penalty,
                           trew_hip_alignment *d_out);
// trew_hip_copies: the wave-per-read kernel of kernels/copies.inc on the grid of launch_tracts; max_k picks Q as in
// launch_monomers, and with it the row of the workspace (64 Q bytes); both counters of `lg` are zero when the kernel starts;
// d_out: the alignment records, d_counts: the items of every (read, monomer, strand)
hipError_t launch_copies(hipStream_t st, u32 n_cu, const DevBatch &B, const trew_hip_monomer *d_monomers, int n_monomers, u32 max_k, int penalty,
                         u32 min_score, const TraceLog &lg, trew_hip_alignment *d_out, u32 *d_counts);
// trew_hip_polish: the wave-per-read kernel of kernels/polish.inc on the grid of launch_tracts; no motifs; max_period picks Q as
// launch_monomers' max_k does
hipError_t launch_polish(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, trew_hip_polished *d_out);
// trew_hip_trace: the wave-per-read kernel of kernels/trace.inc on the grid of launch_tracts; both counters of `lg` are zero
// when the kernel starts; d_out: the alignment records, d_counts: the items of every (read, motif, strand)
hipError_t launch_trace(hipStream_t st, u32 n_cu, const DevBatch &B, const AnnotMotifDev *d_motifs, int n_motifs, int penalty, u32 min_score,
                        const TraceLog &lg, trew_hip_alignment *d_out, u32 *d_counts);
// trew_hip_decompose: the wave-per-read kernel of kernels/decompose.inc on the grid of launch_tracts; no motifs; both counters
// of `lg` are zero when it starts, its rows have 32 bytes
hipError_t launch_decompose(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, const TraceLog &lg,
                            trew_hip_refined *d_out, u32 *d_counts);
// trew_hip_refine: the wave-per-read kernel of kernels/refine.inc on the grid of launch_tracts; no motifs
hipError_t launch_refine(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, trew_hip_refined *d_out);
// trew_hip_tandems: the wave-per-read kernel of kernels/tandems.inc on the grid of launch_tracts; no motifs; `lg` holds records
// of 18 u32, its counter is zero when the kernel starts (the caller's memset on the same stream)
hipError_t launch_tandems(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, const RepeatLog &lg,
                          u32 *d_counts);
// trew_hip_dissect: the wave-per-read kernel of kernels/dissect.inc on the grid of launch_tracts; no motifs; `rl` holds records
// of 18 u32, `lg` items and rows of 32 bytes; all three counters are zero when it starts; d_counts: (tracts, items) per read
hipError_t launch_dissect(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, const RepeatLog &rl,
                          const TraceLog &lg, u32 *d_counts);
// trew_hip_tandems_resolved, _decompose_resolved, _dissect_resolved: the <true> instantiations of the three kernels above, with
// resolve's period choice per piece (kernels/resolve_piece.inc); 1 <= candidates <= 4; logs, counters and counts as their siblings'
hipError_t launch_tandems_resolved(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, int candidates,
                                   const RepeatLog &lg, u32 *d_counts);
hipError_t launch_decompose_resolved(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, int candidates,
                                     const TraceLog &lg, trew_hip_refined *d_out, u32 *d_counts);
hipError_t launch_dissect_resolved(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, int candidates,
                                   const RepeatLog &rl, const TraceLog &lg, u32 *d_counts);
// trew_hip_resolve: the wave-per-read kernel of kernels/resolve.inc on the grid of launch_tracts; no motifs; 1 <= candidates <= 4
hipError_t launch_resolve(hipStream_t st, u32 n_cu, const DevBatch &B, int min_period, int max_period, int penalty, u32 min_score, int candidates,
                          trew_hip_resolved *d_out);
hipError_t launch_synth_short(hipStream_t st, u64 seed, u64 first, u64 n, u32 len, u32 *d_words);
hipError_t launch_synth_long(hipStream_t st, u64 seed, u64 first, u64 n, const u32 *d_qtable, const u32 *d_offsets, u32 *d_words);
hipError_t launch_synth_pair(hipStream_t st, u64 seed, u64 first, u64 n, u32 len, u32 *d_words);

}  // namespace trew
