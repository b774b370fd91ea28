// trew_measures_host.hpp -- the per-read measures computed on the CPU, straight from their definitions
// (include/trew_hip.h: trew_hip_annot, trew_hip_tract, trew_hip_interval, trew_hip_variant, trew_hip_period, trew_hip_chain_item, trew_hip_repeat, trew_hip_satellite, trew_hip_alignment, trew_hip_refined, trew_hip_trace_item; trew_hip_decompose uses the last two), and the argument checks the
// device entry points share with them.  Plain C++17: no HIP, no context.  trew_capi.cpp wraps these into the extern "C"
// trew_*_host functions and keeps the error strings; tests/harness/measures_host_harness.cpp runs them under sanitizers.
//
// Every function that can fail returns nullptr, or the text of the error.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/trew_hip.h"

namespace trew {

uint64_t motif_revcomp(uint64_t w, int k);  // T=0 G=1 C=2 A=3: the complement is 3 - code
uint64_t motif_mask(int k);
const char *motif_error(const trew_hip_motif &m);
const char *motifs_error(const trew_hip_motif *motifs, int n_motifs);
const char *rules_error(const trew_hip_interval_rule *rules, int n_motifs);
void sort_intervals(trew_hip_interval *v, uint64_t n);  // by (read, motif, strand, start)

// 'TTAGGG' -> motif; the error text names the motif, so it is built here: "" when the text is a motif
std::string motif_parse(const char *text, trew_hip_motif *out);

const char *annotate_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                          int n_motifs, trew_hip_annot *out);
const char *tracts_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                        int n_motifs, int penalty, trew_hip_tract *out);
const char *intervals_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                           const trew_hip_interval_rule *rules, int n_motifs, trew_hip_interval *out, uint64_t cap, uint64_t *n, uint32_t *counts);
const char *variants_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                          int n_motifs, trew_hip_variant *out, uint64_t *hist, uint64_t *reads_with);
// de novo repeat period and unit per read: no motifs; periods_error is the argument check the device entry point shares
const char *periods_error(int min_period, int max_period, int penalty, uint32_t min_score);
const char *periods_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                         int penalty, uint32_t min_score, trew_hip_period *out);
// de novo repeats, every tract of a read: the recursion of DESIGN 4.7c over pieces, the arguments and checks of periods_host
const char *repeats_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                         int penalty, uint32_t min_score, trew_hip_repeat *out, uint64_t cap, uint64_t *n, uint32_t *counts);
void sort_repeats(trew_hip_repeat *v, uint64_t n);  // by (read, start)
// de novo repeats with periods up to 256: repeats_host with the wider range, check and record
const char *satellites_error(int min_period, int max_period, int penalty, uint32_t min_score);
const char *satellites_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                            int penalty, uint32_t min_score, trew_hip_satellite *out, uint64_t cap, uint64_t *n, uint32_t *counts);
void sort_satellites(trew_hip_satellite *v, uint64_t n);  // by (read, start)
// ordered unit chain per read: items sorted by (read, motif, strand, start), counts [read][motif][strand]{runs, variants}
void sort_chain_items(trew_hip_chain_item *v, uint64_t n);  // by (read, motif, strand, start)
const char *chain_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                       int n_motifs, trew_hip_chain_item *out, uint64_t cap, uint64_t *n_items, uint32_t *counts);
// indel-aware motif tract per read: the wraparound alignment of include/trew_hip.h, cell by cell; the checks of tracts_host
const char *align_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                       int n_motifs, int penalty, trew_hip_alignment *out);
// wraparound alignment for units of up to 256 bases: align_host's definition and record, the maximum over deleted
// bases in the linear-plus-wrap form, O(n k) a strand; the monomers' check, and 'ACGT...' -> monomer as motif_parse
const char *monomers_error(const trew_hip_monomer *monomers, int n_monomers);
std::string monomer_parse(const char *text, trew_hip_monomer *out);
const char *monomers_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_monomer *monomers,
                          int n_monomers, int penalty, trew_hip_alignment *out);
// de novo repeats under indels: seed, wraparound alignment, re-vote (include/trew_hip.h); the checks of periods_host
const char *refine_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                        int penalty, uint32_t min_score, trew_hip_refined *out);
// the same for periods up to 256: satellites_host's depth-0 record, monomers_host's table; the checks of satellites_host
const char *polish_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                        int penalty, uint32_t min_score, trew_hip_polished *out);
// refine's unit with the period chosen by alignment: refine_host's steps 2 to 6 for the best-scoring periods, the best record kept;
// resolve_error is the argument check the device entry point shares (periods_error, then the candidates)
const char *resolve_error(int min_period, int max_period, int penalty, uint32_t min_score, int candidates);
const char *resolve_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                         int penalty, uint32_t min_score, int candidates, trew_hip_resolved *out);
// de novo repeats under indels, every tract of a read: repeats_host's recursion with the refine definition on a piece
const char *tandems_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                         int penalty, uint32_t min_score, trew_hip_tandem *out, uint64_t cap, uint64_t *n, uint32_t *counts);
void sort_tandems(trew_hip_tandem *v, uint64_t n);  // by (read, start)
// units in place under indels: align_host's table with the three tie rules and the walk from its end cell (include/trew_hip.h)
const char *trace_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_motif *motifs,
                       int n_motifs, int penalty, uint32_t min_score, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint32_t *counts,
                       trew_hip_alignment *records);
void sort_trace_items(trew_hip_trace_item *v, uint64_t n);  // by (read, motif, strand, start)
// copies in place for units of up to 256 bases: monomers_host's table with trace_host's tie rules, a direction
// byte a cell of the traced tract only (one bit for the deleted bases), O(n k) a strand; *n_rows (may be NULL): the sum of
// end - start over the keys with items
const char *copies_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, const trew_hip_monomer *monomers,
                        int n_monomers, int penalty, uint32_t min_score, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint64_t *n_rows,
                        uint32_t *counts, trew_hip_alignment *records);
// units in place with no motif given: refine_host's record, its unit's smallest rotation and trace_host's table for one strand
const char *decompose_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                           int penalty, uint32_t min_score, trew_hip_trace_item *items, uint64_t cap, uint64_t *n_items, uint32_t *counts,
                           trew_hip_refined *records);
// units in place for every tract of a read, no motif given: tandems_host's pieces, decompose_host's anchor and items per record
const char *dissect_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                         int penalty, uint32_t min_score, trew_hip_tandem *records, uint64_t rec_cap, trew_hip_trace_item *items, uint64_t item_cap,
                         uint64_t *n_records, uint64_t *n_items, uint64_t *n_rows, uint32_t *counts);
void sort_dissect_items(trew_hip_trace_item *v, uint64_t n);  // by (read, start)
// tandems, decompose and dissect with resolve's period choice per piece: the three walks above with resolve_host's
// winner among the first `candidates` periods of a piece in the place of refine_host's record, and the periods tract of candidate 0
// for a weak piece; resolve_error is their argument check
const char *tandems_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                                  int penalty, uint32_t min_score, int candidates, trew_hip_tandem *out, uint64_t cap, uint64_t *n, uint32_t *counts);
const char *decompose_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period,
                                    int max_period, int penalty, uint32_t min_score, int candidates, trew_hip_trace_item *items, uint64_t cap,
                                    uint64_t *n_items, uint32_t *counts, trew_hip_refined *records);
const char *dissect_resolved_host(const uint32_t *words, const uint32_t *offsets, const uint32_t *lengths, uint64_t n_reads, int min_period, int max_period,
                                  int penalty, uint32_t min_score, int candidates, trew_hip_tandem *records, uint64_t rec_cap, trew_hip_trace_item *items,
                                  uint64_t item_cap, uint64_t *n_records, uint64_t *n_items, uint64_t *n_rows, uint32_t *counts);
// items sorted by (read, start) whose motif word is the start of their tract, records sorted by (read, start): motif becomes the tract's index in its read
void number_dissect_items(const trew_hip_tandem *records, uint64_t n_records, trew_hip_trace_item *items, uint64_t n_items);

}  // namespace trew
