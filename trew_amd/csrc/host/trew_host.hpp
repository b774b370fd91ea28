// trew_host.hpp -- C++ host side of the MI355X-native `trew` binary.
//
// Mirrors the interface of the reference's kmer.h (Chemical118/TREW) for the parts that stay
// on the CPU -- FASTQ/.gz chunk reading, per-file aggregation, CSV output, Putative_TRM ranking --
// and drives the device hot path through the C ABI of include/trew_hip.h.  Same function names
// and argument meaning as the reference where a counterpart exists:
//   process_kmer / process_kmer_pair / process_kmer_long   kmer.h:218-228, kmer.cpp:1266-1476
//   process_output                                          kmer.cpp:1478-1634
//   check_ans_seq                                           kmer.cpp:2549-2569
//   final_process_output / get_score_map                    kmer.cpp:2571-2761
// Errors follow the reference's convention: message on stderr, exit(EXIT_FAILURE).
#pragma once
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/trew_hip.h"

namespace trew_host {

typedef unsigned __int128 uint128_t;

// the configuration globals of kmer.h:55-63
struct Config {
    int MIN_MER = 5;
    int MAX_MER = 32;
    int NUM_THREAD = 2;
    int SLICE_LENGTH = 150;
    int QUEUE_SIZE = -1;
    double LOW_BASELINE = 0.5;
    double HIGH_BASELINE = 0.8;
    int TABLE_MAX_MER = 12;  // accepted for CLI compatibility; the device path has no tables
    std::vector<int> devices = {0};
    bool stats = false;
    int table_log2_slots = 24;   // device count table: 2^24 slots (256 MiB); emptied into host memory whenever half full
    bool serial_reader = false;  // --serial_reader: plain FASTQ through the reference-shaped single reader as well
    int batch_mib = 32;          // --batch_mib: text per device batch of the block-parallel reader (1..32 MiB)
    bool compat_g1 = false;      // --compat_g1 (short --paired_end): the reference's un-cleared temp_result_left, one consumer, file order
    bool host_pack = false;      // --host_pack: the block-parallel reader packs bases on the CPU (trew_pack_reads) instead of shipping text to the pack kernel
};

// KmerSeq (kmer.h:77) with a total order so that output is deterministic
struct KmerSeq {
    int k;
    uint128_t seq;
    bool operator<(const KmerSeq &o) const { return k != o.k ? k < o.k : seq < o.seq; }
    bool operator==(const KmerSeq &o) const { return k == o.k && seq == o.seq; }
};

// FinalData<int64_t> (kmer.h:65-70)
struct FinalData {
    int64_t forward = 0, backward = 0, both = 0;
};

typedef std::map<KmerSeq, FinalData> FinalFastqData;                  // kmer.h:89 (ordered => deterministic)
typedef std::vector<std::pair<KmerSeq, FinalData>> FinalFastqVector;  // kmer.h:90
struct FinalFastqOutput {                                             // kmer.h:106-109
    FinalFastqVector high, low;
};

typedef std::map<KmerSeq, uint64_t> ResultMap;  // kmer.h:79
struct ResultMapData {                          // kmer.h:81: {forward, backward, both} x {high(first), low(second)}
    ResultMap table[TREW_NUM_TABLES];
};

// ---- primitives (kmer.cpp:39-70, 1815-1892) ----
uint128_t get_rot_seq_128(uint128_t seq, int k);
uint128_t reverse_complement_k(uint128_t seq, int k);  // reverse_complement_128(x) >> 2*(64-k)
int get_dna_count(uint128_t seq, int k);
void int_to_four(char *buffer, uint128_t seq, int n);
bool check_ans_seq(const KmerSeq &seq, int min_mer);

// ---- per-file pipelines: reader on the caller's thread, NUM_THREAD-1 packer threads each
// owning one device slot, then process_output.  file names are printed as given (the CLI passes
// canonical absolute paths, trew.cpp:439-451). ----
struct Scanner;  // device contexts, one per GPU
Scanner *scanner_create(const Config &cfg, int mode);
void scanner_destroy(Scanner *s);

FinalFastqOutput process_kmer(Scanner *s, const Config &cfg, const char *file_name, bool is_gz);
FinalFastqOutput process_kmer_pair(Scanner *s, const Config &cfg, const char *file_name1, const char *file_name2,
                                   bool is_gz1, bool is_gz2);
FinalFastqOutput process_kmer_long(Scanner *s, const Config &cfg, const char *file_name, bool is_gz);

// prints the >H: / >L: sections and returns the folded rows (kmer.cpp:1478-1634)
FinalFastqOutput process_output(const char *file_name, const ResultMapData &result, int min_mer, FILE *out);
// prints >Putative_TRM (kmer.cpp:2571-2691)
void final_process_output(FinalFastqData &total_result_high, FinalFastqData &total_result_low, FILE *out);
std::map<KmerSeq, uint32_t> get_score_map(const FinalFastqData &total_result);

// ---- argument helpers of every subcommand (host/motif_cli.cpp) ----
bool parse_int(const char *s, int *out);
bool parse_devices(const std::string &list, std::vector<int> *devices);  // "0,2": false unless every entry is an ordinal and there is one
bool is_regular_file(const std::string &p);
bool has_gz_ext(const std::string &p);
std::string canonical(const std::string &p);

// ---- trew annotate|tracts|intervals|variants|chain|align|trace MOTIF[,MOTIF...] FASTQ..., trew monomers|copies [--fasta FILE] [MONOMER[,MONOMER...]] FASTQ... and trew periods|repeats|satellites|refine|tandems|decompose|dissect|resolve|polish FASTQ...: the per-read measures.
// One file path for all eighteen (process.cpp), one command-line front end (host/motif_cli.cpp); host/annotate.cpp, tracts.cpp,
// intervals.cpp, variants.cpp, periods.cpp, chain.cpp, repeats.cpp, satellites.cpp, align.cpp, refine.cpp, tandems.cpp, trace.cpp, decompose.cpp, dissect.cpp, resolve.cpp, monomers.cpp, copies.cpp and polish.cpp hold what is a measure's own. ----
enum class Measure { Annotate, Tracts, Intervals, Variants, Periods, Chain, Repeats, Satellites, Align, Refine, Tandems, Trace, Decompose, Dissect, Resolve, Monomers, Copies, Polish };
struct AnnotRequest {
    Measure kind = Measure::Annotate;  // picks the device call and the record type
    trew_hip_motif motifs[TREW_ANNOT_MAX_MOTIFS];
    // a (read, motif) is reported when its longer tract has at least this many bases (variants, chain: MIN_UNITS; intervals: not read)
    uint32_t min_tract[TREW_ANNOT_MAX_MOTIFS];
    trew_hip_monomer monomers[TREW_MONOMERS_MAX];  // monomers, copies: n_motifs of them, in the place of motifs
    int n_motifs = 0;
    int penalty = 0;                                      // tracts, periods, repeats, satellites, align, refine, tandems, trace, monomers
    int min_period = 1, max_period = 32;                  // periods, repeats, satellites, refine, tandems (which take no motifs: n_motifs = 0)
    uint32_t min_score = 24;                              // periods, repeats, satellites, align, refine, tandems, trace, monomers
    trew_hip_interval_rule rules[TREW_ANNOT_MAX_MOTIFS];  // intervals
    int candidates = 3;                                   // resolve; tandems, decompose, dissect: their commands fill in 1 (the plain entry point)
};
struct AnnotRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    int motif;        // index in command-line order
    union {           // the record of the request's kind
        trew_hip_annot a;
        trew_hip_tract t;
        trew_hip_variant v;
        trew_hip_period p;
    };
};
struct IntervalRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_interval iv;  // iv.read is the index inside its batch; iv.motif the index in command-line order
};
struct ChainRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_chain_item it;  // it.read is the index inside its batch; it.motif the index in command-line order
};
struct RepeatRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_repeat rp;  // rp.read is the index inside its batch
};
struct SatelliteRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_satellite st;  // st.read is the index inside its batch
};
struct AlignRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    int motif;        // index in command-line order
    int strand;       // 0 = the motif, 1 = its reverse complement
    uint32_t rec[5];  // score, start, end, consumed, matches: one strand's half of a trew_hip_alignment
};
struct AlignColumns {
    uint32_t copies, mismatches, insertions, deletions;
};
// what follows exactly from one strand's five fields, the motif's length and the penalty (include/trew_hip.h)
AlignColumns align_columns(const uint32_t rec[5], uint32_t k, int penalty);
// the sums of `trew align`'s summary: rows, end - start, score, copies, consumed, matches, mismatches, insertions, deletions
constexpr int kAlignSums = 9;
struct TraceRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_trace_item it;  // it.read is the index inside its batch; it.motif the index in command-line order
    std::string text;        // the item's read bases as the file has them; empty for a run of complete exact copies
};
// the further sums of `trew trace`'s summary, behind align's: units, edited, items
constexpr int kTraceSums = 3;
struct RefineRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_refined rf;
};
struct RefineUnit {
    uint64_t reads = 0, bases = 0, copies = 0;  // rows with such a unit, the sums of their end - start and of their copies
};
struct PolishRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_polished pl;
};
struct ResolveRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_resolved rv;
};
struct ResolveUnit {
    uint64_t reads = 0, bases = 0, copies = 0;  // as RefineUnit
    uint64_t repaired = 0;                      // the rows with rank > 0
};
struct TandemRow {
    uint64_t read;    // ordinal of the read in its file, 0-based
    uint32_t length;  // bases
    trew_hip_tandem td;  // td.read is the index inside its batch
};
struct TandemUnit {
    uint64_t reads = 0, tracts = 0, bases = 0, copies = 0;  // reads with such a tract, the tracts, the sums of their end - start and of their copies
};
struct DecomposeUnit {
    uint64_t reads = 0, bases = 0, copies = 0;  // as RefineUnit
    uint64_t units = 0, edited = 0, items = 0;  // over the rows' items: the copies of the items with consumed = period count, the items with an error, the items
};
struct DissectUnit {
    uint64_t reads = 0, tracts = 0, bases = 0, copies = 0;  // as TandemUnit
    uint64_t units = 0, edited = 0, items = 0;              // over the tracts' items, as DecomposeUnit
};
struct RepeatUnit {
    uint64_t reads = 0, tracts = 0, bases = 0;  // reads with such a tract, the tracts, the sum of their end - start
};
// What one file (or, summed, all files) came to.  What the per-motif counters count depends on the kind: see the function
// of process.cpp that folds the kind's records into them (fold_<kind>).  What the folds share is there once: the six with a log
// size and fetch it through fetch_with_retry, repeats, satellites and tandems tally their units through tally_units, align and
// trace make their rows through align_rows; process_annotate merges and sorts every row vector through merge_rows.
struct AnnotFileResult {
    std::vector<AnnotRow> rows;      // annotate, tracts, variants: sorted by read, then motif
    std::vector<IntervalRow> irows;  // intervals: sorted by read, motif, strand, start
    std::vector<ChainRow> crows;     // chain: the items of the reported (read, motif, strand), sorted by read, motif, strand, start
    std::vector<RepeatRow> rrows;    // repeats: sorted by read, start
    std::vector<SatelliteRow> srows; // satellites: sorted by read, start
    std::vector<AlignRow> arows;     // align, monomers: sorted by read, motif, strand
    uint64_t align_sums[TREW_ANNOT_MAX_MOTIFS][2][kAlignSums] = {};  // align: [motif][strand], over the rows
    std::vector<TraceRow> xrows;     // trace: the items of its arows' keys, sorted by read, motif, strand, start; decompose: the items of its frows (motif = strand = 0); dissect: the items of its trows (motif: the tract's index in its read)
    uint64_t trace_sums[TREW_ANNOT_MAX_MOTIFS][2][kTraceSums] = {};  // trace: [motif][strand], over the rows
    std::vector<RefineRow> frows;    // refine, decompose (rf.reserved: the anchor): sorted by read
    std::vector<ResolveRow> vrows;   // resolve: sorted by read
    std::vector<PolishRow> prows;    // polish: sorted by read
    std::vector<TandemRow> trows;    // tandems, dissect (td.reserved: the anchor): sorted by read, start
    uint64_t reads = 0, bases = 0;
    uint64_t windows_fwd[TREW_ANNOT_MAX_MOTIFS] = {}, windows_rev[TREW_ANNOT_MAX_MOTIFS] = {}, reported[TREW_ANNOT_MAX_MOTIFS] = {};
    uint32_t longest[TREW_ANNOT_MAX_MOTIFS] = {}, longest_tail[TREW_ANNOT_MAX_MOTIFS] = {};
    uint64_t terminal_fwd[TREW_ANNOT_MAX_MOTIFS] = {}, terminal_rev[TREW_ANNOT_MAX_MOTIFS] = {};
    uint64_t interval_retries = 0;  // intervals, chain, repeats, satellites, tandems, trace: batches resubmitted because their log overflowed
    uint64_t batches = 0;           // the non-empty chunks, each of which is one batch
    uint64_t runs_fwd[TREW_ANNOT_MAX_MOTIFS] = {}, runs_rev[TREW_ANNOT_MAX_MOTIFS] = {}, reported_rev[TREW_ANNOT_MAX_MOTIFS] = {};  // chain
    uint64_t variants_fwd[TREW_ANNOT_MAX_MOTIFS] = {}, variants_rev[TREW_ANNOT_MAX_MOTIFS] = {};
    std::vector<uint64_t> var_hist, var_reads_with;  // variants: [motif][strand][bin]; empty for the other kinds
    // periods: (period, strand-canonical unit) -> {reads, sum of end - start}
    std::map<std::pair<uint32_t, uint64_t>, std::pair<uint64_t, uint64_t>> period_units;
    // refine: (period, strand-canonical unit) -> its rows, bases and copies
    std::map<std::pair<uint32_t, uint64_t>, RefineUnit> refine_units;
    // polish: the same, the canonical unit as its codes (as satellite_units)
    std::map<std::pair<uint32_t, std::string>, RefineUnit> polish_units;
    // resolve: the same, and the rows whose period the alignment chose against step 1
    std::map<std::pair<uint32_t, uint64_t>, ResolveUnit> resolve_units;
    // decompose: (period, strand-canonical unit) -> its rows, bases and copies, and the units, edited items and items of their signatures
    std::map<std::pair<uint32_t, uint64_t>, DecomposeUnit> decompose_units;
    // tandems: (period, strand-canonical unit) -> its reads, tracts, bases and copies
    std::map<std::pair<uint32_t, uint64_t>, TandemUnit> tandem_units;
    // dissect: the same, and the units, edited items and items of the tracts' signatures
    std::map<std::pair<uint32_t, uint64_t>, DissectUnit> dissect_units;
    // repeats: (period, strand-canonical unit) -> its reads, tracts and bases
    std::map<std::pair<uint32_t, uint64_t>, RepeatUnit> repeat_units;
    // satellites: the same, the canonical unit as its codes (one char a base, T 0, G 1, C 2, A 3; see satellite_canonical)
    std::map<std::pair<uint32_t, std::string>, RepeatUnit> satellite_units;
};
void add_totals(AnnotFileResult &into, const AnnotFileResult &from);  // everything but the rows: sums, and the larger of longest*
struct Annotator;  // device contexts and one slot per worker
Annotator *annotator_create(const Config &cfg);
void annotator_destroy(Annotator *a);
AnnotFileResult process_annotate(Annotator *a, const Config &cfg, const char *file_name, bool is_gz, const AnnotRequest &rq);

// the command line of one measure: what motif_cli_main does not share
struct MotifOption {
    const char *name;                          // "--min_tract"; takes one argument
    std::function<bool(const char *)> parse;   // false: the argument is refused with `error`
    const char *error;
};
struct MotifFlag {
    const char *name;           // "--items"; takes no argument
    std::function<void()> set;
};
struct MotifCli {
    void (*usage)();
    std::vector<MotifOption> options;
    std::vector<MotifFlag> flags;
    std::function<const char *()> check;  // once all arguments are read: the text of the first complaint about the options, or nullptr
    std::function<void(AnnotRequest &rq, int m, uint32_t k)> per_motif;  // the request's parameters of motif m, which has k bases
    std::function<void(const AnnotFileResult &r, const std::vector<std::string> &names)> print_rows;  // header line and rows of one file
    std::function<void(const AnnotFileResult &total, const std::vector<std::string> &names)> print_summary;
    bool motif_less = false;                      // periods, repeats, satellites, refine, tandems, decompose, dissect, resolve: every positional argument is a file, `names` stays empty
    std::function<void(AnnotRequest &rq)> fill;   // motif_less: the request's parameters
    bool long_units = false;                      // monomers, copies: the units have 3 to 256 bases and fill the request's `monomers`; `names` holds the typed texts or the FASTA names
    std::function<const char *()> fasta;          // long_units: the FILE of --fasta, nullptr when the option was not given; with it every positional argument is a file
};
int motif_cli_main(int argc, char **argv, Measure kind, const MotifCli &cli);
// The command line the measures without motifs share (periods, repeats, refine, tandems: bound 32; satellites, polish: 256):
// --min_period, --max_period (default: bound), --penalty and --min_score with their check, and the request filled from them.
// `o` must outlive `cli`.
struct PeriodOptions {
    int min_period = 1, max_period = 32, penalty = 3, min_score = 24;
};
void period_options(MotifCli &cli, PeriodOptions &o, int bound);
// --candidates C on top of period_options (resolve: default 3; tandems, decompose, dissect: default 1): the option, its range
// check behind the periods' and the request's `candidates`.  `candidates` holds the default and must outlive `cli`.
void candidates_option(MotifCli &cli, int &candidates);
int annotate_main(int argc, char **argv);
int tracts_main(int argc, char **argv);
int intervals_main(int argc, char **argv);
int variants_main(int argc, char **argv);
int periods_main(int argc, char **argv);
int chain_main(int argc, char **argv);
int repeats_main(int argc, char **argv);
int satellites_main(int argc, char **argv);
int align_main(int argc, char **argv);
int refine_main(int argc, char **argv);
int polish_main(int argc, char **argv);
int tandems_main(int argc, char **argv);
int trace_main(int argc, char **argv);
int decompose_main(int argc, char **argv);
int dissect_main(int argc, char **argv);
int resolve_main(int argc, char **argv);
int monomers_main(int argc, char **argv);
int copies_main(int argc, char **argv);
// an item's read bases as a signature prints them (trace.cpp): motif orientation, upper case for a complete copy, lower for an end piece
std::string trace_unit_text(const TraceRow &row, uint32_t k);
uint64_t canonical_unit(uint64_t unit, int k);  // the smaller of the smallest rotations of a unit and of its reverse complement: the form of the scan's rows
// the same for a unit of up to 256 bases: the codes of unit[16] / period (one char a base, first base first) and the smaller,
// base by base in code order, of the smallest rotation of the codes and the smallest rotation of their reverse complement
std::string satellite_codes(const trew_hip_satellite &rec);
std::string unit_codes(const uint32_t (&unit)[16], uint32_t period);  // the codes of a unit packed as trew_hip_satellite.unit
std::string satellite_canonical(const std::string &codes);

struct RunStats {
    uint64_t reads = 0, bases = 0;
    double seconds = 0;
};
const RunStats &last_stats(const Scanner *s);

}  // namespace trew_host
