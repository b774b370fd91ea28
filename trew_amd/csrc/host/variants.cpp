// variants.cpp -- `trew variants MOTIF[,MOTIF...] FASTQ...`: what the repeats of the given motifs are made of.  Per read the
// exact units of the motif as typed and the in-phase units with exactly one substituted base, over all reads the histogram
// of those substitutions (the telomere variant repeats: TCAGGG, TGAGGG, TTGGGG among TTAGGG).  The definition is in
// include/trew_hip.h (trew_hip_variant) and DESIGN 4.7; the file path is `trew annotate`'s (process.cpp) and so are the
// conventions: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,units_fwd,variants_fwd,distinct_fwd,top_fwd,top_count_fwd,units_rev,variants_rev,distinct_rev,top_rev,top_count_rev
//   ... one row per (read, motif) whose larger units_s + variants_s reaches MIN_UNITS (default 4), sorted by read ordinal,
//       then by motif in command-line order; top_s as the variant unit's text in motif orientation, `-` when there is none
//   >Summary
//   motif,reads,reads_reported,bases,units_fwd,units_rev,variants_fwd,variants_rev      (one row per motif, over all files)
//   >Variants
//   motif,variant,pos,base,count_fwd,reads_fwd,count_rev,reads_rev      (one row per bin with count_fwd + count_rev > 0, over
//       all reads and files; sorted by motif, then by count_fwd + count_rev descending, then by bin)
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdlib>

#include "trew_host.hpp"

namespace trew_host {

static void variants_usage() {
    fprintf(stderr,
            "Usage: variants [--help] [--thread THREAD] [--min_units N] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report what the repeats of the given motifs (3 to 32 bases each, at most 8, taken as typed) are made of: per read the exact\n"
            "units and the in-phase units with one substituted base, over all reads the histogram of those substitutions.  A read is\n"
            "listed when its units and variant units on one strand number at least N (1 to 4294967295, default 4).\n");
}

// any number strtoull can hold (the range is checked afterwards, with a message of its own; intervals_u32 refuses it here)
static bool variants_u64(const char *s, unsigned long long *out) {
    char *end = nullptr;
    if (!s[0] || s[0] == '-' || s[0] == '+') return false;
    errno = 0;
    const unsigned long long v = strtoull(s, &end, 10);
    if (*end || errno) return false;
    *out = v;
    return true;
}

// a bin as text: the motif as typed with base pos replaced
static const char kBase[4] = {'T', 'G', 'C', 'A'};
static std::string unit_text(std::string t, uint32_t bin) {
    if (bin == TREW_VARIANT_NONE) return std::string("-");
    for (char &ch : t) ch = (char) toupper((unsigned char) ch);
    if (bin / 4 < t.size()) t[bin / 4] = kBase[bin & 3u];
    return t;
}

int variants_main(int argc, char **argv) {
    unsigned long long min_units = 4;
    MotifCli cli;
    cli.usage = variants_usage;
    cli.options = {{"--min_units", [&](const char *s) { return variants_u64(s, &min_units); }, "MIN_UNITS must be a number."}};
    cli.check = [&]() -> const char * { return min_units < 1 || min_units > 4294967295ull ? "MIN_UNITS must be in range 1 to 4294967295." : nullptr; };
    cli.per_motif = [&](AnnotRequest &rq, int m, uint32_t) { rq.min_tract[m] = (uint32_t) min_units; };
    cli.print_rows = [](const AnnotFileResult &r, const std::vector<std::string> &names) {
        printf("read,length,motif,units_fwd,variants_fwd,distinct_fwd,top_fwd,top_count_fwd,units_rev,variants_rev,distinct_rev,top_rev,top_count_rev\n");
        for (const auto &row : r.rows) {
            const trew_hip_variant &v = row.v;
            const std::string &name = names[(size_t) row.motif];
            printf("%llu,%u,%s,%u,%u,%u,%s,%u,%u,%u,%u,%s,%u\n", (unsigned long long) row.read, row.length, name.c_str(), v.units_fwd, v.variants_fwd,
                   v.distinct_fwd, unit_text(name, v.top_fwd).c_str(), v.top_count_fwd, v.units_rev, v.variants_rev, v.distinct_rev,
                   unit_text(name, v.top_rev).c_str(), v.top_count_rev);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &names) {
        printf(">Summary\nmotif,reads,reads_reported,bases,units_fwd,units_rev,variants_fwd,variants_rev\n");
        for (size_t m = 0; m < names.size(); m++)
            printf("%s,%llu,%llu,%llu,%llu,%llu,%llu,%llu\n", names[m].c_str(), (unsigned long long) total.reads, (unsigned long long) total.reported[m],
                   (unsigned long long) total.bases, (unsigned long long) total.windows_fwd[m], (unsigned long long) total.windows_rev[m],
                   (unsigned long long) total.variants_fwd[m], (unsigned long long) total.variants_rev[m]);
        printf(">Variants\nmotif,variant,pos,base,count_fwd,reads_fwd,count_rev,reads_rev\n");
        std::vector<uint64_t> hist = total.var_hist, reads_with = total.var_reads_with;  // empty when no file held a read
        hist.resize(names.size() * 2 * TREW_VARIANT_BINS);
        reads_with.resize(hist.size());
        for (size_t m = 0; m < names.size(); m++) {
            const uint64_t *hf = &hist[m * 2 * TREW_VARIANT_BINS], *hr = hf + TREW_VARIANT_BINS;
            const uint64_t *rf = &reads_with[m * 2 * TREW_VARIANT_BINS], *rr = rf + TREW_VARIANT_BINS;
            std::vector<uint32_t> bins;
            for (uint32_t b = 0; b < TREW_VARIANT_BINS; b++)
                if (hf[b] + hr[b]) bins.push_back(b);
            std::stable_sort(bins.begin(), bins.end(), [&](uint32_t x, uint32_t y) { return hf[x] + hr[x] > hf[y] + hr[y]; });  // stable: bins ascend on a tie
            for (uint32_t b : bins)
                printf("%s,%s,%u,%c,%llu,%llu,%llu,%llu\n", names[m].c_str(), unit_text(names[m], b).c_str(), b / 4, kBase[b & 3u], (unsigned long long) hf[b],
                       (unsigned long long) rf[b], (unsigned long long) hr[b], (unsigned long long) rr[b]);
        }
    };
    return motif_cli_main(argc, argv, Measure::Variants, cli);
}

}  // namespace trew_host
