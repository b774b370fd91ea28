// intervals.cpp -- `trew intervals MOTIF[,MOTIF...] FASTQ...`: where in every read the repeat lies -- the intervals of bases
// inside matching windows whose gaps are at most MAX_GAP bases, any number per read (a telomere behind an adapter, an
// internal tract, an interstitial telomeric sequence, several tracts).  The definition is in include/trew_hip.h
// (trew_hip_interval) and DESIGN 4.6; the file path is `trew annotate`'s (process.cpp) and so are the conventions: CSV on
// stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,strand,start,end,covered
//   ... one row per kept interval (end - start >= MIN_LEN; default 4 k of that motif, gaps of at most 3 k), sorted by read
//       ordinal, motif in command-line order, strand (+ before -), start
//   >Summary
//   motif,reads,reads_with_interval,bases,intervals_fwd,intervals_rev,longest_fwd,longest_rev,terminal_fwd,terminal_rev
//       (one row per motif, over all files; terminal_s: kept intervals with start == 0 or end == length)
#include <cstdlib>
#include <cstring>

#include "trew_host.hpp"

namespace trew_host {

static void intervals_usage() {
    fprintf(stderr,
            "Usage: intervals [--help] [--thread THREAD] [--max_gap BASES] [--min_len BASES] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report where in every read the given repeat motifs (3 to 32 bases each, at most 8) lie: the intervals of bases inside\n"
            "matching windows whose gaps are at most MAX_GAP bases (default 3 k) and that span at least MIN_LEN bases (default 4 k).\n");
}

// a number in [0, 2^32) of at most ten characters (variants_u64 takes any length and looks at errno instead)
static bool intervals_u32(const char *s, uint32_t *out) {
    char *end = nullptr;
    if (!s[0] || s[0] == '-' || s[0] == '+') return false;
    const unsigned long long v = strtoull(s, &end, 10);
    if (*end || v > 0xffffffffull || strlen(s) > 10) return false;
    *out = (uint32_t) v;
    return true;
}

int intervals_main(int argc, char **argv) {
    uint32_t max_gap = 0, min_len = 0;  // not given: 3 k and 4 k of each motif
    bool max_gap_given = false, min_len_given = false;
    MotifCli cli;
    cli.usage = intervals_usage;
    cli.options = {{"--max_gap", [&](const char *s) { return max_gap_given = intervals_u32(s, &max_gap); }, "MAX_GAP must be a number in range 0 to 4294967295."},
                   {"--min_len", [&](const char *s) { return min_len_given = intervals_u32(s, &min_len); }, "MIN_LEN must be a number in range 1 to 4294967295."}};
    cli.check = [&]() -> const char * { return min_len_given && min_len < 1 ? "MIN_LEN must be a number in range 1 to 4294967295." : nullptr; };
    cli.per_motif = [&](AnnotRequest &rq, int m, uint32_t k) {
        rq.min_tract[m] = 0;  // not read: min_len is part of the rule
        rq.rules[m].max_gap = max_gap_given ? max_gap : 3u * k;
        rq.rules[m].min_len = min_len_given ? min_len : 4u * k;
    };
    cli.print_rows = [](const AnnotFileResult &r, const std::vector<std::string> &names) {
        printf("read,length,motif,strand,start,end,covered\n");
        for (const auto &row : r.irows)
            printf("%llu,%u,%s,%c,%u,%u,%u\n", (unsigned long long) row.read, row.length, names[(size_t) row.iv.motif].c_str(), row.iv.strand ? '-' : '+',
                   row.iv.start, row.iv.end, row.iv.covered);
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &names) {
        printf(">Summary\nmotif,reads,reads_with_interval,bases,intervals_fwd,intervals_rev,longest_fwd,longest_rev,terminal_fwd,terminal_rev\n");
        for (size_t m = 0; m < names.size(); m++)
            printf("%s,%llu,%llu,%llu,%llu,%llu,%u,%u,%llu,%llu\n", names[m].c_str(), (unsigned long long) total.reads, (unsigned long long) total.reported[m],
                   (unsigned long long) total.bases, (unsigned long long) total.windows_fwd[m], (unsigned long long) total.windows_rev[m], total.longest[m],
                   total.longest_tail[m], (unsigned long long) total.terminal_fwd[m], (unsigned long long) total.terminal_rev[m]);
    };
    return motif_cli_main(argc, argv, Measure::Intervals, cli);
}

}  // namespace trew_host
