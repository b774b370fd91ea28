// tracts.cpp -- `trew tracts MOTIF[,MOTIF...] FASTQ...`: how far a repeat reaches in from either end of every read when single
// wrong bases are forgiven (the telomere length of a long read).  The definition is in include/trew_hip.h (trew_hip_tract)
// and DESIGN 4.5; the file path is `trew annotate`'s (process.cpp) and so are the conventions: CSV on stdout, messages on
// stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,covered_fwd,head_len_fwd,head_cov_fwd,tail_len_fwd,tail_cov_fwd,covered_rev,head_len_rev,head_cov_rev,tail_len_rev,tail_cov_rev
//   ... one row per (read, motif) whose longest of the four tract lengths has at least MIN_TRACT bases (default 4 k of that
//       motif), sorted by read ordinal, then by motif in command-line order
//   >Summary
//   motif,reads,reads_reported,bases,covered_fwd,covered_rev,longest_head,longest_tail      (one row per motif, over all files)
#include "trew_host.hpp"

namespace trew_host {

static void tracts_usage() {
    fprintf(stderr,
            "Usage: tracts [--help] [--thread THREAD] [--penalty P] [--min_tract BASES] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report the error-tolerant tracts of the given repeat motifs (3 to 32 bases each, at most 8) at both ends of every read:\n"
            "a base outside every matching window costs P (1 to 64, default 3), a base inside one scores 1.\n");
}

int tracts_main(int argc, char **argv) {
    int min_tract = 0;  // not given: 4 k of each motif
    int penalty = 3;
    bool min_tract_given = false;
    MotifCli cli;
    cli.usage = tracts_usage;
    cli.options = {{"--penalty", [&](const char *s) { return parse_int(s, &penalty); }, "PENALTY must be a number."},
                   {"--min_tract", [&](const char *s) { return min_tract_given = parse_int(s, &min_tract); }, "MIN_TRACT must be a number."}};
    cli.check = [&]() -> const char * {
        if (min_tract_given && min_tract < 1) return "MIN_TRACT must be greater than or equal to 1.";
        return penalty < 1 || penalty > 64 ? "PENALTY must be in range 1 to 64." : nullptr;
    };
    cli.per_motif = [&](AnnotRequest &rq, int m, uint32_t k) {
        rq.penalty = penalty;
        rq.min_tract[m] = min_tract_given ? (uint32_t) min_tract : 4u * k;
    };
    cli.print_rows = [](const AnnotFileResult &r, const std::vector<std::string> &names) {
        printf("read,length,motif,covered_fwd,head_len_fwd,head_cov_fwd,tail_len_fwd,tail_cov_fwd,covered_rev,head_len_rev,head_cov_rev,tail_len_rev,tail_cov_rev\n");
        for (const auto &row : r.rows) {
            const trew_hip_tract &t = row.t;
            printf("%llu,%u,%s,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, names[(size_t) row.motif].c_str(), t.covered_fwd,
                   t.head_len_fwd, t.head_cov_fwd, t.tail_len_fwd, t.tail_cov_fwd, t.covered_rev, t.head_len_rev, t.head_cov_rev, t.tail_len_rev, t.tail_cov_rev);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &names) {
        printf(">Summary\nmotif,reads,reads_reported,bases,covered_fwd,covered_rev,longest_head,longest_tail\n");
        for (size_t m = 0; m < names.size(); m++)
            printf("%s,%llu,%llu,%llu,%llu,%llu,%u,%u\n", names[m].c_str(), (unsigned long long) total.reads, (unsigned long long) total.reported[m],
                   (unsigned long long) total.bases, (unsigned long long) total.windows_fwd[m], (unsigned long long) total.windows_rev[m], total.longest[m],
                   total.longest_tail[m]);
    };
    return motif_cli_main(argc, argv, Measure::Tracts, cli);
}

}  // namespace trew_host
