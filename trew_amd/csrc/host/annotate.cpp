// annotate.cpp -- `trew annotate MOTIF[,MOTIF...] FASTQ...`: which reads carry a motif, how much of each read it covers and
// where the longest tract lies.  The reference has no counterpart (its tables are sums over all reads); the conventions are
// those of `short` and `long`: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,windows_fwd,windows_rev,tract_start_fwd,tract_len_fwd,tract_start_rev,tract_len_rev
//   ... one row per (read, motif) whose longer tract has at least MIN_TRACT bases (default 4 k of that motif),
//       sorted by read ordinal, then by motif in command-line order
//   >Summary
//   motif,reads,reads_reported,bases,windows_fwd,windows_rev,longest_tract      (one row per motif, over all files)
#include "trew_host.hpp"

namespace trew_host {

static void annotate_usage() {
    fprintf(stderr,
            "Usage: annotate [--help] [--thread THREAD] [--min_tract BASES] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report the reads that carry the given repeat motifs (3 to 32 bases each, at most 8) and their longest tracts.\n");
}

int annotate_main(int argc, char **argv) {
    int min_tract = 0;  // not given: 4 k of each motif
    bool min_tract_given = false;
    MotifCli cli;
    cli.usage = annotate_usage;
    cli.options = {{"--min_tract", [&](const char *s) { return min_tract_given = parse_int(s, &min_tract); }, "MIN_TRACT must be a number."}};
    cli.check = [&]() -> const char * { return min_tract_given && min_tract < 1 ? "MIN_TRACT must be greater than or equal to 1." : nullptr; };
    cli.per_motif = [&](AnnotRequest &rq, int m, uint32_t k) { rq.min_tract[m] = min_tract_given ? (uint32_t) min_tract : 4u * k; };
    cli.print_rows = [](const AnnotFileResult &r, const std::vector<std::string> &names) {
        printf("read,length,motif,windows_fwd,windows_rev,tract_start_fwd,tract_len_fwd,tract_start_rev,tract_len_rev\n");
        for (const auto &row : r.rows)
            printf("%llu,%u,%s,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, names[(size_t) row.motif].c_str(), row.a.windows_fwd,
                   row.a.windows_rev, row.a.tract_start_fwd, row.a.tract_len_fwd, row.a.tract_start_rev, row.a.tract_len_rev);
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &names) {
        printf(">Summary\nmotif,reads,reads_reported,bases,windows_fwd,windows_rev,longest_tract\n");
        for (size_t m = 0; m < names.size(); m++)
            printf("%s,%llu,%llu,%llu,%llu,%llu,%u\n", names[m].c_str(), (unsigned long long) total.reads, (unsigned long long) total.reported[m],
                   (unsigned long long) total.bases, (unsigned long long) total.windows_fwd[m], (unsigned long long) total.windows_rev[m], total.longest[m]);
    };
    return motif_cli_main(argc, argv, Measure::Annotate, cli);
}

}  // namespace trew_host
