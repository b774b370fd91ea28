// align.cpp -- `trew align MOTIF[,MOTIF...] FASTQ...`: the indel-aware tract of the given motifs in every read -- a local
// alignment of the read against the motif repeated without end, so that missing and extra bases are errors like wrong ones:
// how many copies of the unit the read holds, where they begin and end, and how many of the errors are substitutions,
// insertions and deletions.  The definition is in include/trew_hip.h (trew_hip_alignment) and DESIGN 4.7e; the file path is
// `trew annotate`'s (process.cpp) and so are the conventions: CSV on stdout, messages on stderr, exit status 1 and an empty
// stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions
//   ... one row per (read, motif, strand) whose score reaches MIN_SCORE (default 24), sorted by read ordinal, motif in
//       command-line order, strand (+ before -)
//   >Summary
//   motif,strand,reads,reads_reported,bases,score,copies,consumed,matches,mismatches,insertions,deletions
//       (one row per motif and strand, over all files; bases: the sum of end - start; the other columns: the sums of the rows')
#include "trew_host.hpp"

namespace trew_host {

static void align_usage() {
    fprintf(stderr,
            "Usage: align [--help] [--thread THREAD] [--penalty P] [--min_score S] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report the best tract of the given repeat motifs (3 to 32 bases each, at most 8) in every read, aligned against the\n"
            "motif repeated without end: a matching base scores 1, a wrong, an extra and a missing base cost P (1 to 64, default 3)\n"
            "each; tracts that score less than S (default 24) are not reported.  One tract per read, motif and strand.\n");
}

AlignColumns align_columns(const uint32_t rec[5], uint32_t k, int penalty) {
    const uint32_t score = rec[0], len = rec[2] - rec[1], consumed = rec[3], matches = rec[4];
    const uint32_t errors = (matches - score) / (uint32_t) penalty;
    AlignColumns c;
    c.deletions = errors - (len - matches);
    c.insertions = errors - (consumed - matches);
    c.mismatches = len - matches - c.insertions;
    c.copies = consumed / k;
    return c;
}

int align_main(int argc, char **argv) {
    int penalty = 3, min_score = 24;
    std::vector<uint32_t> ks;
    MotifCli cli;
    cli.usage = align_usage;
    cli.options = {{"--penalty", [&](const char *s) { return parse_int(s, &penalty); }, "PENALTY must be a number."},
                   {"--min_score", [&](const char *s) { return parse_int(s, &min_score); }, "MIN_SCORE must be a number."}};
    cli.check = [&]() -> const char * {
        if (min_score < 1) return "MIN_SCORE must be greater than or equal to 1.";
        return penalty < 1 || penalty > 64 ? "PENALTY must be in range 1 to 64." : nullptr;
    };
    cli.per_motif = [&](AnnotRequest &rq, int m, uint32_t k) {
        rq.penalty = penalty;
        rq.min_score = (uint32_t) min_score;
        rq.min_tract[m] = 0;  // not read
        ks.push_back(k);
    };
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &names) {
        printf("read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions\n");
        for (const auto &row : r.arows) {
            const AlignColumns c = align_columns(row.rec, ks[(size_t) row.motif], penalty);
            printf("%llu,%u,%s,%c,%u,%u,%u,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, names[(size_t) row.motif].c_str(),
                   row.strand ? '-' : '+', row.rec[1], row.rec[2], row.rec[0], c.copies, row.rec[3], row.rec[4], c.mismatches, c.insertions, c.deletions);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &names) {
        printf(">Summary\nmotif,strand,reads,reads_reported,bases,score,copies,consumed,matches,mismatches,insertions,deletions\n");
        for (size_t m = 0; m < names.size(); m++)
            for (int s = 0; s < 2; s++) {
                const uint64_t *a = total.align_sums[m][s];
                printf("%s,%c,%llu", names[m].c_str(), s ? '-' : '+', (unsigned long long) total.reads);
                for (int i = 0; i < kAlignSums; i++) printf(",%llu", (unsigned long long) a[i]);
                printf("\n");
            }
    };
    return motif_cli_main(argc, argv, Measure::Align, cli);
}

}  // namespace trew_host
