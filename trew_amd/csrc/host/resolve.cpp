// resolve.cpp -- `trew resolve FASTQ...`: `trew refine` with the period chosen by alignment -- the few periods that score best
// at a fixed phase are each refined as `trew refine` refines its one, and the record with the largest final score is reported.
// The definition is in include/trew_hip.h (trew_hip_resolved) and DESIGN 4.7k; the options are `trew refine`'s and
// `--candidates`, the file path is `trew annotate`'s (process.cpp) and so are the conventions: CSV on stdout, messages on stderr,
// exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,changed,scored_period,candidates,rank,first_period,first_score
//   ... one row per read whose final score reaches MIN_SCORE, sorted by read ordinal: the columns of `trew refine`; candidates:
//       the periods that were refined; rank: the winner's place among them by fixed-phase score (0: what `trew refine`
//       reports); first_period and first_score: the period and score of `trew refine`'s record
//   >Summary
//   period,canonical,reads,bases,copies,repaired   (as `trew refine`; repaired = the rows with rank > 0)
#include <algorithm>

#include "trew_host.hpp"

namespace trew_host {

static void resolve_usage() {
    static_assert(TREW_RESOLVE_MAX_CANDIDATES == 4, "the text below");
    fprintf(stderr,
            "Usage: resolve [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--candidates C] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every read, what `refine` reports with the period chosen by alignment: the C (1 to 4, default 3) periods\n"
            "(MIN_PERIOD to MAX_PERIOD, 1 to 32, default all) that score best at a fixed phase are each refined as `refine` refines its\n"
            "one, and the record with the largest final score is kept (on a tie the shorter unit, then the better-scoring period).  A\n"
            "matching base scores 1, a wrong, an extra and a missing base cost P (1 to 64, default 3) each; tracts that score less than S\n"
            "(default 24) are not reported.  One tract per read.\n");
}

int resolve_main(int argc, char **argv) {
    PeriodOptions o;
    int candidates = 3;
    MotifCli cli;
    cli.usage = resolve_usage;
    period_options(cli, o, 32);
    candidates_option(cli, candidates);
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &) {
        printf("read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,"
               "changed,scored_period,candidates,rank,first_period,first_score\n");
        char unit[33], canon[33], seed[33];
        for (const auto &row : r.vrows) {
            const trew_hip_resolved &f = row.rv;
            const uint32_t rec[5] = {f.score, f.start, f.end, f.consumed, f.matches};
            const AlignColumns c = align_columns(rec, f.period, o.penalty);
            int_to_four(unit, f.unit, (int) f.period);
            int_to_four(canon, canonical_unit(f.unit, (int) f.period), (int) f.period);
            int_to_four(seed, f.seed_unit, (int) f.seed_period);
            printf("%llu,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%s,%u,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, f.period, unit, canon,
                   f.start, f.end, f.score, c.copies, f.consumed, f.matches, c.mismatches, c.insertions, c.deletions, f.seed_period, seed, f.seed_score,
                   f.changed, f.scored_period, f.candidates, f.rank, f.first_period, f.first_score);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,bases,copies,repaired\n");
        typedef std::pair<std::pair<uint32_t, uint64_t>, ResolveUnit> Row;
        std::vector<Row> v(total.resolve_units.begin(), total.resolve_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.reads != b.second.reads) return a.second.reads > b.second.reads;
            return a.first < b.first;  // period, then unit
        });
        char canon[33];
        for (const auto &row : v) {
            int_to_four(canon, row.first.second, (int) row.first.first);
            printf("%u,%s,%llu,%llu,%llu,%llu\n", row.first.first, canon, (unsigned long long) row.second.reads, (unsigned long long) row.second.bases,
                   (unsigned long long) row.second.copies, (unsigned long long) row.second.repaired);
        }
    };
    return motif_cli_main(argc, argv, Measure::Resolve, cli);
}

}  // namespace trew_host
