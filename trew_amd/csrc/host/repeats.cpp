// repeats.cpp -- `trew repeats FASTQ...`: every repeat tract of every read, with its unit and its place, without a motif given.
// The definition is in include/trew_hip.h (trew_hip_repeat) and DESIGN 4.7c; the options are `trew periods`'s, the file path
// is `trew annotate`'s (process.cpp) and so are the conventions: CSV on stdout, messages on stderr, exit status 1 and an
// empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,depth,period,unit,canonical,start,end,score,matches,support,scored_period
//   ... one row per tract (score >= MIN_SCORE), sorted by read ordinal, then start; depth 0 is the row of `trew periods`;
//       `canonical` is the unit's strand-canonical smallest rotation, the form of the scan's >H: / >L: rows
//   >Summary
//   period,canonical,reads,tracts,bases   (one row per (period, canonical) over all files; reads = the reads with such a tract,
//                                          bases = the sum of end - start; reads descending, then period, then unit)
#include <algorithm>

#include "trew_host.hpp"

namespace trew_host {

static void repeats_usage() {
    fprintf(stderr,
            "Usage: repeats [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every read, every repeat tract: its period (MIN_PERIOD to MAX_PERIOD, 1 to 32, default all), its consensus\n"
            "unit and its position.  A base equal to the base one period on scores 1, any other costs P (1 to 64, default 3).  The\n"
            "best-scoring tract of a read is the one `periods` reports (depth 0); what lies in front of it and what lies behind it\n"
            "are then searched in the same way, each on its own, until nothing scores S (default 24) or more.\n");
}

int repeats_main(int argc, char **argv) {
    PeriodOptions o;
    MotifCli cli;
    cli.usage = repeats_usage;
    period_options(cli, o, 32);
    cli.print_rows = [](const AnnotFileResult &r, const std::vector<std::string> &) {
        printf("read,length,depth,period,unit,canonical,start,end,score,matches,support,scored_period\n");
        char unit[33], canon[33];
        for (const auto &row : r.rrows) {
            const trew_hip_repeat &p = row.rp;
            int_to_four(unit, p.unit, (int) p.period);
            int_to_four(canon, canonical_unit(p.unit, (int) p.period), (int) p.period);
            printf("%llu,%u,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, p.depth, p.period, unit, canon, p.start, p.end, p.score,
                   p.matches, p.support, p.scored_period);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,tracts,bases\n");
        typedef std::pair<std::pair<uint32_t, uint64_t>, RepeatUnit> Row;
        std::vector<Row> v(total.repeat_units.begin(), total.repeat_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.reads != b.second.reads) return a.second.reads > b.second.reads;
            return a.first < b.first;  // period, then unit
        });
        char canon[33];
        for (const auto &row : v) {
            int_to_four(canon, row.first.second, (int) row.first.first);
            printf("%u,%s,%llu,%llu,%llu\n", row.first.first, canon, (unsigned long long) row.second.reads, (unsigned long long) row.second.tracts,
                   (unsigned long long) row.second.bases);
        }
    };
    return motif_cli_main(argc, argv, Measure::Repeats, cli);
}

}  // namespace trew_host
