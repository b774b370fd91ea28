// periods.cpp -- `trew periods FASTQ...`: what repeats in every read, with which unit, and where, without a motif given.
// The definition is in include/trew_hip.h (trew_hip_period) and DESIGN 4.7a; the file path is `trew annotate`'s
// (process.cpp) and so are the conventions: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an
// argument error.
//
//   >/abs/path/file.fastq
//   read,length,period,unit,canonical,start,end,score,matches,support,scored_period
//   ... one row per read with a record (score >= MIN_SCORE), sorted by read ordinal; `canonical` is the unit's
//       strand-canonical smallest rotation, the form of the scan's >H: / >L: rows
//   >Summary
//   period,canonical,reads,bases      (one row per (period, canonical) over all files; bases = the sum of end - start;
//                                      reads descending, then period, then unit)
#include <algorithm>

#include "trew_host.hpp"

namespace trew_host {

static void periods_usage() {
    fprintf(stderr,
            "Usage: periods [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every read, the period (MIN_PERIOD to MAX_PERIOD, 1 to 32, default all), the consensus unit and the position\n"
            "of its best-scoring repeat tract: a base equal to the base one period on scores 1, any other costs P (1 to 64, default 3);\n"
            "tracts that score less than S (default 24) are not reported.  One tract per read.\n");
}

int periods_main(int argc, char **argv) {
    PeriodOptions o;
    MotifCli cli;
    cli.usage = periods_usage;
    period_options(cli, o, 32);
    cli.print_rows = [](const AnnotFileResult &r, const std::vector<std::string> &) {
        printf("read,length,period,unit,canonical,start,end,score,matches,support,scored_period\n");
        char unit[33], canon[33];
        for (const auto &row : r.rows) {
            const trew_hip_period &p = row.p;
            int_to_four(unit, p.unit, (int) p.period);
            int_to_four(canon, canonical_unit(p.unit, (int) p.period), (int) p.period);
            printf("%llu,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, p.period, unit, canon, p.start, p.end, p.score, p.matches,
                   p.support, p.scored_period);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,bases\n");
        typedef std::pair<std::pair<uint32_t, uint64_t>, std::pair<uint64_t, uint64_t>> Row;
        std::vector<Row> v(total.period_units.begin(), total.period_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.first != b.second.first) return a.second.first > b.second.first;
            return a.first < b.first;  // period, then unit
        });
        char canon[33];
        for (const auto &row : v) {
            int_to_four(canon, row.first.second, (int) row.first.first);
            printf("%u,%s,%llu,%llu\n", row.first.first, canon, (unsigned long long) row.second.first, (unsigned long long) row.second.second);
        }
    };
    return motif_cli_main(argc, argv, Measure::Periods, cli);
}

}  // namespace trew_host
