// tandems.cpp -- `trew tandems FASTQ...`: every repeat tract of every read when bases are missing or extra, without a motif
// given -- the recursion of `trew repeats` over what lies in front of a tract and behind it, with the seed, the wraparound
// alignment and the re-voted unit of `trew refine` for each piece.  The definition is in include/trew_hip.h (trew_hip_tandem) and
// DESIGN 4.7g, with `--candidates` above 1 in 4.7l (trew_hip_tandems_resolved); the options are `trew periods`'s and `--candidates`, the file path is `trew annotate`'s (process.cpp) and so are the conventions: CSV
// on stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,depth,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,changed,scored_period
//   ... one row per tract (score >= MIN_SCORE), sorted by read ordinal, then start; the columns behind `depth` are those of
//       `trew refine` behind `length`
//   >Summary
//   period,canonical,reads,tracts,bases,copies   (one row per (period, canonical) over all files; reads = the reads with such a
//                                                 tract, bases = the sum of end - start, copies = the sum of the rows' copies;
//                                                 reads descending, then period, then unit)
#include <algorithm>

#include "trew_host.hpp"

namespace trew_host {

static void tandems_usage() {
    fprintf(stderr,
            "Usage: tandems [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--candidates C] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every read, every repeat tract when bases are missing or extra: what `refine` reports for the read (period\n"
            "MIN_PERIOD to MAX_PERIOD, 1 to 32, default all; a unit taken from the read, the read aligned against it, the unit voted\n"
            "again), then the same for what lies in front of that tract and for what lies behind it, each on its own, until nothing\n"
            "repeats.  A matching base scores 1, a wrong, an extra and a missing base cost P (1 to 64, default 3) each; a tract that\n"
            "scores less than S (default 24) is not reported, and the search goes on around it.  With C above 1 (1 to 4, default 1)\n"
            "every piece gets what `resolve` reports for it with C candidates, the period chosen by alignment, in the place of\n"
            "`refine`'s; `resolve`'s candidates, rank, first_period and first_score are not reported here.\n");
}

int tandems_main(int argc, char **argv) {
    PeriodOptions o;
    int candidates = 1;  // the plain entry point
    MotifCli cli;
    cli.usage = tandems_usage;
    period_options(cli, o, 32);
    candidates_option(cli, candidates);
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &) {
        printf("read,length,depth,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,"
               "seed_score,changed,scored_period\n");
        char unit[33], canon[33], seed[33];
        for (const auto &row : r.trows) {
            const trew_hip_tandem &f = row.td;
            const uint32_t rec[5] = {f.score, f.start, f.end, f.consumed, f.matches};
            const AlignColumns c = align_columns(rec, f.period, o.penalty);
            int_to_four(unit, f.unit, (int) f.period);
            int_to_four(canon, canonical_unit(f.unit, (int) f.period), (int) f.period);
            int_to_four(seed, f.seed_unit, (int) f.seed_period);
            printf("%llu,%u,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%s,%u,%u,%u\n", (unsigned long long) row.read, row.length, f.depth, f.period, unit, canon,
                   f.start, f.end, f.score, c.copies, f.consumed, f.matches, c.mismatches, c.insertions, c.deletions, f.seed_period, seed, f.seed_score,
                   f.changed, f.scored_period);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,tracts,bases,copies\n");
        typedef std::pair<std::pair<uint32_t, uint64_t>, TandemUnit> Row;
        std::vector<Row> v(total.tandem_units.begin(), total.tandem_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.reads != b.second.reads) return a.second.reads > b.second.reads;
            return a.first < b.first;  // period, then unit
        });
        char canon[33];
        for (const auto &row : v) {
            int_to_four(canon, row.first.second, (int) row.first.first);
            printf("%u,%s,%llu,%llu,%llu,%llu\n", row.first.first, canon, (unsigned long long) row.second.reads, (unsigned long long) row.second.tracts,
                   (unsigned long long) row.second.bases, (unsigned long long) row.second.copies);
        }
    };
    return motif_cli_main(argc, argv, Measure::Tandems, cli);
}

}  // namespace trew_host
