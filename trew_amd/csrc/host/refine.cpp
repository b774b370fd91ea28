// refine.cpp -- `trew refine FASTQ...`: what repeats in every read when bases are missing or extra, without a motif given --
// the period and tract of `trew periods`, a seed unit taken from the read, the wraparound alignment of `trew align` against it
// and the unit re-voted from that alignment: unit, tract, copies and the errors by kind.  The definition is in
// include/trew_hip.h (trew_hip_refined) and DESIGN 4.7f; the options are `trew periods`'s, the file path is `trew annotate`'s
// (process.cpp) and so are the conventions: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an
// argument error.
//
//   >/abs/path/file.fastq
//   read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,changed,scored_period
//   ... one row per read whose final score reaches MIN_SCORE, sorted by read ordinal; `canonical` is the unit's
//       strand-canonical smallest rotation, the form of the scan's >H: / >L: rows
//   >Summary
//   period,canonical,reads,bases,copies   (one row per (period, canonical) over all files; bases = the sum of end - start,
//                                          copies = the sum of the rows' copies; reads descending, then period, then unit)
#include <algorithm>

#include "trew_host.hpp"

namespace trew_host {

static void refine_usage() {
    fprintf(stderr,
            "Usage: refine [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every read, what repeats in it when bases are missing or extra: the period (MIN_PERIOD to MAX_PERIOD, 1 to 32,\n"
            "default all) and tract of `periods`, a unit taken from the read where it repeats longest, the read aligned against that\n"
            "unit repeated without end, and the unit voted again from the alignment.  A matching base scores 1, a wrong, an extra and\n"
            "a missing base cost P (1 to 64, default 3) each; tracts that score less than S (default 24) are not reported.  One tract\n"
            "per read.\n");
}

int refine_main(int argc, char **argv) {
    PeriodOptions o;
    MotifCli cli;
    cli.usage = refine_usage;
    period_options(cli, o, 32);
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &) {
        printf("read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,"
               "changed,scored_period\n");
        char unit[33], canon[33], seed[33];
        for (const auto &row : r.frows) {
            const trew_hip_refined &f = row.rf;
            const uint32_t rec[5] = {f.score, f.start, f.end, f.consumed, f.matches};
            const AlignColumns c = align_columns(rec, f.period, o.penalty);
            int_to_four(unit, f.unit, (int) f.period);
            int_to_four(canon, canonical_unit(f.unit, (int) f.period), (int) f.period);
            int_to_four(seed, f.seed_unit, (int) f.seed_period);
            printf("%llu,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%s,%u,%u,%u\n", (unsigned long long) row.read, row.length, f.period, unit, canon, f.start,
                   f.end, f.score, c.copies, f.consumed, f.matches, c.mismatches, c.insertions, c.deletions, f.seed_period, seed, f.seed_score, f.changed,
                   f.scored_period);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,bases,copies\n");
        typedef std::pair<std::pair<uint32_t, uint64_t>, RefineUnit> Row;
        std::vector<Row> v(total.refine_units.begin(), total.refine_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.reads != b.second.reads) return a.second.reads > b.second.reads;
            return a.first < b.first;  // period, then unit
        });
        char canon[33];
        for (const auto &row : v) {
            int_to_four(canon, row.first.second, (int) row.first.first);
            printf("%u,%s,%llu,%llu,%llu\n", row.first.first, canon, (unsigned long long) row.second.reads, (unsigned long long) row.second.bases,
                   (unsigned long long) row.second.copies);
        }
    };
    return motif_cli_main(argc, argv, Measure::Refine, cli);
}

}  // namespace trew_host
