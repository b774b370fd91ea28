// polish.cpp -- `trew polish FASTQ...`: `trew refine` for periods up to 256 -- where a minisatellite or satellite array lies
// in a noisy read, how many copies it holds, how its errors split and what its monomer is, without a monomer given.  The
// definition is in include/trew_hip.h (trew_hip_polished) and DESIGN 4.7o; the options are `trew satellites`'s, the file path is
// `trew annotate`'s (process.cpp) and so are the conventions: CSV on stdout, messages on stderr, exit status 1 and an empty
// stdout on an argument error.  With --max_period 32 the output is `trew refine`'s.
//
//   >/abs/path/file.fastq
//   read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,changed,scored_period
//   ... one row per read whose final score reaches MIN_SCORE, sorted by read ordinal; `unit` and `seed_unit` hold up to 256
//       letters; `canonical` is `trew satellites`': the smaller of the smallest rotations of the unit and of its reverse complement
//   >Summary
//   period,canonical,reads,bases,copies   (one row per (period, canonical) over all files; bases = the sum of end - start,
//                                          copies = the sum of the rows' copies; reads descending, then period, then unit)
#include <algorithm>

#include "trew_host.hpp"

namespace trew_host {

static std::string polish_text(const std::string &codes) {
    std::string t = codes;
    for (char &x : t) x = "TGCA"[(int) x];
    return t;
}

static void polish_usage() {
    fprintf(stderr,
            "Usage: polish [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every read, what repeats in it when bases are missing or extra, for periods up to 256: the period (MIN_PERIOD\n"
            "to MAX_PERIOD, 1 to 256, default all) and tract of `satellites`, a unit taken from the read where it repeats longest, the\n"
            "read aligned against that unit repeated without end, and the unit voted again from the alignment.  A matching base scores\n"
            "1, a wrong, an extra and a missing base cost P (1 to 64, default 3; use 2 or more for long units) each; tracts that score\n"
            "less than S (default 24) are not reported.  One tract per read.\n");
}

int polish_main(int argc, char **argv) {
    PeriodOptions o;
    MotifCli cli;
    cli.usage = polish_usage;
    period_options(cli, o, TREW_POLISH_MAX_PERIOD);
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &) {
        printf("read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,"
               "changed,scored_period\n");
        for (const auto &row : r.prows) {
            const trew_hip_polished &f = row.pl;
            const uint32_t rec[5] = {f.score, f.start, f.end, f.consumed, f.matches};
            const AlignColumns c = align_columns(rec, f.period, o.penalty);
            const std::string unit = unit_codes(f.unit, f.period);
            printf("%llu,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%s,%u,%u,%u\n", (unsigned long long) row.read, row.length, f.period, polish_text(unit).c_str(),
                   polish_text(satellite_canonical(unit)).c_str(), f.start, f.end, f.score, c.copies, f.consumed, f.matches, c.mismatches, c.insertions,
                   c.deletions, f.seed_period, polish_text(unit_codes(f.seed_unit, f.seed_period)).c_str(), f.seed_score, f.changed, f.scored_period);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,bases,copies\n");
        typedef std::pair<std::pair<uint32_t, std::string>, RefineUnit> Row;
        std::vector<Row> v(total.polish_units.begin(), total.polish_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.reads != b.second.reads) return a.second.reads > b.second.reads;
            return a.first < b.first;  // period, then unit
        });
        for (const auto &row : v)
            printf("%u,%s,%llu,%llu,%llu\n", row.first.first, polish_text(row.first.second).c_str(), (unsigned long long) row.second.reads,
                   (unsigned long long) row.second.bases, (unsigned long long) row.second.copies);
    };
    return motif_cli_main(argc, argv, Measure::Polish, cli);
}

}  // namespace trew_host
