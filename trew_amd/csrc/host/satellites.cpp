// satellites.cpp -- `trew satellites FASTQ...`: `trew repeats` with periods up to 256 -- minisatellites and satellite monomers.
// The definition is in include/trew_hip.h (trew_hip_satellite) and DESIGN 4.7d; the options, the file path (process.cpp) and the
// conventions are `trew repeats`'s: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,depth,period,unit,canonical,start,end,score,matches,support,scored_period
//   ... one row per tract (score >= MIN_SCORE), sorted by read ordinal, then start; `canonical` is the smaller of the smallest
//       rotation of the unit and the smallest rotation of its reverse complement, compared base by base in code order
//       (T < G < C < A): for a period of at most 32 what `trew periods` and `trew repeats` print
//   >Summary
//   period,canonical,reads,tracts,bases   (one row per (period, canonical) over all files, in the order of `trew repeats`: reads
//                                          descending, then period, then unit)
#include <algorithm>

#include "trew_host.hpp"

namespace trew_host {

std::string unit_codes(const uint32_t (&unit)[16], uint32_t period) {
    std::string c((size_t) period, '\0');
    for (uint32_t j = 0; j < period; j++) c[j] = (char) ((unit[j >> 4] >> (2 * (j & 15u))) & 3u);
    return c;
}

std::string satellite_codes(const trew_hip_satellite &rec) { return unit_codes(rec.unit, rec.period); }

// the smallest rotation of a string of codes
static std::string smallest_rotation(const std::string &c) {
    std::string best = c, rot = c;
    for (size_t i = 1; i < c.size(); i++) {
        std::rotate(rot.begin(), rot.begin() + 1, rot.end());
        if (rot < best) best = rot;
    }
    return best;
}

std::string satellite_canonical(const std::string &codes) {
    std::string rc(codes.rbegin(), codes.rend());
    for (char &x : rc) x = (char) (3 - x);  // T=0 G=1 C=2 A=3: the complement is 3 - code
    return std::min(smallest_rotation(codes), smallest_rotation(rc));
}

static std::string codes_text(const std::string &codes) {
    std::string t = codes;
    for (char &x : t) x = "TGCA"[(int) x];
    return t;
}

static void satellites_usage() {
    fprintf(stderr,
            "Usage: satellites [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every read, every repeat tract: its period (MIN_PERIOD to MAX_PERIOD, 1 to 256, default all), its consensus\n"
            "unit and its position, as `repeats` does for periods up to 32.  A base equal to the base one period on scores 1, any\n"
            "other costs P (1 to 64, default 3); tracts that score less than S (default 24) are not reported.  Neighbouring copies\n"
            "are compared, so an array of diverged monomers does not score at the default P.\n");
}

int satellites_main(int argc, char **argv) {
    PeriodOptions o;
    MotifCli cli;
    cli.usage = satellites_usage;
    period_options(cli, o, TREW_SATELLITE_MAX_PERIOD);
    cli.print_rows = [](const AnnotFileResult &r, const std::vector<std::string> &) {
        printf("read,length,depth,period,unit,canonical,start,end,score,matches,support,scored_period\n");
        for (const auto &row : r.srows) {
            const trew_hip_satellite &p = row.st;
            const std::string codes = satellite_codes(p);
            printf("%llu,%u,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, p.depth, p.period, codes_text(codes).c_str(),
                   codes_text(satellite_canonical(codes)).c_str(), p.start, p.end, p.score, p.matches, p.support, p.scored_period);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,tracts,bases\n");
        typedef std::pair<std::pair<uint32_t, std::string>, RepeatUnit> Row;
        std::vector<Row> v(total.satellite_units.begin(), total.satellite_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.reads != b.second.reads) return a.second.reads > b.second.reads;
            return a.first < b.first;  // period, then unit
        });
        for (const auto &row : v)
            printf("%u,%s,%llu,%llu,%llu\n", row.first.first, codes_text(row.first.second).c_str(), (unsigned long long) row.second.reads,
                   (unsigned long long) row.second.tracts, (unsigned long long) row.second.bases);
    };
    return motif_cli_main(argc, argv, Measure::Satellites, cli);
}

}  // namespace trew_host
