// decompose.cpp -- `trew decompose FASTQ...`: in which order the units of every read's own repeat come, without a motif given --
// the unit of `trew refine`, anchored at its smallest rotation, and the traceback of `trew trace` against it on the strand the
// unit was found on: the runs of complete exact copies, the copies with a substituted, an inserted or a deleted base, and the
// end pieces, in place (`=41 TCAGGG =3 TGAGGG =212`).  The definition is in include/trew_hip.h (trew_hip_decompose) and DESIGN
// 4.7i; the options are `trew refine`'s, `--candidates` (above 1: trew_hip_decompose_resolved) and `--items`, the file path is `trew annotate`'s (process.cpp) and so are the
// conventions: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,changed,scored_period,anchor,strand,units,edited,signature
//   ... one row per read whose final score reaches MIN_SCORE, sorted by read ordinal: the columns of `trew refine`; anchor: the
//       unit's smallest rotation M, at which the copies are cut; strand: + when `canonical` is M, - when it is the smallest
//       rotation of M's reverse complement; units, edited and signature as `trew trace` prints them for strand + and k = period
//       (read orientation: signatures compare directly only within one strand value)
//   with --items instead one row per item:
//   read,length,period,anchor,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit      (unit: `=` for a run)
//   >Summary
//   period,canonical,reads,bases,copies,units,edited,items   (one row per (period, canonical) over all files: the summary of
//                                          `trew refine`, then the sums of units and edited and the items; reads descending,
//                                          then period, then unit)
#include <algorithm>
#include <cctype>

#include "trew_host.hpp"

namespace trew_host {

static void decompose_usage() {
    fprintf(stderr,
            "Usage: decompose [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--candidates C] [--items] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every read, in which order the units of its own repeat come when bases are missing or extra, without a motif\n"
            "given: the unit of `refine` (periods MIN_PERIOD to MAX_PERIOD, 1 to 32, default all; a matching base scores 1, a wrong, an\n"
            "extra and a missing base cost P, 1 to 64, default 3, each; tracts that score less than S, default 24, are not reported),\n"
            "turned to its smallest rotation, and the tract cut into copies of it as `trace` does -- runs of exact copies, copies with\n"
            "their errors and the end pieces, in place, in read orientation.  --items lists one item per row.  With C above 1 (1 to 4, default 1) the\n"
            "unit is what `resolve` reports with C candidates, the period chosen by alignment; `resolve`'s candidates and rank are not\n"
            "reported here.\n");
}

// the anchored unit M: rotation `anchor` of the record's unit, M[j] = U[(j + anchor) mod k]
static uint64_t anchored_unit(const trew_hip_refined &f) {
    const uint32_t k = f.period, sh = 2 * f.reserved;
    if (!sh) return f.unit;
    const uint64_t mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1ull;
    return ((f.unit << sh) | (f.unit >> (2 * k - sh))) & mask;
}

// an item's read bases as the signature prints them: upper case for a complete copy, lower for an end piece
static std::string decompose_unit_text(const TraceRow &row, uint32_t k) {
    std::string t = row.text;
    const bool whole = row.it.consumed == k;
    for (char &ch : t) ch = (char) (whole ? toupper((unsigned char) ch) : tolower((unsigned char) ch));
    return t;
}

int decompose_main(int argc, char **argv) {
    PeriodOptions o;
    bool items = false;
    int candidates = 1;  // the plain entry point
    MotifCli cli;
    cli.usage = decompose_usage;
    period_options(cli, o, 32);
    candidates_option(cli, candidates);
    cli.flags = {{"--items", [&]() { items = true; }}};
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &) {
        if (items)
            printf("read,length,period,anchor,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit\n");
        else
            printf("read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,"
                   "changed,scored_period,anchor,strand,units,edited,signature\n");
        char unit[33], canon[33], seed[33], anchor[33];
        size_t i = 0;  // the items are sorted like the rows: a row's items follow those of the row before
        for (const auto &row : r.frows) {
            const trew_hip_refined &f = row.rf;
            const uint32_t k = f.period;
            const uint64_t m = anchored_unit(f), c_unit = canonical_unit(f.unit, (int) k);
            int_to_four(anchor, m, (int) k);
            uint64_t units = 0, edited = 0;
            std::string sig;
            for (; i < r.xrows.size() && r.xrows[i].read == row.read; i++) {
                const trew_hip_trace_item &it = r.xrows[i].it;
                if (items) {
                    printf("%llu,%u,%u,%s,%u,%u,%u,%u,%u,%u,%u,%u,%s\n", (unsigned long long) row.read, row.length, k, anchor, it.start, it.bases, it.count,
                           it.phase, it.consumed, it.mismatches, it.insertions, it.deletions,
                           r.xrows[i].text.empty() ? "=" : decompose_unit_text(r.xrows[i], k).c_str());
                    continue;
                }
                if (it.consumed == k * it.count) units += it.count;
                edited += it.mismatches || it.insertions || it.deletions;
                if (!sig.empty()) sig += ' ';
                sig += r.xrows[i].text.empty() ? "=" + std::to_string(it.count) : decompose_unit_text(r.xrows[i], k);
            }
            if (items) continue;
            const uint32_t rec[5] = {f.score, f.start, f.end, f.consumed, f.matches};
            const AlignColumns c = align_columns(rec, k, o.penalty);
            int_to_four(unit, f.unit, (int) k);
            int_to_four(canon, c_unit, (int) k);
            int_to_four(seed, f.seed_unit, (int) f.seed_period);
            printf("%llu,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%s,%u,%u,%u,%s,%c,%llu,%llu,%s\n", (unsigned long long) row.read, row.length, k, unit, canon,
                   f.start, f.end, f.score, c.copies, f.consumed, f.matches, c.mismatches, c.insertions, c.deletions, f.seed_period, seed, f.seed_score,
                   f.changed, f.scored_period, anchor, c_unit == m ? '+' : '-', (unsigned long long) units, (unsigned long long) edited, sig.c_str());
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,bases,copies,units,edited,items\n");
        typedef std::pair<std::pair<uint32_t, uint64_t>, DecomposeUnit> Row;
        std::vector<Row> v(total.decompose_units.begin(), total.decompose_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.reads != b.second.reads) return a.second.reads > b.second.reads;
            return a.first < b.first;  // period, then unit
        });
        char canon[33];
        for (const auto &row : v) {
            int_to_four(canon, row.first.second, (int) row.first.first);
            printf("%u,%s,%llu,%llu,%llu,%llu,%llu,%llu\n", row.first.first, canon, (unsigned long long) row.second.reads, (unsigned long long) row.second.bases,
                   (unsigned long long) row.second.copies, (unsigned long long) row.second.units, (unsigned long long) row.second.edited,
                   (unsigned long long) row.second.items);
        }
    };
    return motif_cli_main(argc, argv, Measure::Decompose, cli);
}

}  // namespace trew_host
