// dissect.cpp -- `trew dissect FASTQ...`: what every repeat tract of every read is made of, without a motif given -- the tracts of
// `trew tandems`, each with its unit anchored at its smallest rotation and cut into copies of it as `trew decompose` cuts a read's
// best tract: the runs of complete exact copies, the copies with a substituted, an inserted or a deleted base, and the end
// pieces, in place.  The definition is in include/trew_hip.h (trew_hip_dissect) and DESIGN 4.7j; the options are `trew
// decompose`'s (`--candidates` above 1: trew_hip_dissect_resolved), the file path is `trew annotate`'s (process.cpp) and so are the conventions: CSV on stdout, messages on stderr,
// exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,depth,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,changed,scored_period,anchor,strand,units,edited,signature
//   ... one row per tract (score >= MIN_SCORE), sorted by read ordinal, then start: the columns of `trew tandems`, then those
//       that `trew decompose` adds behind `trew refine`'s
//   with --items instead one row per item:
//   read,length,tract,period,anchor,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit
//       (tract: the index of the item's tract among its read's rows, from 0; unit: `=` for a run)
//   >Summary
//   period,canonical,reads,tracts,bases,copies,units,edited,items   (one row per (period, canonical) over all files: the
//                                          summary of `trew tandems`, then the sums of units and edited and the items; reads
//                                          descending, then period, then unit)
#include <algorithm>
#include <cctype>

#include "trew_host.hpp"

namespace trew_host {

static void dissect_usage() {
    fprintf(stderr,
            "Usage: dissect [--help] [--thread THREAD] [--min_period K] [--max_period K] [--penalty P] [--min_score S] [--candidates C] [--items] [--devices LIST] [--stats] FASTQ...\n\n"
            "Report, for every repeat tract of every read, in which order the units of its repeat come when bases are missing or extra,\n"
            "without a motif given: the tracts of `tandems` (periods MIN_PERIOD to MAX_PERIOD, 1 to 32, default all; a matching base\n"
            "scores 1, a wrong, an extra and a missing base cost P, 1 to 64, default 3, each; tracts that score less than S, default 24,\n"
            "are not reported), each with its unit turned to its smallest rotation and cut into copies of it as `decompose` does --\n"
            "runs of exact copies, copies with their errors and the end pieces, in place, in read orientation.  --items lists one item\n"
            "per row.  With C above 1 (1 to 4, default 1) every piece gets what `resolve` reports for it with C candidates, the period\n"
            "chosen by alignment, in the place of `refine`'s; `resolve`'s candidates and rank are not reported here.\n");
}

// the anchored unit M: rotation `anchor` of the record's unit, M[j] = U[(j + anchor) mod k]
static uint64_t anchored_unit(const trew_hip_tandem &f) {
    const uint32_t k = f.period, sh = 2 * f.reserved;
    if (!sh) return f.unit;
    const uint64_t mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1ull;
    return ((f.unit << sh) | (f.unit >> (2 * k - sh))) & mask;
}

// an item's read bases as the signature prints them: upper case for a complete copy, lower for an end piece
static std::string dissect_unit_text(const TraceRow &row, uint32_t k) {
    std::string t = row.text;
    const bool whole = row.it.consumed == k;
    for (char &ch : t) ch = (char) (whole ? toupper((unsigned char) ch) : tolower((unsigned char) ch));
    return t;
}

int dissect_main(int argc, char **argv) {
    PeriodOptions o;
    bool items = false;
    int candidates = 1;  // the plain entry point
    MotifCli cli;
    cli.usage = dissect_usage;
    period_options(cli, o, 32);
    candidates_option(cli, candidates);
    cli.flags = {{"--items", [&]() { items = true; }}};
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &) {
        if (items)
            printf("read,length,tract,period,anchor,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit\n");
        else
            printf("read,length,depth,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,"
                   "seed_score,changed,scored_period,anchor,strand,units,edited,signature\n");
        char unit[33], canon[33], seed[33], anchor[33];
        size_t i = 0;  // the items are sorted like the rows: a row's items follow those of the row before
        for (const auto &row : r.trows) {
            const trew_hip_tandem &f = row.td;
            const uint32_t k = f.period;
            const uint64_t m = anchored_unit(f), c_unit = canonical_unit(f.unit, (int) k);
            int_to_four(anchor, m, (int) k);
            uint64_t units = 0, edited = 0;
            std::string sig;
            for (; i < r.xrows.size() && r.xrows[i].read == row.read && r.xrows[i].it.start < f.end; i++) {
                const trew_hip_trace_item &it = r.xrows[i].it;
                if (items) {
                    printf("%llu,%u,%u,%u,%s,%u,%u,%u,%u,%u,%u,%u,%u,%s\n", (unsigned long long) row.read, row.length, it.motif, k, anchor, it.start, it.bases,
                           it.count, it.phase, it.consumed, it.mismatches, it.insertions, it.deletions,
                           r.xrows[i].text.empty() ? "=" : dissect_unit_text(r.xrows[i], k).c_str());
                    continue;
                }
                if (it.consumed == k * it.count) units += it.count;
                edited += it.mismatches || it.insertions || it.deletions;
                if (!sig.empty()) sig += ' ';
                sig += r.xrows[i].text.empty() ? "=" + std::to_string(it.count) : dissect_unit_text(r.xrows[i], k);
            }
            if (items) continue;
            const uint32_t rec[5] = {f.score, f.start, f.end, f.consumed, f.matches};
            const AlignColumns c = align_columns(rec, k, o.penalty);
            int_to_four(unit, f.unit, (int) k);
            int_to_four(canon, c_unit, (int) k);
            int_to_four(seed, f.seed_unit, (int) f.seed_period);
            printf("%llu,%u,%u,%u,%s,%s,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%s,%u,%u,%u,%s,%c,%llu,%llu,%s\n", (unsigned long long) row.read, row.length, f.depth, k, unit,
                   canon, f.start, f.end, f.score, c.copies, f.consumed, f.matches, c.mismatches, c.insertions, c.deletions, f.seed_period, seed,
                   f.seed_score, f.changed, f.scored_period, anchor, c_unit == m ? '+' : '-', (unsigned long long) units, (unsigned long long) edited,
                   sig.c_str());
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &) {
        printf(">Summary\nperiod,canonical,reads,tracts,bases,copies,units,edited,items\n");
        typedef std::pair<std::pair<uint32_t, uint64_t>, DissectUnit> Row;
        std::vector<Row> v(total.dissect_units.begin(), total.dissect_units.end());
        std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) {
            if (a.second.reads != b.second.reads) return a.second.reads > b.second.reads;
            return a.first < b.first;  // period, then unit
        });
        char canon[33];
        for (const auto &row : v) {
            int_to_four(canon, row.first.second, (int) row.first.first);
            printf("%u,%s,%llu,%llu,%llu,%llu,%llu,%llu,%llu\n", row.first.first, canon, (unsigned long long) row.second.reads,
                   (unsigned long long) row.second.tracts, (unsigned long long) row.second.bases, (unsigned long long) row.second.copies,
                   (unsigned long long) row.second.units, (unsigned long long) row.second.edited, (unsigned long long) row.second.items);
        }
    };
    return motif_cli_main(argc, argv, Measure::Dissect, cli);
}

}  // namespace trew_host
