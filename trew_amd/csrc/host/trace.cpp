// trace.cpp -- `trew trace MOTIF[,MOTIF...] FASTQ...`: in which order the units of the given motifs come in every read when
// bases are missing or extra -- the traceback of `trew align`'s wraparound alignment, cut into copies of the motif: the runs of
// complete exact copies, the copies with a substituted, an inserted or a deleted base, and the end pieces, in place
// (`=41 TCAGGG =3 TGAGGG =212`).  The definition is in include/trew_hip.h (trew_hip_trace_item) and DESIGN 4.7h; the file path
// is `trew annotate`'s (process.cpp) and so are the conventions: CSV on stdout, messages on stderr, exit status 1 and an empty
// stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,signature
//   ... one row per (read, motif, strand) whose score reaches MIN_SCORE (default 24), sorted by read ordinal, motif in
//       command-line order, strand (+ before -): the thirteen columns of `trew align`; units: the copies of the items with
//       consumed = k count; edited: the items with an error; signature: the items in read order joined by single spaces -- `=r`
//       a run of r complete exact copies, a complete copy with errors as its read bases in upper case, an end piece (consumed <
//       k) as its read bases in lower case; on strand - the read bases of an item are reverse-complemented (motif orientation)
//   with --items instead one row per item:
//   read,length,motif,strand,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit      (unit: `=` for a run)
//   >Summary
//   motif,strand,reads,reads_reported,bases,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,items
//       (one row per motif and strand, over all files: the summary of `trew align`, then the sums of units and edited and the items)
#include <cctype>

#include "trew_host.hpp"

namespace trew_host {

static void trace_usage() {
    fprintf(stderr,
            "Usage: trace [--help] [--thread THREAD] [--penalty P] [--min_score S] [--items] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report in which order the units of the given repeat motifs (3 to 32 bases each, at most 8) come in every read when bases\n"
            "are missing or extra: the best tract of `align` (a matching base scores 1, a wrong, an extra and a missing base cost P, 1\n"
            "to 64, default 3, each; tracts that score less than S, default 24, are not reported) cut into copies of the motif -- runs\n"
            "of exact copies, copies with their errors and the end pieces, in place.  --items lists one item per row.\n");
}

// an item's read bases as the signature prints them: motif orientation, upper case for a complete copy, lower for an end piece
std::string trace_unit_text(const TraceRow &row, uint32_t k) {
    std::string t = row.text;
    if (row.it.strand) {
        std::string rc(t.rbegin(), t.rend());
        for (char &ch : rc) {
            const char c = (char) toupper((unsigned char) ch);
            ch = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
        }
        t = rc;
    }
    const bool whole = row.it.consumed == k;
    for (char &ch : t) ch = (char) (whole ? toupper((unsigned char) ch) : tolower((unsigned char) ch));
    return t;
}

int trace_main(int argc, char **argv) {
    int penalty = 3, min_score = 24;
    bool items = false;
    std::vector<uint32_t> ks;
    MotifCli cli;
    cli.usage = trace_usage;
    cli.options = {{"--penalty", [&](const char *s) { return parse_int(s, &penalty); }, "PENALTY must be a number."},
                   {"--min_score", [&](const char *s) { return parse_int(s, &min_score); }, "MIN_SCORE must be a number."}};
    cli.flags = {{"--items", [&]() { items = true; }}};
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
        if (items) {
            printf("read,length,motif,strand,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit\n");
            for (const auto &row : r.xrows) {
                const trew_hip_trace_item &it = row.it;
                printf("%llu,%u,%s,%c,%u,%u,%u,%u,%u,%u,%u,%u,%s\n", (unsigned long long) row.read, row.length, names[(size_t) it.motif].c_str(),
                       it.strand ? '-' : '+', it.start, it.bases, it.count, it.phase, it.consumed, it.mismatches, it.insertions, it.deletions,
                       row.text.empty() ? "=" : trace_unit_text(row, ks[(size_t) it.motif]).c_str());
            }
            return;
        }
        printf("read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,signature\n");
        size_t i = 0;  // the items are sorted like the rows: a row's items follow those of the row before
        for (const auto &row : r.arows) {
            const uint32_t k = ks[(size_t) row.motif];
            const AlignColumns c = align_columns(row.rec, k, penalty);
            uint64_t units = 0, edited = 0;
            std::string sig;
            for (; i < r.xrows.size() && r.xrows[i].read == row.read && (int) r.xrows[i].it.motif == row.motif && (int) r.xrows[i].it.strand == row.strand; i++) {
                const trew_hip_trace_item &it = r.xrows[i].it;
                if (it.consumed == k * it.count) units += it.count;
                edited += it.mismatches || it.insertions || it.deletions;
                if (!sig.empty()) sig += ' ';
                sig += r.xrows[i].text.empty() ? "=" + std::to_string(it.count) : trace_unit_text(r.xrows[i], k);
            }
            printf("%llu,%u,%s,%c,%u,%u,%u,%u,%u,%u,%u,%u,%u,%llu,%llu,%s\n", (unsigned long long) row.read, row.length, names[(size_t) row.motif].c_str(),
                   row.strand ? '-' : '+', row.rec[1], row.rec[2], row.rec[0], c.copies, row.rec[3], row.rec[4], c.mismatches, c.insertions, c.deletions,
                   (unsigned long long) units, (unsigned long long) edited, sig.c_str());
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &names) {
        printf(">Summary\nmotif,strand,reads,reads_reported,bases,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,items\n");
        for (size_t m = 0; m < names.size(); m++)
            for (int s = 0; s < 2; s++) {
                printf("%s,%c,%llu", names[m].c_str(), s ? '-' : '+', (unsigned long long) total.reads);
                for (int i = 0; i < kAlignSums; i++) printf(",%llu", (unsigned long long) total.align_sums[m][s][i]);
                for (int i = 0; i < kTraceSums; i++) printf(",%llu", (unsigned long long) total.trace_sums[m][s][i]);
                printf("\n");
            }
    };
    return motif_cli_main(argc, argv, Measure::Trace, cli);
}

}  // namespace trew_host
