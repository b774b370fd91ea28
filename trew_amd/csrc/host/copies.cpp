// copies.cpp -- `trew copies [--fasta FILE] [--items] [--bases] [MONOMER[,MONOMER...]] FASTQ...`: `trew trace` for units of 3
// to 256 bases -- the monomer decomposition of a satellite array: where each copy of a given monomer begins and ends in every
// read, which copies are intact and which carry which substitutions, insertions and deletions.  The monomers are typed or
// come from a FASTA file, as for `trew monomers`, whose argument errors these are.  The definition is in include/trew_hip.h
// (trew_hip_copies) and DESIGN 4.7n; the file path is `trew annotate`'s (process.cpp), and so are the conventions: CSV on
// stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,signature
//   ... one row per (read, monomer, strand) whose score reaches MIN_SCORE: the thirteen columns of `trew monomers`, then units,
//       edited and signature as `trew trace` defines them.  For a monomer of at most 32 bases, or with --bases, the signature
//       is `trew trace`'s.  Above 32 bases an item that is no run prints as bases:mismatches.insertions.deletions, an end piece
//       (consumed < k) in parentheses: `(40:0.0.0) =3 172:28.2.1 =1`.
//   with --items instead one row per item, `trew trace`'s; unit: `=` for a run, else the item's read bases for a monomer of at
//   most 32 bases or with --bases, and empty otherwise
//   >Summary
//   `trew trace`'s, one row per monomer and strand, over all files
#include "trew_host.hpp"

namespace trew_host {

static void copies_usage() {
    fprintf(stderr,
            "Usage: copies [--help] [--thread THREAD] [--penalty P] [--min_score S] [--items] [--bases] [--devices LIST] [--stats]\n"
            "              [--fasta FILE] [MONOMER[,MONOMER...]] FASTQ...\n\n"
            "Report where each copy of the given units (3 to 256 bases each, at most 8; typed, or the records of the FASTA FILE)\n"
            "begins and ends in every read and which errors it carries: the best tract of `monomers` (a matching base scores 1, a\n"
            "wrong, an extra and a missing base cost P, 1 to 64, default 3, each; tracts that score less than S, default 24, are not\n"
            "reported) cut into copies of the unit -- runs of exact copies, copies with their errors and the end pieces, in place.\n"
            "--items lists one item per row; --bases prints an edited copy of a unit of more than 32 bases as its read bases.\n");
}

int copies_main(int argc, char **argv) {
    int penalty = 3, min_score = 24;
    bool items = false, bases = false, fasta_given = false;
    std::string fasta;
    std::vector<uint32_t> ks;
    MotifCli cli;
    cli.usage = copies_usage;
    cli.long_units = true;
    cli.fasta = [&]() -> const char * { return fasta_given ? fasta.c_str() : nullptr; };
    cli.options = {{"--penalty", [&](const char *s) { return parse_int(s, &penalty); }, "PENALTY must be a number."},
                   {"--min_score", [&](const char *s) { return parse_int(s, &min_score); }, "MIN_SCORE must be a number."},
                   {"--fasta",
                    [&](const char *s) {
                        fasta = s;
                        fasta_given = true;
                        return true;
                    },
                    "FILE must be a path."}};
    cli.flags = {{"--items", [&]() { items = true; }}, {"--bases", [&]() { bases = true; }}};
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
    // an item that is no run, as the signature prints it
    auto edited_text = [&](const TraceRow &row, uint32_t k) -> std::string {
        if (k <= 32 || bases) return trace_unit_text(row, k);
        const trew_hip_trace_item &it = row.it;
        const std::string t = std::to_string(it.bases) + ":" + std::to_string(it.mismatches) + "." + std::to_string(it.insertions) + "." + std::to_string(it.deletions);
        return it.consumed == k ? t : "(" + t + ")";
    };
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &names) {
        if (items) {
            printf("read,length,motif,strand,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit\n");
            for (const auto &row : r.xrows) {
                const trew_hip_trace_item &it = row.it;
                const uint32_t k = ks[(size_t) it.motif];
                printf("%llu,%u,%s,%c,%u,%u,%u,%u,%u,%u,%u,%u,%s\n", (unsigned long long) row.read, row.length, names[(size_t) it.motif].c_str(),
                       it.strand ? '-' : '+', it.start, it.bases, it.count, it.phase, it.consumed, it.mismatches, it.insertions, it.deletions,
                       row.text.empty() ? "=" : k <= 32 || bases ? trace_unit_text(row, k).c_str() : "");
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
                sig += r.xrows[i].text.empty() ? "=" + std::to_string(it.count) : edited_text(r.xrows[i], k);
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
    return motif_cli_main(argc, argv, Measure::Copies, cli);
}

}  // namespace trew_host
