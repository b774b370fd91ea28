// monomers.cpp -- `trew monomers [--fasta FILE] [MONOMER[,MONOMER...]] FASTQ...`: `trew align` for units of 3 to 256 bases --
// where in every read the array of a given satellite monomer lies, how many copies it holds and how its errors split, when
// the copies have diverged from each other and bases are missing or extra.  The monomers are typed, or read from a FASTA file
// of at most 8 records (the name is the header's first word, the sequence may span lines; with --fasta every positional
// argument is a file).  The definition is in include/trew_hip.h (trew_hip_monomers) and DESIGN 4.7m; the file path is
// `trew annotate`'s (process.cpp), rows and summary are `trew align`'s (align.cpp) with the typed text or the FASTA name in
// the `motif` column, and so are the conventions: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an
// argument error.
#include "trew_host.hpp"

namespace trew_host {

static void monomers_usage() {
    fprintf(stderr,
            "Usage: monomers [--help] [--thread THREAD] [--penalty P] [--min_score S] [--devices LIST] [--stats]\n"
            "                [--fasta FILE] [MONOMER[,MONOMER...]] FASTQ...\n\n"
            "Report the best tract of the given units (3 to 256 bases each, at most 8; typed, or the records of the FASTA FILE) in\n"
            "every read, aligned against the unit repeated without end: a matching base scores 1, a wrong, an extra and a missing\n"
            "base cost P (1 to 64, default 3; at 1 a random read scores against a long unit) each; tracts that score less than S\n"
            "(default 24) are not reported.  One tract per read, unit and strand.\n");
}

int monomers_main(int argc, char **argv) {
    int penalty = 3, min_score = 24;
    bool fasta_given = false;
    std::string fasta;
    std::vector<uint32_t> ks;
    MotifCli cli;
    cli.usage = monomers_usage;
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
        printf("read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions\n");
        for (const auto &row : r.arows) {
            const AlignColumns c = align_columns(row.rec, ks[(size_t) row.motif], penalty);
            printf("%llu,%u,%s,%c,%u,%u,%u,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, names[(size_t) row.motif].c_str(),
                   row.strand ? '-' : '+', row.rec[1], row.rec[2], row.rec[0], c.copies, row.rec[3], row.rec[4], c.mismatches, c.insertions, c.deletions);
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &names) {
        printf(">Summary\nmotif,strand,reads,reads_reported,bases,score,copies,consumed,matches,mismatches,insertions,deletions\n");
        for (size_t m = 0; m < names.size(); m++)
            for (int s = 0; s < 2; s++) {
                const uint64_t *a = total.align_sums[m][s];
                printf("%s,%c,%llu", names[m].c_str(), s ? '-' : '+', (unsigned long long) total.reads);
                for (int i = 0; i < kAlignSums; i++) printf(",%llu", (unsigned long long) a[i]);
                printf("\n");
            }
    };
    return motif_cli_main(argc, argv, Measure::Monomers, cli);
}

}  // namespace trew_host
