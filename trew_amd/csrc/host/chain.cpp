// chain.cpp -- `trew chain MOTIF[,MOTIF...] FASTQ...`: in which order the units of the given motifs come in every read -- the
// maximal in-phase runs of exact units and every anchored unit with one substituted base at its position (the variant-repeat
// region next to the subtelomere: `=41 TCAGGG =3 TCAGGG TGAGGG =212`).  The definition is in include/trew_hip.h
// (trew_hip_chain_item) and DESIGN 4.7b; the file path is `trew annotate`'s (process.cpp) and so are the conventions: CSV on
// stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,strand,start,end,units,variants,runs,signature
//   ... one row per (read, motif, strand) whose units + variants reaches MIN_UNITS (default 4), sorted by read ordinal, motif
//       in command-line order, strand (+ before -).  start: the first item's start; end: the largest start + count k of its
//       items; signature: the items in start order (read coordinates on both strands) joined by single spaces -- `=r` a run
//       of r exact units, a variant unit as its text in motif orientation, and between two consecutive items a and b with
//       d = b.start - (a.start + a.count k) != 0 a token `+d` or `-d`
//   with --items instead one row per item:  read,length,motif,strand,start,count,unit     (unit: `=` for a run)
//   >Summary
//   motif,strand,reads,units,variants,runs,longest_run      (one row per motif and strand, over all files; reads: the rows;
//       units, variants and runs over all reads; longest_run in units)
#include <cctype>
#include <cerrno>
#include <cstdlib>

#include "trew_host.hpp"

namespace trew_host {

static void chain_usage() {
    fprintf(stderr,
            "Usage: chain [--help] [--thread THREAD] [--min_units N] [--items] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report in which order the units of the given motifs (3 to 32 bases each, at most 8, taken as typed) come in every read: the\n"
            "runs of exact units and the in-phase units with one substituted base, in place.  A read and strand is listed when its units\n"
            "and variant units number at least N (1 to 4294967295, default 4); --items lists one item per row.\n");
}

static bool chain_u64(const char *s, unsigned long long *out) {
    char *end = nullptr;
    if (!s[0] || s[0] == '-' || s[0] == '+') return false;
    errno = 0;
    const unsigned long long v = strtoull(s, &end, 10);
    if (*end || errno) return false;
    *out = v;
    return true;
}

// a variant's bin as text: the motif as typed with base pos replaced
static std::string chain_unit_text(std::string t, uint32_t bin) {
    static const char kBase[4] = {'T', 'G', 'C', 'A'};
    for (char &ch : t) ch = (char) toupper((unsigned char) ch);
    if (bin / 4 < t.size()) t[bin / 4] = kBase[bin & 3u];
    return t;
}

int chain_main(int argc, char **argv) {
    unsigned long long min_units = 4;
    bool items = false;
    MotifCli cli;
    cli.usage = chain_usage;
    cli.options = {{"--min_units", [&](const char *s) { return chain_u64(s, &min_units); }, "MIN_UNITS must be a number."}};
    cli.flags = {{"--items", [&]() { items = true; }}};
    cli.check = [&]() -> const char * { return min_units < 1 || min_units > 4294967295ull ? "MIN_UNITS must be in range 1 to 4294967295." : nullptr; };
    cli.per_motif = [&](AnnotRequest &rq, int m, uint32_t) { rq.min_tract[m] = (uint32_t) min_units; };
    cli.print_rows = [&](const AnnotFileResult &r, const std::vector<std::string> &names) {
        if (items) {
            printf("read,length,motif,strand,start,count,unit\n");
            for (const auto &row : r.crows) {
                const std::string &name = names[(size_t) row.it.motif];
                printf("%llu,%u,%s,%c,%u,%u,%s\n", (unsigned long long) row.read, row.length, name.c_str(), row.it.strand ? '-' : '+', row.it.start, row.it.count,
                       row.it.bin == TREW_VARIANT_NONE ? "=" : chain_unit_text(name, row.it.bin).c_str());
            }
            return;
        }
        printf("read,length,motif,strand,start,end,units,variants,runs,signature\n");
        for (size_t i = 0; i < r.crows.size();) {
            const ChainRow &first = r.crows[i];
            const std::string &name = names[(size_t) first.it.motif];
            const uint64_t k = name.size();
            uint64_t end = 0, units = 0, nvar = 0, runs = 0, at = 0;
            std::string sig;
            size_t j = i;
            for (; j < r.crows.size() && r.crows[j].read == first.read && r.crows[j].it.motif == first.it.motif && r.crows[j].it.strand == first.it.strand; j++) {
                const trew_hip_chain_item &it = r.crows[j].it;
                if (j > i) {
                    sig += ' ';
                    if (it.start != at) sig += (it.start > at ? "+" + std::to_string(it.start - at) : "-" + std::to_string(at - it.start)) + " ";
                }
                if (it.bin == TREW_VARIANT_NONE) {
                    sig += "=" + std::to_string(it.count);
                    units += it.count;
                    runs++;
                } else {
                    sig += chain_unit_text(name, it.bin);
                    nvar++;
                }
                at = it.start + (uint64_t) it.count * k;
                end = std::max(end, at);
            }
            printf("%llu,%u,%s,%c,%u,%llu,%llu,%llu,%llu,%s\n", (unsigned long long) first.read, first.length, name.c_str(), first.it.strand ? '-' : '+',
                   first.it.start, (unsigned long long) end, (unsigned long long) units, (unsigned long long) nvar, (unsigned long long) runs, sig.c_str());
            i = j;
        }
    };
    cli.print_summary = [](const AnnotFileResult &total, const std::vector<std::string> &names) {
        printf(">Summary\nmotif,strand,reads,units,variants,runs,longest_run\n");
        for (size_t m = 0; m < names.size(); m++) {
            printf("%s,+,%llu,%llu,%llu,%llu,%u\n", names[m].c_str(), (unsigned long long) total.reported[m], (unsigned long long) total.windows_fwd[m],
                   (unsigned long long) total.variants_fwd[m], (unsigned long long) total.runs_fwd[m], total.longest[m]);
            printf("%s,-,%llu,%llu,%llu,%llu,%u\n", names[m].c_str(), (unsigned long long) total.reported_rev[m], (unsigned long long) total.windows_rev[m],
                   (unsigned long long) total.variants_rev[m], (unsigned long long) total.runs_rev[m], total.longest_tail[m]);
        }
    };
    return motif_cli_main(argc, argv, Measure::Chain, cli);
}

}  // namespace trew_host
