// variants.cpp -- `trew variants MOTIF[,MOTIF...] FASTQ...`: what the repeats of the given motifs are made of.  Per read the
// exact units of the motif as typed and the in-phase units with exactly one substituted base, over all reads the histogram
// of those substitutions (the telomere variant repeats: TCAGGG, TGAGGG, TTGGGG among TTAGGG).  The definition is in
// include/trew_hip.h (trew_hip_variant) and DESIGN 4.7; the file path is `trew annotate`'s (process.cpp) and so are the
// conventions: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,units_fwd,variants_fwd,distinct_fwd,top_fwd,top_count_fwd,units_rev,variants_rev,distinct_rev,top_rev,top_count_rev
//   ... one row per (read, motif) whose larger units_s + variants_s reaches MIN_UNITS (default 4), sorted by read ordinal,
//       then by motif in command-line order; top_s as the variant unit's text in motif orientation, `-` when there is none
//   >Summary
//   motif,reads,reads_reported,bases,units_fwd,units_rev,variants_fwd,variants_rev      (one row per motif, over all files)
//   >Variants
//   motif,variant,pos,base,count_fwd,reads_fwd,count_rev,reads_rev      (one row per bin with count_fwd + count_rev > 0, over
//       all reads and files; sorted by motif, then by count_fwd + count_rev descending, then by bin)
#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "trew_host.hpp"

namespace trew_host {

static void variants_usage() {
    fprintf(stderr,
            "Usage: variants [--help] [--thread THREAD] [--min_units N] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report what the repeats of the given motifs (3 to 32 bases each, at most 8, taken as typed) are made of: per read the exact\n"
            "units and the in-phase units with one substituted base, over all reads the histogram of those substitutions.  A read is\n"
            "listed when its units and variant units on one strand number at least N (1 to 4294967295, default 4).\n");
}

static bool variants_u64(const char *s, unsigned long long *out) {
    char *end = nullptr;
    if (!s[0] || s[0] == '-' || s[0] == '+') return false;
    errno = 0;
    const unsigned long long v = strtoull(s, &end, 10);
    if (*end || errno) return false;
    *out = v;
    return true;
}

static bool variants_int(const char *s, int *out) {
    char *end = nullptr;
    const long v = strtol(s, &end, 10);
    if (!s[0] || *end || v < INT_MIN || v > INT_MAX) return false;
    *out = (int) v;
    return true;
}

int variants_main(int argc, char **argv) {
    Config cfg;
    unsigned long long min_units = 4;
    std::vector<std::string> positional;
    auto bad = [&](const std::string &msg) {
        fprintf(stderr, "%s\n", msg.c_str());
        variants_usage();
        return 1;
    };
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        auto need = [&](const char *name) -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "%s: expected 1 argument(s). 0 provided.\n", name);
                variants_usage();
                exit(1);
            }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") {
            variants_usage();
            return 0;
        } else if (a == "-t" || a == "--thread") {
            if (!variants_int(need("--thread"), &cfg.NUM_THREAD)) return bad("THREAD must be a number.");
        } else if (a == "--min_units") {
            if (!variants_u64(need("--min_units"), &min_units)) return bad("MIN_UNITS must be a number.");
        } else if (a == "--stats") {
            cfg.stats = true;
        } else if (a == "--devices") {
            const std::string list = need("--devices");
            cfg.devices.clear();
            size_t pos = 0;
            bool ok = true;
            while (pos <= list.size()) {
                size_t comma = list.find(',', pos);
                if (comma == std::string::npos) comma = list.size();
                int d;
                if (!variants_int(list.substr(pos, comma - pos).c_str(), &d) || d < 0) ok = false;
                else cfg.devices.push_back(d);
                pos = comma + 1;
            }
            if (!ok || cfg.devices.empty()) return bad("DEVICES must be a comma-separated list of device ordinals.");
        } else if (a.size() > 1 && a[0] == '-') {
            return bad("Unknown argument: " + a);
        } else {
            positional.push_back(a);
        }
    }
    if (positional.empty()) return bad("MOTIF is required.");
    if (cfg.NUM_THREAD <= 0) return bad("number of threads must be positive.");
    if (min_units < 1 || min_units > 4294967295ull) return bad("MIN_UNITS must be in range 1 to 4294967295.");

    // MOTIF[,MOTIF...], printed as given
    std::vector<std::string> names;
    {
        const std::string &list = positional[0];
        size_t pos = 0;
        while (pos <= list.size()) {
            size_t comma = list.find(',', pos);
            if (comma == std::string::npos) comma = list.size();
            names.push_back(list.substr(pos, comma - pos));
            pos = comma + 1;
        }
    }
    if (names.size() > TREW_ANNOT_MAX_MOTIFS) return bad("At most 8 motifs can be given.");
    AnnotRequest rq;
    rq.variants = true;
    for (const auto &name : names) {
        for (char ch : name)
            if (!strchr("ACGTacgt", ch) || !ch) return bad("MOTIF '" + name + "' must consist of A, C, G and T.");
        if (name.size() < 3 || name.size() > 32) return bad("MOTIF '" + name + "': the length must be in range 3 to 32.");
        if (trew_motif_parse(name.c_str(), &rq.motifs[rq.n_motifs])) return bad(trew_hip_last_error(nullptr));
        rq.min_tract[rq.n_motifs] = (uint32_t) min_units;
        rq.n_motifs++;
    }
    if (positional.size() < 2) return bad("FASTQ is required.");
    std::vector<std::string> files(positional.begin() + 1, positional.end());
    for (const auto &f : files) {
        struct stat st;
        if (stat(f.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
            fprintf(stderr, "%s : file not found\n", f.c_str());
            variants_usage();
            return 1;
        }
    }
    if (cfg.NUM_THREAD - 1 > 16 * (int) cfg.devices.size()) cfg.NUM_THREAD = 16 * (int) cfg.devices.size() + 1;

    // a bin as text: the motif as typed with base pos replaced
    static const char kBase[4] = {'T', 'G', 'C', 'A'};
    auto unit_text = [&](int m, uint32_t bin) {
        if (bin == TREW_VARIANT_NONE) return std::string("-");
        std::string t = names[(size_t) m];
        for (char &ch : t) ch = (char) toupper((unsigned char) ch);
        if (bin / 4 < t.size()) t[bin / 4] = kBase[bin & 3u];
        return t;
    };
    const size_t hl = (size_t) rq.n_motifs * 2 * TREW_VARIANT_BINS;
    Annotator *an = annotator_create(cfg);
    AnnotFileResult total;
    total.var_hist.assign(hl, 0);
    total.var_reads_with.assign(hl, 0);
    for (const auto &f : files) {
        char buf[PATH_MAX];
        const std::string path = realpath(f.c_str(), buf) ? std::string(buf) : f;
        const size_t dot = f.find_last_of('.'), slash = f.find_last_of('/');
        const std::string ext = dot != std::string::npos && (slash == std::string::npos || dot > slash) ? f.substr(dot) : "";
        const AnnotFileResult r = process_annotate(an, cfg, path.c_str(), ext == ".gz" || ext == ".bgz", rq);
        printf(">%s\n", path.c_str());
        printf("read,length,motif,units_fwd,variants_fwd,distinct_fwd,top_fwd,top_count_fwd,units_rev,variants_rev,distinct_rev,top_rev,top_count_rev\n");
        for (const auto &row : r.rows) {
            const trew_hip_variant &v = row.v;
            printf("%llu,%u,%s,%u,%u,%u,%s,%u,%u,%u,%u,%s,%u\n", (unsigned long long) row.read, row.length, names[(size_t) row.motif].c_str(), v.units_fwd,
                   v.variants_fwd, v.distinct_fwd, unit_text(row.motif, v.top_fwd).c_str(), v.top_count_fwd, v.units_rev, v.variants_rev, v.distinct_rev,
                   unit_text(row.motif, v.top_rev).c_str(), v.top_count_rev);
        }
        total.reads += r.reads;
        total.bases += r.bases;
        for (int m = 0; m < rq.n_motifs; m++) {
            total.windows_fwd[m] += r.windows_fwd[m];
            total.windows_rev[m] += r.windows_rev[m];
            total.variants_fwd[m] += r.variants_fwd[m];
            total.variants_rev[m] += r.variants_rev[m];
            total.reported[m] += r.reported[m];
        }
        for (size_t i = 0; i < r.var_hist.size() && i < hl; i++) {
            total.var_hist[i] += r.var_hist[i];
            total.var_reads_with[i] += r.var_reads_with[i];
        }
    }
    annotator_destroy(an);
    printf(">Summary\nmotif,reads,reads_reported,bases,units_fwd,units_rev,variants_fwd,variants_rev\n");
    for (int m = 0; m < rq.n_motifs; m++)
        printf("%s,%llu,%llu,%llu,%llu,%llu,%llu,%llu\n", names[(size_t) m].c_str(), (unsigned long long) total.reads, (unsigned long long) total.reported[m],
               (unsigned long long) total.bases, (unsigned long long) total.windows_fwd[m], (unsigned long long) total.windows_rev[m],
               (unsigned long long) total.variants_fwd[m], (unsigned long long) total.variants_rev[m]);
    printf(">Variants\nmotif,variant,pos,base,count_fwd,reads_fwd,count_rev,reads_rev\n");
    for (int m = 0; m < rq.n_motifs; m++) {
        const uint64_t *hf = &total.var_hist[(size_t) m * 2 * TREW_VARIANT_BINS], *hr = hf + TREW_VARIANT_BINS;
        const uint64_t *rf = &total.var_reads_with[(size_t) m * 2 * TREW_VARIANT_BINS], *rr = rf + TREW_VARIANT_BINS;
        std::vector<uint32_t> bins;
        for (uint32_t b = 0; b < TREW_VARIANT_BINS; b++)
            if (hf[b] + hr[b]) bins.push_back(b);
        std::stable_sort(bins.begin(), bins.end(), [&](uint32_t x, uint32_t y) { return hf[x] + hr[x] > hf[y] + hr[y]; });  // stable: bins ascend on a tie
        for (uint32_t b : bins)
            printf("%s,%s,%u,%c,%llu,%llu,%llu,%llu\n", names[(size_t) m].c_str(), unit_text(m, b).c_str(), b / 4, kBase[b & 3u], (unsigned long long) hf[b],
                   (unsigned long long) rf[b], (unsigned long long) hr[b], (unsigned long long) rr[b]);
    }
    return 0;
}

}  // namespace trew_host
