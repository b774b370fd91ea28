// tracts.cpp -- `trew tracts MOTIF[,MOTIF...] FASTQ...`: how far a repeat reaches in from either end of every read when single
// wrong bases are forgiven (the telomere length of a long read).  The definition is in include/trew_hip.h (trew_hip_tract)
// and DESIGN 4.5; the file path is `trew annotate`'s (process.cpp) and so are the conventions: CSV on stdout, messages on
// stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,covered_fwd,head_len_fwd,head_cov_fwd,tail_len_fwd,tail_cov_fwd,covered_rev,head_len_rev,head_cov_rev,tail_len_rev,tail_cov_rev
//   ... one row per (read, motif) whose longest of the four tract lengths has at least MIN_TRACT bases (default 4 k of that
//       motif), sorted by read ordinal, then by motif in command-line order
//   >Summary
//   motif,reads,reads_reported,bases,covered_fwd,covered_rev,longest_head,longest_tail      (one row per motif, over all files)
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sys/stat.h>

#include "trew_host.hpp"

namespace trew_host {

static void tracts_usage() {
    fprintf(stderr,
            "Usage: tracts [--help] [--thread THREAD] [--penalty P] [--min_tract BASES] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report the error-tolerant tracts of the given repeat motifs (3 to 32 bases each, at most 8) at both ends of every read:\n"
            "a base outside every matching window costs P (1 to 64, default 3), a base inside one scores 1.\n");
}

static bool tracts_int(const char *s, int *out) {
    char *end = nullptr;
    const long v = strtol(s, &end, 10);
    if (!s[0] || *end || v < INT_MIN || v > INT_MAX) return false;
    *out = (int) v;
    return true;
}

int tracts_main(int argc, char **argv) {
    Config cfg;
    int min_tract = 0;  // 0: 4 k of each motif
    int penalty = 3;
    bool min_tract_given = false;
    std::vector<std::string> positional;
    auto bad = [&](const std::string &msg) {
        fprintf(stderr, "%s\n", msg.c_str());
        tracts_usage();
        return 1;
    };
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        auto need = [&](const char *name) -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "%s: expected 1 argument(s). 0 provided.\n", name);
                tracts_usage();
                exit(1);
            }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") {
            tracts_usage();
            return 0;
        } else if (a == "-t" || a == "--thread") {
            if (!tracts_int(need("--thread"), &cfg.NUM_THREAD)) return bad("THREAD must be a number.");
        } else if (a == "--penalty") {
            if (!tracts_int(need("--penalty"), &penalty)) return bad("PENALTY must be a number.");
        } else if (a == "--min_tract") {
            if (!tracts_int(need("--min_tract"), &min_tract)) return bad("MIN_TRACT must be a number.");
            min_tract_given = true;
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
                if (!tracts_int(list.substr(pos, comma - pos).c_str(), &d) || d < 0) ok = false;
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
    if (min_tract_given && min_tract < 1) return bad("MIN_TRACT must be greater than or equal to 1.");
    if (penalty < 1 || penalty > 64) return bad("PENALTY must be in range 1 to 64.");

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
    rq.penalty = penalty;
    for (const auto &name : names) {
        for (char ch : name)
            if (!strchr("ACGTacgt", ch) || !ch) return bad("MOTIF '" + name + "' must consist of A, C, G and T.");
        if (name.size() < 3 || name.size() > 32) return bad("MOTIF '" + name + "': the length must be in range 3 to 32.");
        if (trew_motif_parse(name.c_str(), &rq.motifs[rq.n_motifs])) return bad(trew_hip_last_error(nullptr));
        rq.min_tract[rq.n_motifs] = min_tract_given ? (uint32_t) min_tract : 4u * (uint32_t) name.size();
        rq.n_motifs++;
    }
    if (positional.size() < 2) return bad("FASTQ is required.");
    std::vector<std::string> files(positional.begin() + 1, positional.end());
    for (const auto &f : files) {
        struct stat st;
        if (stat(f.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
            fprintf(stderr, "%s : file not found\n", f.c_str());
            tracts_usage();
            return 1;
        }
    }
    if (cfg.NUM_THREAD - 1 > 16 * (int) cfg.devices.size()) cfg.NUM_THREAD = 16 * (int) cfg.devices.size() + 1;

    Annotator *an = annotator_create(cfg);
    AnnotFileResult total;
    for (const auto &f : files) {
        char buf[PATH_MAX];
        const std::string path = realpath(f.c_str(), buf) ? std::string(buf) : f;
        const size_t dot = f.find_last_of('.'), slash = f.find_last_of('/');
        const std::string ext = dot != std::string::npos && (slash == std::string::npos || dot > slash) ? f.substr(dot) : "";
        const AnnotFileResult r = process_annotate(an, cfg, path.c_str(), ext == ".gz" || ext == ".bgz", rq);
        printf(">%s\n", path.c_str());
        printf("read,length,motif,covered_fwd,head_len_fwd,head_cov_fwd,tail_len_fwd,tail_cov_fwd,covered_rev,head_len_rev,head_cov_rev,tail_len_rev,tail_cov_rev\n");
        for (const auto &row : r.rows) {
            const trew_hip_tract &t = row.t;
            printf("%llu,%u,%s,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u\n", (unsigned long long) row.read, row.length, names[(size_t) row.motif].c_str(), t.covered_fwd,
                   t.head_len_fwd, t.head_cov_fwd, t.tail_len_fwd, t.tail_cov_fwd, t.covered_rev, t.head_len_rev, t.head_cov_rev, t.tail_len_rev, t.tail_cov_rev);
        }
        total.reads += r.reads;
        total.bases += r.bases;
        for (int m = 0; m < rq.n_motifs; m++) {
            total.windows_fwd[m] += r.windows_fwd[m];
            total.windows_rev[m] += r.windows_rev[m];
            total.reported[m] += r.reported[m];
            total.longest[m] = std::max(total.longest[m], r.longest[m]);
            total.longest_tail[m] = std::max(total.longest_tail[m], r.longest_tail[m]);
        }
    }
    annotator_destroy(an);
    printf(">Summary\nmotif,reads,reads_reported,bases,covered_fwd,covered_rev,longest_head,longest_tail\n");
    for (int m = 0; m < rq.n_motifs; m++)
        printf("%s,%llu,%llu,%llu,%llu,%llu,%u,%u\n", names[(size_t) m].c_str(), (unsigned long long) total.reads, (unsigned long long) total.reported[m],
               (unsigned long long) total.bases, (unsigned long long) total.windows_fwd[m], (unsigned long long) total.windows_rev[m], total.longest[m],
               total.longest_tail[m]);
    return 0;
}

}  // namespace trew_host
