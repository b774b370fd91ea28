// intervals.cpp -- `trew intervals MOTIF[,MOTIF...] FASTQ...`: where in every read the repeat lies -- the intervals of bases
// inside matching windows whose gaps are at most MAX_GAP bases, any number per read (a telomere behind an adapter, an
// internal tract, an interstitial telomeric sequence, several tracts).  The definition is in include/trew_hip.h
// (trew_hip_interval) and DESIGN 4.6; the file path is `trew annotate`'s (process.cpp) and so are the conventions: CSV on
// stdout, messages on stderr, exit status 1 and an empty stdout on an argument error.
//
//   >/abs/path/file.fastq
//   read,length,motif,strand,start,end,covered
//   ... one row per kept interval (end - start >= MIN_LEN; default 4 k of that motif, gaps of at most 3 k), sorted by read
//       ordinal, motif in command-line order, strand (+ before -), start
//   >Summary
//   motif,reads,reads_with_interval,bases,intervals_fwd,intervals_rev,longest_fwd,longest_rev,terminal_fwd,terminal_rev
//       (one row per motif, over all files; terminal_s: kept intervals with start == 0 or end == length)
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sys/stat.h>

#include "trew_host.hpp"

namespace trew_host {

static void intervals_usage() {
    fprintf(stderr,
            "Usage: intervals [--help] [--thread THREAD] [--max_gap BASES] [--min_len BASES] [--devices LIST] [--stats] MOTIF[,MOTIF...] FASTQ...\n\n"
            "Report where in every read the given repeat motifs (3 to 32 bases each, at most 8) lie: the intervals of bases inside\n"
            "matching windows whose gaps are at most MAX_GAP bases (default 3 k) and that span at least MIN_LEN bases (default 4 k).\n");
}

// a number in [0, 2^32)
static bool intervals_u32(const char *s, uint32_t *out) {
    char *end = nullptr;
    if (!s[0] || s[0] == '-' || s[0] == '+') return false;
    const unsigned long long v = strtoull(s, &end, 10);
    if (*end || v > 0xffffffffull || strlen(s) > 10) return false;
    *out = (uint32_t) v;
    return true;
}

static bool intervals_int(const char *s, int *out) {
    char *end = nullptr;
    const long v = strtol(s, &end, 10);
    if (!s[0] || *end || v < INT_MIN || v > INT_MAX) return false;
    *out = (int) v;
    return true;
}

int intervals_main(int argc, char **argv) {
    Config cfg;
    uint32_t max_gap = 0, min_len = 0;  // not given: 3 k and 4 k of each motif
    bool max_gap_given = false, min_len_given = false;
    std::vector<std::string> positional;
    auto bad = [&](const std::string &msg) {
        fprintf(stderr, "%s\n", msg.c_str());
        intervals_usage();
        return 1;
    };
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        auto need = [&](const char *name) -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "%s: expected 1 argument(s). 0 provided.\n", name);
                intervals_usage();
                exit(1);
            }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") {
            intervals_usage();
            return 0;
        } else if (a == "-t" || a == "--thread") {
            if (!intervals_int(need("--thread"), &cfg.NUM_THREAD)) return bad("THREAD must be a number.");
        } else if (a == "--max_gap") {
            if (!intervals_u32(need("--max_gap"), &max_gap)) return bad("MAX_GAP must be a number in range 0 to 4294967295.");
            max_gap_given = true;
        } else if (a == "--min_len") {
            if (!intervals_u32(need("--min_len"), &min_len)) return bad("MIN_LEN must be a number in range 1 to 4294967295.");
            min_len_given = true;
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
                if (!intervals_int(list.substr(pos, comma - pos).c_str(), &d) || d < 0) ok = false;
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
    if (min_len_given && min_len < 1) return bad("MIN_LEN must be a number in range 1 to 4294967295.");

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
    rq.intervals = true;
    for (const auto &name : names) {
        for (char ch : name)
            if (!strchr("ACGTacgt", ch) || !ch) return bad("MOTIF '" + name + "' must consist of A, C, G and T.");
        if (name.size() < 3 || name.size() > 32) return bad("MOTIF '" + name + "': the length must be in range 3 to 32.");
        if (trew_motif_parse(name.c_str(), &rq.motifs[rq.n_motifs])) return bad(trew_hip_last_error(nullptr));
        rq.min_tract[rq.n_motifs] = 0;  // not read: min_len is part of the rule
        rq.rules[rq.n_motifs].max_gap = max_gap_given ? max_gap : 3u * (uint32_t) name.size();
        rq.rules[rq.n_motifs].min_len = min_len_given ? min_len : 4u * (uint32_t) name.size();
        rq.n_motifs++;
    }
    if (positional.size() < 2) return bad("FASTQ is required.");
    std::vector<std::string> files(positional.begin() + 1, positional.end());
    for (const auto &f : files) {
        struct stat st;
        if (stat(f.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
            fprintf(stderr, "%s : file not found\n", f.c_str());
            intervals_usage();
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
        printf("read,length,motif,strand,start,end,covered\n");
        for (const auto &row : r.irows)
            printf("%llu,%u,%s,%c,%u,%u,%u\n", (unsigned long long) row.read, row.length, names[(size_t) row.iv.motif].c_str(), row.iv.strand ? '-' : '+',
                   row.iv.start, row.iv.end, row.iv.covered);
        total.reads += r.reads;
        total.bases += r.bases;
        for (int m = 0; m < rq.n_motifs; m++) {
            total.windows_fwd[m] += r.windows_fwd[m];
            total.windows_rev[m] += r.windows_rev[m];
            total.reported[m] += r.reported[m];
            total.longest[m] = std::max(total.longest[m], r.longest[m]);
            total.longest_tail[m] = std::max(total.longest_tail[m], r.longest_tail[m]);
            total.terminal_fwd[m] += r.terminal_fwd[m];
            total.terminal_rev[m] += r.terminal_rev[m];
        }
    }
    annotator_destroy(an);
    printf(">Summary\nmotif,reads,reads_with_interval,bases,intervals_fwd,intervals_rev,longest_fwd,longest_rev,terminal_fwd,terminal_rev\n");
    for (int m = 0; m < rq.n_motifs; m++)
        printf("%s,%llu,%llu,%llu,%llu,%llu,%u,%u,%llu,%llu\n", names[(size_t) m].c_str(), (unsigned long long) total.reads, (unsigned long long) total.reported[m],
               (unsigned long long) total.bases, (unsigned long long) total.windows_fwd[m], (unsigned long long) total.windows_rev[m], total.longest[m],
               total.longest_tail[m], (unsigned long long) total.terminal_fwd[m], (unsigned long long) total.terminal_rev[m]);
    return 0;
}

}  // namespace trew_host
