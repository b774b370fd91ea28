// motif_cli.cpp -- what the command lines share: the argument helpers of every subcommand, and the front end of the six
// per-read motif subcommands `trew annotate|tracts|intervals|variants|chain|align|trace MOTIF[,MOTIF...] FASTQ...` and of the motif-less
// `trew periods|repeats|satellites|refine|tandems|decompose|dissect|resolve|polish FASTQ...` (motif_cli_main), and of
// `trew monomers [--fasta FILE] [MONOMER[,MONOMER...]] FASTQ...`, whose units have up to 256 bases and may come from a FASTA file.  A
// subcommand's own file (annotate.cpp, ...) holds its usage text, its options and their defaults, its rows and its summary.
// The conventions are those of `short` and `long`: CSV on stdout, messages on stderr, exit status 1 and an empty stdout on an
// argument error.
#include <climits>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sys/stat.h>

#include "trew_host.hpp"

namespace trew_host {

bool is_regular_file(const std::string &p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

bool parse_int(const char *s, int *out) {
    char *end = nullptr;
    long v = strtol(s, &end, 10);
    if (!s[0] || *end || v < INT_MIN || v > INT_MAX) return false;
    *out = (int) v;
    return true;
}

bool parse_devices(const std::string &list, std::vector<int> *devices) {
    devices->clear();
    bool ok = true;
    size_t pos = 0;
    while (pos <= list.size()) {
        size_t comma = list.find(',', pos);
        if (comma == std::string::npos) comma = list.size();
        int d;
        if (!parse_int(list.substr(pos, comma - pos).c_str(), &d) || d < 0) ok = false;
        else devices->push_back(d);
        pos = comma + 1;
    }
    return ok && !devices->empty();
}

bool has_gz_ext(const std::string &p) {  // trew.cpp:407,422-433
    const size_t dot = p.find_last_of('.');
    const size_t slash = p.find_last_of('/');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return false;
    const std::string ext = p.substr(dot);
    return ext == ".gz" || ext == ".bgz";
}

std::string canonical(const std::string &p) {  // std::filesystem::canonical, trew.cpp:439-451
    char buf[PATH_MAX];
    if (realpath(p.c_str(), buf)) return std::string(buf);
    return p;
}

void period_options(MotifCli &cli, PeriodOptions &o, int bound) {
    static_assert(TREW_SATELLITE_MAX_PERIOD == 256, "the text below");
    o.max_period = bound;
    cli.motif_less = true;
    cli.options = {{"--min_period", [&o](const char *s) { return parse_int(s, &o.min_period); }, "MIN_PERIOD must be a number."},
                   {"--max_period", [&o](const char *s) { return parse_int(s, &o.max_period); }, "MAX_PERIOD must be a number."},
                   {"--penalty", [&o](const char *s) { return parse_int(s, &o.penalty); }, "PENALTY must be a number."},
                   {"--min_score", [&o](const char *s) { return parse_int(s, &o.min_score); }, "MIN_SCORE must be a number."}};
    cli.check = [&o, bound]() -> const char * {
        if (o.min_period < 1 || o.max_period > bound)
            return bound == 32 ? "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32." : "MIN_PERIOD and MAX_PERIOD must be in range 1 to 256.";
        if (o.min_period > o.max_period) return "MIN_PERIOD must not be greater than MAX_PERIOD.";
        if (o.penalty < 1 || o.penalty > 64) return "PENALTY must be in range 1 to 64.";
        return o.min_score < 1 ? "MIN_SCORE must be greater than or equal to 1." : nullptr;
    };
    cli.per_motif = [](AnnotRequest &, int, uint32_t) {};
    cli.fill = [&o](AnnotRequest &rq) {
        rq.min_period = o.min_period;
        rq.max_period = o.max_period;
        rq.penalty = o.penalty;
        rq.min_score = (uint32_t) o.min_score;
    };
}

void candidates_option(MotifCli &cli, int &candidates) {
    static_assert(TREW_RESOLVE_MAX_CANDIDATES == 4, "the text below");
    cli.options.push_back({"--candidates", [&candidates](const char *s) { return parse_int(s, &candidates); }, "CANDIDATES must be a number."});
    const auto period_check = cli.check;
    cli.check = [&candidates, period_check]() -> const char * {
        if (const char *e = period_check()) return e;
        return candidates < 1 || candidates > TREW_RESOLVE_MAX_CANDIDATES ? "CANDIDATES must be in range 1 to 4." : nullptr;
    };
    const auto period_fill = cli.fill;
    cli.fill = [&candidates, period_fill](AnnotRequest &rq) {
        period_fill(rq);
        rq.candidates = candidates;
    };
}

// The records of a FASTA file: the name is the header's first word, the sequence may span lines.  "" or the complaint.
static std::string read_fasta(const std::string &path, std::vector<std::string> *names, std::vector<std::string> *units) {
    std::ifstream in(path);
    if (!is_regular_file(path) || !in) return path + " : file not found";
    std::string line;
    while (std::getline(in, line)) {
        while (!line.empty() && strchr(" \t\r", line.back())) line.pop_back();
        if (line.empty()) continue;
        if (line[0] == '>') {
            const size_t end = line.find_first_of(" \t", 1);
            names->push_back(line.substr(1, end == std::string::npos ? std::string::npos : end - 1));
            if (names->back().empty()) names->back() = "monomer" + std::to_string(names->size());
            units->push_back("");
        } else {
            if (units->empty()) return path + " : sequence in front of the first header";
            units->back() += line;
        }
    }
    return names->empty() ? path + " : no FASTA records" : "";
}

int motif_cli_main(int argc, char **argv, Measure kind, const MotifCli &cli) {
    Config cfg;
    std::vector<std::string> positional;
    auto bad = [&](const std::string &msg) {
        fprintf(stderr, "%s\n", msg.c_str());
        cli.usage();
        return 1;
    };
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        auto need = [&](const char *name) -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "%s: expected 1 argument(s). 0 provided.\n", name);
                cli.usage();
                exit(1);
            }
            return argv[++i];
        };
        const MotifOption *own = nullptr;
        for (const auto &o : cli.options)
            if (a == o.name) own = &o;
        const MotifFlag *flag = nullptr;
        for (const auto &o : cli.flags)
            if (a == o.name) flag = &o;
        if (a == "-h" || a == "--help") {
            cli.usage();
            return 0;
        } else if (a == "-t" || a == "--thread") {
            if (!parse_int(need("--thread"), &cfg.NUM_THREAD)) return bad("THREAD must be a number.");
        } else if (own) {
            if (!own->parse(need(own->name))) return bad(own->error);
        } else if (flag) {
            flag->set();
        } else if (a == "--stats") {
            cfg.stats = true;
        } else if (a == "--devices") {
            if (!parse_devices(need("--devices"), &cfg.devices)) return bad("DEVICES must be a comma-separated list of device ordinals.");
        } else if (a.size() > 1 && a[0] == '-') {
            return bad("Unknown argument: " + a);
        } else {
            positional.push_back(a);
        }
    }
    const char *fasta = cli.long_units && cli.fasta ? cli.fasta() : nullptr;
    if (positional.empty()) return bad(cli.motif_less || fasta ? "FASTQ is required." : cli.long_units ? "MONOMER or --fasta FILE is required." : "MOTIF is required.");
    if (cfg.NUM_THREAD <= 0) return bad("number of threads must be positive.");
    if (const char *e = cli.check()) return bad(e);

    // MOTIF[,MOTIF...], printed as given
    std::vector<std::string> names, units;  // units: the bases of a monomer (long_units), typed or from the FASTA file
    size_t first_file = cli.motif_less ? 0 : 1;
    if (cli.long_units && fasta) {  // every positional argument is a file
        const std::string &p0 = positional[0];
        if (!is_regular_file(p0) && p0.find_first_not_of("ACGTacgt,") == std::string::npos)
            return bad("MONOMER and --fasta cannot both be given.");
        const std::string e = read_fasta(fasta, &names, &units);
        if (!e.empty()) return bad(e);
        first_file = 0;
    } else if (cli.long_units && is_regular_file(positional[0])) {
        return bad("MONOMER or --fasta FILE is required.");
    } else if (!cli.motif_less) {
        const std::string &list = positional[0];
        size_t pos = 0;
        while (pos <= list.size()) {
            size_t comma = list.find(',', pos);
            if (comma == std::string::npos) comma = list.size();
            names.push_back(list.substr(pos, comma - pos));
            pos = comma + 1;
        }
    }
    static_assert(TREW_MONOMERS_MAX == TREW_ANNOT_MAX_MOTIFS && TREW_MONOMER_MAX == 256, "the texts below, and the request's n_motifs");
    if (names.size() > TREW_ANNOT_MAX_MOTIFS) return bad(cli.long_units ? "At most 8 monomers can be given." : "At most 8 motifs can be given.");
    AnnotRequest rq;
    rq.kind = kind;
    if (cli.long_units && units.empty()) units = names;
    for (size_t m = 0; m < units.size(); m++) {
        const std::string &unit = units[m], shown = fasta ? names[m] : unit.size() <= 40 ? unit : unit.substr(0, 37) + "...";
        for (char ch : unit)
            if (!strchr("ACGTacgt", ch) || !ch) return bad("MONOMER '" + shown + "' must consist of A, C, G and T.");
        if (unit.size() < 3 || unit.size() > TREW_MONOMER_MAX) return bad("MONOMER '" + shown + "': the length must be in range 3 to 256.");
        if (trew_monomer_parse(unit.c_str(), &rq.monomers[rq.n_motifs])) return bad(trew_hip_last_error(nullptr));
        cli.per_motif(rq, rq.n_motifs, (uint32_t) unit.size());
        rq.n_motifs++;
    }
    for (const auto &name : cli.long_units ? std::vector<std::string>() : names) {
        for (char ch : name)
            if (!strchr("ACGTacgt", ch) || !ch) return bad("MOTIF '" + name + "' must consist of A, C, G and T.");
        if (name.size() < 3 || name.size() > 32) return bad("MOTIF '" + name + "': the length must be in range 3 to 32.");
        if (trew_motif_parse(name.c_str(), &rq.motifs[rq.n_motifs])) return bad(trew_hip_last_error(nullptr));
        cli.per_motif(rq, rq.n_motifs, (uint32_t) name.size());
        rq.n_motifs++;
    }
    if (cli.motif_less) cli.fill(rq);
    if (positional.size() < first_file + 1) return bad("FASTQ is required.");
    std::vector<std::string> files(positional.begin() + (long) first_file, positional.end());
    for (const auto &f : files)
        if (!is_regular_file(f)) return bad(f + " : file not found");
    if (cfg.NUM_THREAD - 1 > 16 * (int) cfg.devices.size()) cfg.NUM_THREAD = 16 * (int) cfg.devices.size() + 1;

    Annotator *an = annotator_create(cfg);
    AnnotFileResult total;
    for (const auto &f : files) {
        const std::string path = canonical(f);
        const AnnotFileResult r = process_annotate(an, cfg, path.c_str(), has_gz_ext(f), rq);
        printf(">%s\n", path.c_str());
        cli.print_rows(r, names);
        add_totals(total, r);
    }
    annotator_destroy(an);
    cli.print_summary(total, names);
    return 0;
}

}  // namespace trew_host
