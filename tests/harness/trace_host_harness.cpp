// trace_host_harness.cpp -- runs the CPU definition of the traceback of the wraparound alignment (trace_host of
// trew_measures_host.cpp) on its own, so that it can be built with sanitizers: no HIP, no library.
//
//   trace_host_harness PENALTY MIN_SCORE CAP MOTIF[,MOTIF...]  < reads (one per line; an empty line is a read of no bases)
//
// Prints the number of items, then every copied item (at most CAP) as text, one line each in the order of the fields of
// trew_hip_trace_item, then the counts on one line, then every alignment record, one line per (read, motif)
// (tests/test_trace_cpu.py compares it with what trew_amd.capi returns through libtrew_hip.so).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/trew_measures_host.hpp"

int main(int argc, char **argv) {
    if (argc != 5) return fprintf(stderr, "usage: trace_host_harness PENALTY MIN_SCORE CAP MOTIF[,MOTIF...]\n"), 2;
    std::vector<trew_hip_motif> motifs;
    const std::string list = argv[4];
    for (size_t pos = 0; pos <= list.size();) {
        size_t comma = list.find(',', pos);
        if (comma == std::string::npos) comma = list.size();
        trew_hip_motif m;
        const std::string e = trew::motif_parse(list.substr(pos, comma - pos).c_str(), &m);
        if (!e.empty()) return fprintf(stderr, "%s\n", e.c_str()), 3;
        motifs.push_back(m);
        pos = comma + 1;
    }
    // the packed layout of trew_hip.h, base by base: three words {lo, hi, nmask} per 32 bases, T=0 G=1 C=2 A=3
    std::vector<uint32_t> words, offsets, lengths;
    words.reserve(64);  // reads of no bases only: still a buffer
    for (std::string line; std::getline(std::cin, line);) {
        offsets.push_back((uint32_t) words.size());
        lengths.push_back((uint32_t) line.size());
        words.resize(words.size() + 3 * ((line.size() + 31) / 32), 0);
        for (size_t i = 0; i < line.size(); i++) {
            uint32_t *w = &words[offsets.back() + 3 * (i / 32)];
            const std::string::size_type c = std::string("TGCA").find(line[i]);
            if (c == std::string::npos) w[2] |= 1u << (i % 32);
            else w[0] |= (uint32_t) (c & 1) << (i % 32), w[1] |= (uint32_t) (c >> 1) << (i % 32);
        }
    }
    const uint64_t n = offsets.size();
    const uint64_t cap = strtoull(argv[3], nullptr, 10);
    std::vector<trew_hip_trace_item> items(cap);  // exactly CAP: a write beyond it is the sanitizer's to find
    std::vector<trew_hip_alignment> a(n * motifs.size());
    std::vector<uint32_t> counts(n * motifs.size() * 2);
    uint64_t found = 0;
    if (const char *e = trew::trace_host(words.data(), offsets.data(), lengths.data(), n, motifs.data(), (int) motifs.size(), atoi(argv[1]),
                                         (uint32_t) strtoul(argv[2], nullptr, 10), cap ? items.data() : nullptr, cap, &found, counts.data(), a.data()))
        return fprintf(stderr, "%s\n", e), 3;
    printf("%llu\n", (unsigned long long) found);
    for (uint64_t i = 0; i < found && i < cap; i++) {
        const trew_hip_trace_item &x = items[i];
        printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", x.read, x.motif, x.strand, x.start, x.bases, x.count, x.phase, x.consumed, x.mismatches, x.insertions,
               x.deletions, x.reserved);
    }
    for (uint32_t c : counts) printf("%u ", c);
    printf("\n");
    for (const auto &x : a)
        printf("%u %u %u %u %u %u %u %u %u %u\n", x.score_fwd, x.start_fwd, x.end_fwd, x.consumed_fwd, x.matches_fwd, x.score_rev, x.start_rev, x.end_rev,
               x.consumed_rev, x.matches_rev);
    return 0;
}
