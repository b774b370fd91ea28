// copies_host_harness.cpp -- runs the CPU definition of the traceback for units of up to 256 bases (copies_host of
// trew_measures_host.cpp) on its own, so that it can be built with sanitizers: no HIP, no library.
//
//   copies_host_harness PENALTY MIN_SCORE CAP MONOMER[,MONOMER...]  < reads (one per line; an empty line is a read of no bases)
//
// Prints n_items and n_rows, then min(CAP, n_items) items, the counts on one line and every alignment record, as text
// (tests/test_copies_cpu.py compares it with what trew_amd.capi returns through libtrew_hip.so).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/trew_measures_host.hpp"

int main(int argc, char **argv) {
    if (argc != 5) return fprintf(stderr, "usage: copies_host_harness PENALTY MIN_SCORE CAP MONOMER[,MONOMER...]\n"), 2;
    std::vector<trew_hip_monomer> monomers;
    const std::string list = argv[4];
    for (size_t pos = 0; pos <= list.size();) {
        size_t comma = list.find(',', pos);
        if (comma == std::string::npos) comma = list.size();
        trew_hip_monomer m;
        const std::string e = trew::monomer_parse(list.substr(pos, comma - pos).c_str(), &m);
        if (!e.empty()) return fprintf(stderr, "%s\n", e.c_str()), 3;
        monomers.push_back(m);
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
    const uint64_t n = offsets.size(), cap = strtoull(argv[3], nullptr, 10);
    const size_t nm = monomers.size();
    std::vector<trew_hip_trace_item> items(cap);  // exactly cap: a write beyond it is the sanitizer's to find
    std::vector<uint32_t> counts(n * nm * 2 + 1);
    std::vector<trew_hip_alignment> a(n * nm);
    uint64_t found = 0, rows = 0;
    if (const char *e = trew::copies_host(words.data(), offsets.data(), lengths.data(), n, monomers.data(), (int) nm, atoi(argv[1]),
                                          (uint32_t) strtoul(argv[2], nullptr, 10), items.data(), cap, &found, &rows, counts.data(), a.data()))
        return fprintf(stderr, "%s\n", e), 3;
    printf("%llu %llu\n", (unsigned long long) found, (unsigned long long) rows);
    for (uint64_t i = 0; i < found && i < cap; i++) {
        const trew_hip_trace_item &it = items[i];
        printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", it.read, it.motif, it.strand, it.start, it.bases, it.count, it.phase, it.consumed, it.mismatches,
               it.insertions, it.deletions, it.reserved);
    }
    for (uint64_t i = 0; i < n * nm * 2; i++) printf("%u ", counts[i]);
    printf("\n");
    for (const auto &x : a)
        printf("%u %u %u %u %u %u %u %u %u %u\n", x.score_fwd, x.start_fwd, x.end_fwd, x.consumed_fwd, x.matches_fwd, x.score_rev, x.start_rev, x.end_rev,
               x.consumed_rev, x.matches_rev);
    return 0;
}
