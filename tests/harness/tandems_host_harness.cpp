// tandems_host_harness.cpp -- runs the CPU definition of the de novo repeats under indels, every tract of a read (tandems_host of
// trew_measures_host.cpp) on its own, so that it can be built with sanitizers: no HIP, no library.
//
//   tandems_host_harness MIN_PERIOD MAX_PERIOD PENALTY MIN_SCORE  < reads (one per line; an empty line is a read of no bases)
//
// Prints "n FOUND", then the counts of the reads on one line, then every record as text, one line per tract in the order of the
// fields of trew_hip_tandem (tests/test_tandems_cpu.py compares it with what trew_amd.capi returns through libtrew_hip.so).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/trew_measures_host.hpp"

int main(int argc, char **argv) {
    if (argc != 5) return fprintf(stderr, "usage: tandems_host_harness MIN_PERIOD MAX_PERIOD PENALTY MIN_SCORE\n"), 2;
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
    const int a1 = atoi(argv[1]), a2 = atoi(argv[2]), a3 = atoi(argv[3]);
    const uint32_t a4 = (uint32_t) atoi(argv[4]);
    // the protocol of the interface: count first, then fetch exactly that many
    uint64_t found = 0, again = 0;
    std::vector<uint32_t> counts(n);
    if (const char *e = trew::tandems_host(words.data(), offsets.data(), lengths.data(), n, a1, a2, a3, a4, nullptr, 0, &found, counts.data()))
        return fprintf(stderr, "%s\n", e), 3;
    std::vector<trew_hip_tandem> a(found);
    if (const char *e = trew::tandems_host(words.data(), offsets.data(), lengths.data(), n, a1, a2, a3, a4, a.data(), found, &again, nullptr))
        return fprintf(stderr, "%s\n", e), 3;
    if (again != found) return fprintf(stderr, "the second call found %llu, the first %llu\n", (unsigned long long) again, (unsigned long long) found), 4;
    printf("n %llu\n", (unsigned long long) found);
    for (uint64_t r = 0; r < n; r++) printf(r + 1 < n ? "%u " : "%u", counts[r]);
    printf("\n");
    for (const auto &x : a)
        printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %llu %llu\n", x.read, x.depth, x.period, x.seed_period, x.scored_period, x.changed, x.score, x.start,
               x.end, x.consumed, x.matches, x.seed_score, x.support, x.reserved, (unsigned long long) x.unit, (unsigned long long) x.seed_unit);
    return 0;
}
