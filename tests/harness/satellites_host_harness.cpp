// satellites_host_harness.cpp -- runs the CPU definition of the de novo repeats with periods up to 256 (satellites_host of
// trew_measures_host.cpp) on its own, so that it can be built with sanitizers: no HIP, no library.
//
//   satellites_host_harness MIN_PERIOD MAX_PERIOD PENALTY MIN_SCORE [CAP]  < reads (one per line; an empty line is a read of no bases)
//
// Prints the number of tracts found, then the count of every read on one line, then every record that fitted as text, one line
// per tract in the order of the fields of trew_hip_satellite, the sixteen unit words last (tests/test_satellites_cpu.py compares it with what trew_amd.capi
// returns through libtrew_hip.so).  Without CAP the buffer holds every tract.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/trew_measures_host.hpp"

int main(int argc, char **argv) {
    if (argc != 5 && argc != 6) return fprintf(stderr, "usage: satellites_host_harness MIN_PERIOD MAX_PERIOD PENALTY MIN_SCORE [CAP]\n"), 2;
    // the packed layout of trew_hip.h, base by base: three words {lo, hi, nmask} per 32 bases, T=0 G=1 C=2 A=3
    std::vector<uint32_t> words, offsets, lengths;
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
    const int lo = atoi(argv[1]), hi = atoi(argv[2]), penalty = atoi(argv[3]);
    const uint32_t min_score = (uint32_t) atoi(argv[4]);
    std::vector<uint32_t> counts(n);
    uint64_t found = 0;
    // first without a buffer: the number alone
    if (const char *e = trew::satellites_host(words.data(), offsets.data(), lengths.data(), n, lo, hi, penalty, min_score, nullptr, 0, &found, counts.data()))
        return fprintf(stderr, "%s\n", e), 3;
    const uint64_t cap = argc == 6 ? (uint64_t) atoll(argv[5]) : found;
    std::vector<trew_hip_satellite> out(cap);  // exactly cap records: a write past them is the sanitizer's to find
    uint64_t again = 0;
    if (const char *e = trew::satellites_host(words.data(), offsets.data(), lengths.data(), n, lo, hi, penalty, min_score, cap ? out.data() : nullptr, cap, &again,
                                           counts.data()))
        return fprintf(stderr, "%s\n", e), 3;
    if (again != found) return fprintf(stderr, "the two calls disagree: %llu and %llu tracts\n", (unsigned long long) found, (unsigned long long) again), 4;
    printf("%llu\n", (unsigned long long) found);
    for (uint64_t r = 0; r < n; r++) printf(r + 1 < n ? "%u " : "%u", counts[r]);
    printf("\n");
    for (uint64_t i = 0; i < cap && i < found; i++) {
        const trew_hip_satellite &x = out[i];
        printf("%u %u %u %u %u %u %u %u %u %u", x.read, x.depth, x.period, x.scored_period, x.score, x.start, x.end, x.matches, x.support, x.reserved);
        for (int j = 0; j < 16; j++) printf(" %u", x.unit[j]);
        printf("\n");
    }
    return 0;
}
