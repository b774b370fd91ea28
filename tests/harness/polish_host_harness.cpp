// polish_host_harness.cpp -- runs the CPU definition of the refined de novo repeat per read for periods up to 256
// (polish_host of trew_measures_host.cpp) on its own, so that it can be built with sanitizers: no HIP, no library.
//
//   polish_host_harness MIN_PERIOD MAX_PERIOD PENALTY MIN_SCORE  < reads (one per line; an empty line is a read of no bases)
//
// Prints every record as text, one line per read: the twelve words of trew_hip_polished, then the sixteen words of unit and
// the sixteen of seed_unit (tests/test_polish_cpu.py compares it with what trew_amd.capi returns through libtrew_hip.so).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/trew_measures_host.hpp"

int main(int argc, char **argv) {
    if (argc != 5) return fprintf(stderr, "usage: polish_host_harness MIN_PERIOD MAX_PERIOD PENALTY MIN_SCORE\n"), 2;
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
    std::vector<trew_hip_polished> a(n);
    if (const char *e = trew::polish_host(words.data(), offsets.data(), lengths.data(), n, atoi(argv[1]), atoi(argv[2]), atoi(argv[3]),
                                          (uint32_t) atoi(argv[4]), a.data()))
        return fprintf(stderr, "%s\n", e), 3;
    for (const auto &x : a) {
        printf("%u %u %u %u %u %u %u %u %u %u %u %u", x.period, x.seed_period, x.scored_period, x.changed, x.score, x.start, x.end, x.consumed, x.matches,
               x.seed_score, x.support, x.reserved);
        for (uint32_t w : x.unit) printf(" %u", w);
        for (uint32_t w : x.seed_unit) printf(" %u", w);
        printf("\n");
    }
    return 0;
}
