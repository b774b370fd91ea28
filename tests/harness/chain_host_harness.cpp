// chain_host_harness.cpp -- runs the CPU definition of the ordered unit chain (chain_host of trew_measures_host.cpp) on its
// own, so that it can be built with sanitizers: no HIP, no library.
//
//   chain_host_harness MOTIF[,MOTIF...] [CAP]  < reads (one per line; an empty line is a read of no bases)
//
// Prints "items N", then every item as text, one line per item in the order of the fields of trew_hip_chain_item, then one
// line "counts" with the [read][motif][strand]{runs, variants} values (tests/test_chain_cpu.py compares it with what
// trew_amd.capi returns through libtrew_hip.so).  With CAP the item buffer holds only that many.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/trew_measures_host.hpp"

int main(int argc, char **argv) {
    if (argc != 2 && argc != 3) return fprintf(stderr, "usage: chain_host_harness MOTIF[,MOTIF...] [CAP]\n"), 2;
    std::vector<trew_hip_motif> motifs;
    const std::string list = argv[1];
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
    std::vector<uint32_t> counts(n * motifs.size() * 4);
    uint64_t found = 0;
    // first the number alone (no buffer), then into a buffer of exactly that size, or of CAP
    if (const char *e = trew::chain_host(words.data(), offsets.data(), lengths.data(), n, motifs.data(), (int) motifs.size(), nullptr, 0, &found, counts.data()))
        return fprintf(stderr, "%s\n", e), 3;
    std::vector<trew_hip_chain_item> items(argc == 3 ? (size_t) atoll(argv[2]) : (size_t) found);
    if (const char *e = trew::chain_host(words.data(), offsets.data(), lengths.data(), n, motifs.data(), (int) motifs.size(), items.data(), items.size(), &found,
                                         counts.data()))
        return fprintf(stderr, "%s\n", e), 3;
    printf("items %llu\n", (unsigned long long) found);
    for (size_t i = 0; i < items.size() && i < found; i++)
        printf("%u %u %u %u %u %u\n", items[i].read, items[i].motif, items[i].strand, items[i].start, items[i].count, items[i].bin);
    printf("counts");
    for (uint32_t c : counts) printf(" %u", c);
    printf("\n");
    return 0;
}
