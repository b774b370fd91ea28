// resolved_host_harness.cpp -- runs the CPU definitions of tandems, decompose and dissect with resolve's period choice per piece
// (tandems_resolved_host, decompose_resolved_host and dissect_resolved_host of trew_measures_host.cpp) on their own, so that
// they can be built with sanitizers: no HIP, no library.
//
//   resolved_host_harness MEASURE MIN_PERIOD MAX_PERIOD PENALTY MIN_SCORE CANDIDATES REC_CAP ITEM_CAP  < reads
//   (MEASURE: tandems, decompose or dissect; one read per line, an empty line is a read of no bases; tandems reads no ITEM_CAP,
//   decompose no REC_CAP: it has a record per read)
//
// Prints the numbers of records, items and rows on one line (tandems: records; decompose: items), then every copied record in
// the order of the fields of trew_hip_tandem (decompose: of trew_hip_refined, one per read), then every copied item in the order
// of the fields of trew_hip_trace_item, one line each, then the counts on one line (tests/test_resolved_cpu.py compares it with
// what trew_amd.capi returns through libtrew_hip.so).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/trew_measures_host.hpp"

static void print_tandem(const trew_hip_tandem &x) {
    printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %llu %llu\n", x.read, x.depth, x.period, x.seed_period, x.scored_period, x.changed, x.score, x.start,
           x.end, x.consumed, x.matches, x.seed_score, x.support, x.reserved, (unsigned long long) x.unit, (unsigned long long) x.seed_unit);
}

static void print_item(const trew_hip_trace_item &x) {
    printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", x.read, x.motif, x.strand, x.start, x.bases, x.count, x.phase, x.consumed, x.mismatches, x.insertions,
           x.deletions, x.reserved);
}

int main(int argc, char **argv) {
    if (argc != 9) return fprintf(stderr, "usage: resolved_host_harness MEASURE MIN_PERIOD MAX_PERIOD PENALTY MIN_SCORE CANDIDATES REC_CAP ITEM_CAP\n"), 2;
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
    const std::string measure = argv[1];
    const uint64_t n = offsets.size();
    const int min_period = atoi(argv[2]), max_period = atoi(argv[3]), penalty = atoi(argv[4]), candidates = atoi(argv[6]);
    const uint32_t min_score = (uint32_t) strtoul(argv[5], nullptr, 10);
    const uint64_t rec_cap = strtoull(argv[7], nullptr, 10), item_cap = strtoull(argv[8], nullptr, 10);
    std::vector<trew_hip_tandem> recs(rec_cap);  // exactly the capacities: a write beyond one is the sanitizer's to find
    std::vector<trew_hip_trace_item> items(item_cap);
    uint64_t n_recs = 0, n_items = 0, n_rows = 0;
    if (measure == "tandems") {
        std::vector<uint32_t> counts(n);
        if (const char *e = trew::tandems_resolved_host(words.data(), offsets.data(), lengths.data(), n, min_period, max_period, penalty, min_score, candidates,
                                                        rec_cap ? recs.data() : nullptr, rec_cap, &n_recs, counts.data()))
            return fprintf(stderr, "%s\n", e), 3;
        printf("%llu\n", (unsigned long long) n_recs);
        for (uint64_t i = 0; i < n_recs && i < rec_cap; i++) print_tandem(recs[i]);
        for (uint32_t c : counts) printf("%u ", c);
    } else if (measure == "decompose") {
        std::vector<uint32_t> counts(n);
        std::vector<trew_hip_refined> refined(n);
        if (const char *e = trew::decompose_resolved_host(words.data(), offsets.data(), lengths.data(), n, min_period, max_period, penalty, min_score, candidates,
                                                          item_cap ? items.data() : nullptr, item_cap, &n_items, counts.data(), refined.data()))
            return fprintf(stderr, "%s\n", e), 3;
        printf("%llu\n", (unsigned long long) n_items);
        for (const trew_hip_refined &x : refined)
            printf("%u %u %u %u %u %u %u %u %u %u %u %u %llu %llu\n", x.period, x.seed_period, x.scored_period, x.changed, x.score, x.start, x.end, x.consumed,
                   x.matches, x.seed_score, x.support, x.reserved, (unsigned long long) x.unit, (unsigned long long) x.seed_unit);
        for (uint64_t i = 0; i < n_items && i < item_cap; i++) print_item(items[i]);
        for (uint32_t c : counts) printf("%u ", c);
    } else if (measure == "dissect") {
        std::vector<uint32_t> counts(2 * n);
        if (const char *e = trew::dissect_resolved_host(words.data(), offsets.data(), lengths.data(), n, min_period, max_period, penalty, min_score, candidates,
                                                        rec_cap ? recs.data() : nullptr, rec_cap, item_cap ? items.data() : nullptr, item_cap, &n_recs,
                                                        &n_items, &n_rows, counts.data()))
            return fprintf(stderr, "%s\n", e), 3;
        printf("%llu %llu %llu\n", (unsigned long long) n_recs, (unsigned long long) n_items, (unsigned long long) n_rows);
        for (uint64_t i = 0; i < n_recs && i < rec_cap; i++) print_tandem(recs[i]);
        for (uint64_t i = 0; i < n_items && i < item_cap; i++) print_item(items[i]);
        for (uint32_t c : counts) printf("%u ", c);
    } else {
        return fprintf(stderr, "MEASURE must be tandems, decompose or dissect\n"), 2;
    }
    printf("\n");
    return 0;
}
