// measures_host_harness.cpp -- runs the CPU definitions of the four per-read motif measures (trew_measures_host.cpp) on
// their own, so that they can be built with sanitizers: no HIP, no library.
//
//   measures_host_harness MOTIF...  < reads (one per line; an empty line is a read of no bases)
//
// Prints every record as text (tests/test_measures_host_cpu.py compares it with what trew_amd.capi returns through
// libtrew_hip.so).  Tracts use penalty 3, intervals the rules 3 k / 4 k; intervals run twice, with no room and with the
// exact count.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/trew_measures_host.hpp"

int main(int argc, char **argv) {
    std::vector<trew_hip_motif> motifs((size_t) argc - 1);
    std::vector<trew_hip_interval_rule> rules(motifs.size());
    for (size_t m = 0; m < motifs.size(); m++) {
        const std::string e = trew::motif_parse(argv[m + 1], &motifs[m]);
        if (!e.empty()) return fprintf(stderr, "%s\n", e.c_str()), 2;
        rules[m] = trew_hip_interval_rule{3u * (uint32_t) motifs[m].k, 4u * (uint32_t) motifs[m].k};
    }
    const int nm = (int) motifs.size();
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
    auto check = [](const char *e) {
        if (e) fprintf(stderr, "%s\n", e), exit(3);
    };

    std::vector<trew_hip_annot> a(n * (size_t) nm);
    check(trew::annotate_host(words.data(), offsets.data(), lengths.data(), n, motifs.data(), nm, a.data()));
    printf("annotate\n");
    for (const auto &x : a) printf("%u %u %u %u %u %u\n", x.windows_fwd, x.windows_rev, x.tract_start_fwd, x.tract_len_fwd, x.tract_start_rev, x.tract_len_rev);

    std::vector<trew_hip_tract> t(n * (size_t) nm);
    check(trew::tracts_host(words.data(), offsets.data(), lengths.data(), n, motifs.data(), nm, 3, t.data()));
    printf("tracts\n");
    for (const auto &x : t)
        printf("%u %u %u %u %u %u %u %u %u %u\n", x.covered_fwd, x.head_len_fwd, x.head_cov_fwd, x.tail_len_fwd, x.tail_cov_fwd, x.covered_rev, x.head_len_rev,
               x.head_cov_rev, x.tail_len_rev, x.tail_cov_rev);

    uint64_t found0 = 0, found = 0;
    std::vector<uint32_t> counts(n * (size_t) nm * 2);
    check(trew::intervals_host(words.data(), offsets.data(), lengths.data(), n, motifs.data(), rules.data(), nm, nullptr, 0, &found0, nullptr));
    std::vector<trew_hip_interval> iv(found0);
    check(trew::intervals_host(words.data(), offsets.data(), lengths.data(), n, motifs.data(), rules.data(), nm, iv.data(), found0, &found, counts.data()));
    printf("intervals %llu %llu\n", (unsigned long long) found0, (unsigned long long) found);
    for (const auto &x : iv) printf("%u %u %u %u %u %u\n", x.read, x.motif, x.strand, x.start, x.end, x.covered);
    printf("counts\n");
    for (size_t i = 0; i < counts.size(); i += 2) printf("%u %u\n", counts[i], counts[i + 1]);

    std::vector<trew_hip_variant> v(n * (size_t) nm);
    std::vector<uint64_t> hist((size_t) nm * 2 * TREW_VARIANT_BINS), reads_with(hist.size());
    check(trew::variants_host(words.data(), offsets.data(), lengths.data(), n, motifs.data(), nm, v.data(), hist.data(), reads_with.data()));
    printf("variants\n");
    for (const auto &x : v)
        printf("%u %u %u %u %u %u %u %u %u %u\n", x.units_fwd, x.variants_fwd, x.distinct_fwd, x.top_fwd, x.top_count_fwd, x.units_rev, x.variants_rev,
               x.distinct_rev, x.top_rev, x.top_count_rev);
    printf("histograms\n");
    for (size_t i = 0; i < hist.size(); i++)
        if (hist[i] || reads_with[i]) printf("%zu %llu %llu\n", i, (unsigned long long) hist[i], (unsigned long long) reads_with[i]);
    return 0;
}
