// Test harness (CPU only): runs the product's serial chunk reader and its line location (host/fastq_chunks.hpp) over a
// file with a given chunk length.  Prints "C num_before total first_read n_lines" per chunk and "L ordinal length hash"
// (FNV-1a, 64 bits, of the line's bytes) per located sequence line, in the order the reader hands the chunks out.  A read
// that does not fit a chunk: the message on stderr, exit status 1 and nothing on stdout.
// Driven by tests/test_fastq_chunks_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../trew_amd/csrc/host/fastq_chunks.hpp"

using namespace trew_host;

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int chunk = atoi(argv[2]);
    if (chunk < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::string out;
    std::vector<uint32_t> nl;
    std::vector<int64_t> st, nd;
    char line[96];
    const ChunkEnd end = read_fastq_chunks([&](char *p, int n) { return (int) fread(p, 1, (size_t) n, f); }, [&] { return feof(f) != 0; }, chunk,
                                           [&](char *buffer, int total, int64_t num_before) {
                                               const uint64_t first_read = locate_chunk_lines(buffer, (size_t) total, num_before, nl, st, nd);
                                               snprintf(line, sizeof line, "C %lld %d %llu %zu\n", (long long) num_before, total, (unsigned long long) first_read, st.size());
                                               out += line;
                                               for (size_t i = 0; i < st.size(); i++) {
                                                   uint64_t h = 1469598103934665603ull;
                                                   for (int64_t p = st[i]; p <= nd[i]; p++) h = (h ^ (unsigned char) buffer[p]) * 1099511628211ull;
                                                   snprintf(line, sizeof line, "L %llu %lld %016llx\n", (unsigned long long) (first_read + i), (long long) (nd[i] - st[i] + 1),
                                                            (unsigned long long) h);
                                                   out += line;
                                               }
                                               free(buffer);
                                           });
    fclose(f);
    if (end == ChunkEnd::TooLong) {
        fprintf(stderr, "a read does not fit one %d-byte chunk\n", chunk);
        return 1;
    }
    if (end != ChunkEnd::Eof) return 3;
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
