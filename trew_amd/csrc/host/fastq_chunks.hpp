// fastq_chunks.hpp -- the serial chunk reader of a FASTQ stream (gzip, BGZF, or plain text on request) and the location
// of the sequence lines of one of its chunks.
//
// The reference reads fixed-size chunks and finds sequence lines by counting newlines from the start of the file: the
// newline that makes `num & 3 == 2` closes one (read_fastq_thread, kmer.cpp:987-1038), whatever the lines contain.  A
// chunk that ends inside a sequence line hands the begun line over to the front of the next chunk (kmer.cpp:1026-1029),
// so a chunk starts at a line start or, after such a carry-over, at the start of a sequence line.  The reader is the
// serial part of a compressed run, so it only COUNTS the newlines of a chunk; the consumer that gets the chunk finds the
// lines itself from the chunk's bytes and the number of newlines that precede the chunk in the file.
//
// Both pieces are pure -- no queue, no device, no process exit -- so that tests/harness/chunks_harness.cpp can drive
// them with any chunk length.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fastq_blocks.hpp"

namespace trew_host {

enum class ChunkEnd {
    Eof,       // the stream ended; the last chunk (possibly empty) has been handed to the sink
    IoError,   // read() returned nothing and eof() is false; the last chunk has been handed to the sink as well
    TooLong,   // a carried sequence line leaves no room in a chunk; the chunk at hand has NOT been handed to the sink
    NoMemory,  // malloc failed
};

// The chunking loop.  `read(p, n)` stores up to n bytes at p and returns how many (<= 0: nothing more), `eof()` tells a
// clean end from an error once read() returned nothing, `chunk` is the chunk length: a chunk holds at most chunk - 1
// bytes, carried ones included, and a closing NUL.  `sink(buffer, total, num_before)` receives every chunk in file order
// and owns `buffer` (malloc, `chunk` bytes) from then on; num_before is the number of newlines in front of the chunk's
// NEW bytes -- which, as a carry-over never holds a newline, is also the number in front of the chunk.
// A carried line of chunk - 2 bytes or more ends the loop with TooLong: every sequence line of at most chunk - 3 bytes
// passes, one of chunk - 1 or more never does, and one of chunk - 2 bytes is refused where a chunk border falls directly
// in front of its header's newline.
template <class ReadFn, class EofFn, class Sink>
inline ChunkEnd read_fastq_chunks(ReadFn &&read, EofFn &&eof, int chunk, Sink &&sink) {
    int64_t num = 0;
    int shift = 0;
    char *buffer = (char *) malloc((size_t) chunk);
    if (!buffer) return ChunkEnd::NoMemory;
    for (;;) {
        const int bytes_read = read(buffer + shift, chunk - 1 - shift);
        const int total = (bytes_read > 0 ? bytes_read : 0) + shift;
        buffer[total] = '\0';
        const int64_t num_before = num;
        num += (int64_t) count_newlines(buffer, (size_t) total);
        if (bytes_read <= 0) {
            sink(buffer, total, num_before);
            return eof() ? ChunkEnd::Eof : ChunkEnd::IoError;  // kmer.cpp:1021-1022
        }
        char *buffer_new = (char *) malloc((size_t) chunk);
        if (!buffer_new) {
            free(buffer);
            return ChunkEnd::NoMemory;
        }
        shift = 0;
        if ((num & 3) == 1) {  // inside a sequence line: carry it over (kmer.cpp:1026-1029)
            const char *last = (const char *) memrchr(buffer, '\n', (size_t) total);
            const int idx = last ? (int) (last - buffer) : -1;
            const int rest = total - idx - 1;
            memcpy(buffer_new, buffer + idx + 1, (size_t) rest);
            shift = rest;
            if (shift >= chunk - 2) {
                free(buffer);
                free(buffer_new);
                return ChunkEnd::TooLong;
            }
        }
        sink(buffer, total, num_before);
        buffer = buffer_new;
    }
}

// The sequence lines of one chunk: st / nd receive the inclusive byte ranges [st, nd] (offsets into `buffer`, the
// LocationVector convention of kmer.h:73) of the lines whose closing newline lies in buffer[0, total); returns the ordinal
// of the first of them among the file's sequence lines.  Newline j of the chunk closes line number num_before + j, and
// sequence lines are the numbers 1 mod 4.  nl is scratch for the chunk's newline offsets.
inline uint64_t locate_chunk_lines(const char *buffer, size_t total, int64_t num_before, std::vector<uint32_t> &nl, std::vector<int64_t> &st,
                                   std::vector<int64_t> &nd) {
    if (nl.size() < total + 2) nl.resize(total + 2);  // + 2: scan_newlines stores two slots ahead
    const size_t cnt = scan_newlines(buffer, total, nl.data());
    const size_t j0 = (size_t) ((1 - num_before) & 3);
    const uint64_t first_read = (uint64_t) (num_before + (int64_t) j0) >> 2;
    st.clear();
    nd.clear();
    for (size_t j = j0; j < cnt; j += 4) {
        const int64_t start = j > 0 ? (int64_t) nl[j - 1] + 1 : 0, len = (int64_t) nl[j] - start;
        st.push_back(start);
        nd.push_back(start + len - 1);
    }
    return first_read;
}

}  // namespace trew_host
