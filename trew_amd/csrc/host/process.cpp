// process.cpp -- per-file pipelines of the `trew` host: FASTQ decode on CPU threads, packing into
// pinned buffers, one device slot (HIP stream) per worker thread, device tables collected per file.
//
// Two pipelines, same results:
//
//  * serial reader (gzip / BGZF input): the shape of the reference
//    (kmer.cpp:987-1476) -- one producer reading 4 MiB chunks (LENGTH, kmer.h:8), sequence lines found by
//    counting newlines (num & 3 == 2), a sequence line split across two chunks carried over, pairs
//    re-synchronised by read index; NUM_THREAD-1 consumers.  A consumer does not scan the reads itself: it
//    packs the chunk into pinned memory and submits it to its own HIP stream (trew_hip_submit), so
//    decode/pack of chunk i+1 overlaps the device scan of chunk i.
//
//  * block-parallel reader (plain FASTQ; paired files have their own variant further down): the file is mapped and cut into 4 MiB
//    blocks that the NUM_THREAD-1 workers claim in file order.  A worker records the newlines of its block,
//    learns the line number its block starts at from its predecessor (a chain of additions, the only serial
//    part), and then packs the sequence lines that END in its block -- a line that starts in an earlier
//    block is simply read from there, which is what the reference's carry-over achieves -- straight into its
//    pinned buffers.  Line numbering is exact (no record-boundary heuristics): the same reads as
//    read_fastq_thread, in any block order, since counts are sums.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <type_traits>

#include "bgzf_reader.hpp"
#include "fastq_blocks.hpp"
#include "fastq_chunks.hpp"
#include "trew_host.hpp"

namespace trew_host {

static const int LENGTH = 1 << 22;  // kmer.h:8
static const int MAX_SEQ = 1000;    // kmer.h:10
// Text a worker of the block-parallel reader gathers (over several 4 MiB blocks) before it submits one batch.  The
// device scans a batch of this size in well under a millisecond; what a submit costs is its handful of HIP calls and
// the stream's hand-overs (copy -> prefilter -> exact kernel), which at 4 MiB per batch and 15 workers were the whole
// end-to-end time (tools/e2e_cli.py, profiles/r02/README.md).
static const size_t kSubmitBytes = (size_t) 32 << 20;  // capacity; Config::batch_mib (<= 32) is what a batch is closed at

// Errors follow the reference: message on stderr, exit status 1 (kmer.cpp:84-87, 1007-1008).  The other host
// threads may be inside HIP calls on live streams at this moment; running atexit handlers and the HIP runtime's
// teardown under them can hang, so the process leaves through _exit after flushing its own output.
[[noreturn]] static void die(const char *msg) {
    fprintf(stderr, "%s\n", msg);
    fflush(stdout);
    fflush(stderr);
    _exit(EXIT_FAILURE);
}

// FileReader, kmer.h:157-204
struct FileReader {
    bool is_gz = false;
    FILE *fp = nullptr;
    gzFile gz_fp = nullptr;
    BgzfReader *bgzf = nullptr;  // block-gzip input: members inflated on several threads
    int read(char *buffer, int length) {
        if (bgzf) return bgzf->read(buffer, length);
        return is_gz ? gzread(gz_fp, buffer, (unsigned) length) : (int) fread(buffer, 1, (size_t) length, fp);
    }
    bool eof() {
        if (bgzf) return bgzf->eof();
        return is_gz ? gzeof(gz_fp) != 0 : feof(fp) != 0;
    }
    const char *error() {
        if (bgzf) return bgzf->error();
        if (is_gz) {
            int err_num;
            return gzerror(gz_fp, &err_num);
        }
        return strerror(errno);
    }
    void close() {
        if (bgzf)
            delete bgzf;
        else if (is_gz)
            gzclose(gz_fp);
        else
            fclose(fp);
        bgzf = nullptr;
    }
};

[[noreturn]] static void open_failed(const char *file_name) {  // kmer.cpp:1288-1289
    fprintf(stderr, "File open failed: %s\n", file_name);
    fflush(stdout);
    fflush(stderr);
    _exit(EXIT_FAILURE);
}

static FileReader open_reader(const char *file_name, bool is_gz, int n_threads) {
    FileReader r;
    r.is_gz = is_gz;
    if (is_gz && BgzfReader::sniff(file_name)) {
        // inflate is the bottleneck of compressed input and the packers are nearly idle beside it: as many inflate
        // threads as the user gave the run (-t), within what the machine has
        const unsigned hw = std::max(2u, std::thread::hardware_concurrency());
        r.bgzf = new BgzfReader(file_name, (int) std::min<unsigned>(hw, (unsigned) std::max(2, std::min(n_threads, 32))));
        if (!r.bgzf->ok()) open_failed(file_name);
        return r;
    }
    if (is_gz) {
        r.gz_fp = gzopen(file_name, "r");
        if (!r.gz_fp) open_failed(file_name);
        gzbuffer(r.gz_fp, 1 << 20);
    } else {
        r.fp = fopen(file_name, "r");
        if (!r.fp) open_failed(file_name);
    }
    return r;
}

// QueueData / PairQueueData, kmer.h:93-103
struct Chunk {
    char *buffer1 = nullptr, *buffer2 = nullptr;
    std::vector<int64_t> st1, nd1, st2, nd2;
    bool sentinel = false;
    // single-file chunks leave the reader with their lines only COUNTED (the reader is the serial part of a compressed
    // run: it inflates, counts newlines and carries a split sequence line over); the consumer that gets the chunk finds
    // the sequence lines itself from `total` bytes and the number of newlines that precede the chunk in the file
    bool located = true;
    int total = 0;
    int64_t num_before = 0;
};

class ChunkQueue {  // the role of tbb::concurrent_bounded_queue (kmer.h:111-112)
public:
    explicit ChunkQueue(size_t cap) : cap_(cap) {}
    void push(Chunk *c) {
        std::unique_lock<std::mutex> lk(m_);
        not_full_.wait(lk, [&] { return q_.size() < cap_; });
        q_.push_back(c);
        not_empty_.notify_one();
    }
    Chunk *pop() {
        std::unique_lock<std::mutex> lk(m_);
        not_empty_.wait(lk, [&] { return !q_.empty(); });
        Chunk *c = q_.front();
        q_.pop_front();
        not_full_.notify_one();
        return c;
    }

private:
    std::mutex m_;
    std::condition_variable not_full_, not_empty_;
    std::deque<Chunk *> q_;
    size_t cap_;
};

struct Worker {
    int dev_index = 0;  // index into Scanner::dev
    int slot = 0;
    // the block-parallel reader alternates between two slots (and two pinned buffers): it fills one batch while the previous
    // one is still on its way to the device, instead of waiting for the copy (13 % of a worker's time with one, --stats)
    int slot_b = 0;
    uint32_t *h_buf_b = nullptr;
    // one pinned allocation; a batch is laid out [offsets n][lengths n][words] (serial reader: n is known before
    // packing) or [words][offsets n][lengths n] (block reader: reads accumulate), either of which trew_hip_submit
    // ships with a single copy (include/trew_hip.h, trew_hip_batch)
    uint32_t *h_buf = nullptr;
    std::vector<uint32_t> tmp_off, tmp_len;  // block reader: offsets / lengths until the batch is closed
    uint64_t words_cap = 0, reads_cap = 0, text_cap = 0;
    std::vector<uint32_t> tmp_woff;  // text batches: word offset of every read (running sum of the packed sizes)
    uint64_t reads = 0, bases = 0, submits = 0;
    double t_scan = 0, t_wait = 0, t_pack = 0, t_submit = 0, t_pressure = 0;  // seconds per phase, for --stats (t_pressure is part of t_submit)
    std::vector<int64_t> st, nd;      // block-parallel reader: sequence lines of the current block
    std::vector<uint32_t> nl;         // newline offsets of the current block
};

// one GPU: its context and the lock that keeps a table drain apart from running submits
struct Device {
    trew_hip_ctx *ctx = nullptr;
    std::shared_mutex drain_mu;  // shared: trew_hip_submit; exclusive: collect + reset
};

struct Scanner {
    Config cfg;
    int mode = TREW_MODE_SHORT;
    std::vector<std::unique_ptr<Device>> dev;
    std::vector<Worker> workers;
    RunStats stats;
    // rows drained from the device tables in the middle of a file (the reference's hash maps grow without
    // bound; the device table is fixed-size, so it is emptied into host memory whenever it runs half full)
    std::mutex pending_mu;
    ResultMapData pending;
    std::atomic<uint64_t> drains{0};
    double t_map = 0, t_workers = 0, t_unmap = 0, t_collect = 0;  // --stats: wall seconds of the block-parallel reader's stages
};

[[noreturn]] static void hip_die(trew_hip_ctx *ctx, const char *what) {
    fprintf(stderr, "%s: %s\n", what, trew_hip_last_error(ctx));
    fflush(stdout);
    fflush(stderr);
    _exit(EXIT_FAILURE);
}

Scanner *scanner_create(const Config &cfg, int mode) {
    Scanner *s = new Scanner();
    s->cfg = cfg;
    s->mode = mode;
    // --compat_g1: the reference's 64-bit pair branch with its un-cleared temp_result_left is only defined for ONE
    // consumer that sees the pairs in file order: one worker, one slot.  With MAX_MER > 32 the reference runs the 128-bit
    // branch, which clears the map: nothing to reproduce, the flag is not passed on.
    const bool compat_g1 = cfg.compat_g1 && mode == TREW_MODE_PAIR && cfg.MAX_MER <= 32;
    const int n_workers = compat_g1 ? 1 : std::max(1, cfg.NUM_THREAD - 1);  // the caller's thread is the reader (kmer.cpp:1278-1301)
    const int ndev = (int) cfg.devices.size();
    const bool pair = mode == TREW_MODE_PAIR;
    const uint64_t reads_cap = (pair ? 2ull : 1ull) << 20;
    // serial reader: one 4 MiB chunk per mate; block reader: kSubmitBytes of text per batch plus the line that ends in a
    // block but started before it; every read may waste up to one triple of padding
    const uint64_t words_cap = 3ull * ((uint64_t) (kSubmitBytes + 2 * LENGTH) / 32 + reads_cap) + 64;
    // text batches of the block-parallel reader (the device packs): the sequence bytes of a batch + 12 B of index arrays per read
    const uint64_t text_cap = (uint64_t) (kSubmitBytes + 2 * LENGTH) + 12ull * reads_cap;
    std::vector<int> slots_on_dev((size_t) ndev, 0);
    for (int w = 0; w < n_workers; w++) slots_on_dev[(size_t) (w % ndev)]++;
    for (int d = 0; d < ndev; d++) {
        trew_hip_params p;
        memset(&p, 0, sizeof(p));
        p.min_mer = cfg.MIN_MER;
        p.max_mer = cfg.MAX_MER;
        p.low_baseline = cfg.LOW_BASELINE;
        p.high_baseline = cfg.HIGH_BASELINE;
        p.slice_length = cfg.SLICE_LENGTH;
        p.mode = mode;
        p.device = cfg.devices[(size_t) d];
        p.n_slots = compat_g1 ? 1 : 2 * std::max(1, slots_on_dev[(size_t) d]);
        p.max_batch_words = words_cap;
        p.max_batch_reads = reads_cap;
        p.table_log2_slots = (uint32_t) cfg.table_log2_slots;
        p.max_batch_ascii_bytes = cfg.host_pack ? 0 : text_cap;
        // ~10^4 small batches a second: every HIP call per batch counts -- no timing events, and the table's fill state comes
        // back with every batch instead of being asked for before every batch (0.4 ms a query with 15 threads asking)
        p.flags = TREW_FLAG_NO_TIMING | TREW_FLAG_TRACK_PRESSURE | (compat_g1 ? TREW_FLAG_COMPAT_G1 : 0);
        trew_hip_ctx *c = nullptr;
        if (trew_hip_init(&p, &c) != 0) die(trew_hip_last_error(nullptr));
        s->dev.emplace_back(new Device());
        s->dev.back()->ctx = c;
    }
    std::vector<int> next_slot((size_t) ndev, 0);
    for (int w = 0; w < n_workers; w++) {
        Worker wk;
        wk.dev_index = w % ndev;
        wk.slot = next_slot[(size_t) wk.dev_index]++;
        wk.slot_b = compat_g1 ? wk.slot : next_slot[(size_t) wk.dev_index]++;
        wk.words_cap = words_cap;
        wk.reads_cap = reads_cap;
        trew_hip_ctx *c = s->dev[(size_t) wk.dev_index]->ctx;
        wk.text_cap = text_cap;
        if (trew_hip_host_alloc(c, std::max<uint64_t>((words_cap + 2 * reads_cap) * 4, text_cap + 64), (void **) &wk.h_buf)) hip_die(c, "pinned allocation");
        if (trew_hip_host_alloc(c, std::max<uint64_t>((words_cap + 2 * reads_cap) * 4, text_cap + 64), (void **) &wk.h_buf_b)) hip_die(c, "pinned allocation");
        s->workers.push_back(std::move(wk));
    }
    return s;
}

void scanner_destroy(Scanner *s) {
    if (!s) return;
    for (auto &w : s->workers) {
        trew_hip_ctx *c = s->dev[(size_t) w.dev_index]->ctx;
        trew_hip_host_free(c, w.h_buf);
        trew_hip_host_free(c, w.h_buf_b);
    }
    for (auto &d : s->dev) trew_hip_destroy(d->ctx);
    delete s;
}

const RunStats &last_stats(const Scanner *s) { return s->stats; }

static void add_rows_to(ResultMapData &r, const std::vector<trew_hip_row> &rows, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) {
        const uint128_t w = ((uint128_t) rows[i].word_hi << 64) | rows[i].word_lo;
        r.table[rows[i].table][KmerSeq{rows[i].k, w}] += rows[i].count;  // thread merge, kmer.cpp:1486-1515
    }
}

// empties one device's tables into host memory; the caller holds the device's drain lock exclusively
// (or no worker is running)
static void drain_device(Scanner *s, Device *d) {
    uint64_t n = 0;
    if (trew_hip_collect(d->ctx, -1, nullptr, 0, &n)) hip_die(d->ctx, "trew_hip_collect");
    std::vector<trew_hip_row> rows((size_t) std::max<uint64_t>(n, 1));
    if (trew_hip_collect(d->ctx, -1, rows.data(), n, &n)) hip_die(d->ctx, "trew_hip_collect");
    {
        std::lock_guard<std::mutex> lk(s->pending_mu);
        add_rows_to(s->pending, rows, n);
    }
    if (trew_hip_reset_tables(d->ctx)) hip_die(d->ctx, "trew_hip_reset_tables");
}

// true when the device table should be emptied before more rows arrive
static bool under_pressure(trew_hip_ctx *c) {
    uint64_t used = 0, total = 0, spilled = 0, spill_cap = 0;
    if (trew_hip_table_pressure(c, &used, &total, &spilled, &spill_cap)) hip_die(c, "trew_hip_table_pressure");
    return used * 2 > total || spilled > 0;
}

// hand one packed batch (already in the worker's pinned buffers) to the worker's device slot
static void submit_packed(Scanner *s, Worker *w, uint32_t *h_words, uint32_t *h_offsets, uint32_t *h_lengths, uint64_t n_reads, uint64_t n_words) {
    Device *d = s->dev[(size_t) w->dev_index].get();
    trew_hip_ctx *c = d->ctx;
    if (n_words == (uint64_t) -1) die("internal error: packed chunk exceeds the slot buffer");
    uint32_t max_len = 0;
    uint64_t bases = 0;
    for (uint64_t i = 0; i < n_reads; i++) {
        bases += h_lengths[i];
        max_len = std::max(max_len, h_lengths[i]);
    }
    w->bases += bases;
    w->reads += n_reads;
    if (n_reads == 0) return;
    // before every batch: has the fixed-size device table run half full (or started to spill)?  Then it is emptied
    // into host memory before this batch adds to it.  Counts can only be lost if one batch fills what is left of the
    // table AND the spill log (>= 64 k rows, 1 M at the default table size); trew_hip_collect reports that as an error.
    w->submits++;
    const auto tp0 = std::chrono::steady_clock::now();
    const bool pressed = under_pressure(c);
    w->t_pressure += std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count();
    if (pressed) {
        // emptying the table mid-file also empties the stale map of --compat_g1 (trew_hip_reset_tables starts a new input): say so
        if (s->cfg.compat_g1 && s->mode == TREW_MODE_PAIR && s->cfg.MAX_MER <= 32)
            die("--compat_g1: the device count table filled up in the middle of a file; raise --table_log2_slots");
        std::unique_lock<std::shared_mutex> lk(d->drain_mu);  // waits for running submits, blocks new ones
        if (under_pressure(c)) {                              // nobody drained in the meantime
            drain_device(s, d);
            s->drains++;
        }
    }
    trew_hip_batch b;
    memset(&b, 0, sizeof(b));
    b.words = h_words;
    b.n_words = n_words;
    b.offsets = h_offsets;
    b.lengths = h_lengths;
    b.n_reads = n_reads;
    b.max_length = (int32_t) max_len;
    std::shared_lock<std::shared_mutex> lk(d->drain_mu);
    if (trew_hip_submit(c, &b, w->slot)) hip_die(c, "trew_hip_submit");
}

// the same for a batch of TEXT (sequence bytes + index arrays, see trew_hip_ascii_batch): the device packs
static void submit_text(Scanner *s, Worker *w, const trew_hip_ascii_batch &b, uint64_t bases) {
    Device *d = s->dev[(size_t) w->dev_index].get();
    trew_hip_ctx *c = d->ctx;
    w->bases += bases;
    w->reads += b.n_reads;
    if (b.n_reads == 0) return;
    w->submits++;
    const auto tp0 = std::chrono::steady_clock::now();
    const bool pressed = under_pressure(c);
    w->t_pressure += std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count();
    if (pressed) {
        // emptying the table mid-file also empties the stale map of --compat_g1 (trew_hip_reset_tables starts a new input): say so
        if (s->cfg.compat_g1 && s->mode == TREW_MODE_PAIR && s->cfg.MAX_MER <= 32)
            die("--compat_g1: the device count table filled up in the middle of a file; raise --table_log2_slots");
        std::unique_lock<std::shared_mutex> lk(d->drain_mu);  // waits for running submits, blocks new ones
        if (under_pressure(c)) {                              // nobody drained in the meantime
            drain_device(s, d);
            s->drains++;
        }
    }
    std::shared_lock<std::shared_mutex> lk(d->drain_mu);
    if (trew_hip_submit_ascii(c, &b, w->slot)) hip_die(c, "trew_hip_submit_ascii");
}

// the consumer: buffer_task* (kmer.cpp:80-985) with the scan itself moved to the device
static void worker_loop(Scanner *s, Worker *w, ChunkQueue *q) {
    trew_hip_ctx *c = s->dev[(size_t) w->dev_index]->ctx;
    for (;;) {
        Chunk *ch = q->pop();
        if (ch->sentinel) {  // loc_vector == nullptr, kmer.cpp:108-110
            delete ch;
            break;
        }
        if (!ch->located) {
            // the newline that makes num & 3 == 2 closes a sequence line (read_fastq_thread, kmer.cpp:1002-1011); a chunk
            // starts at a line start or, after a carry-over, at the start of a sequence line
            if (w->nl.size() < (size_t) LENGTH + 2) w->nl.resize((size_t) LENGTH + 2);  // + 2: scan_newlines stores two slots ahead
            const size_t cnt = scan_newlines(ch->buffer1, (size_t) ch->total, w->nl.data());
            const bool long_mode = s->mode == TREW_MODE_LONG;
            for (size_t j = (size_t) ((1 - ch->num_before) & 3); j < cnt; j += 4) {
                const int64_t start = j > 0 ? (int64_t) w->nl[j - 1] + 1 : 0, len = (int64_t) w->nl[j] - start;
                if (long_mode) {
                    if (len < s->cfg.SLICE_LENGTH) continue;  // kmer.cpp:1184
                } else if (len > MAX_SEQ) {
                    die("This mode is designed for short-read sequencing. Please use 'trew long'.");  // kmer.cpp:1006-1009
                }
                ch->st1.push_back(start);
                ch->nd1.push_back(start + len - 1);
            }
        }
        if (trew_hip_wait(c, w->slot)) hip_die(c, "trew_hip_wait");  // the slot's pinned buffers are free again
        uint64_t nw, n_reads;
        if (s->mode == TREW_MODE_PAIR) {
            const uint64_t np = std::min(ch->st1.size(), ch->st2.size());  // kmer.cpp:321
            n_reads = 2 * np;
            nw = trew_pack_pairs(ch->buffer1, ch->st1.data(), ch->nd1.data(), ch->buffer2, ch->st2.data(), ch->nd2.data(), np, w->h_buf + 2 * n_reads,
                                 w->words_cap, w->h_buf, w->h_buf + n_reads);
        } else {
            n_reads = ch->st1.size();
            nw = trew_pack_reads(ch->buffer1, ch->st1.data(), ch->nd1.data(), n_reads, w->h_buf + 2 * n_reads, w->words_cap, w->h_buf, w->h_buf + n_reads);
        }
        submit_packed(s, w, w->h_buf + 2 * n_reads, w->h_buf, w->h_buf + n_reads, n_reads, nw);
        free(ch->buffer1);  // the consumer owns and frees the chunk, kmer.cpp:175-176
        free(ch->buffer2);
        delete ch;
    }
    if (trew_hip_wait(c, w->slot)) hip_die(c, "trew_hip_wait");
}

static char *alloc_buffer() {
    char *b = (char *) malloc(LENGTH);
    if (!b) die("memory allocation failure");
    return b;
}

// read_fastq_thread (kmer.cpp:987-1038) and read_fastq_long_thread (1166-1213): 4 MiB chunks, sequence lines by counting
// newlines, a sequence line split across two chunks carried over.  This thread is the serial part of a compressed run, so it
// only COUNTS the newlines of a chunk (AVX2) and leaves finding the lines to the consumer (Chunk::located).
static void read_fastq_thread(FileReader &fr, ChunkQueue *q, int chunk = LENGTH) {
    const ChunkEnd end = read_fastq_chunks([&](char *p, int n) { return fr.read(p, n); }, [&] { return fr.eof(); }, chunk,
                                           [&](char *buffer, int total, int64_t num_before) {
                                               Chunk *ch = new Chunk();
                                               ch->buffer1 = buffer;
                                               ch->located = false;
                                               ch->total = total;
                                               ch->num_before = num_before;
                                               q->push(ch);
                                           });
    if (end == ChunkEnd::NoMemory) die("memory allocation failure");
    if (end == ChunkEnd::TooLong) {
        if (chunk == LENGTH) die("a read does not fit one 4 MiB chunk");
        fprintf(stderr, "a read does not fit one %d-byte chunk\n", chunk);
        fflush(stdout);
        fflush(stderr);
        _exit(EXIT_FAILURE);
    }
    if (end == ChunkEnd::IoError) {
        fprintf(stderr, "File-IO Error: %s.\n", fr.error());  // kmer.cpp:1021-1022
        fflush(stdout);
        fflush(stderr);
        _exit(EXIT_FAILURE);
    }
}

// read_pair_fastq_thread, kmer.cpp:1040-1164: mates are matched by read index; the side that
// decoded more reads in a chunk carries the surplus over to the next one
static void read_pair_fastq_thread(FileReader &f1, FileReader &f2, ChunkQueue *q) {
    struct Side {
        FileReader *fr;
        int num = 0, shift = 0, idx = -1, bytes_read = 0;
        bool is_end = false;
        char *buffer = nullptr;
        std::vector<int64_t> st, nd;
    } s[2];
    s[0].fr = &f1;
    s[1].fr = &f2;
    s[0].buffer = alloc_buffer();
    s[1].buffer = alloc_buffer();
    for (;;) {
        for (int m = 0; m < 2; m++) {
            Side &x = s[m];
            x.st.clear();
            x.nd.clear();
            if (!x.is_end) {
                x.bytes_read = x.fr->read(x.buffer + x.shift, LENGTH - 1 - x.shift);
                if (x.bytes_read <= 0) {
                    if (x.fr->eof()) {
                        x.is_end = true;
                        x.bytes_read = 0;
                    } else {
                        fprintf(stderr, "File %d IO Error: %s.\n", m + 1, x.fr->error());  // kmer.cpp:1065,1080
                        fflush(stdout);
                        fflush(stderr);
                        _exit(EXIT_FAILURE);
                    }
                }
            } else {
                x.bytes_read = 0;
            }
            const int total = x.bytes_read + x.shift;
            x.buffer[total] = '\0';
            for (const char *nl = (const char *) memchr(x.buffer, '\n', (size_t) total); nl;
                 nl = (const char *) memchr(nl + 1, '\n', (size_t) (x.buffer + total - nl - 1))) {
                const int i = (int) (nl - x.buffer);
                x.num += 1;
                if ((x.num & 3) == 2) {
                    if ((i - 1) - (x.idx + 1) + 1 > MAX_SEQ)  // the reference leaves pair mode unchecked
                        die("This mode is designed for short-read sequencing. Please use 'trew long'.");
                    x.st.push_back(x.idx + 1);
                    x.nd.push_back(i - 1);
                }
                x.idx = i;
            }
        }
        Chunk *ch = new Chunk();
        if (s[0].is_end && s[1].is_end) {
            if (s[0].num != s[1].num) {  // kmer.cpp:1112-1114
                fprintf(stderr, "Error: Mismatched record counts between files (num1: %d, num2: %d).\n", s[0].num, s[1].num);
                fflush(stdout);
                fflush(stderr);
                _exit(EXIT_FAILURE);
            }
            ch->buffer1 = s[0].buffer;
            ch->buffer2 = s[1].buffer;
            ch->st1 = s[0].st;
            ch->nd1 = s[0].nd;
            ch->st2 = s[1].st;
            ch->nd2 = s[1].nd;
            q->push(ch);
            break;
        }
        if ((s[0].st.empty() && !s[1].st.empty()) || (!s[0].st.empty() && s[1].st.empty())) die("Paired-end error");  // kmer.cpp:1120-1124
        const size_t min_size = std::min(s[0].st.size(), s[1].st.size());
        char *nb[2] = {alloc_buffer(), alloc_buffer()};
        for (int m = 0; m < 2; m++) {
            Side &x = s[m];
            const int total = x.bytes_read + x.shift;
            if (x.st.size() > min_size) {  // surplus reads: restart the next chunk at the first unmatched sequence line
                x.idx = (int) x.st[min_size] - 1;
                const int rest = total - x.idx - 1;
                memcpy(nb[m], x.buffer + x.idx + 1, (size_t) rest);
                x.num = ((x.num - 2) / 4) * 4 + 1 - 4 * (int) (x.st.size() - min_size - 1);  // kmer.cpp:1135
                x.shift = rest;
                x.idx = -1;
            } else if ((x.num & 3) == 1) {
                const int rest = total - x.idx - 1;
                memcpy(nb[m], x.buffer + x.idx + 1, (size_t) rest);
                x.shift = rest;
                x.idx = -1;
            } else {
                x.shift = 0;
                x.idx = -1;
            }
        }
        ch->buffer1 = s[0].buffer;
        ch->buffer2 = s[1].buffer;
        ch->st1.assign(s[0].st.begin(), s[0].st.begin() + (long) min_size);
        ch->nd1.assign(s[0].nd.begin(), s[0].nd.begin() + (long) min_size);
        ch->st2.assign(s[1].st.begin(), s[1].st.begin() + (long) min_size);
        ch->nd2.assign(s[1].nd.begin(), s[1].nd.begin() + (long) min_size);
        q->push(ch);
        s[0].buffer = nb[0];
        s[1].buffer = nb[1];
    }
}

// ------------------------------------------------------------------ block-parallel reader (plain FASTQ)
struct BlockJob {
    BlockScan scan;
    bool long_mode = false;
    int slice_length = 0;
};

#if defined(__x86_64__)
__attribute__((target("avx2"))) static inline void copy_short_line(unsigned char *dst, const char *src, uint32_t len) {
    for (uint32_t o = 0; o < len; o += 32) _mm256_storeu_si256((__m256i *) (dst + o), _mm256_loadu_si256((const __m256i *) (src + o)));
}
#else
static inline void copy_short_line(unsigned char *dst, const char *src, uint32_t len) { memcpy(dst, src, len); }
#endif

static void block_worker_loop(Scanner *s, Worker *w, BlockJob *job) {
    trew_hip_ctx *c = s->dev[(size_t) w->dev_index]->ctx;
    typedef std::chrono::steady_clock clk;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    // ship the sequence bytes, the device applies codes[] (pack kernel); else trew_pack_reads here.  Long reads are packed on the
    // host: their kernels take longer per base and a byte per base over PCIe (against 3 bits) then makes the workers wait for
    // their slots -- 29.0 against 30.7 Gbases/s on 300 k ONT-like reads (tools/e2e_long.py, profiles/r03/README.md)
    const bool text = !s->cfg.host_pack && !job->long_mode;
#if defined(__x86_64__)
    const bool inline_copy = __builtin_cpu_supports("avx2") && !getenv("TREW_AB_MEMCPY");
#else
    const bool inline_copy = false;
#endif
    uint64_t acc_reads = 0, acc_words = 0, acc_bytes = 0, acc_bases = 0;
    size_t acc_text = 0;
    bool buffers_free = false;  // has the slot's previous submit been waited for
    bool same_len = true;       // text batches: every read so far has the length of the first one
    if (w->tmp_off.size() < w->reads_cap) {
        w->tmp_off.resize(w->reads_cap);
        w->tmp_len.resize(w->reads_cap);
        w->tmp_woff.resize(w->reads_cap);
    }
    // text batches: the bases start at a fixed place of the pinned buffer, the three index arrays are put right in front of
    // them when the batch is closed -- [word_offsets][byte_offsets][lengths][bases], which trew_hip_submit_ascii ships in one copy
    unsigned char *h_bases = (unsigned char *) w->h_buf + 12ull * w->reads_cap;
    const uint64_t bytes_cap = w->text_cap - 12ull * w->reads_cap;
    auto close_batch = [&]() {
        if (acc_reads == 0) return;
        const clk::time_point t3 = clk::now();
        if (text) {
            trew_hip_ascii_batch b;
            memset(&b, 0, sizeof(b));
            b.bases = (const char *) h_bases;
            b.n_bytes = acc_bytes;
            b.n_reads = acc_reads;
            // an ordinary Illumina run: no index arrays, and the prefilter takes its uniform-geometry path.  (A batch of EMPTY
            // sequence lines has one length too, but a uniform batch needs a length: it goes with index arrays and yields nothing,
            // as in the reference.)
            if (same_len && w->tmp_len[0] > 0 && !job->long_mode) {
                b.uniform_length = w->tmp_len[0];
            } else {
                uint32_t *arr = (uint32_t *) (h_bases - 12ull * acc_reads);
                memcpy(arr, w->tmp_woff.data(), acc_reads * 4);
                memcpy(arr + acc_reads, w->tmp_off.data(), acc_reads * 4);
                memcpy(arr + 2 * acc_reads, w->tmp_len.data(), acc_reads * 4);
                b.word_offsets = arr;
                b.byte_offsets = arr + acc_reads;
                b.lengths = arr + 2 * acc_reads;
            }
            submit_text(s, w, b, acc_bases);
        } else {
            uint32_t *h_off = w->h_buf + acc_words, *h_len = h_off + acc_reads;  // [words][offsets][lengths]
            memcpy(h_off, w->tmp_off.data(), acc_reads * 4);
            memcpy(h_len, w->tmp_len.data(), acc_reads * 4);
            submit_packed(s, w, w->h_buf, h_off, h_len, acc_reads, acc_words);
        }
        acc_reads = acc_words = acc_bytes = acc_bases = 0;
        acc_text = 0;
        same_len = true;
        // the next batch goes to the other slot and the other pinned buffer (that slot's previous batch was submitted one
        // batch ago: the wait below rarely blocks)
        std::swap(w->slot, w->slot_b);
        std::swap(w->h_buf, w->h_buf_b);
        h_bases = (unsigned char *) w->h_buf + 12ull * w->reads_cap;
        buffers_free = false;
        w->t_submit += secs(t3, clk::now());
    };
    for (;;) {
        const clk::time_point t0 = clk::now();
        size_t blk = 0;
        if (!job->scan.claim(w->nl, w->st, w->nd, &blk)) break;
        // the limits of the chunk reader, applied to the same lines
        size_t keep = 0;
        uint64_t need_words = 0, need_bytes = 0;
        for (size_t i = 0; i < w->st.size(); i++) {
            const int64_t len = w->nd[i] - w->st[i] + 1;
            if (job->long_mode) {
                if (len >= LENGTH - 2) die("a read does not fit one 4 MiB chunk");
                if (len < job->slice_length) continue;                              // kmer.cpp:1184
            } else if (len > MAX_SEQ) {
                die("This mode is designed for short-read sequencing. Please use 'trew long'.");  // kmer.cpp:1006-1009
            }
            w->st[keep] = w->st[i];
            w->nd[keep] = w->nd[i];
            need_words += 3ull * (((uint64_t) len + 31) / 32);
            need_bytes += (uint64_t) (len > 0 ? len : 0);
            keep++;
        }
        const clk::time_point t1 = clk::now();
        w->t_scan += secs(t0, t1);
        // a block holds at most reads_cap sequence lines and words_cap/2 words: it always fits an empty batch
        if (acc_reads + keep > w->reads_cap || acc_words + need_words > w->words_cap || (text && acc_bytes + need_bytes > bytes_cap)) close_batch();
        if (keep > w->reads_cap || need_words > w->words_cap || (text && need_bytes > bytes_cap)) die("internal error: one block's reads do not fit the slot buffer");
        if (!buffers_free) {
            const clk::time_point tw = clk::now();
            if (trew_hip_wait(c, w->slot)) hip_die(c, "trew_hip_wait");  // the slot's pinned buffer is free again
            buffers_free = true;
            w->t_wait += secs(tw, clk::now());
        }
        const clk::time_point t2 = clk::now();
        if (text) {
            // locate + copy: the bytes of the sequence lines back to back; packing is the device's job
            const char *base = job->scan.base;
            uint64_t words = acc_words, bytes = acc_bytes;
            const uint32_t first_len = acc_reads ? w->tmp_len[0] : (keep ? (uint32_t) (w->nd[0] - w->st[0] + 1 > 0 ? w->nd[0] - w->st[0] + 1 : 0) : 0u);
            // short lines are copied 32 bytes at a time past their end (the next line overwrites the excess, the pinned buffer
            // has 64 bytes of slack, and the source stays inside the mapping): a libc memcpy call per 150-byte line costs as
            // much as finding the line (profiles/r03/README.md, end to end)
            const int64_t safe_src = (int64_t) job->scan.size - 288;
            for (size_t i = 0; i < keep; i++) {
                const int64_t n = w->nd[i] - w->st[i] + 1;
                const uint32_t len = n > 0 ? (uint32_t) n : 0u;
                if (inline_copy && len <= 256 && w->st[i] <= safe_src)
                    copy_short_line(h_bases + bytes, base + w->st[i], len);
                else
                    memcpy(h_bases + bytes, base + w->st[i], len);
                w->tmp_woff[acc_reads + i] = (uint32_t) words;
                w->tmp_off[acc_reads + i] = (uint32_t) bytes;
                w->tmp_len[acc_reads + i] = len;
                same_len = same_len && len == first_len;
                words += 3ull * (((uint64_t) len + 31) / 32);
                bytes += len;
            }
            acc_bases += bytes - acc_bytes;
            acc_words = words;
            acc_bytes = bytes;
            acc_reads += keep;
        } else {
            const uint64_t nw = trew_pack_reads(job->scan.base, w->st.data(), w->nd.data(), keep, w->h_buf + acc_words, w->words_cap - acc_words,
                                                w->tmp_off.data() + acc_reads, w->tmp_len.data() + acc_reads);
            if (nw == (uint64_t) -1) die("internal error: packed block exceeds the slot buffer");
            for (size_t i = 0; i < keep; i++) w->tmp_off[acc_reads + i] += (uint32_t) acc_words;  // offsets count from the batch's first word
            acc_reads += keep;
            acc_words += nw;
        }
        acc_text += job->scan.block;
        w->t_pack += secs(t2, clk::now());
        job->scan.release(blk);  // the block's bytes are in the pinned buffer: drop its page-table entries (see BlockScan::release)
        if (acc_text >= (size_t) s->cfg.batch_mib << 20) close_batch();
    }
    close_batch();
    if (trew_hip_wait(c, w->slot) || trew_hip_wait(c, w->slot_b)) hip_die(c, "trew_hip_wait");
}

// ------------------------------------------------------------------ block-parallel reader, paired files
// Mates are matched by read index (read r = lines 4r .. 4r+3 of each file, read_pair_fastq_thread, kmer.cpp:1040-1164).
// Pass 1 counts the newlines of every 4 MiB block of both files (all workers, any order); with the prefix sums a worker
// finds where any line starts.  Pass 2: workers claim ranges of read indices, walk the two files side by side from the
// start of that range and pack the pairs.  No carry-over, no re-synchronisation: both fall out of the line numbers.
struct PairJob {
    LineIndex index[2];
    std::atomic<size_t> next_block{0}, next_item{0};
    size_t n_pairs = 0, pairs_per_item = 1 << 16;  // run_pair_blocks picks the item size (text batches: small items, see pair_worker_loop)
};

// page-table entries of [lo, hi) of a mapped file: in with one call instead of a fault per 64 KiB (before the first pass), out
// again once a worker is done with the range (one munmap of both files at the end is single-threaded: 0.1 s for 10 GB)
static void map_range(const LineIndex &ix, size_t lo, size_t hi, bool in) {
    const size_t page = 4096;
    hi = std::min(hi, ix.size);
    if (in) {
#ifdef MADV_POPULATE_READ
        const size_t plo = lo & ~(page - 1);
        if (hi > plo) (void) madvise(const_cast<char *>(ix.base) + plo, hi - plo, MADV_POPULATE_READ);
#endif
    } else {
        const size_t plo = (lo + page - 1) & ~(page - 1), phi = hi & ~(page - 1);
        if (phi > plo) (void) madvise(const_cast<char *>(ix.base) + plo, phi - plo, MADV_DONTNEED);
    }
}

static void pair_count_loop(PairJob *job) {
    const size_t n0 = job->index[0].n_blocks, total = n0 + job->index[1].n_blocks;
    for (;;) {
        const size_t i = job->next_block.fetch_add(1);
        if (i >= total) break;
        LineIndex &ix = job->index[i < n0 ? 0 : 1];
        const size_t b = i < n0 ? i : i - n0;
        map_range(ix, b * ix.block, (b + 1) * ix.block, true);
        ix.count_block(b);
    }
}

static void pair_worker_loop(Scanner *s, Worker *w, PairJob *job) {
    trew_hip_ctx *c = s->dev[(size_t) w->dev_index]->ctx;
    typedef std::chrono::steady_clock clk;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    LineCursor cur[2];
    std::vector<int64_t> st[2], nd[2];
    // Text batches (default): the sequence bytes of both mates, interleaved, accumulate over several work items until a
    // batch is full; the device packs (as block_worker_loop).  An item is small enough (pairs_per_item) for the copy to find
    // the lines that the cursor has just scanned still in cache.
    const bool text = !s->cfg.host_pack;
    unsigned char *h_bases = (unsigned char *) w->h_buf + 12ull * w->reads_cap;
    const uint64_t bytes_cap = w->text_cap - 12ull * w->reads_cap;
    uint64_t acc_reads = 0, acc_words = 0, acc_bytes = 0;
    bool same_len = true, buffers_free = false;
    uint32_t first_len = 0;
    if (text && w->tmp_off.size() < w->reads_cap) {
        w->tmp_off.resize(w->reads_cap);
        w->tmp_len.resize(w->reads_cap);
        w->tmp_woff.resize(w->reads_cap);
    }
    auto close_text_batch = [&]() {
        if (acc_reads == 0) return;
        const clk::time_point t3 = clk::now();
        trew_hip_ascii_batch b;
        memset(&b, 0, sizeof(b));
        b.bases = (const char *) h_bases;
        b.n_bytes = acc_bytes;
        b.n_reads = acc_reads;
        if (same_len && first_len > 0) {
            b.uniform_length = first_len;
        } else {
            uint32_t *arr = (uint32_t *) (h_bases - 12ull * acc_reads);
            memcpy(arr, w->tmp_woff.data(), acc_reads * 4);
            memcpy(arr + acc_reads, w->tmp_off.data(), acc_reads * 4);
            memcpy(arr + 2 * acc_reads, w->tmp_len.data(), acc_reads * 4);
            b.word_offsets = arr;
            b.byte_offsets = arr + acc_reads;
            b.lengths = arr + 2 * acc_reads;
        }
        submit_text(s, w, b, acc_bytes);
        acc_reads = acc_words = acc_bytes = 0;
        same_len = true;
        std::swap(w->slot, w->slot_b);  // two slots, two pinned buffers: fill the next batch while this one travels
        std::swap(w->h_buf, w->h_buf_b);
        h_bases = (unsigned char *) w->h_buf + 12ull * w->reads_cap;
        buffers_free = false;
        w->t_submit += secs(t3, clk::now());
    };
    for (;;) {
        const size_t item = job->next_item.fetch_add(1);
        const size_t r0 = item * job->pairs_per_item;
        if (r0 >= job->n_pairs) break;
        const size_t r1 = std::min(job->n_pairs, r0 + job->pairs_per_item);
        const clk::time_point tc = clk::now();
        for (int m = 0; m < 2; m++) cur[m].init(job->index[m].base, job->index[m].size, job->index[m].line_start((int64_t) (4 * r0), w->nl));
        w->t_scan += secs(tc, clk::now());
        int64_t first_byte[2] = {-1, -1}, last_byte[2] = {-1, -1};
        // text batches: the item is walked in pieces small enough for the copy to find the lines just scanned in cache (the
        // cursors carry on from piece to piece; locating a line from the block counts costs a scan of its 4 MiB block)
        const size_t piece = text ? (size_t) 8192 : job->pairs_per_item;
        for (size_t q0 = r0; q0 < r1; q0 += piece) {
        const size_t q1 = std::min(r1, q0 + piece);
        const clk::time_point t0 = clk::now();
        uint64_t need_words = 0, need_bytes = 0;
        for (int m = 0; m < 2; m++) {
            st[m].clear();
            nd[m].clear();
            for (size_t r = q0; r < q1; r++) {
                const int64_t a = cur[m].next(), b = cur[m].next(), x = cur[m].next(), y = cur[m].next();
                if (a < 0 || b < 0) die("internal error: the paired reader ran past the end of a file");
                (void) x;
                (void) y;  // the last record may lack its final newline(s): the sequence line is complete
                if (b - a - 1 > MAX_SEQ)  // the reference leaves pair mode unchecked
                    die("This mode is designed for short-read sequencing. Please use 'trew long'.");
                st[m].push_back(a + 1);
                nd[m].push_back(b - 1);
                const uint64_t len = (uint64_t) std::max<int64_t>(0, b - a - 1);
                need_words += 3ull * ((len + 31) / 32);
                need_bytes += len;
            }
            if (!st[m].empty()) {
                if (first_byte[m] < 0) first_byte[m] = st[m].front();
                last_byte[m] = nd[m].back();
            }
        }
        const clk::time_point t1 = clk::now();
        w->t_scan += secs(t0, t1);
        if (text) {
            const uint64_t item_reads = 2 * (uint64_t) st[0].size();
            if (acc_reads + item_reads > w->reads_cap || acc_words + need_words > w->words_cap || acc_bytes + need_bytes > bytes_cap) close_text_batch();
            if (item_reads > w->reads_cap || need_words > w->words_cap || need_bytes > bytes_cap) die("internal error: one item's pairs do not fit the slot buffer");
            if (!buffers_free) {
                const clk::time_point tw = clk::now();
                if (trew_hip_wait(c, w->slot)) hip_die(c, "trew_hip_wait");  // the slot's pinned buffer is free again
                buffers_free = true;
                w->t_wait += secs(tw, clk::now());
            }
            const clk::time_point t2 = clk::now();
            if (acc_reads == 0 && !st[0].empty()) first_len = (uint32_t) std::max<int64_t>(0, nd[0][0] - st[0][0] + 1);
            uint64_t wo = acc_words, bo = acc_bytes, rr = acc_reads;
            const int64_t safe_src[2] = {(int64_t) job->index[0].size - 288, (int64_t) job->index[1].size - 288};
            for (size_t i = 0; i < st[0].size(); i++) {
                for (int m = 0; m < 2; m++) {
                    const int64_t a = st[m][i], len64 = nd[m][i] - a + 1;
                    const uint32_t len = len64 > 0 ? (uint32_t) len64 : 0u;
                    if (len <= 256 && a <= safe_src[m])
                        copy_short_line(h_bases + bo, job->index[m].base + a, len);
                    else
                        memcpy(h_bases + bo, job->index[m].base + a, len);
                    w->tmp_woff[rr] = (uint32_t) wo;
                    w->tmp_off[rr] = (uint32_t) bo;
                    w->tmp_len[rr] = len;
                    rr++;
                    same_len = same_len && len == first_len;
                    wo += 3ull * (((uint64_t) len + 31) / 32);
                    bo += len;
                }
            }
            acc_words = wo;
            acc_bytes = bo;
            acc_reads = rr;
            w->t_pack += secs(t2, clk::now());
            if (acc_bytes >= ((uint64_t) s->cfg.batch_mib << 19)) close_text_batch();  // batch_mib of FASTQ text is about half as many sequence bytes
        } else {
            // as many pairs per batch as the slot's buffers hold
            for (size_t at = 0; at < st[0].size();) {
                size_t n = 0;
                uint64_t words = 0;
                while (at + n < st[0].size() && 2 * (n + 1) <= w->reads_cap) {
                    const uint64_t need = 3ull * (((uint64_t) (nd[0][at + n] - st[0][at + n] + 1) + 31) / 32) + 3ull * (((uint64_t) (nd[1][at + n] - st[1][at + n] + 1) + 31) / 32);
                    if (words + need > w->words_cap) break;
                    words += need;
                    n++;
                }
                if (n == 0) die("internal error: a pair does not fit the slot buffer");  // MAX_SEQ bounds a pair far below words_cap; never spin
                const clk::time_point tw = clk::now();
                if (trew_hip_wait(c, w->slot)) hip_die(c, "trew_hip_wait");  // the slot's pinned buffer is free again
                const clk::time_point t2 = clk::now();
                const uint64_t n_reads = 2 * n;
                const uint64_t nw = trew_pack_pairs(job->index[0].base, st[0].data() + at, nd[0].data() + at, job->index[1].base, st[1].data() + at, nd[1].data() + at, n,
                                                    w->h_buf + 2 * n_reads, w->words_cap, w->h_buf, w->h_buf + n_reads);
                const clk::time_point t3 = clk::now();
                submit_packed(s, w, w->h_buf + 2 * n_reads, w->h_buf, w->h_buf + n_reads, n_reads, nw);
                w->t_wait += secs(tw, t2);
                w->t_pack += secs(t2, t3);
                w->t_submit += secs(t3, clk::now());
                at += n;
                std::swap(w->slot, w->slot_b);  // two slots, two pinned buffers: pack the next batch while this one travels
                std::swap(w->h_buf, w->h_buf_b);
            }
        }
        }  // pieces
        // the item's bytes are in pinned buffers: give the page-table entries of its stretch of both files back
        for (int m = 0; m < 2; m++)
            if (first_byte[m] >= 0) map_range(job->index[m], (size_t) first_byte[m], (size_t) last_byte[m], false);
    }
    if (text) close_text_batch();
    if (trew_hip_wait(c, w->slot) || trew_hip_wait(c, w->slot_b)) hip_die(c, "trew_hip_wait");
}

struct Mapping {
    void *p = MAP_FAILED;
    size_t size = 0;
    bool map(const char *name) {
        const int fd = open(name, O_RDONLY);
        if (fd < 0) open_failed(name);
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0) {
            close(fd);
            return false;
        }
        size = (size_t) st.st_size;
        p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (p == MAP_FAILED) return false;
        (void) madvise(p, size, MADV_SEQUENTIAL);
        (void) madvise(p, size, MADV_WILLNEED);
        return true;
    }
    ~Mapping() {
        if (p != MAP_FAILED) munmap(p, size);
    }
};

// false when a file cannot be mapped: the caller falls back to the serial reader
static bool run_pair_blocks(Scanner *s, const char *name1, const char *name2) {
    typedef std::chrono::steady_clock clk;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const clk::time_point t0 = clk::now();
    {
        Mapping m1, m2;
        if (!m1.map(name1) || !m2.map(name2)) return false;
        PairJob job;
        job.index[0].init((const char *) m1.p, m1.size, (size_t) LENGTH);
        job.index[1].init((const char *) m2.p, m2.size, (size_t) LENGTH);
        {
            std::vector<std::thread> th;
            for (size_t i = 0; i < s->workers.size(); i++) th.emplace_back(pair_count_loop, &job);
            for (auto &t : th) t.join();
        }
        job.index[0].finish();
        job.index[1].finish();
        const long long num1 = job.index[0].total(), num2 = job.index[1].total();
        if (num1 != num2) {  // kmer.cpp:1112-1114
            fprintf(stderr, "Error: Mismatched record counts between files (num1: %lld, num2: %lld).\n", num1, num2);
            fflush(stdout);
            fflush(stderr);
            _exit(EXIT_FAILURE);
        }
        job.n_pairs = (size_t) ((num1 + 2) / 4);  // sequence lines closed by a newline: line numbers 1, 5, 9, ...
        if (const char *e = getenv("TREW_PAIR_ITEM")) job.pairs_per_item = (size_t) std::max(1L, atol(e));  // experiments
        const clk::time_point t1 = clk::now();
        std::vector<std::thread> th;
        for (auto &w : s->workers) th.emplace_back(pair_worker_loop, s, &w, &job);
        for (auto &t : th) t.join();
        const clk::time_point t2 = clk::now();
        s->t_map = secs(t0, t1);  // mapping + the counting pass over both files
        s->t_workers = secs(t1, t2);
        s->t_unmap = -secs(t0, t2);  // completed below, once the mappings are gone
    }
    s->t_unmap += secs(t0, clk::now());
    return true;
}

// maps the file and runs the block workers; false when the file cannot be mapped (empty file, special file):
// the caller falls back to the serial reader
static bool run_blocks(Scanner *s, const char *name, bool long_mode, int slice_length) {
    typedef std::chrono::steady_clock clk;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const clk::time_point t0 = clk::now();
    {
        Mapping m;
        if (!m.map(name)) return false;
        BlockJob job;
        // Blocks the workers claim: the reference's chunk size (LENGTH, 4 MiB).  Smaller blocks were measured on the GPU box
        // (TREW_SCAN_BLOCK_KIB, profiles/r03/README.md) in the hope that the copy of the sequence lines would still find the
        // block in L2: 2 MiB is 10 % slower, 1 MiB 35 %, 256 KiB five times -- one madvise pair and one hand-over of the line
        // count per block cost more than the cache misses they save.
        size_t blk = (size_t) LENGTH;
        if (const char *e = getenv("TREW_SCAN_BLOCK_KIB")) {
            const long v = atol(e);
            if (v >= 64 && v <= 4096) blk = (size_t) v << 10;
        }
        job.scan.init((const char *) m.p, m.size, blk);
        job.scan.populate = true;
        job.long_mode = long_mode;
        job.slice_length = slice_length;
        const clk::time_point t1 = clk::now();
        std::vector<std::thread> th;
        for (auto &w : s->workers) th.emplace_back(block_worker_loop, s, &w, &job);
        for (auto &t : th) t.join();
        const clk::time_point t2 = clk::now();
        s->t_map = secs(t0, t1);
        s->t_workers = secs(t1, t2);
        s->t_unmap = -secs(t0, t2);  // completed below, once the mapping is gone
    }
    s->t_unmap += secs(t0, clk::now());
    return true;
}

// The same for block-gzip input (round 4): the decompressed stream is given an address range of its own (reserved, not
// committed); a block is a group of consecutive members with ~4 MiB of text, and the worker that claims it inflates its
// members into their place before it scans them (BlockScan::fill) -- inflate, newline scan, line copy and submit all run on the
// workers, nothing is serial but the chain of line counts.  false when the file is not BGZF from end to end (a plain gzip
// member, trailing bytes, a damaged member: the serial reader handles or reports those as before) or cannot be mapped.
static bool run_blocks_bgzf(Scanner *s, const char *name, bool long_mode, int slice_length) {
    typedef std::chrono::steady_clock clk;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const clk::time_point t0 = clk::now();
    {
        Mapping m;
        if (!m.map(name)) return false;
        BgzfIndex idx;
        std::string why;
        if (!idx.build((const unsigned char *) m.p, m.size, &why)) return false;
        if (idx.text_size == 0) return true;  // nothing in it
        const size_t span = (size_t) idx.text_size + 8192;
        void *text = mmap(nullptr, span, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (text == MAP_FAILED) return false;
        std::vector<size_t> bounds, first_member;
        size_t acc = 0;
        for (size_t i = 0; i < idx.members.size(); i++) {
            if (i == 0 || acc >= (size_t) LENGTH - 65536) {
                bounds.push_back((size_t) idx.members[i].toff);
                first_member.push_back(i);
                acc = 0;
            }
            acc += idx.members[i].isize;
        }
        bounds.push_back((size_t) idx.text_size);
        first_member.push_back(idx.members.size());
        BlockJob job;
        job.scan.init_bounds((const char *) text, (size_t) idx.text_size, bounds);
        job.scan.anonymous = true;
        job.scan.fill = [&](size_t b, size_t, size_t) {
            for (size_t i = first_member[b]; i < first_member[b + 1]; i++)
                if (!idx.inflate_member((const unsigned char *) m.p, i, (unsigned char *) text + idx.members[i].toff)) {
                    fprintf(stderr, "File-IO Error: BGZF member fails to inflate (data error).\n");  // as the serial reader reports it (kmer.cpp:1021-1022)
                    fflush(stdout);
                    fflush(stderr);
                    _exit(EXIT_FAILURE);
                }
        };
        job.long_mode = long_mode;
        job.slice_length = slice_length;
        const clk::time_point t1 = clk::now();
        std::vector<std::thread> th;
        for (auto &w : s->workers) th.emplace_back(block_worker_loop, s, &w, &job);
        for (auto &t : th) t.join();
        const clk::time_point t2 = clk::now();
        munmap(text, span);
        s->t_map = secs(t0, t1);
        s->t_workers = secs(t1, t2);
        s->t_unmap = -secs(t0, t2);
    }
    s->t_unmap += secs(t0, clk::now());
    return true;
}

// thread merge of process_output (kmer.cpp:1486-1515): what was drained during the file + what the devices
// still hold.  With several devices the tables are first reduced on the GPUs (trew_hip_merge, one peer copy
// per device) and only the merged rows cross PCIe.
static ResultMapData collect_tables(Scanner *s) {
    for (size_t d = 1; d < s->dev.size(); d++) {
        // Mid-file drains only keep EACH device at or below half full; the union of several devices' keys can exceed
        // device 0's partitions plus its spill log.  So device 0 is emptied into host memory whenever it is under
        // pressure before it takes another device's rows (no worker is running any more: no lock needed).
        if (under_pressure(s->dev[0]->ctx)) {
            drain_device(s, s->dev[0].get());
            s->drains++;
        }
        if (trew_hip_merge(s->dev[0]->ctx, s->dev[d]->ctx)) hip_die(s->dev[0]->ctx, "trew_hip_merge");
        if (trew_hip_reset_tables(s->dev[d]->ctx)) hip_die(s->dev[d]->ctx, "trew_hip_reset_tables");
    }
    drain_device(s, s->dev[0].get());
    ResultMapData r;
    std::lock_guard<std::mutex> lk(s->pending_mu);
    std::swap(r, s->pending);
    return r;
}

static FinalFastqOutput run_file(Scanner *s, const Config &cfg, const char *name1, const char *name2, bool gz1, bool gz2) {
    const auto t0 = std::chrono::steady_clock::now();
    for (auto &w : s->workers) {
        w.reads = 0;
        w.bases = 0;
        w.t_scan = w.t_wait = w.t_pack = w.t_submit = w.t_pressure = 0;
        w.submits = 0;
    }
    const uint64_t drains0 = s->drains;
    bool done = false;
    const char *how = "serial reader";
    if (s->mode != TREW_MODE_PAIR && !gz1 && !cfg.serial_reader) {
        done = run_blocks(s, name1, s->mode == TREW_MODE_LONG, cfg.SLICE_LENGTH);
        if (done) how = "block-parallel reader";
    } else if (s->mode != TREW_MODE_PAIR && gz1 && !cfg.serial_reader && BgzfReader::sniff(name1)) {
        done = run_blocks_bgzf(s, name1, s->mode == TREW_MODE_LONG, cfg.SLICE_LENGTH);
        if (done) how = "block-parallel BGZF reader";
    } else if (s->mode == TREW_MODE_PAIR && !gz1 && !gz2 && !cfg.serial_reader) {
        done = run_pair_blocks(s, name1, name2);
        if (done) how = "block-parallel paired reader";
    }
    if (!done) {
        size_t qcap = cfg.QUEUE_SIZE >= 4 ? (size_t) (cfg.QUEUE_SIZE / 4) : 256;  // kmer.cpp:1274-1276; "unlimited" is capped at 1 GiB
        ChunkQueue q(qcap);
        std::vector<std::thread> th;
        for (auto &w : s->workers) th.emplace_back(worker_loop, s, &w, &q);
        const int inflaters = s->mode == TREW_MODE_PAIR ? std::max(2, cfg.NUM_THREAD / 2) : cfg.NUM_THREAD;
        FileReader f1 = open_reader(name1, gz1, inflaters);
        if (s->mode == TREW_MODE_PAIR) {
            FileReader f2 = open_reader(name2, gz2, inflaters);
            read_pair_fastq_thread(f1, f2, &q);
            f2.close();
        } else {
            read_fastq_thread(f1, &q);
        }
        f1.close();
        for (size_t i = 0; i < s->workers.size(); i++) {  // sentinels, kmer.cpp:1304-1310
            Chunk *c = new Chunk();
            c->sentinel = true;
            q.push(c);
        }
        for (auto &t : th) t.join();
    }
    const auto tc0 = std::chrono::steady_clock::now();
    ResultMapData r = collect_tables(s);
    s->t_collect = std::chrono::duration<double>(std::chrono::steady_clock::now() - tc0).count();
    s->stats = RunStats();
    for (auto &w : s->workers) {
        s->stats.reads += w.reads;
        s->stats.bases += w.bases;
    }
    s->stats.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (cfg.stats)
        fprintf(stderr, "[trew] %s: %llu reads, %llu bases, %.3f s, %.3f Gbases/s end-to-end (decode + pack + scan; %s, %d worker(s), %llu table drain(s))\n",
                name1, (unsigned long long) s->stats.reads, (unsigned long long) s->stats.bases, s->stats.seconds,
                s->stats.bases / s->stats.seconds / 1e9, how, (int) s->workers.size(), (unsigned long long) (s->drains - drains0));
    if (cfg.stats && done) {
        double a = 0, b = 0, c = 0, d = 0, e = 0;
        uint64_t nsub = 0;
        for (auto &w : s->workers) a += w.t_scan, b += w.t_wait, c += w.t_pack, d += w.t_submit, e += w.t_pressure, nsub += w.submits;
        const double n = (double) s->workers.size();
        fprintf(stderr,
                "[trew]   per worker (mean seconds): newline scan + line chain %.3f, wait for the slot %.3f, pack %.3f, submit %.3f (of which table "
                "pressure query %.3f); %llu batches\n",
                a / n, b / n, c / n, d / n, e / n, (unsigned long long) nsub);
        fprintf(stderr, "[trew]   wall seconds: map the file %.3f, workers %.3f, unmap %.3f, collect the tables %.3f\n", s->t_map, s->t_workers, s->t_unmap, s->t_collect);
    }
    return process_output(name1, r, cfg.MIN_MER, stdout);  // pair mode prints file 1 only (kmer.cpp:1409)
}

FinalFastqOutput process_kmer(Scanner *s, const Config &cfg, const char *file_name, bool is_gz) {
    return run_file(s, cfg, file_name, nullptr, is_gz, false);
}
FinalFastqOutput process_kmer_pair(Scanner *s, const Config &cfg, const char *file_name1, const char *file_name2, bool is_gz1, bool is_gz2) {
    return run_file(s, cfg, file_name1, file_name2, is_gz1, is_gz2);
}
FinalFastqOutput process_kmer_long(Scanner *s, const Config &cfg, const char *file_name, bool is_gz) {
    return run_file(s, cfg, file_name, nullptr, is_gz, false);
}

// ---------------------------------------------------------------- trew annotate, tracts, intervals, variants, periods, chain, repeats, satellites, align, refine, tandems, trace, decompose, dissect, resolve, monomers, copies, polish
// A per-read measure of one FASTQ file (plain or .gz) through the serial reader shape: read_fastq_thread hands out
// 4 MiB chunks, every worker finds the sequence lines of its chunk, packs them, queues the measure that AnnotRequest::kind
// names on a slot of its own, fetches the records and folds them into its part of the file's result (fold_annotate,
// fold_tracts, fold_intervals, fold_variants, fold_periods, fold_chain, fold_repeats, fold_satellites, fold_align, fold_refine, fold_tandems, fold_trace, fold_decompose, fold_dissect, fold_resolve, fold_monomers, fold_copies, fold_polish).  The ordinal of a read is the index of its sequence line among the file's
// sequence lines: Chunk::num_before (newlines in front of the chunk) gives the ordinal of the chunk's first read, so the rows
// come out the same for any number of workers once they are sorted.
struct Annotator {
    std::vector<trew_hip_ctx *> ctx;
    struct Worker {
        int dev_index = 0, slot = 0;
        uint32_t *h_buf = nullptr;  // pinned: [offsets n][lengths n][words]
        // One buffer per role, not per measure: a request names one measure, so a worker holds one kind of record at a time.
        void *recs = nullptr;                  // the fixed-size records or the log of the batch at hand (records<T>), malloc'ed
        size_t recs_bytes = 0;
        std::vector<uint32_t> counts;          // intervals, chain: the counts per (read, motif, strand)
        std::vector<uint64_t> vhist;           // variants: hist, then reads_with, of one batch
        std::vector<trew_hip_alignment> arecs; // trace: the alignment records that come with its items
        std::vector<trew_hip_refined> drecs;   // decompose: the refined records that come with its items
        std::vector<trew_hip_tandem> trecs;    // dissect: the records that come with its items
        AnnotFileResult part;
        std::vector<uint32_t> nl;
        std::vector<int64_t> st, nd;
    };
    std::vector<Worker> workers;
    uint64_t words_cap = 0, reads_cap = 0;
};

Annotator *annotator_create(const Config &cfg) {
    Annotator *a = new Annotator();
    const int n_workers = std::max(1, cfg.NUM_THREAD - 1);  // the caller's thread is the reader
    const int ndev = (int) cfg.devices.size();
    a->reads_cap = 1ull << 20;                                               // a 4 MiB chunk holds fewer FASTQ records than this
    a->words_cap = 3ull * ((uint64_t) LENGTH / 32 + a->reads_cap) + 64;      // every read may waste up to one triple of padding
    std::vector<int> slots_on_dev((size_t) ndev, 0);
    for (int w = 0; w < n_workers; w++) slots_on_dev[(size_t) (w % ndev)]++;
    for (int d = 0; d < ndev; d++) {
        trew_hip_params p;
        memset(&p, 0, sizeof(p));
        p.min_mer = 5;  // the scan's parameters only shape the scan; the annotation does not read them
        p.max_mer = 32;
        p.low_baseline = 0.5;
        p.high_baseline = 0.8;
        p.slice_length = 150;
        p.mode = TREW_MODE_SHORT;
        p.device = cfg.devices[(size_t) d];
        p.n_slots = std::max(1, slots_on_dev[(size_t) d]);
        p.max_batch_words = a->words_cap;
        p.max_batch_reads = a->reads_cap;
        p.table_log2_slots = 12;  // no scan: the smallest table there is
        p.flags = TREW_FLAG_NO_TIMING;
        trew_hip_ctx *c = nullptr;
        if (trew_hip_init(&p, &c) != 0) die(trew_hip_last_error(nullptr));
        a->ctx.push_back(c);
    }
    std::vector<int> next_slot((size_t) ndev, 0);
    a->workers.resize((size_t) n_workers);
    for (int w = 0; w < n_workers; w++) {
        Annotator::Worker &wk = a->workers[(size_t) w];
        wk.dev_index = w % ndev;
        wk.slot = next_slot[(size_t) wk.dev_index]++;
        trew_hip_ctx *c = a->ctx[(size_t) wk.dev_index];
        if (trew_hip_host_alloc(c, (a->words_cap + 2 * a->reads_cap) * 4, (void **) &wk.h_buf)) hip_die(c, "pinned allocation");
    }
    return a;
}

void annotator_destroy(Annotator *a) {
    if (!a) return;
    for (auto &w : a->workers) {
        trew_hip_host_free(a->ctx[(size_t) w.dev_index], w.h_buf);
        free(w.recs);
    }
    for (auto c : a->ctx) trew_hip_destroy(c);
    delete a;
}

// one packed chunk on its way through a worker's slot
struct AnnotBatch {
    trew_hip_ctx *c;
    Annotator::Worker *w;
    const AnnotRequest *rq;
    trew_hip_batch b;
    const uint32_t *lengths;
    uint64_t n, first_read;  // reads of the chunk, ordinal of the first
    const char *text;        // the chunk: read r is text[w->st[r] .. w->nd[r]]
};

// The worker's record buffer as room for n records of T.  It only grows, and nothing of an earlier batch is kept: every fold
// reads only what the results call of its batch wrote.
template <class T>
static T *records(Annotator::Worker *w, uint64_t n) {
    static_assert(std::is_trivially_copyable<T>::value && alignof(T) <= alignof(std::max_align_t), "plain records of the C ABI");
    if (w->recs_bytes < n * sizeof(T)) {
        free(w->recs);
        w->recs_bytes = 0;
        if (!(w->recs = malloc(n * sizeof(T)))) die("out of memory");
        w->recs_bytes = n * sizeof(T);
    }
    return static_cast<T *>(w->recs);
}

// The "queue, size the buffer, fetch, retry once with the exact numbers or die" loop of the six measures with a log.  queue(room)
// queues the measure with a log (and, trace, a workspace) of `room`; fetch(room) fetches into buffers of that size and returns
// what the batch needs, which the library reports exactly also when it did not fit -- so one retry always suffices, and a
// second overflow is a bug (`twice`).  Returns what was found.
struct LogRoom {
    uint64_t log, rows;   // records (chain: events) of the log; rows of trace's workspace, 0 for the others
    uint64_t tracts = 0;  // dissect: the records of its second log, 0 for the others
};
template <class Queue, class Fetch>
static LogRoom fetch_with_retry(AnnotFileResult &p, LogRoom room, const char *twice, Queue queue, Fetch fetch) {
    for (int attempt = 0;; attempt++) {
        queue(room);
        const LogRoom need = fetch(room);
        if (need.log <= room.log && need.rows <= room.rows && need.tracts <= room.tracts) return need;
        if (attempt) die(twice);
        room = LogRoom{std::max(room.log, need.log), std::max(room.rows, need.rows), std::max(room.tracts, need.tracts)};
        p.interval_retries++;
    }
}

static AnnotRow annot_row(const AnnotBatch &x, uint64_t r, int m) {
    AnnotRow row;
    row.read = x.first_read + r;
    row.length = x.lengths[r];
    row.motif = m;
    return row;
}

// trew annotate.  windows_fwd / windows_rev: the matching windows of each strand; longest: the longest tract of either
// strand; reported: the (read, motif) whose longer tract reaches MIN_TRACT, which are the rows.
static void fold_annotate(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    if (trew_hip_annotate(x.c, &x.b, w->slot, x.rq->motifs, nm)) hip_die(x.c, "trew_hip_annotate");
    trew_hip_annot *recs = records<trew_hip_annot>(w, x.n * (uint64_t) nm);
    uint64_t got = 0;
    if (trew_hip_annotate_results(x.c, w->slot, recs, x.n * (uint64_t) nm, &got, nullptr)) hip_die(x.c, "trew_hip_annotate_results");
    for (uint64_t r = 0; r < x.n; r++)
        for (int m = 0; m < nm; m++) {
            const trew_hip_annot &rec = recs[r * (size_t) nm + (size_t) m];
            const uint32_t longest = std::max(rec.tract_len_fwd, rec.tract_len_rev);
            p.windows_fwd[m] += rec.windows_fwd;
            p.windows_rev[m] += rec.windows_rev;
            p.longest[m] = std::max(p.longest[m], longest);
            if (longest >= x.rq->min_tract[m]) {
                p.reported[m]++;
                p.rows.push_back(annot_row(x, r, m));
                p.rows.back().a = rec;
            }
        }
}

// trew tracts.  windows_fwd / windows_rev: the covered bases of each strand; longest / longest_tail: the longest head / tail
// tract of either strand; reported: the (read, motif) whose longest of the four tracts reaches MIN_TRACT, which are the rows.
static void fold_tracts(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    if (trew_hip_tracts(x.c, &x.b, w->slot, x.rq->motifs, nm, x.rq->penalty)) hip_die(x.c, "trew_hip_tracts");
    trew_hip_tract *recs = records<trew_hip_tract>(w, x.n * (uint64_t) nm);
    uint64_t got = 0;
    if (trew_hip_tracts_results(x.c, w->slot, recs, x.n * (uint64_t) nm, &got, nullptr)) hip_die(x.c, "trew_hip_tracts_results");
    for (uint64_t r = 0; r < x.n; r++)
        for (int m = 0; m < nm; m++) {
            const trew_hip_tract &rec = recs[r * (size_t) nm + (size_t) m];
            const uint32_t head = std::max(rec.head_len_fwd, rec.head_len_rev), tail = std::max(rec.tail_len_fwd, rec.tail_len_rev);
            p.windows_fwd[m] += rec.covered_fwd;
            p.windows_rev[m] += rec.covered_rev;
            p.longest[m] = std::max(p.longest[m], head);
            p.longest_tail[m] = std::max(p.longest_tail[m], tail);
            if (std::max(head, tail) >= x.rq->min_tract[m]) {
                p.reported[m]++;
                p.rows.push_back(annot_row(x, r, m));
                p.rows.back().t = rec;
            }
        }
}

// trew intervals: a variable number of records, every one a row (min_len is part of the kernel's rule).  windows_fwd /
// windows_rev: the kept intervals of each strand; longest / longest_tail: the longest one of the forward / reverse strand;
// reported: the reads with at least one; terminal_s: the intervals that touch an end of their read.  The log starts at one
// record per read; a batch whose log overflows is resubmitted once, with the exact number.
static void fold_intervals(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    if (w->counts.size() < x.n * (size_t) nm * 2) w->counts.resize(x.n * (size_t) nm * 2);
    const uint64_t found = fetch_with_retry(
        p, LogRoom{x.n, 0}, "internal error: the interval log overflowed twice",
        [&](LogRoom room) {
            if (trew_hip_intervals(x.c, &x.b, w->slot, x.rq->motifs, x.rq->rules, nm, room.log)) hip_die(x.c, "trew_hip_intervals");
        },
        [&](LogRoom room) {
            uint64_t n = 0;
            if (trew_hip_intervals_results(x.c, w->slot, records<trew_hip_interval>(w, room.log), room.log, &n, w->counts.data(), nullptr))
                hip_die(x.c, "trew_hip_intervals_results");
            return LogRoom{n, 0};
        }).log;
    const trew_hip_interval *recs = static_cast<const trew_hip_interval *>(w->recs);
    for (uint64_t r = 0; r < x.n; r++)
        for (int m = 0; m < nm; m++)
            if (w->counts[(r * (size_t) nm + (size_t) m) * 2] + w->counts[(r * (size_t) nm + (size_t) m) * 2 + 1]) p.reported[m]++;
    for (uint64_t i = 0; i < found; i++) {
        const trew_hip_interval &rec = recs[i];
        const uint32_t len = x.lengths[rec.read];
        const bool terminal = rec.start == 0 || rec.end == len;
        if (rec.strand) {
            p.windows_rev[rec.motif]++;
            p.longest_tail[rec.motif] = std::max(p.longest_tail[rec.motif], rec.end - rec.start);
            p.terminal_rev[rec.motif] += terminal;
        } else {
            p.windows_fwd[rec.motif]++;
            p.longest[rec.motif] = std::max(p.longest[rec.motif], rec.end - rec.start);
            p.terminal_fwd[rec.motif] += terminal;
        }
        p.irows.push_back(IntervalRow{x.first_read + rec.read, len, rec});
    }
}

// trew variants: one record per (read, motif) and the batch's two histograms.  windows_fwd / windows_rev: the exact units
// of each strand; variants_s: the anchored variant units; reported: the (read, motif) whose larger units_s + variants_s
// reaches MIN_UNITS (AnnotRequest::min_tract), which are the rows; var_hist / var_reads_with: the histograms summed over the
// batches, over all reads and not only the reported ones.
static void fold_variants(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    const size_t hl = (size_t) nm * 2 * TREW_VARIANT_BINS;
    if (trew_hip_variants(x.c, &x.b, w->slot, x.rq->motifs, nm)) hip_die(x.c, "trew_hip_variants");
    trew_hip_variant *recs = records<trew_hip_variant>(w, x.n * (uint64_t) nm);
    w->vhist.resize(2 * hl);
    uint64_t got = 0;
    if (trew_hip_variants_results(x.c, w->slot, recs, x.n * (uint64_t) nm, &got, w->vhist.data(), w->vhist.data() + hl, nullptr))
        hip_die(x.c, "trew_hip_variants_results");
    p.var_hist.resize(hl);
    p.var_reads_with.resize(hl);
    for (size_t i = 0; i < hl; i++) {
        p.var_hist[i] += w->vhist[i];
        p.var_reads_with[i] += w->vhist[hl + i];
    }
    for (uint64_t r = 0; r < x.n; r++)
        for (int m = 0; m < nm; m++) {
            const trew_hip_variant &rec = recs[r * (size_t) nm + (size_t) m];
            p.windows_fwd[m] += rec.units_fwd;
            p.windows_rev[m] += rec.units_rev;
            p.variants_fwd[m] += rec.variants_fwd;
            p.variants_rev[m] += rec.variants_rev;
            const uint64_t most = std::max((uint64_t) rec.units_fwd + rec.variants_fwd, (uint64_t) rec.units_rev + rec.variants_rev);
            if (most >= x.rq->min_tract[m]) {
                p.reported[m]++;
                p.rows.push_back(annot_row(x, r, m));
                p.rows.back().v = rec;
            }
        }
}

uint64_t canonical_unit(uint64_t unit, int k) {
    return (uint64_t) std::min(get_rot_seq_128(unit, k), get_rot_seq_128(reverse_complement_k(unit, k), k));
}

// trew periods: one record per read and no motif.  A read with a record (period > 0) is a row; period_units counts the
// reads and the bases of their tracts per (period, strand-canonical unit).
static void fold_periods(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const AnnotRequest &rq = *x.rq;
    if (trew_hip_periods(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score)) hip_die(x.c, "trew_hip_periods");
    trew_hip_period *recs = records<trew_hip_period>(w, x.n);
    uint64_t got = 0;
    if (trew_hip_periods_results(x.c, w->slot, recs, x.n, &got, nullptr)) hip_die(x.c, "trew_hip_periods_results");
    for (uint64_t r = 0; r < x.n; r++) {
        const trew_hip_period &rec = recs[r];
        if (rec.period == 0) continue;
        auto &u = p.period_units[{rec.period, canonical_unit(rec.unit, (int) rec.period)}];
        u.first++;
        u.second += rec.end - rec.start;
        p.rows.push_back(annot_row(x, r, 0));
        p.rows.back().p = rec;
    }
}

// trew chain: a variable number of items.  windows_fwd / windows_rev: the exact units of each strand (the sum of the runs'
// counts); variants_s: the variant items; runs_s: the runs; longest / longest_tail: the longest run in units of the forward /
// reverse strand; reported / reported_rev: the (read, motif) whose units + variants on that strand reach MIN_UNITS
// (AnnotRequest::min_tract) -- only their items become rows.  The log starts at four events per read; a batch whose log
// overflows is resubmitted once, with the exact number.
static void fold_chain(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    uint64_t items = 0;
    if (w->counts.size() < x.n * (size_t) nm * 4) w->counts.resize(x.n * (size_t) nm * 4);
    fetch_with_retry(
        p, LogRoom{4 * x.n, 0}, "internal error: the chain log overflowed twice",
        [&](LogRoom room) {
            if (trew_hip_chain(x.c, &x.b, w->slot, x.rq->motifs, nm, room.log)) hip_die(x.c, "trew_hip_chain");
        },
        [&](LogRoom room) {
            // an item takes at least one event, so a log that fitted holds at most room.log items
            uint64_t events = 0;
            if (trew_hip_chain_results(x.c, w->slot, records<trew_hip_chain_item>(w, room.log), room.log, &items, &events, w->counts.data(), nullptr))
                hip_die(x.c, "trew_hip_chain_results");
            return LogRoom{events, 0};
        });
    const trew_hip_chain_item *recs = static_cast<const trew_hip_chain_item *>(w->recs);
    // the items are sorted by (read, motif, strand, start): a key's items are consecutive
    for (uint64_t i = 0; i < items;) {
        const trew_hip_chain_item &first = recs[i];
        uint64_t j = i, units = 0, nvar = 0;
        uint32_t longest = 0;
        for (; j < items && recs[j].read == first.read && recs[j].motif == first.motif && recs[j].strand == first.strand; j++) {
            const trew_hip_chain_item &it = recs[j];
            if (it.bin == TREW_VARIANT_NONE) {
                units += it.count;
                longest = std::max(longest, it.count);
            } else {
                nvar++;
            }
        }
        const uint32_t m = first.motif;
        (first.strand ? p.windows_rev : p.windows_fwd)[m] += units;
        (first.strand ? p.variants_rev : p.variants_fwd)[m] += nvar;
        (first.strand ? p.runs_rev : p.runs_fwd)[m] += (j - i) - nvar;
        uint32_t &lg = (first.strand ? p.longest_tail : p.longest)[m];
        lg = std::max(lg, longest);
        if (units + nvar >= x.rq->min_tract[m]) {
            (first.strand ? p.reported_rev : p.reported)[m]++;
            for (uint64_t q = i; q < j; q++) p.crows.push_back(ChainRow{x.first_read + first.read, x.lengths[first.read], recs[q]});
        }
        i = j;
    }
}

// The unit tally of repeats, satellites and tandems: per key -- key_of(record): (period, strand-canonical unit) -- the reads
// that have such a tract, the tracts and their bases.  The records are sorted by (read, start), so a read's tracts are
// consecutive and `seen` holds the keys of the read at hand.  each(record, unit): what the measure does with a record besides
// (its row; tandems: the copies).
template <class Rec, class Map, class KeyOf, class Each>
static void tally_units(const Rec *recs, uint64_t found, Map &units, KeyOf key_of, Each each) {
    std::vector<typename Map::key_type> seen;
    for (uint64_t i = 0; i < found; i++) {
        const Rec &rec = recs[i];
        if (i == 0 || recs[i - 1].read != rec.read) seen.clear();
        const typename Map::key_type key = key_of(rec);
        auto &u = units[key];
        if (std::find(seen.begin(), seen.end(), key) == seen.end()) {
            seen.push_back(key);
            u.reads++;
        }
        u.tracts++;
        u.bases += rec.end - rec.start;
        each(rec, u);
    }
}

// What repeats, satellites and tandems share: their queue and results calls differ in the record type only.  The log starts at
// one record per read; a batch whose log overflows is resubmitted once, with the exact number.  Then tally_units.
template <class Rec, class Queue, class Map, class KeyOf, class Each>
static void fold_tract_log(const AnnotBatch &x, AnnotFileResult &p, const char *queue_name, const char *results_name, const char *twice,
                           Queue queue,  // the queue call: (ctx, batch, slot, min_period, max_period, penalty, min_score, max_records)
                           int (*results)(trew_hip_ctx *, int, Rec *, uint64_t, uint64_t *, uint32_t *, float *), Map &units, KeyOf key_of, Each each) {
    Annotator::Worker *w = x.w;
    const AnnotRequest &rq = *x.rq;
    const uint64_t found = fetch_with_retry(
        p, LogRoom{x.n, 0}, twice,
        [&](LogRoom room) {
            if (queue(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score, room.log)) hip_die(x.c, queue_name);
        },
        [&](LogRoom room) {
            uint64_t n = 0;
            if (results(x.c, w->slot, records<Rec>(w, room.log), room.log, &n, nullptr, nullptr)) hip_die(x.c, results_name);
            return LogRoom{n, 0};
        }).log;
    tally_units(static_cast<const Rec *>(w->recs), found, units, key_of, each);
}

// trew repeats: a variable number of records and no motif; every record is a row.  repeat_units counts per (period,
// strand-canonical unit) the reads that have such a tract, the tracts and their bases.
static void fold_repeats(const AnnotBatch &x, AnnotFileResult &p) {
    fold_tract_log<trew_hip_repeat>(
        x, p, "trew_hip_repeats", "trew_hip_repeats_results", "internal error: the repeat log overflowed twice", trew_hip_repeats, trew_hip_repeats_results, p.repeat_units,
        [](const trew_hip_repeat &rec) { return std::pair<uint32_t, uint64_t>{rec.period, canonical_unit(rec.unit, (int) rec.period)}; },
        [&](const trew_hip_repeat &rec, RepeatUnit &) { p.rrows.push_back(RepeatRow{x.first_read + rec.read, x.lengths[rec.read], rec}); });
}

// trew satellites: fold_repeats with the wide record; the key's unit is a string of codes.
static void fold_satellites(const AnnotBatch &x, AnnotFileResult &p) {
    fold_tract_log<trew_hip_satellite>(
        x, p, "trew_hip_satellites", "trew_hip_satellites_results", "internal error: the satellite log overflowed twice", trew_hip_satellites, trew_hip_satellites_results,
        p.satellite_units, [](const trew_hip_satellite &rec) { return std::pair<uint32_t, std::string>{rec.period, satellite_canonical(satellite_codes(rec))}; },
        [&](const trew_hip_satellite &rec, RepeatUnit &) { p.srows.push_back(SatelliteRow{x.first_read + rec.read, x.lengths[rec.read], rec}); });
}

// trew tandems: fold_repeats with the refined record; every record is a row (the kernel stores only those that reach MIN_SCORE).
// tandem_units counts per (period, strand-canonical unit) the reads that have such a tract, the tracts, their bases and copies.
// --candidates above 1: trew_hip_tandems_resolved queues, the results call is the same.
static void fold_tandems(const AnnotBatch &x, AnnotFileResult &p) {
    const int candidates = x.rq->candidates;
    auto queue = [candidates](trew_hip_ctx *c, const trew_hip_batch *b, int slot, int min_period, int max_period, int penalty, uint32_t min_score,
                              uint64_t max_records) {
        return candidates == 1 ? trew_hip_tandems(c, b, slot, min_period, max_period, penalty, min_score, max_records)
                               : trew_hip_tandems_resolved(c, b, slot, min_period, max_period, penalty, min_score, candidates, max_records);
    };
    fold_tract_log<trew_hip_tandem>(
        x, p, candidates == 1 ? "trew_hip_tandems" : "trew_hip_tandems_resolved", "trew_hip_tandems_results", "internal error: the tandem log overflowed twice",
        queue, trew_hip_tandems_results, p.tandem_units,
        [](const trew_hip_tandem &rec) { return std::pair<uint32_t, uint64_t>{rec.period, canonical_unit(rec.unit, (int) rec.period)}; },
        [&](const trew_hip_tandem &rec, TandemUnit &u) {
            u.copies += rec.consumed / rec.period;
            p.trows.push_back(TandemRow{x.first_read + rec.read, x.lengths[rec.read], rec});
        });
}

// A row per (read, motif, strand) of `recs` whose score reaches MIN_SCORE; align_sums: the sums over those rows.  What trew
// align and trew monomers print, and trew trace from the records that come with its items.
static void align_rows(const AnnotBatch &x, const trew_hip_alignment *recs, AnnotFileResult &p) {
    const int nm = x.rq->n_motifs;
    for (uint64_t r = 0; r < x.n; r++)
        for (int m = 0; m < nm; m++) {
            const trew_hip_alignment &rec = recs[r * (size_t) nm + (size_t) m];
            for (int s = 0; s < 2; s++) {
                const uint32_t *f = s ? &rec.score_rev : &rec.score_fwd;  // five consecutive u32
                if (f[0] < x.rq->min_score) continue;
                AlignRow row;
                row.read = x.first_read + r;
                row.length = x.lengths[r];
                row.motif = m;
                row.strand = s;
                for (int i = 0; i < 5; i++) row.rec[i] = f[i];
                p.arows.push_back(row);
                const uint32_t k = (uint32_t) (x.rq->kind == Measure::Monomers || x.rq->kind == Measure::Copies ? x.rq->monomers[m].k : x.rq->motifs[m].k);
                const AlignColumns c = align_columns(row.rec, k, x.rq->penalty);
                const uint64_t add[kAlignSums] = {1, (uint64_t) f[2] - f[1], f[0], c.copies, f[3], f[4], c.mismatches, c.insertions, c.deletions};
                for (int i = 0; i < kAlignSums; i++) p.align_sums[m][s][i] += add[i];
            }
        }
}

// trew align: align_rows of one record per (read, motif).
static void fold_align(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    if (trew_hip_align(x.c, &x.b, w->slot, x.rq->motifs, nm, x.rq->penalty)) hip_die(x.c, "trew_hip_align");
    trew_hip_alignment *recs = records<trew_hip_alignment>(w, x.n * (uint64_t) nm);
    uint64_t got = 0;
    if (trew_hip_align_results(x.c, w->slot, recs, x.n * (uint64_t) nm, &got, nullptr)) hip_die(x.c, "trew_hip_align_results");
    align_rows(x, recs, p);
}

// trew monomers: align_rows of one record per (read, monomer).
static void fold_monomers(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    if (trew_hip_monomers(x.c, &x.b, w->slot, x.rq->monomers, nm, x.rq->penalty)) hip_die(x.c, "trew_hip_monomers");
    trew_hip_alignment *recs = records<trew_hip_alignment>(w, x.n * (uint64_t) nm);
    uint64_t got = 0;
    if (trew_hip_monomers_results(x.c, w->slot, recs, x.n * (uint64_t) nm, &got, nullptr)) hip_die(x.c, "trew_hip_monomers_results");
    align_rows(x, recs, p);
}

// trew refine: one record per read and no motif.  A read whose final score reaches MIN_SCORE is a row; refine_units counts
// the rows, the bases of their tracts and their copies per (period, strand-canonical unit).
static void fold_refine(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const AnnotRequest &rq = *x.rq;
    if (trew_hip_refine(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score)) hip_die(x.c, "trew_hip_refine");
    trew_hip_refined *recs = records<trew_hip_refined>(w, x.n);
    uint64_t got = 0;
    if (trew_hip_refine_results(x.c, w->slot, recs, x.n, &got, nullptr)) hip_die(x.c, "trew_hip_refine_results");
    for (uint64_t r = 0; r < x.n; r++) {
        const trew_hip_refined &rec = recs[r];
        if (rec.period == 0 || rec.score < rq.min_score) continue;
        RefineUnit &u = p.refine_units[{rec.period, canonical_unit(rec.unit, (int) rec.period)}];
        u.reads++;
        u.bases += rec.end - rec.start;
        u.copies += rec.consumed / rec.period;
        p.frows.push_back(RefineRow{x.first_read + r, x.lengths[r], rec});
    }
}

// trew polish: fold_refine with the wide record; the key's unit is a string of codes, as in fold_satellites.
static void fold_polish(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const AnnotRequest &rq = *x.rq;
    if (trew_hip_polish(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score)) hip_die(x.c, "trew_hip_polish");
    trew_hip_polished *recs = records<trew_hip_polished>(w, x.n);
    uint64_t got = 0;
    if (trew_hip_polish_results(x.c, w->slot, recs, x.n, &got, nullptr)) hip_die(x.c, "trew_hip_polish_results");
    for (uint64_t r = 0; r < x.n; r++) {
        const trew_hip_polished &rec = recs[r];
        if (rec.period == 0 || rec.score < rq.min_score) continue;
        RefineUnit &u = p.polish_units[{rec.period, satellite_canonical(unit_codes(rec.unit, rec.period))}];
        u.reads++;
        u.bases += rec.end - rec.start;
        u.copies += rec.consumed / rec.period;
        p.prows.push_back(PolishRow{x.first_read + r, x.lengths[r], rec});
    }
}

// trew resolve: fold_refine with the resolved record; resolve_units also counts the rows with rank > 0.
static void fold_resolve(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const AnnotRequest &rq = *x.rq;
    if (trew_hip_resolve(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score, rq.candidates)) hip_die(x.c, "trew_hip_resolve");
    trew_hip_resolved *recs = records<trew_hip_resolved>(w, x.n);
    uint64_t got = 0;
    if (trew_hip_resolve_results(x.c, w->slot, recs, x.n, &got, nullptr)) hip_die(x.c, "trew_hip_resolve_results");
    for (uint64_t r = 0; r < x.n; r++) {
        const trew_hip_resolved &rec = recs[r];
        if (rec.period == 0 || rec.score < rq.min_score) continue;
        ResolveUnit &u = p.resolve_units[{rec.period, canonical_unit(rec.unit, (int) rec.period)}];
        u.reads++;
        u.bases += rec.end - rec.start;
        u.copies += rec.consumed / rec.period;
        u.repaired += rec.rank > 0;
        p.vrows.push_back(ResolveRow{x.first_read + r, x.lengths[r], rec});
    }
}

// One item of trace, decompose or dissect against its unit of k bases: its row, with the read bases of an item that is no run
// (the signature prints them), and the three sums of its unit: units (the copies of the items with consumed = k count), edited
// (the items with an error), items.
static void fold_item(const AnnotBatch &x, AnnotFileResult &p, const trew_hip_trace_item &it, uint32_t k, uint64_t &units, uint64_t &edited, uint64_t &items) {
    const bool errors = it.mismatches || it.insertions || it.deletions;
    if (it.consumed == k * it.count) units += it.count;
    edited += errors;
    items++;
    const bool run = it.phase == 0 && it.consumed == k * it.count && !errors;
    p.xrows.push_back(TraceRow{x.first_read + it.read, x.lengths[it.read], it,
                               run ? std::string() : std::string(x.text + x.w->st[it.read] + it.start, (size_t) it.bases)});
}

// trew trace: align_rows from the records that come with the items, and fold_item for the items of those keys, into
// trace_sums.  The workspace holds a row for every base and motif, which no batch exceeds; the log starts at sixteen items
// per read and motif, and a batch whose log overflows is resubmitted once, with the exact numbers.
static void fold_trace(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    uint64_t bases = 0;
    for (uint64_t r = 0; r < x.n; r++) bases += x.lengths[r];
    if (w->arecs.size() < x.n * (size_t) nm) w->arecs.resize(x.n * (size_t) nm);
    const uint64_t items = fetch_with_retry(
        p, LogRoom{16 * x.n * (uint64_t) nm + 1024, std::max<uint64_t>(bases * (uint64_t) nm, 1)}, "internal error: the trace log overflowed twice",
        [&](LogRoom room) {
            if (trew_hip_trace(x.c, &x.b, w->slot, x.rq->motifs, nm, x.rq->penalty, x.rq->min_score, room.log, room.rows)) hip_die(x.c, "trew_hip_trace");
        },
        [&](LogRoom room) {
            LogRoom need{0, 0};
            if (trew_hip_trace_results(x.c, w->slot, records<trew_hip_trace_item>(w, room.log), room.log, &need.log, &need.rows, nullptr, w->arecs.data(), nullptr))
                hip_die(x.c, "trew_hip_trace_results");
            return need;
        }).log;
    align_rows(x, w->arecs.data(), p);
    const trew_hip_trace_item *recs = static_cast<const trew_hip_trace_item *>(w->recs);
    for (uint64_t i = 0; i < items; i++) {
        const trew_hip_trace_item &it = recs[i];
        uint64_t *sums = p.trace_sums[it.motif][it.strand];
        fold_item(x, p, it, (uint32_t) x.rq->motifs[it.motif].k, sums[0], sums[1], sums[2]);
    }
}

// trew copies: fold_trace for monomers.  The workspace and the log are sized as fold_trace's are (a row for every base and
// monomer: a key claims end - start rows, so a batch in which both strands of long tracts reach MIN_SCORE can exceed it);
// a batch whose log or workspace overflows is resubmitted once, with the exact numbers.
static void fold_copies(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const int nm = x.rq->n_motifs;
    uint64_t bases = 0;
    for (uint64_t r = 0; r < x.n; r++) bases += x.lengths[r];
    if (w->arecs.size() < x.n * (size_t) nm) w->arecs.resize(x.n * (size_t) nm);
    const uint64_t items = fetch_with_retry(
        p, LogRoom{16 * x.n * (uint64_t) nm + 1024, std::max<uint64_t>(bases * (uint64_t) nm, 1)}, "internal error: the copies log overflowed twice",
        [&](LogRoom room) {
            if (trew_hip_copies(x.c, &x.b, w->slot, x.rq->monomers, nm, x.rq->penalty, x.rq->min_score, room.log, room.rows)) hip_die(x.c, "trew_hip_copies");
        },
        [&](LogRoom room) {
            LogRoom need{0, 0};
            if (trew_hip_copies_results(x.c, w->slot, records<trew_hip_trace_item>(w, room.log), room.log, &need.log, &need.rows, nullptr, w->arecs.data(), nullptr))
                hip_die(x.c, "trew_hip_copies_results");
            return need;
        }).log;
    align_rows(x, w->arecs.data(), p);
    const trew_hip_trace_item *recs = static_cast<const trew_hip_trace_item *>(w->recs);
    for (uint64_t i = 0; i < items; i++) {
        const trew_hip_trace_item &it = recs[i];
        uint64_t *sums = p.trace_sums[it.motif][it.strand];
        fold_item(x, p, it, (uint32_t) x.rq->monomers[it.motif].k, sums[0], sums[1], sums[2]);
    }
}

// trew decompose: fold_refine's rows from the records that come with the items (reserved: the anchor), and fold_trace's items
// of those reads, against each read's own unit.  decompose_units counts per (period, strand-canonical unit) the rows, their
// bases and copies, and the units, edited items and items of their signatures.  The workspace holds a row of 32 bytes for every
// base of the batch, which no batch exceeds; the log starts at sixteen items per read, and a batch whose log overflows is
// resubmitted once, with the exact numbers.
static void fold_decompose(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const AnnotRequest &rq = *x.rq;
    uint64_t bases = 0;
    for (uint64_t r = 0; r < x.n; r++) bases += x.lengths[r];
    if (w->drecs.size() < x.n) w->drecs.resize(x.n);
    const uint64_t items = fetch_with_retry(
        p, LogRoom{16 * x.n, std::max<uint64_t>(bases, 1)}, "internal error: the decompose log overflowed twice",
        [&](LogRoom room) {
            if (rq.candidates == 1) {
                if (trew_hip_decompose(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score, room.log, room.rows))
                    hip_die(x.c, "trew_hip_decompose");
            } else if (trew_hip_decompose_resolved(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score, rq.candidates, room.log,
                                                   room.rows)) {
                hip_die(x.c, "trew_hip_decompose_resolved");
            }
        },
        [&](LogRoom room) {
            LogRoom need{0, 0};
            if (trew_hip_decompose_results(x.c, w->slot, records<trew_hip_trace_item>(w, room.log), room.log, &need.log, &need.rows, nullptr, w->drecs.data(), nullptr))
                hip_die(x.c, "trew_hip_decompose_results");
            return need;
        }).log;
    for (uint64_t r = 0; r < x.n; r++) {
        const trew_hip_refined &rec = w->drecs[r];
        if (rec.period == 0 || rec.score < rq.min_score) continue;
        DecomposeUnit &u = p.decompose_units[{rec.period, canonical_unit(rec.unit, (int) rec.period)}];
        u.reads++;
        u.bases += rec.end - rec.start;
        u.copies += rec.consumed / rec.period;
        p.frows.push_back(RefineRow{x.first_read + r, x.lengths[r], rec});
    }
    const trew_hip_trace_item *recs = static_cast<const trew_hip_trace_item *>(w->recs);
    for (uint64_t i = 0; i < items; i++) {
        const trew_hip_trace_item &it = recs[i];
        const trew_hip_refined &rec = w->drecs[it.read];
        DecomposeUnit &u = p.decompose_units[{rec.period, canonical_unit(rec.unit, (int) rec.period)}];
        fold_item(x, p, it, rec.period, u.units, u.edited, u.items);
    }
}

// trew dissect: fold_tandems' rows and tally from the records (reserved: the anchor), and fold_decompose's items of those tracts,
// each against its tract's own unit (it.motif: the tract's index among its read's records).  dissect_units counts per (period,
// strand-canonical unit) what tandem_units counts, and the units, edited items and items of the tracts' signatures.  The
// workspace holds a row of 32 bytes for every base of the batch, which no batch exceeds; the logs start at sixteen items and four
// records per read, and a batch of which either overflows is resubmitted once, with the exact numbers.
static void fold_dissect(const AnnotBatch &x, AnnotFileResult &p) {
    Annotator::Worker *w = x.w;
    const AnnotRequest &rq = *x.rq;
    uint64_t bases = 0;
    for (uint64_t r = 0; r < x.n; r++) bases += x.lengths[r];
    const LogRoom found = fetch_with_retry(
        p, LogRoom{16 * x.n, std::max<uint64_t>(bases, 1), 4 * x.n + 16}, "internal error: the dissect logs overflowed twice",
        [&](LogRoom room) {
            if (rq.candidates == 1) {
                if (trew_hip_dissect(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score, room.tracts, room.log, room.rows))
                    hip_die(x.c, "trew_hip_dissect");
            } else if (trew_hip_dissect_resolved(x.c, &x.b, w->slot, rq.min_period, rq.max_period, rq.penalty, rq.min_score, rq.candidates, room.tracts,
                                                 room.log, room.rows)) {
                hip_die(x.c, "trew_hip_dissect_resolved");
            }
        },
        [&](LogRoom room) {
            LogRoom need{0, 0, 0};
            if (w->trecs.size() < room.tracts) w->trecs.resize(room.tracts);
            if (trew_hip_dissect_results(x.c, w->slot, w->trecs.data(), room.tracts, records<trew_hip_trace_item>(w, room.log), room.log, &need.tracts, &need.log,
                                         &need.rows, nullptr, nullptr))
                hip_die(x.c, "trew_hip_dissect_results");
            return need;
        });
    const trew_hip_tandem *trecs = w->trecs.data();
    tally_units(
        trecs, found.tracts, p.dissect_units,
        [](const trew_hip_tandem &rec) { return std::pair<uint32_t, uint64_t>{rec.period, canonical_unit(rec.unit, (int) rec.period)}; },
        [&](const trew_hip_tandem &rec, DissectUnit &u) {
            u.copies += rec.consumed / rec.period;
            p.trows.push_back(TandemRow{x.first_read + rec.read, x.lengths[rec.read], rec});
        });
    const trew_hip_trace_item *recs = static_cast<const trew_hip_trace_item *>(w->recs);
    uint64_t q = 0;  // items and records are sorted alike: the record of an item is found going forward
    for (uint64_t i = 0; i < found.log; i++) {
        const trew_hip_trace_item &it = recs[i];
        while (q < found.tracts && (trecs[q].read < it.read || (trecs[q].read == it.read && trecs[q].end <= it.start))) q++;
        if (q >= found.tracts) die("internal error: a dissect item without its record");
        const trew_hip_tandem &rec = trecs[q];
        DissectUnit &u = p.dissect_units[{rec.period, canonical_unit(rec.unit, (int) rec.period)}];
        fold_item(x, p, it, rec.period, u.units, u.edited, u.items);
    }
}

static void annotate_worker_loop(Annotator *a, Annotator::Worker *w, ChunkQueue *q, const AnnotRequest *rq) {
    trew_hip_ctx *c = a->ctx[(size_t) w->dev_index];
    for (;;) {
        Chunk *ch = q->pop();
        if (ch->sentinel) {
            delete ch;
            break;
        }
        // the newline that makes num & 3 == 2 closes a sequence line (locate_chunk_lines); no length limit here
        if (w->nl.size() < (size_t) LENGTH + 2) w->nl.resize((size_t) LENGTH + 2);
        const uint64_t first_read = locate_chunk_lines(ch->buffer1, (size_t) ch->total, ch->num_before, w->nl, w->st, w->nd);
        const uint64_t n = w->st.size();
        if (n > a->reads_cap) die("internal error: a chunk holds more reads than the slot");
        if (n) {
            uint32_t *offsets = w->h_buf, *lengths = w->h_buf + n, *words = w->h_buf + 2 * n;
            const uint64_t nw = trew_pack_reads(ch->buffer1, w->st.data(), w->nd.data(), n, words, a->words_cap, offsets, lengths);
            if (nw == (uint64_t) -1) die("internal error: packed chunk exceeds the slot buffer");
            AnnotBatch x{c, w, rq, trew_hip_batch(), lengths, n, first_read, ch->buffer1};
            memset(&x.b, 0, sizeof(x.b));
            x.b.words = words;
            x.b.n_words = nw;
            x.b.offsets = offsets;
            x.b.lengths = lengths;
            x.b.n_reads = n;
            AnnotFileResult &p = w->part;
            p.batches++;
            p.reads += n;
            for (uint64_t r = 0; r < n; r++) p.bases += lengths[r];
            switch (rq->kind) {
            case Measure::Annotate: fold_annotate(x, p); break;
            case Measure::Tracts: fold_tracts(x, p); break;
            case Measure::Intervals: fold_intervals(x, p); break;
            case Measure::Variants: fold_variants(x, p); break;
            case Measure::Periods: fold_periods(x, p); break;
            case Measure::Chain: fold_chain(x, p); break;
            case Measure::Repeats: fold_repeats(x, p); break;
            case Measure::Satellites: fold_satellites(x, p); break;
            case Measure::Align: fold_align(x, p); break;
            case Measure::Refine: fold_refine(x, p); break;
            case Measure::Tandems: fold_tandems(x, p); break;
            case Measure::Trace: fold_trace(x, p); break;
            case Measure::Decompose: fold_decompose(x, p); break;
            case Measure::Dissect: fold_dissect(x, p); break;
            case Measure::Resolve: fold_resolve(x, p); break;
            case Measure::Monomers: fold_monomers(x, p); break;
            case Measure::Copies: fold_copies(x, p); break;
            case Measure::Polish: fold_polish(x, p); break;
            }
        }
        free(ch->buffer1);
        delete ch;
    }
}

// one (period, unit) map into another: add(into's entry, from's entry)
template <class Map, class Add>
static void merge_units(Map &into, const Map &from, Add add) {
    for (const auto &kv : from) add(into[kv.first], kv.second);
}

void add_totals(AnnotFileResult &into, const AnnotFileResult &from) {
    into.reads += from.reads;
    into.bases += from.bases;
    for (int m = 0; m < TREW_ANNOT_MAX_MOTIFS; m++) {
        into.windows_fwd[m] += from.windows_fwd[m];
        into.windows_rev[m] += from.windows_rev[m];
        into.reported[m] += from.reported[m];
        into.longest[m] = std::max(into.longest[m], from.longest[m]);
        into.longest_tail[m] = std::max(into.longest_tail[m], from.longest_tail[m]);
        into.terminal_fwd[m] += from.terminal_fwd[m];
        into.terminal_rev[m] += from.terminal_rev[m];
        into.variants_fwd[m] += from.variants_fwd[m];
        into.variants_rev[m] += from.variants_rev[m];
        into.runs_fwd[m] += from.runs_fwd[m];
        into.runs_rev[m] += from.runs_rev[m];
        into.reported_rev[m] += from.reported_rev[m];
        for (int s = 0; s < 2; s++)
            for (int i = 0; i < kAlignSums; i++) into.align_sums[m][s][i] += from.align_sums[m][s][i];
        for (int s = 0; s < 2; s++)
            for (int i = 0; i < kTraceSums; i++) into.trace_sums[m][s][i] += from.trace_sums[m][s][i];
    }
    if (into.var_hist.size() < from.var_hist.size()) {
        into.var_hist.resize(from.var_hist.size());
        into.var_reads_with.resize(from.var_hist.size());
    }
    for (size_t i = 0; i < from.var_hist.size(); i++) {
        into.var_hist[i] += from.var_hist[i];
        into.var_reads_with[i] += from.var_reads_with[i];
    }
    into.interval_retries += from.interval_retries;
    into.batches += from.batches;
    auto add_repeat_unit = [](RepeatUnit &u, const RepeatUnit &v) {
        u.reads += v.reads;
        u.tracts += v.tracts;
        u.bases += v.bases;
    };
    merge_units(into.period_units, from.period_units, [](std::pair<uint64_t, uint64_t> &u, const std::pair<uint64_t, uint64_t> &v) {
        u.first += v.first;
        u.second += v.second;
    });
    merge_units(into.repeat_units, from.repeat_units, add_repeat_unit);
    merge_units(into.satellite_units, from.satellite_units, add_repeat_unit);
    merge_units(into.refine_units, from.refine_units, [](RefineUnit &u, const RefineUnit &v) {
        u.reads += v.reads;
        u.bases += v.bases;
        u.copies += v.copies;
    });
    merge_units(into.polish_units, from.polish_units, [](RefineUnit &u, const RefineUnit &v) {
        u.reads += v.reads;
        u.bases += v.bases;
        u.copies += v.copies;
    });
    merge_units(into.resolve_units, from.resolve_units, [](ResolveUnit &u, const ResolveUnit &v) {
        u.reads += v.reads;
        u.bases += v.bases;
        u.copies += v.copies;
        u.repaired += v.repaired;
    });
    merge_units(into.tandem_units, from.tandem_units, [](TandemUnit &u, const TandemUnit &v) {
        u.reads += v.reads;
        u.tracts += v.tracts;
        u.bases += v.bases;
        u.copies += v.copies;
    });
    merge_units(into.dissect_units, from.dissect_units, [](DissectUnit &u, const DissectUnit &v) {
        u.reads += v.reads;
        u.tracts += v.tracts;
        u.bases += v.bases;
        u.copies += v.copies;
        u.units += v.units;
        u.edited += v.edited;
        u.items += v.items;
    });
    merge_units(into.decompose_units, from.decompose_units, [](DecomposeUnit &u, const DecomposeUnit &v) {
        u.reads += v.reads;
        u.bases += v.bases;
        u.copies += v.copies;
        u.units += v.units;
        u.edited += v.edited;
        u.items += v.items;
    });
}

static const char *const kMeasureNames[] = {"annotate", "tracts", "intervals", "variants", "periods", "chain", "repeats", "satellites", "align", "refine", "tandems", "trace", "decompose", "dissect", "resolve", "monomers", "copies", "polish"};  // in the order of Measure

// The chunk length of the measure path: LENGTH, or TREW_MEASURE_CHUNK_BYTES where it names a value in [64, LENGTH] (a test and
// experiment knob, like TREW_SCAN_BLOCK_KIB: it moves the chunk borders, and with them the batches, to chosen places; buffers and
// slots stay sized for LENGTH).  Anything else is ignored.
static int measure_chunk_bytes() {
    if (const char *e = getenv("TREW_MEASURE_CHUNK_BYTES")) {
        int v;
        if (parse_int(e, &v) && v >= 64 && v <= LENGTH) return v;
    }
    return LENGTH;
}

// The rows `rows` of every worker's part, in the order `less`: the same for any number of workers.
template <class Row, class Less>
static void merge_rows(Annotator *a, std::vector<Row> AnnotFileResult::*rows, AnnotFileResult &out, Less less) {
    for (auto &w : a->workers) (out.*rows).insert((out.*rows).end(), (w.part.*rows).begin(), (w.part.*rows).end());
    std::sort((out.*rows).begin(), (out.*rows).end(), less);
}
// the sort keys: (read, motif, strand, start) and (read, start) of the record `rec` of a row
template <class Row, class Rec>
static auto by_read_motif_strand_start(Rec Row::*rec) {
    return [rec](const Row &x, const Row &y) {
        const Rec &a = x.*rec, &b = y.*rec;
        if (x.read != y.read) return x.read < y.read;
        if (a.motif != b.motif) return a.motif < b.motif;
        if (a.strand != b.strand) return a.strand < b.strand;
        return a.start < b.start;
    };
}
template <class Row, class Rec>
static auto by_read_start(Rec Row::*rec) {
    return [rec](const Row &x, const Row &y) { return x.read != y.read ? x.read < y.read : (x.*rec).start < (y.*rec).start; };
}

AnnotFileResult process_annotate(Annotator *a, const Config &cfg, const char *file_name, bool is_gz, const AnnotRequest &rq) {
    const auto t0 = std::chrono::steady_clock::now();
    for (auto &w : a->workers) w.part = AnnotFileResult();
    ChunkQueue q(256);
    std::vector<std::thread> th;
    for (auto &w : a->workers) th.emplace_back(annotate_worker_loop, a, &w, &q, &rq);
    FileReader f = open_reader(file_name, is_gz, cfg.NUM_THREAD);
    const int chunk = measure_chunk_bytes();
    read_fastq_thread(f, &q, chunk);
    f.close();
    for (size_t i = 0; i < a->workers.size(); i++) {
        Chunk *c = new Chunk();
        c->sentinel = true;
        q.push(c);
    }
    for (auto &t : th) t.join();
    AnnotFileResult out;
    for (auto &w : a->workers) add_totals(out, w.part);
    merge_rows(a, &AnnotFileResult::rows, out, [](const AnnotRow &x, const AnnotRow &y) { return x.read != y.read ? x.read < y.read : x.motif < y.motif; });
    merge_rows(a, &AnnotFileResult::irows, out, by_read_motif_strand_start(&IntervalRow::iv));
    merge_rows(a, &AnnotFileResult::crows, out, by_read_motif_strand_start(&ChainRow::it));
    merge_rows(a, &AnnotFileResult::xrows, out, by_read_motif_strand_start(&TraceRow::it));
    merge_rows(a, &AnnotFileResult::rrows, out, by_read_start(&RepeatRow::rp));
    merge_rows(a, &AnnotFileResult::srows, out, by_read_start(&SatelliteRow::st));
    merge_rows(a, &AnnotFileResult::trows, out, by_read_start(&TandemRow::td));
    merge_rows(a, &AnnotFileResult::frows, out, [](const RefineRow &x, const RefineRow &y) { return x.read < y.read; });
    merge_rows(a, &AnnotFileResult::prows, out, [](const PolishRow &x, const PolishRow &y) { return x.read < y.read; });
    merge_rows(a, &AnnotFileResult::vrows, out, [](const ResolveRow &x, const ResolveRow &y) { return x.read < y.read; });
    merge_rows(a, &AnnotFileResult::arows, out, [](const AlignRow &x, const AlignRow &y) {
        if (x.read != y.read) return x.read < y.read;
        return x.motif != y.motif ? x.motif < y.motif : x.strand < y.strand;
    });
    if (cfg.stats) {
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[trew] %s: %llu reads, %llu bases, %.3f s, %.3f Gbases/s end-to-end (decode + pack + %s; serial reader, %d worker(s))\n", file_name,
                (unsigned long long) out.reads, (unsigned long long) out.bases, sec, out.bases / sec / 1e9, kMeasureNames[(int) rq.kind], (int) a->workers.size());
        fprintf(stderr, "[trew] %s: %llu batch(es) submitted, chunk length %d bytes\n", file_name, (unsigned long long) out.batches, chunk);
        // the kinds with a log: what their rows are called, and how many there are
        const struct {
            Measure kind;
            const char *noun;
            size_t rows;
        } logs[] = {{Measure::Intervals, "intervals", out.irows.size()}, {Measure::Chain, "items", out.crows.size()},
                    {Measure::Repeats, "tracts", out.rrows.size()},      {Measure::Satellites, "tracts", out.srows.size()},
                    {Measure::Tandems, "tracts", out.trows.size()},      {Measure::Trace, "items", out.xrows.size()},
                    {Measure::Decompose, "items", out.xrows.size()},     {Measure::Dissect, "items", out.xrows.size()},
                    {Measure::Copies, "items", out.xrows.size()}};
        for (const auto &l : logs)
            if (rq.kind == l.kind)
                fprintf(stderr, "[trew] %s: %llu %s, %llu batch(es) resubmitted with a larger log\n", file_name, (unsigned long long) l.rows, l.noun,
                        (unsigned long long) out.interval_retries);
    }
    return out;
}

}  // namespace trew_host
