// trew_measures_host.cpp -- the per-read measures on the CPU, base by base from their definitions (see
// trew_measures_host.hpp).  These are what the kernels are checked against: they are written to be read, not to be fast.
#include "trew_measures_host.hpp"

#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace trew {

typedef uint32_t u32;
typedef uint64_t u64;

u64 motif_revcomp(u64 w, int k) {
    u64 r = 0;
    for (int i = 0; i < k; i++) {
        r = (r << 2) | (3u - (w & 3u));
        w >>= 2;
    }
    return r;
}

u64 motif_mask(int k) { return k >= 32 ? ~0ull : (1ull << (2 * k)) - 1ull; }

const char *motif_error(const trew_hip_motif &m) {
    if (m.k < 3 || m.k > 32) return "motif: k must be in [3, 32]";
    if (m.word & ~motif_mask(m.k)) return "motif: word has bits above 2k";
    return nullptr;
}

const char *motifs_error(const trew_hip_motif *motifs, int n_motifs) {
    if (n_motifs < 1 || n_motifs > TREW_ANNOT_MAX_MOTIFS) return "n_motifs must be in [1, 8]";
    if (!motifs) return "motifs is NULL";
    for (int m = 0; m < n_motifs; m++)
        if (const char *e = motif_error(motifs[m])) return e;
    return nullptr;
}

const char *rules_error(const trew_hip_interval_rule *rules, int n_motifs) {
    if (!rules) return "rules must not be null";
    for (int m = 0; m < n_motifs; m++)
        if (rules[m].min_len < 1) return "min_len must be at least 1";
    return nullptr;
}

void sort_intervals(trew_hip_interval *v, u64 n) {
    std::sort(v, v + n, [](const trew_hip_interval &a, const trew_hip_interval &b) {
        if (a.read != b.read) return a.read < b.read;
        if (a.motif != b.motif) return a.motif < b.motif;
        if (a.strand != b.strand) return a.strand < b.strand;
        return a.start < b.start;
    });
}

std::string motif_parse(const char *text, trew_hip_motif *out) {
    if (!text || !out) return "trew_motif_parse: null argument";
    const size_t k = strlen(text);
    u64 w = 0;
    for (size_t i = 0; i < k; i++) {
        u32 c;
        switch (text[i]) {
        case 'T': case 't': c = 0; break;
        case 'G': case 'g': c = 1; break;
        case 'C': case 'c': c = 2; break;
        case 'A': case 'a': c = 3; break;
        default: return std::string("motif '") + text + "': only A, C, G and T are allowed";
        }
        if (i < 32) w = (w << 2) | c;
    }
    if (k < 3 || k > 32) return std::string("motif '") + text + "': the length must be in [3, 32]";
    out->k = (int32_t) k;
    out->reserved = 0;
    out->word = w;
    return "";
}

// base i of a read's packed planes: its code, or 4 with its nmask bit set
static u32 base_at(const u32 *w, u32 i) {
    const u32 j = i >> 5, b = i & 31u;
    if ((w[3 * j + 2] >> b) & 1u) return 4;
    return ((w[3 * j] >> b) & 1u) | (((w[3 * j + 1] >> b) & 1u) << 1);
}

// a window matches strand s of a motif when its word is one of the k rotations of the strand's target
struct Rotations {
    int k;
    u64 rot[32];
    Rotations(const trew_hip_motif &motif, int s) : k(motif.k) {
        const u64 mask = motif_mask(k);
        u64 t = s ? motif_revcomp(motif.word, k) : motif.word;
        for (int i = 0; i < k; i++) {
            rot[i] = t;
            t = ((t << 2) | (t >> (2 * (k - 1)))) & mask;
        }
    }
    bool match(u64 word) const {
        bool hit = false;
        for (int x = 0; x < k && !hit; x++) hit = word == rot[x];
        return hit;
    }
};

// ---------------------------------------------------------------- per-read annotation against given motifs
const char *annotate_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_motif *motifs, int n_motifs,
                          trew_hip_annot *out) {
    if (const char *e = motifs_error(motifs, n_motifs)) return e;
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_annotate_host: null argument";
    std::vector<Rotations> rots;
    for (int m = 0; m < n_motifs; m++)
        for (int s = 0; s < 2; s++) rots.emplace_back(motifs[m], s);
    for (u64 r = 0; r < n_reads; r++) {
        const u32 *w = words + offsets[r];
        const u32 n = lengths[r];
        for (int m = 0; m < n_motifs; m++) {
            const int k = motifs[m].k;
            const u64 mask = motif_mask(k);
            u32 cnt[2] = {0, 0}, best_len[2] = {0, 0}, best_start[2] = {0, 0}, run[2] = {0, 0};
            u64 word = 0;
            u32 clean = 0;  // bases since the last one with its nmask bit set
            for (u32 i = 0; i < n; i++) {
                const u32 c = base_at(w, i);
                clean = c > 3 ? 0 : clean + 1;
                word = ((word << 2) | (c & 3u)) & mask;
                if (i + 1 < (u32) k) continue;
                const u32 start = i + 1 - (u32) k;  // the window that ends with base i
                for (int s = 0; s < 2; s++) {
                    if (clean >= (u32) k && rots[(size_t) m * 2 + s].match(word)) {
                        cnt[s]++;
                        if (++run[s] > best_len[s]) {  // strictly longer: the earliest run wins a tie
                            best_len[s] = run[s];
                            best_start[s] = start + 1 - run[s];
                        }
                    } else {
                        run[s] = 0;
                    }
                }
            }
            trew_hip_annot &o = out[r * (u64) n_motifs + (u64) m];
            o.windows_fwd = cnt[0];
            o.windows_rev = cnt[1];
            o.tract_start_fwd = best_len[0] ? best_start[0] : 0;
            o.tract_len_fwd = best_len[0] ? best_len[0] + (u32) k - 1 : 0;
            o.tract_start_rev = best_len[1] ? best_start[1] : 0;
            o.tract_len_rev = best_len[1] ? best_len[1] + (u32) k - 1 : 0;
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------- per-read error-tolerant terminal tracts
// cov[p] (p < n) = some matching window of strand s of the motif contains base p: the definition, base by base over the
// packed planes of one read.  Shared by tracts_host and intervals_host.
static void host_coverage(const u32 *w, u32 n, const trew_hip_motif &motif, int s, std::vector<unsigned char> &cov) {
    const int k = motif.k;
    const u64 mask = motif_mask(k);
    const Rotations rots(motif, s);
    cov.assign((size_t) n, 0);
    u64 word = 0;
    u32 clean = 0;  // bases since the last one with its nmask bit set
    for (u32 i = 0; i < n; i++) {
        const u32 c = base_at(w, i);
        clean = c > 3 ? 0 : clean + 1;
        word = ((word << 2) | (c & 3u)) & mask;
        if (clean < (u32) k) continue;  // also: fewer than k bases so far
        if (rots.match(word))
            for (u32 p = i + 1 - (u32) k; p <= i; p++) cov[p] = 1;
    }
}

const char *tracts_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_motif *motifs, int n_motifs,
                        int penalty, trew_hip_tract *out) {
    if (const char *e = motifs_error(motifs, n_motifs)) return e;
    if (penalty < 1 || penalty > 64) return "penalty must be in [1, 64]";
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_tracts_host: null argument";
    std::vector<unsigned char> cov;
    for (u64 r = 0; r < n_reads; r++) {
        const u32 *w = words + offsets[r];
        const u32 n = lengths[r];
        for (int m = 0; m < n_motifs; m++) {
            u32 res[2][5];
            for (int s = 0; s < 2; s++) {
                host_coverage(w, n, motifs[m], s, cov);
                // S(e), e = 0 .. n: the earliest largest value and the latest smallest value; covered counts alongside
                long long S = 0, hi = 0, lo = 0;
                u32 e_hi = 0, e_lo = 0, c = 0, c_hi = 0, c_lo = 0;
                for (u32 p = 0; p < n; p++) {
                    S += cov[p] ? 1 : -(long long) penalty;
                    c += cov[p];
                    if (S > hi) {
                        hi = S;
                        e_hi = p + 1;
                        c_hi = c;
                    }
                    if (S <= lo) {
                        lo = S;
                        e_lo = p + 1;
                        c_lo = c;
                    }
                }
                res[s][0] = c;
                res[s][1] = e_hi;
                res[s][2] = c_hi;
                res[s][3] = n - e_lo;
                res[s][4] = c - c_lo;
            }
            trew_hip_tract &o = out[r * (u64) n_motifs + (u64) m];
            o.covered_fwd = res[0][0];
            o.head_len_fwd = res[0][1];
            o.head_cov_fwd = res[0][2];
            o.tail_len_fwd = res[0][3];
            o.tail_cov_fwd = res[0][4];
            o.covered_rev = res[1][0];
            o.head_len_rev = res[1][1];
            o.head_cov_rev = res[1][2];
            o.tail_len_rev = res[1][3];
            o.tail_cov_rev = res[1][4];
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------- gap-tolerant motif intervals anywhere in a read
const char *intervals_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_motif *motifs,
                           const trew_hip_interval_rule *rules, int n_motifs, trew_hip_interval *out, u64 cap, u64 *n, u32 *counts) {
    if (const char *e = motifs_error(motifs, n_motifs)) return e;
    if (const char *e = rules_error(rules, n_motifs)) return e;
    if (!n || (cap && !out)) return "trew_intervals_host: null argument";
    if (n_reads && (!words || !offsets || !lengths)) return "trew_intervals_host: null argument";
    if (n_reads > 0xffffffffull) return "trew_intervals_host: more than 2^32 - 1 reads";
    std::vector<unsigned char> cov;
    u64 found = 0;
    for (u64 r = 0; r < n_reads; r++) {
        const u32 *w = words + offsets[r];
        const u32 len = lengths[r];
        for (int m = 0; m < n_motifs; m++) {
            for (int s = 0; s < 2; s++) {
                host_coverage(w, len, motifs[m], s, cov);
                u32 kept = 0;
                bool open = false;
                u32 start = 0, last = 0, c = 0;  // of the open interval: first and last covered position, covered bases
                auto close = [&]() {
                    if (open && last + 1 - start >= rules[m].min_len) {
                        if (found < cap) out[found] = trew_hip_interval{(u32) r, (u32) m, (u32) s, start, last + 1, c};
                        found++;
                        kept++;
                    }
                };
                for (u32 p = 0; p < len; p++) {
                    if (!cov[p]) continue;
                    if (open && p - last - 1 > rules[m].max_gap) {
                        close();
                        open = false;
                    }
                    if (!open) {
                        open = true;
                        start = p;
                        c = 0;
                    }
                    last = p;
                    c++;
                }
                close();
                if (counts) counts[(r * (u64) n_motifs + (u64) m) * 2ull + (u64) s] = kept;
            }
        }
    }
    *n = found;
    sort_intervals(out, std::min<u64>(found, cap));  // already in this order: reads, motifs, strands and positions ascend
    return nullptr;
}

// ---------------------------------------------------------------- telomere variant repeats
const char *variants_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_motif *motifs, int n_motifs,
                          trew_hip_variant *out, uint64_t *hist, uint64_t *reads_with) {
    if (const char *e = motifs_error(motifs, n_motifs)) return e;
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_variants_host: null argument";
    const size_t hl = (size_t) n_motifs * 2 * TREW_VARIANT_BINS;
    if (hist) memset(hist, 0, hl * sizeof(uint64_t));
    if (reads_with) memset(reads_with, 0, hl * sizeof(uint64_t));
    std::vector<unsigned char> base, state;  // per base: code, or 4 with its nmask bit set; per window: 1 exact, 2 variant
    std::vector<u32> bin_of;
    for (u64 r = 0; r < n_reads; r++) {
        const u32 *w = words + offsets[r];
        const u32 n = lengths[r];
        base.resize(n);
        for (u32 i = 0; i < n; i++) base[i] = (unsigned char) base_at(w, i);
        for (int m = 0; m < n_motifs; m++) {
            const u32 k = (u32) motifs[m].k;
            u32 res[2][5];
            for (int s = 0; s < 2; s++) {
                const u64 t = s ? motif_revcomp(motifs[m].word, (int) k) : motifs[m].word;
                u32 *o = res[s];
                o[0] = o[1] = o[2] = o[4] = 0;
                o[3] = TREW_VARIANT_NONE;
                if (n < k) continue;
                const u32 nwin = n - k + 1;
                state.assign(nwin, 0);
                bin_of.assign(nwin, 0);
                for (u32 i = 0; i < nwin; i++) {
                    u32 mism = 0, jj = 0, cc = 0;
                    bool valid = true;
                    for (u32 j = 0; j < k && valid; j++) {
                        const u32 c = base[i + j];
                        if (c > 3) valid = false;
                        else if (c != ((u32) (t >> (2 * (k - 1 - j))) & 3u)) {
                            mism++;
                            jj = j;
                            cc = c;
                        }
                    }
                    if (!valid) continue;
                    if (mism == 0) state[i] = 1;
                    if (mism == 1) {
                        state[i] = 2;
                        bin_of[i] = s ? 4u * (k - 1u - jj) + (3u - cc) : 4u * jj + cc;
                    }
                }
                u32 bins[TREW_VARIANT_BINS] = {};
                for (u32 i = 0; i < nwin; i++) {
                    if (state[i] == 1) o[0]++;
                    if (state[i] != 2) continue;
                    const bool anchored = (i >= k && state[i - k] == 1) || ((u64) i + k < nwin && state[i + k] == 1);
                    if (anchored) {
                        o[1]++;
                        bins[bin_of[i]]++;
                    }
                }
                for (u32 b = 0; b < TREW_VARIANT_BINS; b++) {
                    if (!bins[b]) continue;
                    o[2]++;
                    if (bins[b] > o[4]) {  // strictly: the smallest bin keeps a tie
                        o[4] = bins[b];
                        o[3] = b;
                    }
                    const size_t at = ((size_t) m * 2 + (size_t) s) * TREW_VARIANT_BINS + b;
                    if (hist) hist[at] += bins[b];
                    if (reads_with) reads_with[at]++;
                }
            }
            memcpy(&out[r * (u64) n_motifs + (u64) m], res, sizeof(trew_hip_variant));
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------- ordered unit chain per read
void sort_chain_items(trew_hip_chain_item *v, u64 n) {
    std::sort(v, v + n, [](const trew_hip_chain_item &a, const trew_hip_chain_item &b) {
        if (a.read != b.read) return a.read < b.read;
        if (a.motif != b.motif) return a.motif < b.motif;
        if (a.strand != b.strand) return a.strand < b.strand;
        return a.start < b.start;
    });
}

const char *chain_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_motif *motifs, int n_motifs,
                       trew_hip_chain_item *out, u64 cap, u64 *n_items, u32 *counts) {
    if (const char *e = motifs_error(motifs, n_motifs)) return e;
    if (!n_items || (cap && !out)) return "trew_chain_host: null argument";
    if (n_reads && (!words || !offsets || !lengths)) return "trew_chain_host: null argument";
    if (n_reads > 0xffffffffull) return "trew_chain_host: more than 2^32 - 1 reads";
    std::vector<unsigned char> base, state;  // per base: code, or 4 with its nmask bit set; per window: 1 exact, 2 variant
    std::vector<u32> bin_of;
    u64 found = 0;
    for (u64 r = 0; r < n_reads; r++) {
        const u32 *w = words + offsets[r];
        const u32 n = lengths[r];
        base.resize(n);
        for (u32 i = 0; i < n; i++) base[i] = (unsigned char) base_at(w, i);
        for (int m = 0; m < n_motifs; m++) {
            const u32 k = (u32) motifs[m].k;
            for (int s = 0; s < 2; s++) {
                u32 runs = 0, nvar = 0;
                const u32 nwin = n < k ? 0 : n - k + 1;
                const u64 t = s ? motif_revcomp(motifs[m].word, (int) k) : motifs[m].word;
                state.assign(nwin, 0);
                bin_of.assign(nwin, 0);
                for (u32 i = 0; i < nwin; i++) {
                    u32 mism = 0, jj = 0, cc = 0;
                    bool valid = true;
                    for (u32 j = 0; j < k && valid; j++) {
                        const u32 c = base[i + j];
                        if (c > 3) valid = false;
                        else if (c != ((u32) (t >> (2 * (k - 1 - j))) & 3u)) {
                            mism++;
                            jj = j;
                            cc = c;
                        }
                    }
                    if (!valid) continue;
                    if (mism == 0) state[i] = 1;
                    if (mism == 1) {
                        state[i] = 2;
                        bin_of[i] = s ? 4u * (k - 1u - jj) + (3u - cc) : 4u * jj + cc;
                    }
                }
                // windows ascend, so the items come out in the order of their starts
                for (u32 i = 0; i < nwin; i++) {
                    const bool before = i >= k && state[i - k] == 1, after = (u64) i + k < nwin && state[i + k] == 1;
                    trew_hip_chain_item it = {(u32) r, (u32) m, (u32) s, i, 1, TREW_VARIANT_NONE};
                    if (state[i] == 1 && !before) {  // a run starts here: walk its residue class to its end
                        for (u64 e = (u64) i + k; e < nwin && state[e] == 1; e += k) it.count++;
                        runs++;
                    } else if (state[i] == 2 && (before || after)) {
                        it.bin = bin_of[i];
                        nvar++;
                    } else {
                        continue;
                    }
                    if (found < cap) out[found] = it;
                    found++;
                }
                if (counts) {
                    u32 *c = counts + ((r * (u64) n_motifs + (u64) m) * 2ull + (u64) s) * 2ull;
                    c[0] = runs;
                    c[1] = nvar;
                }
            }
        }
    }
    *n_items = found;
    return nullptr;
}

// ---------------------------------------------------------------- de novo repeat period and unit per read
static const char *penalty_score_error(int penalty, u32 min_score) {
    if (penalty < 1 || penalty > 64) return "penalty must be in [1, 64]";
    if (min_score < 1) return "min_score must be at least 1";
    return nullptr;
}

const char *periods_error(int min_period, int max_period, int penalty, u32 min_score) {
    if (min_period < 1 || max_period > 32 || min_period > max_period) return "periods: 1 <= min_period <= max_period <= 32 is required";
    return penalty_score_error(penalty, min_score);
}

static_assert(TREW_SATELLITE_MAX_PERIOD == 256, "the text below");
const char *satellites_error(int min_period, int max_period, int penalty, u32 min_score) {
    if (min_period < 1 || max_period > TREW_SATELLITE_MAX_PERIOD || min_period > max_period)
        return "satellites: 1 <= min_period <= max_period <= 256 is required";
    return penalty_score_error(penalty, min_score);
}

// The best-scoring segment of eq_k of a read of n bases for one k < n: its score, 0 without one, and [b, e), the
// smallest e and then the largest b.  The per-period entry of piece_record, which trew_resolve_host asks for every k as well.
static long long period_segment(const unsigned char *base, u32 n, u32 k, int penalty, u32 &b, u32 &e) {
    long long S = 0, low = 0, score = 0;  // S(e), the smallest S(b) over b <= e, the largest S(e) - low so far
    u32 b_lo = 0;                         // the latest b at which S is low
    b = e = 0;
    for (u32 i = 0; i + k < n; i++) {
        const bool eq = base[i] < 4 && base[i] == base[i + k];
        S += eq ? 1 : -(long long) penalty;
        if (S <= low) {  // the latest b keeps a tie: the shorter segment
            low = S;
            b_lo = i + 1;
        }
        if (S - low > score) {  // strictly: the earliest e keeps a tie
            score = S - low;
            e = i + 1;
            b = b_lo;
        }
    }
    return score;
}

// the unreduced consensus u[0 .. k - 1] of [start, end) at period k, the smallest code on a tie; returns the sum of its counts
template <u32 kMaxK>
static u32 period_consensus_host(const unsigned char *base, u32 start, u32 end, u32 k, u32 *u) {
    u32 cnt[kMaxK][4] = {};
    for (u32 p = start; p < end; p++)
        if (base[p] < 4) cnt[(p - start) % k][base[p]]++;
    u32 support = 0;
    for (u32 j = 0; j < k; j++) {
        u[j] = 0;
        for (u32 c = 1; c < 4; c++)
            if (cnt[j][c] > cnt[j][u[j]]) u[j] = c;  // strictly: the smallest code keeps a tie
        support += cnt[j][u[j]];
    }
    return support;
}

// The record of the piece [lo, hi) of a read, its bases taken as a read of their own: nothing outside the piece is seen, start
// and end are in read coordinates.  base: per base of the read its code, or 4 with its nmask bit set.  All zero without a record.
// What period_piece and satellite_piece share: everything but the packing of the unit.  u: the codes of the primitive unit,
// u[0 .. period - 1] (kMaxK entries, kMaxK >= max_period).  False without a record; o's fields but `unit` are set otherwise.
template <u32 kMaxK, class Rec>
static bool piece_record(const unsigned char *base, u32 lo, u32 hi, int min_period, int max_period, int penalty, u32 min_score, Rec &o, u32 *u) {
    const u32 n = hi - lo;
    base += lo;
    // the best-scoring segment of eq_k for every k; a later k must score strictly more
    long long best = 0;
    u32 ks = 0, bs = 0, es = 0;
    for (u32 k = (u32) min_period; k <= (u32) max_period && k < n; k++) {
        u32 b = 0, e = 0;
        const long long score = period_segment(base, n, k, penalty, b, e);
        if (score > best) {
            best = score;
            ks = k;
            bs = b;
            es = e;
        }
    }
    if (ks == 0 || best < (long long) min_score) return false;
    o.scored_period = ks;
    o.score = (u32) best;
    o.matches = (u32) (((u64) best + (u64) penalty * (u64) (es - bs)) / (u64) (1 + penalty));
    const u32 start = bs, end = es + ks;  // in the piece
    o.support += period_consensus_host<kMaxK>(base, start, end, ks, u);
    for (u32 d = 1; d <= ks; d++) {
        if (ks % d) continue;
        bool periodic = true;
        for (u32 j = 0; j < ks && periodic; j++) periodic = u[j] == u[(j + d) % ks];
        if (periodic) {
            o.period = d;
            break;
        }
    }
    o.start = lo + start;
    o.end = lo + end;
    return true;
}

static void period_piece(const unsigned char *base, u32 lo, u32 hi, int min_period, int max_period, int penalty, u32 min_score, trew_hip_period &o) {
    memset(&o, 0, sizeof(o));
    u32 u[32];
    if (!piece_record<32>(base, lo, hi, min_period, max_period, penalty, min_score, o, u)) return;
    for (u32 j = 0; j < o.period; j++) o.unit = (o.unit << 2) | u[j];
}

// the same with periods up to 256 and the unit of trew_hip_satellite; read and depth are the caller's
static void satellite_piece(const unsigned char *base, u32 lo, u32 hi, int min_period, int max_period, int penalty, u32 min_score, trew_hip_satellite &o) {
    memset(&o, 0, sizeof(o));
    u32 u[TREW_SATELLITE_MAX_PERIOD];
    if (!piece_record<TREW_SATELLITE_MAX_PERIOD>(base, lo, hi, min_period, max_period, penalty, min_score, o, u)) return;
    for (u32 j = 0; j < o.period; j++) o.unit[j >> 4] |= u[j] << (2 * (j & 15u));
}

static void unpack_bases(const u32 *w, u32 n, std::vector<unsigned char> &base) {
    base.resize(n);
    for (u32 i = 0; i < n; i++) base[i] = (unsigned char) base_at(w, i);
}

const char *periods_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                         u32 min_score, trew_hip_period *out) {
    if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_periods_host: null argument";
    std::vector<unsigned char> base;  // per base: code, or 4 with its nmask bit set
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        period_piece(base.data(), 0, lengths[r], min_period, max_period, penalty, min_score, out[r]);  // the whole read
    }
    return nullptr;
}

// ---------------------------------------------------------------- the every-tract measures: one walk over the pieces of a read
// "<name>: <what>", kept for the calling thread until its next failed check
static const char *named_error(const char *name, const char *what) {
    static thread_local std::string text;
    text = std::string(name) + ": " + what;
    return text.c_str();
}

// what a measure's `piece` says of a piece [lo, hi)
enum class PieceResult {
    none,        // no tract: the branch ends here
    split_only,  // a tract [start, end) that is used up without a record: the pieces around it are walked
    record,      // a tract with its record
};

// The part of trew_hip_repeats, trew_hip_satellites and trew_hip_tandems that is one definition: tracts([lo, hi)) is what
// piece(base, read, lo, hi, depth, rec, start, end) gives [lo, hi), then tracts([lo, start)) and tracts([end, hi)) one level
// deeper; the tracts of a read are tracts([0, n)) at depth 0.  No piece is pruned; a piece without a tract ends its branch.
// A read's records go out in the order of their starts (they are disjoint); *n counts them all, out holds the first cap.
// `name` is the entry point's, for the texts of the argument checks.
template <class Rec, class PieceFn>
static const char *every_tract_host(const char *name, const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, Rec *out, u64 cap, u64 *n,
                                    u32 *counts, PieceFn piece) {
    if (!n) return named_error(name, "n must not be null");
    if (cap && !out) return named_error(name, "out must not be null");
    if (n_reads && (!words || !offsets || !lengths)) return named_error(name, "null argument");
    if (n_reads > 0xffffffffull) return named_error(name, "a batch holds at most 2^32 - 1 reads");
    struct Todo {
        u32 lo, hi, depth;
    };
    std::vector<unsigned char> base;  // per base: code, or 4 with its nmask bit set
    std::vector<Todo> todo;
    std::vector<Rec> mine;  // the tracts of one read
    u64 found = 0;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        mine.clear();
        todo.assign(1, Todo{0, lengths[r], 0});
        while (!todo.empty()) {
            const Todo t = todo.back();
            todo.pop_back();
            Rec rec;
            u32 start = 0, end = 0;
            const PieceResult what = piece(base.data(), (u32) r, t.lo, t.hi, t.depth, rec, start, end);
            if (what == PieceResult::none) continue;
            if (what == PieceResult::record) mine.push_back(rec);
            todo.push_back(Todo{end, t.hi, t.depth + 1});
            todo.push_back(Todo{t.lo, start, t.depth + 1});
        }
        std::sort(mine.begin(), mine.end(), [](const Rec &a, const Rec &b) { return a.start < b.start; });
        for (const Rec &x : mine) {
            if (found < cap) out[found] = x;
            found++;
        }
        if (counts) counts[r] = (u32) mine.size();
    }
    *n = found;
    return nullptr;
}

// ---------------------------------------------------------------- de novo repeats: every tract of a read
void sort_repeats(trew_hip_repeat *v, u64 n) {
    std::sort(v, v + n, [](const trew_hip_repeat &a, const trew_hip_repeat &b) { return a.read != b.read ? a.read < b.read : a.start < b.start; });
}

const char *repeats_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                         u32 min_score, trew_hip_repeat *out, u64 cap, u64 *n, u32 *counts) {
    if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
    return every_tract_host("trew_repeats_host", words, offsets, lengths, n_reads, out, cap, n, counts,
                            [&](const unsigned char *base, u32 r, u32 lo, u32 hi, u32 depth, trew_hip_repeat &rec, u32 &start, u32 &end) {
                                trew_hip_period p;
                                period_piece(base, lo, hi, min_period, max_period, penalty, min_score, p);
                                if (p.scored_period == 0) return PieceResult::none;
                                rec = trew_hip_repeat{r, depth, p.period, p.scored_period, p.score, p.start, p.end, p.matches, p.support, 0, p.unit};
                                start = p.start, end = p.end;
                                return PieceResult::record;
                            });
}

// ---------------------------------------------------------------- de novo repeats with periods up to 256
void sort_satellites(trew_hip_satellite *v, u64 n) {
    std::sort(v, v + n, [](const trew_hip_satellite &a, const trew_hip_satellite &b) { return a.read != b.read ? a.read < b.read : a.start < b.start; });
}

const char *satellites_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                            u32 min_score, trew_hip_satellite *out, u64 cap, u64 *n, u32 *counts) {
    if (const char *e = satellites_error(min_period, max_period, penalty, min_score)) return e;
    return every_tract_host("trew_satellites_host", words, offsets, lengths, n_reads, out, cap, n, counts,
                            [&](const unsigned char *base, u32 r, u32 lo, u32 hi, u32 depth, trew_hip_satellite &rec, u32 &start, u32 &end) {
                                satellite_piece(base, lo, hi, min_period, max_period, penalty, min_score, rec);
                                if (rec.scored_period == 0) return PieceResult::none;
                                rec.read = r;
                                rec.depth = depth;
                                start = rec.start, end = rec.end;
                                return PieceResult::record;
                            });
}

// ---------------------------------------------------------------- indel-aware motif tract per read (wraparound alignment)
// A cell of the alignment (trew_hip_alignment, include/trew_hip.h): compared field by field in this order, the larger wins.
struct AlignCell {
    long long score;
    u32 start, consumed, matches;
    bool operator<(const AlignCell &o) const {
        if (score != o.score) return score < o.score;
        if (start != o.start) return start < o.start;
        if (consumed != o.consumed) return consumed < o.consumed;
        return matches < o.matches;
    }
};

// The table of the alignment of a read against the unit t[0 .. k - 1] repeated without end (1 <= k <= 32): o = {score,
// start, end, consumed, matches}.  base[i]: the read's codes, 4: an N, which matches nothing.  With cnt (trew_hip_refined's
// vote) also the forward decode: at every row the phase j* with the largest V, the smallest on a tie, and cnt[j*][base] += 1
// when the base is valid and the diagonal is that cell.  With dirs (trew_hip_trace_item) also a direction byte a cell, n + 1
// rows of k (op of V in bits 0 .. 1: 0 fresh, 1 diagonal, 2 inserted read base; d of H above them), and the end cell's phase,
// under the three tie rules; without dirs nothing is allocated.  The cells are the same either way: equal tuples are equal.
static void wrap_table_host(const unsigned char *base, u32 n, const u32 *t, int k, int penalty, u32 (&o)[5], u32 (*cnt)[4] = nullptr,
                            std::vector<unsigned char> *dirs = nullptr, int *end_phase = nullptr) {
    AlignCell H[32], V[32], D[32];
    for (int j = 0; j < k; j++) H[j] = AlignCell{0, 0, 0, 0};
    if (dirs) dirs->assign(((size_t) n + 1) * (size_t) k, 0);
    unsigned char unkept[32];
    AlignCell best{0, 0, 0, 0};
    u32 best_end = 0;
    int best_j = 0;
    for (u32 i = 1; i <= n; i++) {
        const u32 c = base[i - 1];
        unsigned char *row = dirs ? dirs->data() + (size_t) i * (size_t) k : unkept;
        for (int j = 0; j < k; j++) {
            const AlignCell &d = H[(j + k - 1) % k];
            D[j] = c == t[j] ? AlignCell{d.score + 1, d.start, d.consumed + 1, d.matches + 1}
                             : AlignCell{d.score - penalty, d.start, d.consumed + 1, d.matches};
            const AlignCell ins{H[j].score - penalty, H[j].start, H[j].consumed, H[j].matches};
            V[j] = AlignCell{0, i, 0, 0}, row[j] = 0;  // rule 1: the fresh start, then the diagonal, then the inserted read base
            if (V[j] < D[j]) V[j] = D[j], row[j] = 1;
            if (V[j] < ins) V[j] = ins, row[j] = 2;
        }
        if (cnt) {
            int js = 0;
            for (int j = 1; j < k; j++)
                if (V[js] < V[j]) js = j;  // strictly: the smallest j keeps a tie
            if (c < 4 && !(D[js] < V[js])) cnt[js][c]++;  // V >= D always: equal
        }
        for (int j = 0; j < k; j++) {
            H[j] = V[j];
            for (int d = 1; d < k; d++) {  // rule 2: the smallest d
                const AlignCell &v = V[(j + k - d) % k];
                const AlignCell cand{v.score - (long long) penalty * d, v.start, v.consumed + (u32) d, v.matches};
                if (H[j] < cand) H[j] = cand, row[j] = (unsigned char) ((row[j] & 3) | (d << 2));
            }
        }
        // the largest (score, -end, start, consumed, matches): rows come in the order of their end; rule 3: the smallest j
        for (int j = 0; j < k; j++)
            if (H[j].score > best.score || (H[j].score == best.score && best_end == i && best < H[j])) {
                best = H[j];
                best_end = i;
                best_j = j;
            }
    }
    if (end_phase) *end_phase = best_j;
    if (best.score <= 0) {
        for (u32 &x : o) x = 0;
        return;
    }
    o[0] = (u32) best.score;
    o[1] = best.start;
    o[2] = best_end;
    o[3] = best.consumed;
    o[4] = best.matches;
}

// the codes of strand s of a motif, first base most significant
static void target_codes(const trew_hip_motif &motif, int s, u32 (&t)[32]) {
    const int k = motif.k;
    const u64 target = s ? motif_revcomp(motif.word, k) : motif.word;
    for (int j = 0; j < k; j++) t[j] = (u32) (target >> (2 * (k - 1 - j))) & 3u;
}

// two strands' {score, start, end, consumed, matches} as a record
static void spread_alignment(const u32 (&f)[5], const u32 (&v)[5], trew_hip_alignment &o) {
    o.score_fwd = f[0], o.start_fwd = f[1], o.end_fwd = f[2], o.consumed_fwd = f[3], o.matches_fwd = f[4];
    o.score_rev = v[0], o.start_rev = v[1], o.end_rev = v[2], o.consumed_rev = v[3], o.matches_rev = v[4];
}

const char *align_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_motif *motifs, int n_motifs,
                       int penalty, trew_hip_alignment *out) {
    if (const char *e = motifs_error(motifs, n_motifs)) return e;
    if (penalty < 1 || penalty > 64) return "penalty must be in [1, 64]";
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_align_host: null argument";
    std::vector<unsigned char> base;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        for (int m = 0; m < n_motifs; m++) {
            u32 rec[2][5], t[32];
            for (int s = 0; s < 2; s++) {
                target_codes(motifs[m], s, t);
                wrap_table_host(base.data(), lengths[r], t, motifs[m].k, penalty, rec[s]);
            }
            spread_alignment(rec[0], rec[1], out[r * (u64) n_motifs + (u64) m]);
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------- wraparound alignment for units of up to 256 bases
const char *monomer_error(const trew_hip_monomer &m) {
    if (m.k < 3 || m.k > TREW_MONOMER_MAX) return "monomer: k must be in [3, 256]";
    for (int j = m.k; j < TREW_MONOMER_MAX; j++)
        if ((m.unit[j >> 4] >> (2 * (j & 15))) & 3u) return "monomer: unit has bits at or above base k";
    return nullptr;
}

const char *monomers_error(const trew_hip_monomer *monomers, int n_monomers) {
    if (n_monomers < 1 || n_monomers > TREW_MONOMERS_MAX) return "n_monomers must be in [1, 8]";
    if (!monomers) return "monomers is NULL";
    for (int m = 0; m < n_monomers; m++)
        if (const char *e = monomer_error(monomers[m])) return e;
    return nullptr;
}

std::string monomer_parse(const char *text, trew_hip_monomer *out) {
    if (!text || !out) return "trew_monomer_parse: null argument";
    const size_t k = strlen(text);
    const std::string shown = k <= 40 ? std::string(text) : std::string(text, 37) + "...";
    trew_hip_monomer m;
    memset(&m, 0, sizeof(m));
    for (size_t i = 0; i < k; i++) {
        u32 c;
        switch (text[i]) {
        case 'T': case 't': c = 0; break;
        case 'G': case 'g': c = 1; break;
        case 'C': case 'c': c = 2; break;
        case 'A': case 'a': c = 3; break;
        default: return "monomer '" + shown + "': only A, C, G and T are allowed";
        }
        if (i < TREW_MONOMER_MAX) m.unit[i >> 4] |= c << (2 * (i & 15));
    }
    if (k < 3 || k > TREW_MONOMER_MAX) return "monomer '" + shown + "': the length must be in [3, 256]";
    m.k = (int32_t) k;
    *out = m;
    return "";
}

// c shifted by d deleted unit bases; a candidate that does not score can never win (it loses to the fresh start every V holds)
static AlignCell shifted(const AlignCell &c, int penalty, u32 d) { return AlignCell{c.score - (long long) penalty * d, c.start, c.consumed + d, c.matches}; }
static void take_scoring(AlignCell &into, const AlignCell &cand) {
    if (cand.score > 0 && into < cand) into = cand;
}

// wrap_table_host's cells and record for 1 <= k <= 256, the maximum over d in the linear-plus-wrap form: L[j] = max(V[j],
// L[j-1] shifted by 1) is the maximum over the sources j' <= j; W = L[k-1]; H[j] = max(L[j], W shifted by j + 1), which
// adds the sources j' > j with exactly d = j + k - j' and, a whole turn and so P k lower, the sources j' <= j once more.
// With end_phase also the end cell's phase, the smallest on equal tuples (rule 3 of 4.7h).  With dirs the table is the one
// that starts from (0, row0, 0, 0) in row row0 and ends with row n, and dirs gets a byte a cell of the rows row0 .. n (row
// row0: zeros): op of V in bits 0 .. 1 under rule 1, and in bit 2 whether H is strictly larger than V was before the closure
// -- whether the smallest d of rule 2 is not 0 (4.7n).  With cnt (trew_hip_polished's vote) also wrap_table_host's forward
// decode: the phase j* with the largest V in front of the closure, the smallest on a tie, and cnt[j*][base] += 1 when the
// base is valid and the diagonal candidate is that cell.
static void monomer_table_host(const unsigned char *base, u32 n, const u32 *t, int k, int penalty, u32 (&o)[5], int *end_phase = nullptr,
                               std::vector<unsigned char> *dirs = nullptr, u32 row0 = 0, u32 (*cnt)[4] = nullptr) {
    std::vector<AlignCell> H((size_t) k, AlignCell{0, row0, 0, 0}), V((size_t) k), V0((size_t) k), Dg(cnt ? (size_t) k : 0);
    AlignCell best{0, 0, 0, 0};
    u32 best_end = 0;
    int best_j = 0;
    if (dirs) dirs->assign(((size_t) (n - row0) + 1) * (size_t) k, 0);
    for (u32 i = row0 + 1; i <= n; i++) {
        const u32 c = base[i - 1];
        unsigned char *row = dirs ? dirs->data() + (size_t) (i - row0) * (size_t) k : nullptr;
        for (int j = 0; j < k; j++) {
            const AlignCell &d = H[(size_t) ((j + k - 1) % k)];
            const AlignCell D = c == t[j] ? AlignCell{d.score + 1, d.start, d.consumed + 1, d.matches + 1}
                                          : AlignCell{d.score - penalty, d.start, d.consumed + 1, d.matches};
            const AlignCell ins{H[(size_t) j].score - penalty, H[(size_t) j].start, H[(size_t) j].consumed, H[(size_t) j].matches};
            V[(size_t) j] = AlignCell{0, i, 0, 0};
            unsigned char op = 0;
            if (V[(size_t) j] < D) V[(size_t) j] = D, op = 1;
            if (V[(size_t) j] < ins) V[(size_t) j] = ins, op = 2;
            if (row) row[j] = op, V0[(size_t) j] = V[(size_t) j];
            if (cnt) Dg[(size_t) j] = D;
        }
        if (cnt) {
            size_t js = 0;
            for (size_t j = 1; j < (size_t) k; j++)
                if (V[js] < V[j]) js = j;  // strictly: the smallest j keeps a tie
            if (c < 4 && !(Dg[js] < V[js])) cnt[js][c]++;  // V >= D always: equal
        }
        for (int j = 1; j < k; j++) take_scoring(V[(size_t) j], shifted(V[(size_t) j - 1], penalty, 1));
        const AlignCell W = V[(size_t) k - 1];
        for (int j = 0; j < k; j++) {
            take_scoring(V[(size_t) j], shifted(W, penalty, (u32) j + 1u));
            H[(size_t) j] = V[(size_t) j];
            if (row && V0[(size_t) j] < H[(size_t) j]) row[j] |= 4;
            if (H[(size_t) j].score > best.score || (H[(size_t) j].score == best.score && best_end == i && best < H[(size_t) j])) {
                best = H[(size_t) j];
                best_end = i;
                best_j = j;
            }
        }
    }
    if (end_phase) *end_phase = best_j;
    if (best.score <= 0) {
        for (u32 &x : o) x = 0;
        return;
    }
    o[0] = (u32) best.score, o[1] = best.start, o[2] = best_end, o[3] = best.consumed, o[4] = best.matches;
}

// the codes of strand s of a monomer: the unit's base j, or the complement of its base k - 1 - j
static void monomer_codes(const trew_hip_monomer &mono, int s, u32 (&t)[TREW_MONOMER_MAX]) {
    const int k = mono.k;
    for (int j = 0; j < k; j++) {
        const int src = s ? k - 1 - j : j;
        const u32 code = (mono.unit[src >> 4] >> (2 * (src & 15))) & 3u;
        t[j] = s ? 3u - code : code;
    }
}

const char *monomers_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_monomer *monomers, int n_monomers,
                          int penalty, trew_hip_alignment *out) {
    if (const char *e = monomers_error(monomers, n_monomers)) return e;
    if (penalty < 1 || penalty > 64) return "penalty must be in [1, 64]";
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_monomers_host: null argument";
    std::vector<unsigned char> base;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        for (int m = 0; m < n_monomers; m++) {
            const int k = monomers[m].k;
            u32 rec[2][5], t[TREW_MONOMER_MAX];
            for (int s = 0; s < 2; s++) {
                monomer_codes(monomers[m], s, t);
                monomer_table_host(base.data(), lengths[r], t, k, penalty, rec[s]);
            }
            spread_alignment(rec[0], rec[1], out[r * (u64) n_monomers + (u64) m]);
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------- de novo repeats under indels: seed, align, re-vote
// the length of the primitive root of u[0 .. k - 1]
static u32 primitive_root(const u32 *u, u32 k) {
    for (u32 d = 1; d < k; d++) {
        if (k % d) continue;
        bool periodic = true;
        for (u32 j = 0; j < k && periodic; j++) periodic = u[j] == u[(j + d) % k];
        if (periodic) return d;
    }
    return k;
}

static u64 pack_unit(const u32 *u, u32 k) {
    u64 w = 0;
    for (u32 j = 0; j < k; j++) w = (w << 2) | u[j];
    return w;
}

static void refine_at_period(const unsigned char *base, u32 n, u32 k, u32 b, u32 e, const u32 *cons, int penalty, trew_hip_refined &o);

// the record of one read, step by step from the definition (trew_hip_refined, include/trew_hip.h); R: the periods record of step 1
// (scored_period 0 without one), for trew_hip_tandems' weak pieces
static void refine_read_host(const unsigned char *base, u32 n, int min_period, int max_period, int penalty, u32 min_score, trew_hip_refined &o,
                             trew_hip_period &R) {
    memset(&o, 0, sizeof(o));
    // 1. periods: the record and the unreduced consensus
    memset(&R, 0, sizeof(R));
    u32 cons[32];
    if (!piece_record<32>(base, 0, n, min_period, max_period, penalty, min_score, R, cons)) return;
    refine_at_period(base, n, R.scored_period, R.start, R.end - R.scored_period, cons, penalty, o);
}

// steps 2 to 6 of the definition for the period k with the segment [b, e) of its eq_k and the unreduced consensus of [b, e + k) at
// k: what refine_read_host does with the one period of step 1 and trew_resolve_host with each of its candidates
static void refine_at_period(const unsigned char *base, u32 n, u32 k, u32 b, u32 e, const u32 *cons, int penalty, trew_hip_refined &o) {
    memset(&o, 0, sizeof(o));
    // 2. seed: the longest run of eq_k in [b, e), the first of the longest
    u32 rs = b, longest = 0, run = 0;
    for (u32 i = b; i < e; i++) {
        run = base[i] < 4 && base[i] == base[i + k] ? run + 1 : 0;
        if (run > longest) {
            longest = run;
            rs = i + 1 - run;
        }
    }
    u32 S[32], U[32];
    for (u32 j = 0; j < k; j++) S[j] = base[rs + j] < 4 ? base[rs + j] : cons[(rs + j - b) % k];
    const u32 ks = primitive_root(S, k);
    // 3. align against the seed
    u32 a1[5], a2[5];
    wrap_table_host(base, n, S, (int) ks, penalty, a1);
    // 4. vote over the tract alone
    u32 cnt[32][4] = {};
    wrap_table_host(base + a1[1], a1[2] - a1[1], S, (int) ks, penalty, a2, cnt);
    // 5. re-vote
    u32 changed = 0, support = 0;
    for (u32 j = 0; j < ks; j++) {
        u32 top = 0;
        for (u32 c = 1; c < 4; c++)
            if (cnt[j][c] > cnt[j][top]) top = c;  // strictly: the smallest code among the largest
        U[j] = cnt[j][S[j]] == cnt[j][top] ? S[j] : top;
        support += cnt[j][U[j]];
        changed += U[j] != S[j];
    }
    u32 ku = primitive_root(U, ks);
    // 6. final
    for (int i = 0; i < 5; i++) a2[i] = a1[i];
    if (changed) {
        wrap_table_host(base, n, U, (int) ku, penalty, a2);
        if (a2[0] < a1[0]) {  // the seed is kept
            for (int i = 0; i < 5; i++) a2[i] = a1[i];
            for (u32 j = 0; j < ks; j++) U[j] = S[j];
            ku = ks;
            changed = 0;
        }
    }
    o.period = ku;
    o.seed_period = ks;
    o.scored_period = k;
    o.changed = changed;
    o.score = a2[0], o.start = a2[1], o.end = a2[2], o.consumed = a2[3], o.matches = a2[4];
    o.seed_score = a1[0];
    o.support = support;
    o.unit = pack_unit(U, ku);
    o.seed_unit = pack_unit(S, ks);
}

const char *refine_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                        u32 min_score, trew_hip_refined *out) {
    if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_refine_host: null argument";
    std::vector<unsigned char> base;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        trew_hip_period R;
        refine_read_host(base.data(), lengths[r], min_period, max_period, penalty, min_score, out[r], R);
    }
    return nullptr;
}

// ---------------------------------------------------------------- de novo repeats under indels for periods up to 256
static_assert(TREW_POLISH_MAX_PERIOD == TREW_SATELLITE_MAX_PERIOD, "step 1 is satellites' depth-0 record");
static void pack_unit_words(const u32 *u, u32 k, u32 (&w)[16]) {
    for (u32 j = 0; j < k; j++) w[j >> 4] |= u[j] << (2 * (j & 15u));
}

// the record of one read, step by step from the definition (trew_hip_polished, include/trew_hip.h): refine_read_host and
// refine_at_period with arrays of 256 and monomer_table_host in the place of wrap_table_host
static void polish_read_host(const unsigned char *base, u32 n, int min_period, int max_period, int penalty, u32 min_score, trew_hip_polished &o) {
    memset(&o, 0, sizeof(o));
    // 1. periods: satellites' depth-0 record and the unreduced consensus
    trew_hip_satellite R;
    memset(&R, 0, sizeof(R));
    u32 cons[TREW_POLISH_MAX_PERIOD];
    if (!piece_record<TREW_SATELLITE_MAX_PERIOD>(base, 0, n, min_period, max_period, penalty, min_score, R, cons)) return;
    const u32 k = R.scored_period, b = R.start, e = R.end - k;
    // 2. seed: the longest run of eq_k in [b, e), the first of the longest
    u32 rs = b, longest = 0, run = 0;
    for (u32 i = b; i < e; i++) {
        run = base[i] < 4 && base[i] == base[i + k] ? run + 1 : 0;
        if (run > longest) {
            longest = run;
            rs = i + 1 - run;
        }
    }
    u32 S[TREW_POLISH_MAX_PERIOD], U[TREW_POLISH_MAX_PERIOD];
    for (u32 j = 0; j < k; j++) S[j] = base[rs + j] < 4 ? base[rs + j] : cons[(rs + j - b) % k];
    const u32 ks = primitive_root(S, k);
    // 3. align against the seed
    u32 a1[5], a2[5];
    monomer_table_host(base, n, S, (int) ks, penalty, a1);
    // 4. vote over the tract alone
    u32 cnt[TREW_POLISH_MAX_PERIOD][4] = {};
    monomer_table_host(base + a1[1], a1[2] - a1[1], S, (int) ks, penalty, a2, nullptr, nullptr, 0, cnt);
    // 5. re-vote
    u32 changed = 0, support = 0;
    for (u32 j = 0; j < ks; j++) {
        u32 top = 0;
        for (u32 c = 1; c < 4; c++)
            if (cnt[j][c] > cnt[j][top]) top = c;  // strictly: the smallest code among the largest
        U[j] = cnt[j][S[j]] == cnt[j][top] ? S[j] : top;
        support += cnt[j][U[j]];
        changed += U[j] != S[j];
    }
    u32 ku = primitive_root(U, ks);
    // 6. final
    for (int i = 0; i < 5; i++) a2[i] = a1[i];
    if (changed) {
        monomer_table_host(base, n, U, (int) ku, penalty, a2);
        if (a2[0] < a1[0]) {  // the seed is kept
            for (int i = 0; i < 5; i++) a2[i] = a1[i];
            for (u32 j = 0; j < ks; j++) U[j] = S[j];
            ku = ks;
            changed = 0;
        }
    }
    o.period = ku;
    o.seed_period = ks;
    o.scored_period = k;
    o.changed = changed;
    o.score = a2[0], o.start = a2[1], o.end = a2[2], o.consumed = a2[3], o.matches = a2[4];
    o.seed_score = a1[0];
    o.support = support;
    pack_unit_words(U, ku, o.unit);
    pack_unit_words(S, ks, o.seed_unit);
}

const char *polish_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                        u32 min_score, trew_hip_polished *out) {
    if (const char *e = satellites_error(min_period, max_period, penalty, min_score)) return e;
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_polish_host: null argument";
    std::vector<unsigned char> base;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        polish_read_host(base.data(), lengths[r], min_period, max_period, penalty, min_score, out[r]);
    }
    return nullptr;
}

// ---------------------------------------------------------------- refine's unit with the period chosen by alignment
const char *resolve_error(int min_period, int max_period, int penalty, u32 min_score, int candidates) {
    if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
    static_assert(TREW_RESOLVE_MAX_CANDIDATES == 4, "the text below");
    return candidates < 1 || candidates > TREW_RESOLVE_MAX_CANDIDATES ? "resolve: 1 <= candidates <= 4 is required" : nullptr;
}

// the record of one read, step by step from the definition (trew_hip_resolved, include/trew_hip.h); t0, where given: the periods
// tract [t0[0], t0[1]) of candidate 0, which is refine_read_host's R (untouched without a candidate), for the weak pieces of 4.7l
static void resolve_read_host(const unsigned char *base, u32 n, int min_period, int max_period, int penalty, u32 min_score, int candidates,
                              trew_hip_resolved &o, u32 *t0 = nullptr) {
    memset(&o, 0, sizeof(o));
    // 1. scores: the first C of the order (score descending, k ascending) that reach min_score
    struct Candidate {
        long long score;
        u32 k, b, e;
    };
    Candidate cand[TREW_RESOLVE_MAX_CANDIDATES];
    u32 m = 0;
    for (u32 k = (u32) min_period; k <= (u32) max_period && k < n; k++) {
        Candidate x{0, k, 0, 0};
        x.score = period_segment(base, n, k, penalty, x.b, x.e);
        if (x.score < (long long) min_score) continue;
        u32 at = m;  // k ascends: strictly greater displaces, so the smaller k keeps a tie
        while (at > 0 && cand[at - 1].score < x.score) at--;
        if (at >= (u32) candidates) continue;
        if (m < (u32) candidates) m++;
        for (u32 i = m - 1; i > at; i--) cand[i] = cand[i - 1];
        cand[at] = x;
    }
    // 2. per candidate: steps 2 to 6 of refine with its own segment; 3. the largest score, then the smaller period, then the smaller c
    trew_hip_refined win{};
    for (u32 c = 0; c < m; c++) {
        u32 cons[32];
        period_consensus_host<32>(base, cand[c].b, cand[c].e + cand[c].k, cand[c].k, cons);
        trew_hip_refined x;
        refine_at_period(base, n, cand[c].k, cand[c].b, cand[c].e, cons, penalty, x);
        if (c == 0) o.first_period = x.period, o.first_score = x.score;
        if (c == 0 || x.score > win.score || (x.score == win.score && x.period < win.period)) {
            win = x;
            o.rank = c;
        }
    }
    if (m == 0) return;
    memcpy(&o, &win, sizeof(win));  // the first sixteen words are trew_hip_refined's
    o.candidates = m;
    if (t0) t0[0] = cand[0].b, t0[1] = cand[0].e + cand[0].k;
}

const char *resolve_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                         u32 min_score, int candidates, trew_hip_resolved *out) {
    if (const char *e = resolve_error(min_period, max_period, penalty, min_score, candidates)) return e;
    if (n_reads && (!words || !offsets || !lengths || !out)) return "trew_resolve_host: null argument";
    std::vector<unsigned char> base;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        resolve_read_host(base.data(), lengths[r], min_period, max_period, penalty, min_score, candidates, out[r]);
    }
    return nullptr;
}

// ---------------------------------------------------------------- what the every-tract and in-place measures ask of a piece
// The bases of a piece as a read of their own: false without a periods record; otherwise x the record the measure works with and
// [t_start, t_end) the periods tract that a weak piece is split around, all in the piece's coordinates.
// refine's one period (4.7g, 4.7i, 4.7j)
static bool refined_piece_host(const unsigned char *base, u32 n, int min_period, int max_period, int penalty, u32 min_score, trew_hip_refined &x,
                               u32 &t_start, u32 &t_end) {
    trew_hip_period R;
    refine_read_host(base, n, min_period, max_period, penalty, min_score, x, R);
    t_start = R.start, t_end = R.end;
    return R.scored_period != 0;
}

// resolve's winner among the first `candidates` periods, and the periods tract of candidate 0 (4.7l)
static bool resolved_piece_host(const unsigned char *base, u32 n, int min_period, int max_period, int penalty, u32 min_score, int candidates,
                                trew_hip_refined &x, u32 &t_start, u32 &t_end) {
    trew_hip_resolved o;
    u32 t0[2] = {0, 0};
    resolve_read_host(base, n, min_period, max_period, penalty, min_score, candidates, o, t0);
    memcpy(&x, &o, sizeof(x));  // the first sixteen words are trew_hip_refined's
    t_start = t0[0], t_end = t0[1];
    return o.candidates != 0;
}

// ---------------------------------------------------------------- de novo repeats under indels: every tract of a read
void sort_tandems(trew_hip_tandem *v, u64 n) {
    std::sort(v, v + n, [](const trew_hip_tandem &a, const trew_hip_tandem &b) { return a.read != b.read ? a.read < b.read : a.start < b.start; });
}

// tandems_host and tandems_resolved_host: every_tract_host over `piece`, one of the two entries above
template <class PieceFn>
static const char *tandems_walk_host(const char *name, const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, u32 min_score,
                                     trew_hip_tandem *out, u64 cap, u64 *n, u32 *counts, PieceFn piece) {
    return every_tract_host(name, words, offsets, lengths, n_reads, out, cap, n, counts,
                            [&](const unsigned char *base, u32 r, u32 lo, u32 hi, u32 depth, trew_hip_tandem &rec, u32 &start, u32 &end) {
                                trew_hip_refined x;
                                u32 t_start = 0, t_end = 0;
                                if (!piece(base + lo, hi - lo, x, t_start, t_end)) return PieceResult::none;  // the piece as a read of its own
                                start = lo + t_start, end = lo + t_end;  // a weak piece: around the periods tract
                                if (x.score < min_score) return PieceResult::split_only;
                                start = lo + x.start, end = lo + x.end;
                                rec = trew_hip_tandem{r, depth, x.period, x.seed_period, x.scored_period, x.changed, x.score, start, end, x.consumed,
                                                      x.matches, x.seed_score, x.support, 0, x.unit, x.seed_unit};
                                return PieceResult::record;
                            });
}

const char *tandems_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                         u32 min_score, trew_hip_tandem *out, u64 cap, u64 *n, u32 *counts) {
    if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
    return tandems_walk_host("trew_tandems_host", words, offsets, lengths, n_reads, min_score, out, cap, n, counts,
                             [&](const unsigned char *base, u32 len, trew_hip_refined &x, u32 &t_start, u32 &t_end) {
                                 return refined_piece_host(base, len, min_period, max_period, penalty, min_score, x, t_start, t_end);
                             });
}

const char *tandems_resolved_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                                  u32 min_score, int candidates, trew_hip_tandem *out, u64 cap, u64 *n, u32 *counts) {
    if (const char *e = resolve_error(min_period, max_period, penalty, min_score, candidates)) return e;
    return tandems_walk_host("trew_tandems_resolved_host", words, offsets, lengths, n_reads, min_score, out, cap, n, counts,
                             [&](const unsigned char *base, u32 len, trew_hip_refined &x, u32 &t_start, u32 &t_end) {
                                 return resolved_piece_host(base, len, min_period, max_period, penalty, min_score, candidates, x, t_start, t_end);
                             });
}

// ---------------------------------------------------------------- units in place under indels: the traceback of the alignment
void sort_trace_items(trew_hip_trace_item *v, u64 n) {
    std::sort(v, v + n, [](const trew_hip_trace_item &a, const trew_hip_trace_item &b) {
        if (a.read != b.read) return a.read < b.read;
        if (a.motif != b.motif) return a.motif < b.motif;
        if (a.strand != b.strand) return a.strand < b.strand;
        return a.start < b.start;
    });
}

// The walk over the direction bytes of wrap_table_host from the end cell (row end, phase j) to the fresh start, against the
// unit t[0 .. k - 1].  It meets the columns last to first, so a segment closes at its first column, an item is known when
// its segment closes, and a run of complete exact copies when a segment that is none closes behind it; the items, proto with
// their own fields filled in, are appended to `items` last to first.  dirs holds the rows from row0 on.  Bits 2 and above of a
// byte are d, or (copies_host) whether d > 0: the walk looks again after the d columns, and with the whole d in the byte it then
// finds 0 (the cell d phases down attains its tuple at d = 0).
static void wrap_walk_host(const unsigned char *base, const u32 *t, int k, const std::vector<unsigned char> &dirs, u32 end, int j,
                           trew_hip_trace_item proto, std::vector<trew_hip_trace_item> &items, u32 row0 = 0) {
    u32 i = end, seg_end = end, consumed = 0, sub = 0, ins = 0, del = 0, phase = 0, cols = 0, run = 0, run_start = 0;
    auto flush_run = [&]() {
        if (!run) return;
        trew_hip_trace_item it = proto;
        it.start = run_start, it.bases = it.consumed = run * (u32) k, it.count = run;
        items.push_back(it);
        run = 0;
    };
    auto close = [&]() {  // the running segment begins at read base i
        if (phase == 0 && consumed == (u32) k && !sub && !ins && !del) {
            run++;
            run_start = i;
        } else {
            flush_run();
            trew_hip_trace_item it = proto;
            it.start = i, it.bases = seg_end - i, it.count = 1, it.phase = phase, it.consumed = consumed;
            it.mismatches = sub, it.insertions = ins, it.deletions = del;
            items.push_back(it);
        }
        seg_end = i;
        consumed = sub = ins = del = phase = cols = 0;
    };
    for (;;) {
        while (const u32 d = dirs[(size_t) (i - row0) * (size_t) k + (size_t) j] >> 2)
            for (u32 q = 0; q < d; q++) {
                phase = (u32) j;
                consumed++, del++, cols++;
                if (j == 0) close();
                j = j ? j - 1 : k - 1;
            }
        const u32 op = dirs[(size_t) (i - row0) * (size_t) k + (size_t) j] & 3u;
        if (op == 0) break;
        i--;
        cols++;
        if (op == 1) {
            phase = (u32) j;
            consumed++;
            sub += base[i] != t[j];
            if (j == 0) close();
            j = j ? j - 1 : k - 1;
        } else {
            ins++;
        }
    }
    if (cols) close();
    flush_run();
}

// one unit over one read: the record o of wrap_table_host and, from min_score (>= 1) on, the items of its path, last to first
static void trace_unit_host(const unsigned char *base, u32 n, const u32 *t, int k, int penalty, u32 min_score, u32 (&o)[5],
                            std::vector<unsigned char> &dirs, trew_hip_trace_item proto, std::vector<trew_hip_trace_item> &items) {
    int j;
    wrap_table_host(base, n, t, k, penalty, o, nullptr, &dirs, &j);
    if (o[0] >= min_score) wrap_walk_host(base, t, k, dirs, o[2], j, proto, items);
}

// `mine`, which a walk left last to first, behind items[found ..] in ascending starts; nothing at or beyond cap while found counts on
static void append_reversed(const std::vector<trew_hip_trace_item> &mine, trew_hip_trace_item *items, u64 cap, u64 &found) {
    for (size_t q = mine.size(); q-- > 0;) {
        if (found < cap) items[found] = mine[q];
        found++;
    }
}

const char *trace_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_motif *motifs, int n_motifs,
                       int penalty, u32 min_score, trew_hip_trace_item *items, u64 cap, u64 *n_items, u32 *counts, trew_hip_alignment *records) {
    if (const char *e = motifs_error(motifs, n_motifs)) return e;
    if (penalty < 1 || penalty > 64) return "penalty must be in [1, 64]";
    if (min_score < 1) return "min_score must be at least 1";
    if (!n_items || (cap && !items)) return "trew_trace_host: null argument";
    if (n_reads && (!words || !offsets || !lengths)) return "trew_trace_host: null argument";
    if (n_reads > 0xffffffffull) return "trew_trace_host: more than 2^32 - 1 reads";
    std::vector<unsigned char> base, dirs;
    std::vector<trew_hip_trace_item> mine;
    u64 found = 0;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        for (int m = 0; m < n_motifs; m++) {
            const int k = motifs[m].k;
            u32 rec[2][5], t[32];
            for (int s = 0; s < 2; s++) {
                target_codes(motifs[m], s, t);
                mine.clear();
                trace_unit_host(base.data(), lengths[r], t, k, penalty, min_score, rec[s], dirs, trew_hip_trace_item{(u32) r, (u32) m, (u32) s, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                mine);
                append_reversed(mine, items, cap, found);
                if (counts) counts[(r * (u64) n_motifs + (u64) m) * 2ull + (u64) s] = (u32) mine.size();
            }
            if (records) spread_alignment(rec[0], rec[1], records[r * (u64) n_motifs + (u64) m]);
        }
    }
    *n_items = found;
    return nullptr;
}

// ---------------------------------------------------------------- copies in place for units of up to 256 bases: the traceback of monomers' alignment
//  monomer_table_host's record and end phase over the whole read; then, from min_score on, the table of the tract
// alone, started again in row start (fact (b) of 4.7h), with a direction byte a cell, and wrap_walk_host over it: O(n k) time a
// strand and (end - start + 1) k bytes.
const char *copies_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, const trew_hip_monomer *monomers, int n_monomers,
                        int penalty, u32 min_score, trew_hip_trace_item *items, u64 cap, u64 *n_items, u64 *n_rows, u32 *counts,
                        trew_hip_alignment *records) {
    if (const char *e = monomers_error(monomers, n_monomers)) return e;
    if (penalty < 1 || penalty > 64) return "penalty must be in [1, 64]";
    if (min_score < 1) return "min_score must be at least 1";
    if (!n_items || (cap && !items)) return "trew_copies_host: null argument";
    if (n_reads && (!words || !offsets || !lengths)) return "trew_copies_host: null argument";
    if (n_reads > 0xffffffffull) return "trew_copies_host: more than 2^32 - 1 reads";
    std::vector<unsigned char> base, dirs;
    std::vector<trew_hip_trace_item> mine;
    u64 found = 0, rows = 0;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        for (int m = 0; m < n_monomers; m++) {
            const int k = monomers[m].k;
            u32 rec[2][5], again[5], t[TREW_MONOMER_MAX];
            for (int s = 0; s < 2; s++) {
                int j = 0;
                monomer_codes(monomers[m], s, t);
                monomer_table_host(base.data(), lengths[r], t, k, penalty, rec[s], &j);
                mine.clear();
                if (rec[s][0] >= min_score) {
                    monomer_table_host(base.data(), rec[s][2], t, k, penalty, again, nullptr, &dirs, rec[s][1]);
                    wrap_walk_host(base.data(), t, k, dirs, rec[s][2], j, trew_hip_trace_item{(u32) r, (u32) m, (u32) s, 0, 0, 0, 0, 0, 0, 0, 0, 0}, mine,
                                   rec[s][1]);
                    rows += rec[s][2] - rec[s][1];
                }
                append_reversed(mine, items, cap, found);
                if (counts) counts[(r * (u64) n_monomers + (u64) m) * 2ull + (u64) s] = (u32) mine.size();
            }
            if (records) spread_alignment(rec[0], rec[1], records[r * (u64) n_monomers + (u64) m]);
        }
    }
    *n_items = found;
    if (n_rows) *n_rows = rows;
    return nullptr;
}

// ---------------------------------------------------------------- units in place with no motif given: refine's unit, anchored, traced
//  refine_read_host's record, the rotations of its unit compared as packed words, and trace_unit_host's table and walk
// for the forward strand against the smallest one, for any unit length >= 1.
// steps 2 and 3 of 4.7i for the read `base` of n bases with the refined record R: R.reserved becomes the anchor and the items of
// the forward strand against the smallest rotation are appended to `mine`, last to first; nothing without a record of min_score
static void anchor_and_trace_host(const unsigned char *base, u32 n, trew_hip_refined &R, int penalty, u32 min_score, std::vector<unsigned char> &dirs,
                                  trew_hip_trace_item proto, std::vector<trew_hip_trace_item> &mine) {
    if (!R.period || R.score < min_score) return;
    const u32 k = R.period;
    u32 u[32], t[32], rho = 0;
    for (u32 j = 0; j < k; j++) u[j] = (u32) (R.unit >> (2 * (k - 1 - j))) & 3u;  // first base most significant
    u64 smallest = R.unit;
    for (u32 q = 1; q < k; q++) {  // rotation q: its base j is U[(j + q) mod k]
        u32 rot[32];
        for (u32 j = 0; j < k; j++) rot[j] = u[(j + q) % k];
        const u64 w = pack_unit(rot, k);
        if (w < smallest) smallest = w, rho = q;  // U is primitive: the rotations are distinct
    }
    for (u32 j = 0; j < k; j++) t[j] = u[(j + rho) % k];
    u32 rec[5];
    trace_unit_host(base, n, t, (int) k, penalty, min_score, rec, dirs, proto, mine);
    R.reserved = rho;
}

// decompose_host and decompose_resolved_host: the walk over the reads with `piece` for the whole read
template <class PieceFn>
static const char *decompose_walk_host(const char *name, const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int penalty, u32 min_score,
                                       trew_hip_trace_item *items, u64 cap, u64 *n_items, u32 *counts, trew_hip_refined *records, PieceFn piece) {
    if (!n_items || (cap && !items)) return named_error(name, "null argument");
    if (n_reads && (!words || !offsets || !lengths)) return named_error(name, "null argument");
    if (n_reads > 0xffffffffull) return named_error(name, "more than 2^32 - 1 reads");
    std::vector<unsigned char> base, dirs;
    std::vector<trew_hip_trace_item> mine;
    u64 found = 0;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        trew_hip_refined R;
        u32 t_start, t_end;
        piece(base.data(), lengths[r], R, t_start, t_end);
        mine.clear();
        anchor_and_trace_host(base.data(), lengths[r], R, penalty, min_score, dirs, trew_hip_trace_item{(u32) r, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, mine);
        append_reversed(mine, items, cap, found);
        if (counts) counts[r] = (u32) mine.size();
        if (records) records[r] = R;
    }
    *n_items = found;
    return nullptr;
}

const char *decompose_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                           u32 min_score, trew_hip_trace_item *items, u64 cap, u64 *n_items, u32 *counts, trew_hip_refined *records) {
    if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
    return decompose_walk_host("trew_decompose_host", words, offsets, lengths, n_reads, penalty, min_score, items, cap, n_items, counts, records,
                               [&](const unsigned char *base, u32 len, trew_hip_refined &x, u32 &t_start, u32 &t_end) {
                                   return refined_piece_host(base, len, min_period, max_period, penalty, min_score, x, t_start, t_end);
                               });
}

const char *decompose_resolved_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                                    u32 min_score, int candidates, trew_hip_trace_item *items, u64 cap, u64 *n_items, u32 *counts,
                                    trew_hip_refined *records) {
    if (const char *e = resolve_error(min_period, max_period, penalty, min_score, candidates)) return e;
    return decompose_walk_host("trew_decompose_resolved_host", words, offsets, lengths, n_reads, penalty, min_score, items, cap, n_items, counts, records,
                               [&](const unsigned char *base, u32 len, trew_hip_refined &x, u32 &t_start, u32 &t_end) {
                                   return resolved_piece_host(base, len, min_period, max_period, penalty, min_score, candidates, x, t_start, t_end);
                               });
}

// ---------------------------------------------------------------- units in place for every tract of a read, no motif given
//  tandems_host's piece walk, and for every piece that gives a record decompose_host's anchor and traceback of the
// piece's bases as a read of their own, its items shifted into read coordinates and numbered by the tract's place in the read.
// dissect_host and dissect_resolved_host: the walk over the pieces of every read with `piece` for each
template <class PieceFn>
static const char *dissect_walk_host(const char *name, const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int penalty, u32 min_score,
                                     trew_hip_tandem *records, u64 rec_cap, trew_hip_trace_item *items, u64 item_cap, u64 *n_records, u64 *n_items,
                                     u64 *n_rows, u32 *counts, PieceFn piece) {
    if (!n_records || !n_items || (rec_cap && !records) || (item_cap && !items)) return named_error(name, "null argument");
    if (n_reads && (!words || !offsets || !lengths)) return named_error(name, "null argument");
    if (n_reads > 0xffffffffull) return named_error(name, "more than 2^32 - 1 reads");
    struct Tract {
        trew_hip_tandem rec;
        std::vector<trew_hip_trace_item> items;  // last to first
    };
    struct Todo {
        u32 lo, hi, depth;
    };
    std::vector<unsigned char> base, dirs;
    std::vector<Todo> todo;
    std::vector<Tract> mine;
    u64 found = 0, found_items = 0, rows = 0;
    for (u64 r = 0; r < n_reads; r++) {
        unpack_bases(words + offsets[r], lengths[r], base);
        mine.clear();
        todo.assign(1, Todo{0, lengths[r], 0});
        while (!todo.empty()) {
            const Todo t = todo.back();
            todo.pop_back();
            trew_hip_refined x;
            u32 t_start = 0, t_end = 0;
            if (!piece(base.data() + t.lo, t.hi - t.lo, x, t_start, t_end)) continue;  // the piece as a read of its own
            u32 start = t.lo + t_start, end = t.lo + t_end;  // a weak piece: around the periods tract
            if (x.score >= min_score) {
                Tract tr;
                anchor_and_trace_host(base.data() + t.lo, t.hi - t.lo, x, penalty, min_score, dirs, trew_hip_trace_item{(u32) r, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                      tr.items);
                start = t.lo + x.start, end = t.lo + x.end;
                tr.rec = trew_hip_tandem{(u32) r, t.depth, x.period, x.seed_period, x.scored_period, x.changed, x.score, start, end, x.consumed,
                                         x.matches, x.seed_score, x.support, x.reserved, x.unit, x.seed_unit};
                for (trew_hip_trace_item &it : tr.items) it.start += t.lo;
                mine.push_back(std::move(tr));
            }
            todo.push_back(Todo{end, t.hi, t.depth + 1});
            todo.push_back(Todo{t.lo, start, t.depth + 1});
        }
        std::sort(mine.begin(), mine.end(), [](const Tract &a, const Tract &b) { return a.rec.start < b.rec.start; });
        u32 my_items = 0;
        for (size_t q = 0; q < mine.size(); q++) {
            if (found < rec_cap) records[found] = mine[q].rec;
            found++;
            rows += mine[q].rec.end - mine[q].rec.start;
            for (trew_hip_trace_item &it : mine[q].items) it.motif = (u32) q;
            append_reversed(mine[q].items, items, item_cap, found_items);
            my_items += (u32) mine[q].items.size();
        }
        if (counts) counts[2 * r] = (u32) mine.size(), counts[2 * r + 1] = my_items;
    }
    *n_records = found;
    *n_items = found_items;
    if (n_rows) *n_rows = rows;
    return nullptr;
}

const char *dissect_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                         u32 min_score, trew_hip_tandem *records, u64 rec_cap, trew_hip_trace_item *items, u64 item_cap, u64 *n_records, u64 *n_items,
                         u64 *n_rows, u32 *counts) {
    if (const char *e = periods_error(min_period, max_period, penalty, min_score)) return e;
    return dissect_walk_host("trew_dissect_host", words, offsets, lengths, n_reads, penalty, min_score, records, rec_cap, items, item_cap, n_records,
                             n_items, n_rows, counts, [&](const unsigned char *base, u32 len, trew_hip_refined &x, u32 &t_start, u32 &t_end) {
                                 return refined_piece_host(base, len, min_period, max_period, penalty, min_score, x, t_start, t_end);
                             });
}

const char *dissect_resolved_host(const u32 *words, const u32 *offsets, const u32 *lengths, u64 n_reads, int min_period, int max_period, int penalty,
                                  u32 min_score, int candidates, trew_hip_tandem *records, u64 rec_cap, trew_hip_trace_item *items, u64 item_cap,
                                  u64 *n_records, u64 *n_items, u64 *n_rows, u32 *counts) {
    if (const char *e = resolve_error(min_period, max_period, penalty, min_score, candidates)) return e;
    return dissect_walk_host("trew_dissect_resolved_host", words, offsets, lengths, n_reads, penalty, min_score, records, rec_cap, items, item_cap,
                             n_records, n_items, n_rows, counts, [&](const unsigned char *base, u32 len, trew_hip_refined &x, u32 &t_start, u32 &t_end) {
                                 return resolved_piece_host(base, len, min_period, max_period, penalty, min_score, candidates, x, t_start, t_end);
                             });
}

// `items` sorted by (read, start) with `motif` still the start of each item's tract, `records` sorted by (read, start): motif
// becomes the index of that tract among its read's records.  The tracts of a read are disjoint and an item starts inside its own.
void number_dissect_items(const trew_hip_tandem *records, u64 n_records, trew_hip_trace_item *items, u64 n_items) {
    u64 q = 0, first = 0;  // the record at hand, the first record of its read
    for (u64 i = 0; i < n_items; i++) {
        while (q < n_records && (records[q].read < items[i].read || (records[q].read == items[i].read && records[q].start < items[i].motif))) {
            q++;
            if (q < n_records && records[q].read != records[first].read) first = q;
        }
        if (q >= n_records) break;  // never: every item has its record
        items[i].motif = (u32) (q - first);
    }
}

void sort_dissect_items(trew_hip_trace_item *v, u64 n) {
    std::sort(v, v + n, [](const trew_hip_trace_item &a, const trew_hip_trace_item &b) {
        if (a.read != b.read) return a.read < b.read;
        return a.start < b.start;
    });
}

}  // namespace trew
