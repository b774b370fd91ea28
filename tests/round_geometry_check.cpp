// tests/round_geometry_check.cpp -- compiled and run by tests/test_round_geometry_cpu.py (plain C++, no GPU).
// build_filter_geom (trew_common.hpp), the block the host hands the prefilter once per read length, against get_segment and the
// predicates evaluated directly, in the order filter_kernel's round used to evaluate them: for every read length 20 .. 320, the
// modes with halves and one without, several (min_mer, max_mer) and the debug flags the block folds in.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
struct uint4 { unsigned x, y, z, w; };  // HIP's vector type, which trew_common.hpp names in a struct this program does not use
#include "trew_common.hpp"
using namespace trew;
static int pick_nw(u32 m) { return m <= 95 ? 3 : m <= 159 ? 5 : m <= 319 ? 10 : 32; }
static u32 low_mask(int bits) { return bits >= 32 ? 0xffffffffu : (bits <= 0 ? 0u : ((1u << bits) - 1u)); }
static long fails = 0, checks = 0;
#define EQ(a, b) do { checks++; if ((long long) (a) != (long long) (b)) { fails++; if (fails < 30) printf("MISMATCH %s=%lld %s=%lld  (mode %d UL %u k %d..%d flags %x pair %d) line %d\n", #a, (long long) (a), #b, (long long) (b), P.mode, UL, P.min_mer, P.max_mer, P.flags, p, __LINE__); } } while (0)
int main() {
    const int ranges[][2] = {{5, 32}, {9, 32}, {5, 16}, {3, 64}, {12, 40}, {1, 8}};
    const u32 flagsets[] = {0u, TREW_FLAG_DEBUG_NO_JOINT, TREW_FLAG_DEBUG_NO_KLOOP};
    for (int mode : {TREW_MODE_SHORT, TREW_MODE_PAIR, TREW_MODE_SEGMENT})
        for (auto &r : ranges)
            for (u32 fl : flagsets)
                for (u32 UL = 20; UL <= 320; UL++) {
                    DevParams P;
                    memset(&P, 0, sizeof P);
                    P.min_mer = r[0], P.max_mer = r[1], P.mode = mode, P.flags = fl, P.slice_len = 150;
                    const int nslots = mode_slots(mode);
                    u32 ms = 0;
                    for (int s = 0; s < nslots; s++) {
                        Segment sg = get_segment(mode, s, UL, UL, P.min_mer, P.max_mer, P.slice_len);
                        if (sg.valid) ms = std::max(ms, sg.len);
                    }
                    const int NW = pick_nw(ms);
                    FilterGeom g;
                    memset(&g, 0xee, sizeof g);
                    build_filter_geom(P, UL, NW, &g);
                    int p = -1;
                    const int gmax_run = (P.flags & TREW_FLAG_DEBUG_NO_KLOOP) ? P.min_mer - 1 : P.max_mer;
                    // ---- the round as the kernel derived it
                    int slot0 = 0;
                    const int n_halves = P.mode == TREW_MODE_PAIR ? 4 : (P.mode == TREW_MODE_SHORT ? 2 : 0);
                    EQ(g.head.n_halves, n_halves);
                    EQ(g.head.nw, NW);
                    if (NW == 3) {
                        for (; slot0 + 1 < n_halves && !(P.flags & TREW_FLAG_DEBUG_NO_JOINT); slot0 += 2) {
                            p = slot0 / 2;
                            const Segment sA = get_segment(P.mode, slot0, UL, UL, P.min_mer, P.max_mer, P.slice_len);
                            const Segment sB = get_segment(P.mode, slot0 + 1, UL, UL, P.min_mer, P.max_mer, P.slice_len);
                            const int L = (int) sA.len;
                            const int klo = sA.kmin > P.min_mer ? sA.kmin : P.min_mer, khi = sA.kmax < gmax_run ? sA.kmax : gmax_run;
                            const bool uneq = sB.len == sA.len + 1u;
                            if (!(sA.valid && sB.valid && (sA.len == sB.len || uneq) && sA.len <= 95u && sA.kmin == sB.kmin && sA.kmax == sB.kmax &&
                                  klo >= L + 1 - kUniSubsetMax && khi <= L - 32 && klo <= 31))
                                break;
                            const HalvesRound &hr = g.round[p];
                            const HalvesLoads &hl = g.loads[p];
                            u32 slot_p = (u32) slot0, slot_q = (u32) slot0 + 1u;
                            const bool a_left = sA.start == 0u;
                            const u32 h = a_left ? sB.start : sA.start, len_l = a_left ? sA.len : sB.len, len_r = a_left ? sB.len : sA.len;
                            const bool one_load = UL <= 159u && sA.mate == sB.mate && (a_left ? sA.start : sB.start) == 0u && (h >> 5) == 2u && h + len_r <= UL;
                            EQ(hr.L, L); EQ(hr.klo, klo); EQ(hr.khi, khi); EQ(hr.read_words, (UL + 31) / 32);
                            EQ(hr.row, (uneq ? 2 + slot0 / 2 : slot0 / 2));
                            EQ(hr.one_load, one_load);
                            if (one_load) {
                                EQ(hr.mate, sA.mate);
                                EQ(hr.bs, h & 31u);
                                if (!a_left) slot_p = (u32) slot0 + 1u, slot_q = (u32) slot0;
                                for (int j = 0; j < 3; j++) EQ(hr.nl[j], low_mask((int) len_l - 32 * j));
                                for (int j = 2; j < 5; j++) EQ(hr.nr[j - 2], (low_mask((int) h + (int) len_r - 32 * j) & ~low_mask((int) h - 32 * j)));
                            } else {
                                EQ(hl.mate_a, sA.mate); EQ(hl.start_a, sA.start); EQ(hl.mate_b, sB.mate); EQ(hl.start_b, sB.start);
                                for (int j = 0; j < 3; j++) { EQ(hr.nl[j], low_mask(L - 32 * j)); EQ(hr.nr[j], low_mask((int) sB.len - 32 * j)); }
                            }
                            EQ(hr.slot_p, slot_p); EQ(hr.slot_q, slot_q);
                        }
                    }
                    p = -1;
                    EQ(2 * g.head.n_joint, slot0);
                    // the slot loop: valid slots from slot0 on, in order
                    u32 idx = (u32) slot0;
                    for (int s = 0; s < slot0; s++) { EQ(g.slot[s].slot, s); }
                    for (int s = slot0; s < nslots; s++) {
                        const Segment sg = get_segment(P.mode, s, UL, UL, P.min_mer, P.max_mer, P.slice_len);
                        if (!sg.valid) continue;
                        // where is it in the list?
                        u32 at = 0;
                        while (at < g.head.n_slots && g.slot[at].slot != (u32) s) at++;
                        EQ(at < g.head.n_slots, 1);
                        if (at >= g.head.n_slots) continue;
                        EQ(at >= idx, 1);
                        const SlotGeom &o = g.slot[at];
                        EQ(o.mate, sg.mate); EQ(o.start, sg.start); EQ(o.len, sg.len); EQ(o.kmin, sg.kmin); EQ(o.kmax, sg.kmax);
                        EQ(o.too_long, sg.len > (u32) (32 * NW - 1));
                    }
                    u32 nvalid = 0;
                    for (int s = 0; s < nslots; s++) nvalid += get_segment(P.mode, s, UL, UL, P.min_mer, P.max_mer, P.slice_len).valid;
                    EQ(g.head.n_slots, nvalid);
                    for (u32 i = 1; i < g.head.n_slots; i++) EQ(g.slot[i].slot > g.slot[i - 1].slot, 1);
                    // drains
                    const bool dok = drain_uni_applies(P, UL, gmax_run);
                    EQ(g.head.drain_ok, dok);
                    if (dok) {
                        int Lmax = 0;
                        for (int s = 0; s < n_halves; s++) {
                            const Segment o = get_segment(P.mode, s, UL, UL, P.min_mer, P.max_mer, P.slice_len);
                            Lmax = std::max(Lmax, (int) o.len);
                            EQ(g.slot[s].slot, s); EQ(g.slot[s].mate, o.mate); EQ(g.slot[s].start, o.start); EQ(g.slot[s].len, o.len);
                            EQ(g.head.drain_klo, (o.kmin > P.min_mer ? o.kmin : P.min_mer));
                            EQ(g.head.drain_khi, (o.kmax < gmax_run ? o.kmax : gmax_run));
                        }
                        EQ(g.head.drain_lmax, Lmax);
                    }
                }
    printf("%ld checks, %ld mismatches\n", checks, fails);
    return fails != 0;
}
