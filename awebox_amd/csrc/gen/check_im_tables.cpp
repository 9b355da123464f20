// Host check of the instance-minor tables (im_tables.hpp): the slot table of each generated node
// header for d = 1..5, and the builder of the destination tables on a small synthetic problem.
//
//   check_im_tables
//
// Prints one JSON line with the d = 4 totals per header; a failed check prints its text to stderr and
// the exit status is 1.
#include <cstdio>
#include <vector>

#include "../../../include/awedual.h"
#include "../../../include/awegpu.h"
#include "../../../include/awempc.h"
#include "../ap2_nodejac.gen.hpp"
#include "../dual_nodejac.gen.hpp"
#include "../im_tables.hpp"
#include "../kite3_nodejac.gen.hpp"

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::fprintf(stderr, "FAILED %s: ", #cond);      \
            std::fprintf(stderr, __VA_ARGS__);               \
            std::fprintf(stderr, "\n");                      \
            g_failed = 1;                                    \
        }                                                    \
    } while (0)

// the evaluators' instantiations (awegpu.hip, awempc.hip, awedual_gen.hip)
using Ap2 = im::SlotTraits<awe_gen::kTanIdx, awe_gen::kNTan, AWE_NX, 512>;
using Kite3 = im::SlotTraits<awe_k3gen::kTanIdx, awe_k3gen::kNTan, K3_NX, 128>;
using Dual = im::SlotTraits<awe_dgen::kTanIdx, awe_dgen::kNTan, ADL_NX, 1024>;

// total[] at d = 4 of the tables this header replaced (SoaSlotTab<4> of awegpu.hip, GenSlotTab(4) of
// awempc.hip, SlotTab(4) of awedual_gen.hip), printed from those constructors before they went
constexpr int kAp2Total4[2] = {347, 431}, kKite3Total4[2] = {81, 153}, kDualTotal4[2] = {860, 1067};

template <class Traits>
void check_slots(const char* name, const int (&total4)[2]) {
    for (int d = 1; d <= 5; ++d) {
        const im::SlotTab<Traits> st(d);
        for (int kind = 0; kind < 2; ++kind) {
            int sum = 0;
            for (int s = 0; s < Traits::kNTan[kind]; ++s) {
                CHECK(st.first[kind][s] == sum, "%s d=%d kind=%d slot=%d", name, d, kind, s);
                // the slot's directions, straight from the generated index table
                int n_xd = 0, n_other = 0;
                for (int r = 0; r < Traits::kRows; ++r)
                    for (int l = 0; l < Traits::kDirs; ++l)
                        if (Traits::kTanIdx[kind][r][l] == s)
                            ++(l >= Traits::kNX && l < 2 * Traits::kNX ? n_xd : n_other);
                CHECK(n_xd == 0 || n_other == 0, "%s kind=%d slot=%d mixes direction kinds", name, kind, s);
                const int want = kind == 1 && n_xd > 0 ? d : 1;
                CHECK(st.cnt[kind][s] == want, "%s d=%d kind=%d slot=%d: cnt %d, expected %d", name, d, kind, s,
                      st.cnt[kind][s], want);
                sum += st.cnt[kind][s];
            }
            CHECK(st.total[kind] == sum, "%s d=%d kind=%d: total %d, sum %d", name, d, kind, st.total[kind], sum);
            if (d == 4)
                CHECK(st.total[kind] == total4[kind], "%s kind=%d: total %d, before %d", name, kind, st.total[kind],
                      total4[kind]);
        }
    }
}

// synthetic node code: two slots per kind; direction 1 is the xdot direction (NX = 1), so slot 1 of
// the Radau kind has d destinations
constexpr short kSynTan[2][1][2] = {{{0, 1}}, {{0, 1}}};
constexpr int kSynNTan[2] = {2, 2};
using Syn = im::SlotTraits<kSynTan, kSynNTan, 1, 4>;
using SynTables = im::DestTables<Syn>;

// the destinations of (k, n) in row order, at positions 100 + 20 k + 5 n + i
const char* place_node(SynTables& t, int k, int n, int skip = -1) {
    const int kind = n > 0;
    const int slot_of[3] = {0, 1, 1}, q_of[3] = {0, 0, 1};
    for (int i = (kind ? 3 : 2) - 1; i >= 0; --i) {   // back to front: the order must not matter
        if (i == skip) continue;
        const unsigned pos = (unsigned)(100 + 20 * k + 5 * n + i);
        if (const char* why = t.place(k, n, kind, slot_of[i], q_of[i], pos)) return why;
    }
    return nullptr;
}

void check_builder() {
    {
        SynTables t(2, 2);
        CHECK(t.dstride == 3 && t.st.total[0] == 2 && t.st.total[1] == 3, "synthetic slot table");
        const char* why = nullptr;
        for (int k = 0; k < 2 && !why; ++k) {
            for (int n = 2; n >= 0 && !why; --n) why = place_node(t, k, n);
            if (k == 0) {
                t.add_const(0, 7, 1);
                t.add_const(0, 9, 2);
            } else {
                t.add_const(1, 11, 0);
            }
            t.close_interval(k);
        }
        if (!why) why = t.finish();
        CHECK(why == nullptr, "complete placement refused: %s", why);
        const std::vector<unsigned> dtab = {100, 101, 0,   105, 106, 107, 110, 111, 112,
                                            120, 121, 0,   125, 126, 127, 130, 131, 132};
        const std::vector<unsigned> ctab = {7u | 1u << 24, 9u | 2u << 24, 11u};
        const std::vector<int> coff = {0, 2, 3};
        CHECK(t.dtab == dtab, "dtab");
        CHECK(t.ctab == ctab, "ctab");
        CHECK(t.coff == coff, "coff");
    }
    {   // a second entry for one destination
        SynTables t(2, 2);
        CHECK(place_node(t, 0, 1) == nullptr, "first placement");
        const char* why = t.place(0, 1, 1, 1, 1, 999u);
        CHECK(why != nullptr && why[0] != 0, "duplicate destination accepted");
        CHECK(t.dtab[1 * 3 + 2] == 107u, "the refused entry overwrote the first");
    }
    {   // a destination that nothing fills
        SynTables t(2, 2);
        const char* why = nullptr;
        for (int k = 0; k < 2 && !why; ++k) {
            for (int n = 0; n < 3 && !why; ++n) why = place_node(t, k, n, k == 1 && n == 2 ? 1 : -1);
            t.close_interval(k);
        }
        CHECK(why == nullptr, "placement refused: %s", why);
        why = t.finish();
        CHECK(why != nullptr && why[0] != 0, "missing destination accepted");
    }
    {   // q >= cnt: slot 0 has one destination, slot 1 of a Radau node has d = 2
        SynTables t(2, 2);
        const char* why = t.place(0, 1, 1, 0, 1, 5u);
        CHECK(why != nullptr && why[0] != 0, "q = 1 of a one-destination slot accepted");
        why = t.place(0, 1, 1, 1, 2, 5u);
        CHECK(why != nullptr && why[0] != 0, "q = d accepted");
        why = t.place(0, 0, 0, 1, 1, 5u);
        CHECK(why != nullptr && why[0] != 0, "q = 1 at the shooting node accepted");
    }
    {   // no constant entries: ctab still has one element
        SynTables t(2, 2);
        const char* why = nullptr;
        for (int k = 0; k < 2 && !why; ++k) {
            for (int n = 0; n < 3 && !why; ++n) why = place_node(t, k, n);
            t.close_interval(k);
        }
        if (!why) why = t.finish();
        CHECK(why == nullptr, "placement without constants refused: %s", why);
        CHECK(t.ctab.size() == 1, "ctab has %d elements", (int)t.ctab.size());
        CHECK(t.coff == std::vector<int>({0, 0, 0}), "coff without constants");
    }
}

}  // namespace

int main() {
    check_slots<Ap2>("ap2", kAp2Total4);
    check_slots<Kite3>("kite3", kKite3Total4);
    check_slots<Dual>("dual", kDualTotal4);
    check_builder();
    const im::SlotTab<Ap2> a(4);
    const im::SlotTab<Kite3> m(4);
    const im::SlotTab<Dual> u(4);
    std::printf("{\"ok\": %s, \"ap2\": [%d, %d], \"kite3\": [%d, %d], \"dual\": [%d, %d]}\n",
                g_failed ? "false" : "true", a.total[0], a.total[1], m.total[0], m.total[1], u.total[0], u.total[1]);
    return g_failed;
}
