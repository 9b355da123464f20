// Tables of the generated instance-minor paths (awegpu.hip, awempc.hip, awedual_gen.hip): where the
// node code's tangent slots go in J_g.  Plain C++ (host compilers build it, csrc/gen/check_im_tables.cpp);
// the device-side users are in im_layout.hpp.
//
// A node's generated code numbers its tangents ("slots").  A slot has one J_g destination, except the
// xdot directions of a Radau node, which have d: the other polynomial columns X_r, r != n.  A node's
// row of the destination table lists the CCS positions of its slots' destinations in slot order.
#pragma once

#include <algorithm>
#include <type_traits>
#include <vector>

#include "scalar.hpp"   // AWE_HD

namespace im {

// What a slot table is built from: kTanIdx[2][rows][dirs] and kNTan[2] of the generated namespace,
// the model's state count (directions [NX, 2 NX) are the xdot ones) and the table's capacity.
template <const auto& TanIdx, const auto& NTan, int NX, int CAP>
struct SlotTraits {
    static constexpr const auto& kTanIdx = TanIdx;
    static constexpr const auto& kNTan = NTan;
    static constexpr int kRows = std::extent_v<std::remove_reference_t<decltype(TanIdx)>, 1>;
    static constexpr int kDirs = std::extent_v<std::remove_reference_t<decltype(TanIdx)>, 2>;
    static constexpr int kNX = NX, kCap = CAP;
    static_assert(NTan[0] <= CAP && NTan[1] <= CAP, "slot table too small");
};

// destination count of every tangent slot (1, or d for the xdot directions of a Radau node) and its
// first entry in the node's destination row; compile-time on the device (the generated code's slot
// numbers are constants), built with the run-time d on the host
template <class Traits>
struct SlotTab {
    int first[2][Traits::kCap];
    int cnt[2][Traits::kCap];
    int total[2];
    AWE_HD constexpr SlotTab(int d) : first(), cnt(), total() {
        for (int kind = 0; kind < 2; ++kind) {
            int dir_of[Traits::kCap] = {};
            for (int s = 0; s < Traits::kCap; ++s) dir_of[s] = -1;
            for (int r = 0; r < Traits::kRows; ++r)
                for (int l = 0; l < Traits::kDirs; ++l)
                    if (Traits::kTanIdx[kind][r][l] >= 0) dir_of[Traits::kTanIdx[kind][r][l]] = l;
            int f = 0;
            for (int s = 0; s < Traits::kNTan[kind]; ++s) {
                const bool xd = kind == 1 && dir_of[s] >= Traits::kNX && dir_of[s] < 2 * Traits::kNX;
                first[kind][s] = f;
                cnt[kind][s] = xd ? d : 1;
                f += cnt[kind][s];
            }
            total[kind] = f;
        }
    }
};

// Host builder of an evaluator's destination tables (n_k intervals, nodes 0 = shooting, 1..d Radau):
//   dtab[(k (d + 1) + n) dstride + first[kind][slot] + q]: CCS position of destination q of the slot;
//   ctab[coff[k] .. coff[k + 1]): the interval's constant J_g entries, pos | value index << 24.
// The evaluator decodes its own gather entries and feeds them in interval order.  place() and
// finish() return the reason of the first violation (nullptr: none); what it means is the caller's.
template <class Traits>
struct DestTables {
    static constexpr unsigned kUnset = 0xffffffffu;
    const SlotTab<Traits> st;
    const int n_k, nn, dstride;
    std::vector<unsigned> dtab, ctab;
    std::vector<int> coff;

    DestTables(int n_k_, int d)
        : st(d), n_k(n_k_), nn(d + 1), dstride(std::max(st.total[0], st.total[1])),
          dtab((size_t)n_k * nn * dstride, kUnset), coff(n_k + 1, 0) {}

    const char* place(int k, int n, int kind, int slot, int q, unsigned pos) {
        if (k < 0 || k >= n_k || n < 0 || n >= nn || kind != (n > 0) || slot < 0 || slot >= Traits::kNTan[kind] ||
            q < 0)
            return "internal: generated destination outside the table";
        if (q >= st.cnt[kind][slot]) return "internal: destination count of a generated tangent";
        unsigned& dst = dtab[(size_t)(k * nn + n) * dstride + st.first[kind][slot] + q];
        if (dst != kUnset) return "internal: two J_g entries for one generated destination";
        dst = pos;
        return nullptr;
    }
    void add_const(int k, unsigned pos, unsigned idx) {
        (void)k;   // intervals come in order: the entry joins the list that close_interval(k) ends
        ctab.push_back(pos | (idx << 24));
    }
    void close_interval(int k) { coff[k + 1] = (int)ctab.size(); }
    const char* finish() {
        for (int kn = 0; kn < n_k * nn; ++kn) {
            unsigned* row = &dtab[(size_t)kn * dstride];
            const int used = st.total[kn % nn > 0];
            for (int i = 0; i < used; ++i)
                if (row[i] == kUnset) return "internal: generated destination without a J_g entry";
            for (int i = used; i < dstride; ++i) row[i] = 0;   // padding of the shorter node kind
        }
        if (ctab.empty()) ctab.push_back(0);   // never empty: it is uploaded as it stands
        return nullptr;
    }
};

}  // namespace im
