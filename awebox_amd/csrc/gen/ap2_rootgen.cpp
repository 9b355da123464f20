// Build-time generator of the AP2 kite's rootfinder node code (awebox_amd/csrc/ap2_noderoot.gen.hpp).
//
//   ap2_rootgen <consts file> <output header>
//
// The reference re-integrates a trajectory with rk4root (tools/integrator_routines.py:32-96): at every
// Runge-Kutta stage the shooting node's 24 model equalities are solved for the 24 unknowns y = (xdot, z) at
// the stage state.  This generator traces ap2_node (ap2_model.hpp) on the symbolic scalar of gen/sym.hpp
// as a shooting node without the nine path inequalities and without the side slip, keeps the 24 equality
// rows and the power integrand p = lambda10 l_t dl_t [W] (dynamics.py:318-330), and differentiates the tape
// along those 24 unknowns only (unknown j < 23 is xdot_j = node input 23 + j, unknown 23 is z.lambda10 =
// node input 56).  Same shape as kite3_rootgen.cpp.
//
// A dense 24 x 24 system per lane does not fit the LDS of a compute unit, and the model does not need one.
// The partition is read off the tape, not off a list of names:
//   * a row is EXPLICIT when its tangent list holds exactly one unknown and that tangent is a constant of
//     the model constants alone (no node input, no theta0 entry below it): its Newton step
//     dy = row / coefficient is exact;
//   * the other rows and the unknowns no explicit row owns form the dense K x K block;
//   * a dense row's tangents along explicit unknowns (couplings) are emitted like any other tangent and
//     applied to the right-hand side before the dense solve.
// Generation fails when the partition is not square or the dense block and right-hand side of 64 lanes
// exceed 96 KiB.  Every tangent takes a slot; kDest tells the kernel where a slot goes (dense entry, or
// the list of explicit coefficients and couplings).
//
// The model constants enter as run-time loads (cst[i]); only the integer structure read from them (tether
// elements, stability-table lengths) is fixed at generation time and written out with the list of theta0
// entries and parameter inputs the code reads, so that the entry points can check and pack them.
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../ap2_model.hpp"
#include "sym.hpp"

namespace {

using awe::Op;
using awe::Sym;

constexpr int kNUnk = AWE_NX + AWE_NZ;   // 24
constexpr int kZInput = 2 * AWE_NX + AWE_NU;   // 56
constexpr int kFirstPar = kZInput + AWE_NZ;    // 57: theta.diam_t, theta.t_f, then phi.gamma (AWE_NW)
constexpr int unknown_input(int j) { return j < AWE_NX ? AWE_NX + j : kZInput; }
int unknown_of(int input) {
    for (int j = 0; j < kNUnk; ++j) if (unknown_input(j) == input) return j;
    return -1;
}

struct RowSink {
    int rows[AWE_N_EQ];
    int pw = -1;
    RowSink() { for (int& r : rows) r = -1; }
    void eq_row(int r, const Sym& v) { rows[r] = v.id; }
    void ineq_row(int, const Sym&) {}
    void power(const Sym& v) { pw = v.id; }
    void beta(const Sym&) {}
};

struct SymIn {
    const Sym* w;
    Sym operator()(int i) const { return w[i]; }
};

// whether tape node v is a function of the model constants alone
bool constants_only(const awe::Tape& t, int v, std::vector<signed char>& memo) {
    if (memo[v] >= 0) return memo[v];
    const awe::SNode& s = t.n[v];
    bool ok = true;
    if (s.op == Op::Input || s.op == Op::Th || s.op == Op::Extra) ok = false;
    if (ok && s.a >= 0) ok = constants_only(t, s.a, memo);
    if (ok && s.b >= 0) ok = constants_only(t, s.b, memo);
    memo[v] = ok;
    return ok;
}

// indices i of "<name>i<close>" in an emitted body
std::vector<int> reads_of(const std::string& body, const std::string& name, int n) {
    std::vector<char> seen(n, 0);
    for (size_t p = body.find(name); p != std::string::npos; p = body.find(name, p + name.size())) {
        if (p > 0 && (std::isalnum((unsigned char)body[p - 1]) || body[p - 1] == '_')) continue;
        const int i = std::atoi(body.c_str() + p + name.size());
        if (i >= 0 && i < n) seen[i] = 1;
    }
    std::vector<int> out;
    for (int i = 0; i < n; ++i) if (seen[i]) out.push_back(i);
    return out;
}

template <class V>
void list(std::ostringstream& o, const char* type, const char* name, const V& v) {
    o << "constexpr " << type << " " << name << "[" << std::max<size_t>(1, v.size()) << "] = {";
    for (size_t i = 0; i < v.size(); ++i) o << (i ? "," : "") << v[i];
    if (v.empty()) o << "-1";
    o << "};\n";
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: ap2_rootgen <consts file> <output header>\n");
        return 2;
    }
    std::vector<double> cst;
    {
        std::ifstream f(argv[1]);
        double x;
        while (f >> x) cst.push_back(x);
    }
    if ((int)cst.size() != AWE_NCONST) {
        std::fprintf(stderr, "expected %d constants, read %zu\n", AWE_NCONST, cst.size());
        return 2;
    }

    awe::Tape tape;
    awe::active_tape() = &tape;
    std::vector<Sym> w(AWE_NW + 1), th(AWE_NTHETA0), cs(cst.size());
    for (int i = 0; i <= AWE_NW; ++i) w[i] = Sym::of(tape.leaf(Op::Input, i));
    for (int i = 0; i < AWE_NTHETA0; ++i) th[i] = Sym::of(tape.leaf(Op::Th, i));
    for (size_t i = 0; i < cst.size(); ++i) cs[i] = Sym::of(tape.leaf(Op::Cs, (int)i, cst[i]));
    RowSink sink;
    awe::ap2_node<Sym>(SymIn{w.data()}, w[AWE_NW], th.data(), cs.data(), sink, false);
    // the integral output in W: the model returns it over the energy scaling
    const int integrand = (Sym::of(sink.pw) * cs[AWE_C_ENERGY_SCALING]).id;
    const int n0 = (int)tape.n.size();
    const int one = tape.cnst(1.0);
    std::vector<awe::SparseGrad> G = awe::forward_grads(tape, n0, [&](int i) -> awe::SparseGrad {
        const int j = unknown_of(i);
        return j < 0 ? awe::SparseGrad{} : awe::SparseGrad{{j, one}};
    });

    // ---- the partition, from the tape ---------------------------------------------------------------
    std::vector<signed char> memo(tape.n.size(), -1);
    std::vector<int> expl_row, expl_unk, dense_row, dense_unk, owner_row(kNUnk, -1);
    for (int r = 0; r < AWE_N_EQ; ++r) {
        const int v = sink.rows[r];
        if (v < 0) { std::fprintf(stderr, "row %d not produced\n", r); return 1; }
        const awe::SparseGrad& g = G[v];
        if (g.size() == 1 && constants_only(tape, g[0].second, memo) && owner_row[g[0].first] < 0) {
            owner_row[g[0].first] = r;
            expl_row.push_back(r);
            expl_unk.push_back(g[0].first);
        } else {
            dense_row.push_back(r);
        }
    }
    for (int j = 0; j < kNUnk; ++j) if (owner_row[j] < 0) dense_unk.push_back(j);
    const int K = (int)dense_row.size();
    if (dense_unk.size() != dense_row.size()) {
        std::fprintf(stderr, "the partition is not square: %zu dense rows, %zu dense unknowns\n", dense_row.size(),
                     dense_unk.size());
        return 1;
    }
    const long lds = (long)K * K * 64 * 8 + (long)K * 64 * 8;
    if (lds > 96 * 1024) {
        std::fprintf(stderr, "K = %d: the dense block and right-hand side of 64 lanes take %ld B of LDS (> 96 KiB)\n", K, lds);
        return 1;
    }
    std::vector<int> dpos_row(AWE_N_EQ, -1), dpos_unk(kNUnk, -1), epos_unk(kNUnk, -1);
    for (int i = 0; i < K; ++i) { dpos_row[dense_row[i]] = i; dpos_unk[dense_unk[i]] = i; }
    for (size_t n = 0; n < expl_unk.size(); ++n) epos_unk[expl_unk[n]] = (int)n;
    // an explicit unknown may appear in dense rows (a coupling), never in another explicit row
    for (size_t n = 0; n < expl_row.size(); ++n)
        if (G[sink.rows[expl_row[n]]].size() != 1) { std::fprintf(stderr, "explicit row lost its shape\n"); return 1; }

    // ---- stores: rows, every non-zero tangent, the integrand ----------------------------------------
    std::vector<awe::Store> stores;
    for (int r = 0; r < AWE_N_EQ; ++r) {
        stores.push_back({sink.rows[r], 0, r, -1});
        for (auto& e : G[sink.rows[r]]) stores.push_back({e.second, 1, r, e.first});
    }
    stores.push_back({integrand, 3, 0, -1});
    awe::EmitStats st;
    const std::string body = awe::emit(tape, stores, st, true, 32, false, 0);
    if (body.find("::sin(") != std::string::npos || body.find("::cos(") != std::string::npos) {
        std::fprintf(stderr, "the node code holds a sin / cos: on the device that is a branch in the middle of it\n");
        return 1;
    }
    // slot tables: kDest[s] >= 0 is entry i * K + j of the dense block, < 0 is extra -(1 + e)
    std::vector<int> slot(AWE_N_EQ * kNUnk, -1), entry(st.n_tan, -1), dest(st.n_tan, 0);
    std::vector<int> expl_extra(expl_row.size(), -1), coup_row, coup_expl, coup_extra;
    int n_extra = 0, n_dense_nz = 0;
    for (auto& s : stores) {
        if (s.kind != 1) continue;
        slot[s.row * kNUnk + s.dir] = s.slot;
        entry[s.slot] = s.row * kNUnk + s.dir;
    }
    for (int s = 0; s < st.n_tan; ++s) {
        const int r = entry[s] / kNUnk, j = entry[s] % kNUnk;
        if (dpos_row[r] >= 0 && dpos_unk[j] >= 0) {
            dest[s] = dpos_row[r] * K + dpos_unk[j];
            ++n_dense_nz;
            continue;
        }
        dest[s] = -(1 + n_extra);
        if (dpos_row[r] < 0) {
            expl_extra[epos_unk[j]] = n_extra;
        } else {
            coup_row.push_back(dpos_row[r]);
            coup_expl.push_back(epos_unk[j]);
            coup_extra.push_back(n_extra);
        }
        ++n_extra;
    }
    for (int e : expl_extra) if (e < 0) { std::fprintf(stderr, "an explicit coefficient was not stored\n"); return 1; }
    const std::vector<int> th_used = reads_of(body, "th[", AWE_NTHETA0);
    std::vector<int> par_in;
    for (int i : reads_of(body, "in(", AWE_NW + 1)) if (i >= kFirstPar) par_in.push_back(i);
    std::vector<int> th_row(AWE_NTHETA0, -1), par_row(AWE_NW + 1 - kFirstPar, -1);
    for (size_t i = 0; i < par_in.size(); ++i) par_row[par_in[i] - kFirstPar] = (int)i;
    for (size_t i = 0; i < th_used.size(); ++i) th_row[th_used[i]] = (int)(par_in.size() + i);
    awe::active_tape() = nullptr;

    std::ostringstream o;
    o << "// GENERATED by awebox_amd/csrc/gen/ap2_rootgen.cpp from ap2_model.hpp -- do not edit.\n"
         "// Straight-line values of the AP2 shooting node's 24 equalities, the power integrand and the non-zero\n"
         "// entries of their 24 x 24 block along the rootfinder's unknowns (xdot, z), partitioned into explicit\n"
         "// rows and a dense K x K block (see the generator's header comment).\n"
         "#pragma once\n\n#include \"scalar.hpp\"\n\n"
         "#ifndef AWE_GEN_FENCE\n#if defined(__HIP_DEVICE_COMPILE__)\n"
         "#define AWE_GEN_FENCE() __builtin_amdgcn_sched_barrier(0)\n"
         "#else\n#define AWE_GEN_FENCE() ((void)0)\n#endif\n#endif\n\nnamespace awe_ap2root {\n\n";
    o << "// integer structure of the model constants the code was generated for (the entry points check it)\n";
    o << "constexpr int kNElements = " << (int)cst[AWE_C_N_ELEMENTS] << ";\n";
    o << "constexpr int kSdLen[54] = {";
    for (int i = 0; i < 54; ++i) o << (i ? ", " : "") << (int)cst[AWE_C_SD_LEN + i];
    o << "};\n";
    o << "// rows and unknowns: unknown j < " << AWE_NX << " is xdot_j (node input " << AWE_NX << " + j), unknown " << AWE_NX
      << " is z.lambda10 (node input " << kZInput << ")\n";
    o << "constexpr int kNRows = " << AWE_N_EQ << ", kNUnk = " << kNUnk << ";\n";
    o << "// the partition: kNExpl explicit rows (row kExplRow[n] holds unknown kExplUnk[n] alone, its coefficient is\n"
         "// extra kExplExtra[n]) and the dense K x K block of rows kDenseRow and unknowns kDenseUnk\n";
    o << "constexpr int K = " << K << ", kNExpl = " << expl_row.size() << ";\n";
    list(o, "short", "kDenseRow", dense_row);
    list(o, "short", "kDenseUnk", dense_unk);
    list(o, "short", "kExplRow", expl_row);
    list(o, "short", "kExplUnk", expl_unk);
    list(o, "short", "kExplExtra", expl_extra);
    o << "// couplings: dense row kCoupRow[m] (position in kDenseRow) holds explicit unknown kCoupExpl[m] (position in\n"
         "// kExplUnk) with the coefficient extra kCoupExtra[m]\n";
    o << "constexpr int kNCoup = " << coup_row.size() << ";\n";
    list(o, "short", "kCoupRow", coup_row);
    list(o, "short", "kCoupExpl", coup_expl);
    list(o, "short", "kCoupExtra", coup_extra);
    o << "// tangents stored: kNSlots = kNDenseNz entries of the dense block + kNExtra explicit coefficients and couplings\n";
    o << "constexpr int kNSlots = " << st.n_tan << ", kNDenseNz = " << n_dense_nz << ", kNExtra = " << n_extra << ";\n";
    o << "// algorithmic operations: adds/muls/reciprocals, transcendental calls; peak of live values as emitted\n";
    o << "constexpr int kFlops = " << st.flops << ", kTranscendental = " << st.transcendental << ", kMaxLive = "
      << st.max_live << ";\n";
    o << "// slot of (row, unknown), -1 outside the pattern\n";
    o << "constexpr short kSlot[" << AWE_N_EQ << "][" << kNUnk << "] = {\n";
    for (int r = 0; r < AWE_N_EQ; ++r) {
        o << "    {";
        for (int j = 0; j < kNUnk; ++j) o << (j ? "," : "") << slot[r * kNUnk + j];
        o << "},\n";
    }
    o << "};\n";
    o << "// row * kNUnk + unknown of every slot, and where it goes: >= 0 entry i * K + j of the dense block, < 0 extra -(1 + e)\n";
    list(o, "short", "kEntry", entry);
    list(o, "short", "kDest", dest);
    o << "// a task's parameter row: first the node inputs past z the code reads (kParIn: " << kFirstPar << " theta.diam_t, "
      << kFirstPar + 1 << " theta.t_f, " << AWE_NW << " phi.gamma),\n// then the theta0 entries it reads (kThUsed); "
         "kParRow / kThRow give an input's / a theta0 entry's place in the row (-1: not read)\n";
    o << "constexpr int kNParIn = " << par_in.size() << ", kNThUsed = " << th_used.size() << ", kNPar = "
      << par_in.size() + th_used.size() << ";\n";
    list(o, "short", "kParIn", par_in);
    list(o, "short", "kThUsed", th_used);
    list(o, "short", "kParRow", par_row);
    list(o, "short", "kThRow", th_row);
    o << "\n// in(i): node variable i (" << AWE_NW << " = phi.gamma); th[i]: theta0 entry i; val[r]: row r; tan[s * TS]: slot s;\n"
         "// obv[0]: the power integrand lambda10 l_t dl_t [W]\n";
    o << "template <int TS, class In, class Th, class Val, class Tan, class Obv>\nAWE_HD void ap2_node_root(const In& in, Th th, "
         "const double* __restrict__ cst, Val val, Tan tan, Obv obv) {\n";
    o << body << "}\n\n}  // namespace awe_ap2root\n";

    std::ofstream out(argv[2]);
    out << o.str();
    std::printf("{\"ops\": %d, \"flops\": %d, \"transcendental\": %d, \"slots\": %d, \"K\": %d, \"explicit\": %zu, "
                "\"couplings\": %zu, \"dense_nz\": %d, \"theta0\": %zu, \"max_live\": %d}\n",
                st.ops, st.flops, st.transcendental, st.n_tan, K, expl_row.size(), coup_row.size(), n_dense_nz,
                th_used.size(), st.max_live);
    return 0;
}
