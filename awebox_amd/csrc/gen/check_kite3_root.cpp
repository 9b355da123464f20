// Host check of the generated rootfinder node code (kite3_noderoot.gen.hpp) against the templated 3-DOF
// model on dual numbers: one forward pass of kite3_node per unknown (xdot_0..10, z.lambda), seeded on that
// node input alone.
//
//   check_kite3_root <consts (55)> <node values (31 + gamma)> <u_ref>
//
// Prints one JSON line: the largest relative value and block-entry differences, the number of slots that
// are pattern entries, and the dense 12 x 12 block (row-major) for the caller to test its rank.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../kite3_noderoot.gen.hpp"
#include "../kite3_tables.hpp"

namespace {

std::vector<double> read(const char* path) {
    std::vector<double> v;
    std::ifstream f(path);
    double x;
    while (f >> x) v.push_back(x);
    return v;
}

struct PlainIn {
    const double* w;
    double operator()(int i) const { return w[i]; }
};

struct SeedIn {
    const double* w;
    int input;
    awe::Dual operator()(int i) const { return awe::Dual(w[i], i == input ? 1.0 : 0.0); }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    using namespace awe_k3root;
    std::vector<double> cst = read(argv[1]), w = read(argv[2]);
    const double u_ref = std::atof(argv[3]);
    if ((int)cst.size() != K3_NCONST || (int)w.size() != k3t::kLanes) return 3;
    std::vector<double> val(kNRows, 0.0), tan(kNSlots, 0.0);
    k3_node_root<1>(PlainIn{w.data()}, u_ref, cst.data(), val.data(), tan.data());
    double dv = 0.0, dt = 0.0, tmax = 0.0;
    int covered = 0, tables = 0;
    std::vector<double> block(kNRows * kNUnk, 0.0);
    for (int j = 0; j < kNUnk; ++j) {
        const int input = j < K3_NX ? K3_NX + j : awe::k3::Z_LAMBDA;
        awe::Kite3Result<awe::Dual> res;
        awe::kite3_node<awe::Dual>(SeedIn{w.data(), input}, awe::Dual(w[k3t::kDirGamma]), u_ref, cst.data(), res, false);
        for (int r = 0; r < kNRows; ++r) {
            const awe::Dual ref = res.eq[r];
            if (j == 0) dv = std::fmax(dv, std::fabs(val[r] - ref.v) / std::fmax(1.0, std::fabs(ref.v)));
            const int s = kSlot[r][j];
            const double got = s >= 0 ? tan[s] : 0.0;
            if (s >= 0) {
                ++covered;
                if (s < kNSlots && kEntry[s] == r * kNUnk + j) ++tables;
            }
            block[r * kNUnk + j] = got;
            tmax = std::fmax(tmax, std::fabs(ref.d));
            dt = std::fmax(dt, std::fabs(got - ref.d) / std::fmax(1.0, std::fabs(ref.d)));
        }
    }
    std::printf("{\"value_rel\": %.3e, \"entry_rel\": %.3e, \"entry_max\": %.3e, \"entries\": %d, \"entry_table\": %d, "
                "\"n_slots\": %d, \"block\": [", dv, dt, tmax, covered, tables, kNSlots);
    for (int e = 0; e < kNRows * kNUnk; ++e) std::printf("%s%.17g", e ? ", " : "", block[e]);
    std::printf("]}\n");
    return 0;
}
