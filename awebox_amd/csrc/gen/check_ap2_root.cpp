// Host check of the generated AP2 rootfinder node code (ap2_noderoot.gen.hpp) against the templated model on
// dual numbers: one forward pass of ap2_node per unknown (xdot_0..22, z.lambda10), seeded on that node input
// alone, and of the structured Newton step (explicit rows in closed form, couplings, dense K x K LU) against
// a dense 24 x 24 LU step with partial pivoting on the same dual-number Jacobian.
//
//   check_ap2_root <consts (135)> <node values (59 + gamma)> <theta0 (200)>
//
// Prints one JSON line: the largest relative row, entry and integrand differences, the number of slots that
// are pattern entries, the partition's sizes and the largest difference of the two Newton steps relative to
// the largest step entry.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../ap2_model.hpp"
#include "../ap2_noderoot.gen.hpp"
#include "../plant_rk4root.hpp"

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

using namespace awe_ap2root;

struct DenseSys {   // the K x K block as rk4root_lu_solve sees it
    double A[K * K], b[K];
    double& a(int i, int j) { return A[i * K + j]; }
    double& r(int i) { return b[i]; }
};
struct FullSys {
    double A[kNUnk * kNUnk], b[kNUnk];
    double& a(int i, int j) { return A[i * kNUnk + j]; }
    double& r(int i) { return b[i]; }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<double> cst = read(argv[1]), w = read(argv[2]), th = read(argv[3]);
    if ((int)cst.size() != AWE_NCONST || (int)w.size() != AWE_NW + 1 || (int)th.size() != AWE_NTHETA0) return 3;
    std::vector<double> val(kNRows, 0.0), tan(kNSlots, 0.0);
    double pw = 0.0;
    ap2_node_root<1>(PlainIn{w.data()}, th.data(), cst.data(), val.data(), tan.data(), &pw);

    double dv = 0.0, dt = 0.0, tmax = 0.0, dp = 0.0;
    int covered = 0, tables = 0;
    FullSys full;
    for (int j = 0; j < kNUnk; ++j) {
        const int input = j < AWE_NX ? AWE_NX + j : 2 * AWE_NX + AWE_NU;
        awe::NodeResult<awe::Dual> res;
        awe::ap2_node<awe::Dual>(SeedIn{w.data(), input}, awe::Dual(w[AWE_NW]), th.data(), cst.data(), res, false);
        if (j == 0) {
            const double ref = res.pw.v * cst[AWE_C_ENERGY_SCALING];
            dp = std::fabs(pw - ref) / std::fmax(1.0, std::fabs(ref));
        }
        for (int r = 0; r < kNRows; ++r) {
            const awe::Dual ref = res.eq[r];
            if (j == 0) {
                dv = std::fmax(dv, std::fabs(val[r] - ref.v) / std::fmax(1.0, std::fabs(ref.v)));
                full.r(r) = ref.v;
            }
            const int s = kSlot[r][j];
            const double got = s >= 0 ? tan[s] : 0.0;
            if (s >= 0) {
                ++covered;
                if (s < kNSlots && kEntry[s] == r * kNUnk + j) ++tables;
            }
            full.a(r, j) = ref.d;
            tmax = std::fmax(tmax, std::fabs(ref.d));
            dt = std::fmax(dt, std::fabs(got - ref.d) / std::fmax(1.0, std::fabs(ref.d)));
        }
    }

    // the structured step from the generated values
    std::vector<double> step(kNUnk, 0.0), ex(kNExtra > 0 ? kNExtra : 1, 0.0), expl(kNExpl > 0 ? kNExpl : 1, 0.0);
    DenseSys ds;
    for (int e = 0; e < K * K; ++e) ds.A[e] = 0.0;
    for (int s = 0; s < kNSlots; ++s) {
        if (kDest[s] >= 0) ds.A[kDest[s]] = tan[s];
        else ex[-1 - kDest[s]] = tan[s];
    }
    for (int i = 0; i < K; ++i) ds.b[i] = val[kDenseRow[i]];
    for (int n = 0; n < kNExpl; ++n) {
        expl[n] = val[kExplRow[n]] / ex[kExplExtra[n]];
        step[kExplUnk[n]] = expl[n];
    }
    for (int m = 0; m < kNCoup; ++m) ds.b[kCoupRow[m]] -= ex[kCoupExtra[m]] * expl[kCoupExpl[m]];
    awe::rk4root_lu_solve<K>(ds);
    for (int i = 0; i < K; ++i) step[kDenseUnk[i]] = ds.b[i];
    // the dense 24 x 24 step from the dual-number Jacobian
    awe::rk4root_lu_solve<kNUnk>(full);
    double smax = 0.0, dstep = 0.0;
    for (int j = 0; j < kNUnk; ++j) smax = std::fmax(smax, std::fabs(full.b[j]));
    for (int j = 0; j < kNUnk; ++j) dstep = std::fmax(dstep, std::fabs(step[j] - full.b[j]) / smax);

    std::printf("{\"value_rel\": %.3e, \"entry_rel\": %.3e, \"entry_max\": %.3e, \"integrand_rel\": %.3e, \"entries\": %d, "
                "\"entry_table\": %d, \"n_slots\": %d, \"K\": %d, \"explicit\": %d, \"couplings\": %d, \"step_rel\": %.3e, "
                "\"step_max\": %.3e}\n",
                dv, dt, tmax, dp, covered, tables, kNSlots, K, kNExpl, kNCoup, dstep, smax);
    return 0;
}
