// Stand-alone driver of the reference generator's core (../ref_pp.hpp) for a sanitizer build on the host:
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//         check_ref_pp.cpp -o check_ref_pp && ./check_ref_pp
//
// Three loops through every point of a small window, each output row in a heap block of exactly n_v
// doubles and every table in a block of exactly its size, so a read or write one past any of them is
// reported: an ordinary start time, a NaN one and one far beyond the period; then tables that
// ref_check must refuse.  Exit status 0 and "check_ref_pp: OK" when everything held.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../ref_pp.hpp"

int main() {
    using namespace awe;
    const int n_k = 3, d = 2, nx = 11, nu = 6, nz = 1, n_head = 11, batch = 3;
    const int stride = 2 * nx + nu + nz + d * (nx + nz), n_v = n_head + n_k * stride + nx;
    const double T = 0.75;
    const int pieces[kRefGrids] = {7, 5, 4}, degree[kRefGrids] = {3, 1, 0}, channels[kRefGrids] = {nx, nz, nu + nx + nz};
    std::vector<double> brk;
    std::vector<std::vector<double>> coef(kRefGrids);
    for (int g = 0; g < kRefGrids; ++g) {
        for (int i = 0; i <= pieces[g]; ++i) brk.push_back(i == pieces[g] ? T : T * i / pieces[g]);
        coef[g].resize((size_t)pieces[g] * channels[g] * (degree[g] + 1));
        for (size_t i = 0; i < coef[g].size(); ++i) coef[g][i] = 0.25 + 0.001 * (double)i;
    }
    if (ref_check(pieces, degree, brk.data(), T)) return std::puts("check_ref_pp: a valid table was refused"), 1;
    std::vector<double> offs, head(n_head, 0.5);
    const double ts = 0.1, tau[2] = {1.0 / 3.0, 1.0};
    for (int k = 0; k <= n_k; ++k) offs.push_back(k * ts);
    for (int k = 0; k < n_k; ++k)
        for (int j = 0; j < d; ++j) offs.push_back((k + tau[j]) * ts);
    for (int k = 0; k < n_k; ++k) offs.push_back(k * ts);
    const std::vector<double> t0 = {0.2, std::numeric_limits<double>::quiet_NaN(), 1e9 * T + 0.3};
    RefArgs a{};
    int b0 = 0;
    for (int g = 0; g < kRefGrids; ++g) {
        a.g[g] = RefGrid{b0, pieces[g], degree[g], channels[g], coef[g].data()};
        b0 += pieces[g] + 1;
    }
    a.period = T, a.offs = offs.data(), a.head = head.data(), a.t0 = t0.data();
    a.n_k = n_k, a.d = d, a.n_head = n_head, a.nx = nx, a.nu = nu, a.nz = nz, a.batch = batch;
    a.ld = 0, a.off = 0;
    if ((int)offs.size() != ref_points(n_k, d)) return std::puts("check_ref_pp: point count"), 1;
    int bad = 0;
    for (int b = 0; b < batch; ++b) {
        std::vector<double> row((size_t)n_v, -7.0);          // its own block: b * ld = 0
        RefArgs ab = a;
        ab.t0 = t0.data() + b, ab.out = row.data();
        for (int q = 0; q < ref_points(n_k, d); ++q) ref_point(ab, brk.data(), 0, q);
        int finite = 0, untouched = 0;
        for (double v : row) finite += std::isfinite(v), untouched += v == -7.0;
        std::printf("loop %d: t0 = %g, %d of %d entries finite, %d not written\n", b, t0[b], finite, n_v, untouched);
        bad += untouched != 0;
        bad += (b == 1) ? !std::isnan(row[n_head]) : finite != n_v;
    }
    // refused: degree, piece count, breakpoints out of order, a period that is not one
    const int deg_big[kRefGrids] = {kRefMaxDeg + 1, 1, 0}, pc_big[kRefGrids] = {kRefMaxBrk, 5, 4};
    std::vector<double> many((size_t)kRefMaxBrk + 16, 0.0), unsorted = brk;
    for (size_t i = 0; i < many.size(); ++i) many[i] = (double)i;
    unsorted[2] = unsorted[1];
    bad += !ref_check(pieces, deg_big, brk.data(), T);
    bad += !ref_check(pc_big, degree, many.data(), T);
    bad += !ref_check(pieces, degree, unsorted.data(), T);
    bad += !ref_check(pieces, degree, brk.data(), std::numeric_limits<double>::quiet_NaN());
    std::printf("refused: %s\n", ref_check(pieces, deg_big, brk.data(), T));
    std::puts(bad ? "check_ref_pp: FAILED" : "check_ref_pp: OK");
    return bad ? 1 : 0;
}
