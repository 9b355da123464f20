// The tracking MPC's reference generator (pmpc.py:408-550: __create_reference_interpolator,
// get_reference) for ONE (loop, time point): a periodic trajectory given as piecewise polynomials is
// evaluated at the point's time, reduced modulo the period, and the values are written into the loop's
// V-shaped reference window.  Compiles for the host and the device: the kernel runs one thread per
// (loop, point) with the breakpoints in LDS (awempc.hip: mpc_ref_window_kernel), the host entry point a
// loop over the same function.
//
// Nothing here knows the model or the interpolator.  A trajectory is three grids -- the states, the
// algebraic variables, and what is held over an interval (the control, then the shooting node's xdot and
// z) -- each with ascending breakpoints b_0 = 0 .. b_pieces = period, one degree and coefficients
// coef[piece][channel][degree + 1] in the local variable s = (t - b_i) / (b_{i+1} - b_i), lowest power
// first, evaluated by Horner's rule.
//
// Every operation is rounded on its own (contraction off) and Horner's steps are explicit fma's, so the
// host and the device execute the same IEEE operations in the same order.  The piece index is clamped as
// an integer after the search: a NaN or infinite time fails every comparison, lands in a valid piece and
// yields non-finite values, never an out-of-range read.
#pragma once

#include <cmath>
#include <cstddef>

#include "scalar.hpp"

namespace awe {

constexpr int kRefGrids = 3;          // x, z, held
constexpr int kRefMaxBrk = 2048;      // breakpoints of the three grids together (the kernel's LDS staging)
constexpr int kRefMaxDeg = 7;         // polynomial degree per piece

struct RefGrid {
    int brk0;             // first breakpoint of the grid in the shared breakpoint array
    int pieces, degree, channels;
    const double* coef;   // [pieces][channels][degree + 1]
};

struct RefArgs {
    RefGrid g[kRefGrids];
    double period;
    const double* offs;   // [n_pt] time offsets: n_k + 1 shooting, n_k d collocation, n_k control points
    const double* head;   // [n_head] the window's leading entries (theta, phi, xi)
    const double* t0;     // [batch] start time of every loop's window
    double* out;          // out[b * ld + off + i], i < n_head + n_k stride + nx
    size_t ld, off;
    int n_k, d, n_head, nx, nu, nz, batch;
};

AWE_HD int ref_points(int n_k, int d) { return (n_k + 1) + n_k * d + n_k; }

// t - T floor(t / T): in [0, T] for a finite t (T itself where the quotient rounds up to an integer)
AWE_HD double ref_reduce(double t, double T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double q = ::floor(t / T);
    const double w = T * q;
    return t - w;
}

// the grid's channels at time t (already reduced) -> dst[0 .. channels).  A time on a breakpoint belongs
// to the piece it opens, or with `closing` to the piece it closes: a collocation node (tau in (0, 1], Radau's
// tau_d = 1) is read from the interval it lies in, so a window aligned with the trajectory's grid
// reproduces the stored node values, the algebraic ones included.
AWE_HD void ref_eval(const RefGrid& g, const double* brk_all, double t, double* dst, bool closing) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double* brk = brk_all + g.brk0;
    int lo = 0, hi = g.pieces;                     // b[lo] <= t < b[hi]; m stays in [1, pieces - 1]
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (closing ? t > brk[m] : t >= brk[m]) lo = m;
        else hi = m;
    }
    lo = lo < 0 ? 0 : (lo > g.pieces - 1 ? g.pieces - 1 : lo);
    const double b0 = brk[lo], b1 = brk[lo + 1];
    const double num = t - b0, den = b1 - b0;
    const double s = num / den;
    const int nc = g.degree + 1;
    const double* c = g.coef + (size_t)lo * g.channels * nc;
    for (int ch = 0; ch < g.channels; ++ch, c += nc) {
        double v = c[g.degree];
        for (int p = g.degree - 1; p >= 0; --p) v = ::fma(v, s, c[p]);
        dst[ch] = v;
    }
}

// point q of loop b: its entries of the window
AWE_HD void ref_point(const RefArgs& a, const double* brk_all, size_t b, int q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t_raw = a.t0[b] + a.offs[q];
    const double t = ref_reduce(t_raw, a.period);
    const int stride = a.nx + a.nu + a.nx + a.nz + a.d * (a.nx + a.nz);
    double* o = a.out + b * a.ld + a.off;
    if (q <= a.n_k) {                                            // shooting state x[q]
        if (q == 0)
            for (int i = 0; i < a.n_head; ++i) o[i] = a.head[i];
        ref_eval(a.g[0], brk_all, t, o + a.n_head + (size_t)q * stride, false);
        return;
    }
    const int c = q - (a.n_k + 1);
    if (c < a.n_k * a.d) {                                       // collocation node (k, j): x, then z
        const int k = c / a.d, j = c - k * a.d;
        double* dst = o + a.n_head + (size_t)k * stride + 2 * a.nx + a.nu + a.nz + (size_t)j * (a.nx + a.nz);
        ref_eval(a.g[0], brk_all, t, dst, true);
        ref_eval(a.g[1], brk_all, t, dst + a.nx, true);
        return;
    }
    const int k = c - a.n_k * a.d;                               // what interval k holds: u, xdot, z
    ref_eval(a.g[2], brk_all, t, o + a.n_head + (size_t)k * stride + a.nx, false);
}

// Why a table cannot be served, or nullptr.  brk: the grids' breakpoints one after another.
inline const char* ref_check(const int* pieces, const int* degree, const double* brk, double period) {
    if (!pieces || !degree || !brk) return "null argument";
    if (!(period > 0.0) || !std::isfinite(period)) return "the period must be positive and finite";
    long total = 0;
    for (int g = 0; g < kRefGrids; ++g) {
        if (pieces[g] < 1) return "a grid needs at least one piece";
        if (degree[g] < 0 || degree[g] > kRefMaxDeg) return "polynomial degree beyond the kernel's limit (7)";
        if (pieces[g] > kRefMaxBrk) return "more breakpoints than the kernel's LDS staging holds (2048)";
        total += pieces[g] + 1;
    }
    if (total > kRefMaxBrk) return "more breakpoints than the kernel's LDS staging holds (2048)";
    const double* b = brk;
    for (int g = 0; g < kRefGrids; ++g) {
        for (int i = 0; i < pieces[g]; ++i)
            if (!(b[i + 1] > b[i])) return "breakpoints must be finite and strictly ascending";
        b += pieces[g] + 1;
    }
    return nullptr;
}

}  // namespace awe
