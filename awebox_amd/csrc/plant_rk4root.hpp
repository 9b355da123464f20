// The reference's simulation plant, rk4root (sim.py:72-78 -> tools/integrator_routines.py:32-96), for ONE
// instance: n_fe classical Runge-Kutta steps per sampling time on x' = xdot(x), where the derivative and
// algebraic variables y = (xdot, z) solve the shooting node's NUNK model equalities at the stage state
// (a Newton rootfinder, warm-started from the previous one), the applied control held over the sampling
// time, and a rootfinder at the end of every sampling time, which gives z there.  Compiles for the host
// and the device: the kernel runs one lane per instance (awempc.hip: mpc_plant_rk4root_kernel), the host
// entry point a loop over the instances.
//
// Nothing here knows the model.  `Node` supplies
//     void begin(int step)                            the sampling time's control becomes the applied one;
//     void eval(int step, const double* x, const double* y, Sys& sys) const
//         rows sys.r(i) and the dense block sys.a(i, j) = d row_i / d y_j at (x, y), control of `step`;
//     void solve(Sys& sys, double* y) const           one Newton step y -= A^-1 r from what eval left in sys: a
//         dense node calls rk4root_solve_update<NUNK>; a node whose rows partly hold one unknown alone (the
//         AP2 kite: 17 of 24) solves those in closed form and hands rk4root_lu_solve<K> the K x K rest;
//     double integrand(int step, const double* x, const double* y) const     the quadrature's integrand at
//         the (x, y) of the rootfinder call before it;
//     double rate(int i, double ydot_i) const         dx_i / dt [1/s] from y_i (the scaling ratio);
// and `Sys` holds the matrix and the NUNK-row right-hand side of the instance wherever its owner keeps them
// (the kernel: LDS, lane-minor; the host: a plain array), through r(i) and a(i, j) returning references.
//
// Every loop's trip count is an argument or a constant: no loop waits on convergence.  A comparison with
// a NaN is false, so an instance that meets one keeps its pivot row, takes max_newton iterations and
// runs to the end with a non-finite residual.
#pragma once

#include "scalar.hpp"

namespace awe {

// LU with partial pivoting of sys.a in place and the solve of sys.a dy = sys.r; dy is left in sys.r.
// Fully unrolled: every index but the pivot row's is a constant, so the pivot row lives in registers
// and the matrix is addressed at fixed offsets.  The row exchange is unconditional (row k with itself
// when the pivot is in place): no divergence between the lanes of a wavefront.
template <int N, class Sys>
AWE_HD void rk4root_lu_solve(Sys& sys) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int p = k;
        double amax = ::fabs(sys.a(k, k));
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const double v = ::fabs(sys.a(i, k));
            if (v > amax) { amax = v; p = i; }
        }
        double row[N];
#pragma unroll
        for (int j = k; j < N; ++j) {
            const double t = sys.a(k, j);
            row[j] = sys.a(p, j);
            sys.a(p, j) = t;
            sys.a(k, j) = row[j];
        }
        const double tb = sys.r(k), bk = sys.r(p);
        sys.r(p) = tb;
        sys.r(k) = bk;
        const double inv = 1.0 / row[k];
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const double m = sys.a(i, k) * inv;
#pragma unroll
            for (int j = k + 1; j < N; ++j) sys.a(i, j) -= m * row[j];
            sys.r(i) -= m * bk;
        }
    }
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
        double s = sys.r(k);
#pragma unroll
        for (int j = k + 1; j < N; ++j) s -= sys.a(k, j) * sys.r(j);
        sys.r(k) = s / sys.a(k, k);
    }
}

// The dense Newton step: y -= A^-1 r with all NUNK rows in the LU.
template <int NUNK, class Sys>
AWE_HD void rk4root_solve_update(Sys& sys, double* y) {
    rk4root_lu_solve<NUNK>(sys);
#pragma unroll
    for (int i = 0; i < NUNK; ++i) y[i] -= sys.r(i);
}

// Newton on the node rows for y at the state x: evaluate, res = max |row|, stop when res < tol or after
// max_newton solves, otherwise node.solve (y -= A^-1 r).  Returns res at exit.
template <int NUNK, class Node, class Sys>
AWE_HD double rk4root_find(const Node& node, int step, const double* x, double* y, Sys& sys, int max_newton,
                           double tol) {
    double res = 0.0;
#pragma unroll 1
    for (int it = 0; it <= max_newton; ++it) {
        node.eval(step, x, y, sys);
        res = 0.0;
        bool nan = false;
#pragma unroll
        for (int i = 0; i < NUNK; ++i) {
            const double v = ::fabs(sys.r(i));
            nan = nan || (v != v);
            res = v > res ? v : res;
        }
        if (nan) res = __builtin_nan("");
        if (res < tol || it == max_newton) break;
        node.solve(sys, y);
    }
    return res;
}

// n_steps sampling times of length ts from x (in: x0, out: the last state) with the warm start y (out:
// (xdot, z) at the last state).  xf(s, i, v) / qf(s, v) receive state i and the quadrature of sampling time s.
// Returns the largest rootfinder residual at exit over all rootfinder calls.
template <int NX, int NUNK, class Node, class Sys, class XOut, class QOut>
AWE_HD double rk4root_run(Node& node, Sys& sys, double* x, double* y, double ts, int n_fe, int n_steps,
                          int max_newton, double tol, XOut xf, QOut qf) {
    const double h = ts / n_fe;
    double worst = 0.0;
    auto track = [&](double res) { worst = (res > worst || res != res) ? res : worst; };
#pragma unroll 1
    for (int s = 0; s < n_steps; ++s) {
        node.begin(s);
        double q = 0.0;
#pragma unroll 1
        for (int fe = 0; fe < n_fe; ++fe) {
            double xs[NX], acc[NX];
            double pacc = 0.0;
#pragma unroll
            for (int i = 0; i < NX; ++i) { xs[i] = x[i]; acc[i] = 0.0; }
            // stage st < 4 at x + c h k_{st-1}, c = 0, 1/2, 1/2, 1, weights 1, 2, 2, 1; the sampling time's
            // last step runs a fifth rootfinder at its end state (one call site for the node code)
            const int n_st = fe == n_fe - 1 ? 5 : 4;
#pragma unroll 1
            for (int st = 0; st < n_st; ++st) {
                const double ch = st == 3 ? h : 0.5 * h;
                const double wt = (st == 1 || st == 2) ? 2.0 : 1.0;
                if (st > 0) {
#pragma unroll
                    for (int i = 0; i < NX; ++i) xs[i] = st == 4 ? x[i] : x[i] + ch * node.rate(i, y[i]);
                }
                track(rk4root_find<NUNK>(node, s, xs, y, sys, max_newton, tol));
                if (st == 4) break;
#pragma unroll
                for (int i = 0; i < NX; ++i) acc[i] = st == 0 ? node.rate(i, y[i]) : acc[i] + wt * node.rate(i, y[i]);
                const double p = node.integrand(s, xs, y);
                pacc = st == 0 ? p : pacc + wt * p;
                if (st == 3) {
#pragma unroll
                    for (int i = 0; i < NX; ++i) x[i] = x[i] + h * acc[i] / 6.0;
                    q = q + h * pacc / 6.0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) xf(s, i, x[i]);
        qf(s, q);
    }
    return worst;
}

}  // namespace awe
