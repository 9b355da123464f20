/*
 * awegpu, rk4root re-integration -- the part of libawegpu.so's C ABI that integrates the AP2 kite's DAE
 * (same conventions as awegpu.h: extern "C", plain pointers and sizes, 0 on success, awe_last_error()).
 *
 * Kept beside awegpu.h, not in it: awegpu.h carries the layout constants of the node models and is a hashed
 * input of every generated node header, so a declaration added there rewrites all of them.
 */
#ifndef AWEGPU_RK4ROOT_H
#define AWEGPU_RK4ROOT_H

#include "awegpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rk4root re-integration (the reference's tools/integrator_routines.py:32-96, as its
 * test/reg/test_discretization.py and sim.py's open_loop run it): n_fe classical Runge-Kutta steps per
 * sampling time on x' = xdot, where y = (xdot[23], z[1]) solves the shooting node's 24 model equalities at
 * every stage state (Newton, warm-started, at most max_newton solves, stop below tol) and once more at the
 * end of every sampling time; the power integrand lambda10 l_t dl_t [W] is integrated by the same stages.
 * One lane per task, one launch (ap2_rk4root_kernel).  Per-task rows, task t:
 *   x0[t][23], y0[t][24] (warm start), u[t][n_steps][AWE_NU] (the control held over sampling time s),
 *   par[t][n_par] (awe_rk4root_par_layout), ts[t] (length of one sampling time, s);
 *   xf[t][n_steps][23], yf[t][24] at the last state, qf[t][n_steps] in J, res[t] the largest rootfinder
 *   residual at exit (non-finite for a task that met a NaN; the other tasks are not affected).
 * n_tasks is any positive number (it is not the handle's batch).  Device pointers, asynchronous on
 * `stream`.  Constants whose integer structure (tether elements, stability-table lengths) is not the one
 * the node code was generated for are refused. */
int awe_integrate_rk4root(awe_handle h, int n_tasks, const double* x0, const double* u, const double* y0,
                          const double* par, const double* ts, int n_fe, int n_steps, int max_newton, double tol,
                          double* xf, double* yf, double* qf, double* res, void* stream);
/* The same core on the host: host pointers, no device and no handle. */
int awe_integrate_rk4root_cpu(const double* consts, int n_consts, int n_tasks, const double* x0, const double* u,
                              const double* y0, const double* par, const double* ts, int n_fe, int n_steps,
                              int max_newton, double tol, double* xf, double* yf, double* qf, double* res);
/* A task's parameter row: *n_par entries; src[i] < 1000 is node variable src[i] (57 theta.diam_t,
 * 58 theta.t_f, 59 phi.gamma), src[i] >= 1000 is theta0 entry src[i] - 1000.  src may be NULL. */
int awe_rk4root_par_layout(int* n_par, int* src);
/* Kernel time of the last awe_integrate_rk4root call (HIP events), milliseconds. */
int awe_last_integrate_ms(awe_handle h, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* AWEGPU_RK4ROOT_H */
