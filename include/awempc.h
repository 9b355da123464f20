/*
 * awempc -- MI355X evaluator for the awebox tracking-MPC NLP of a 3-DOF kite (SURVEY.md section 8
 * row a37, config 5: examples/mpc_closed_loop.py, horizon N, radau d, zoh controls).
 *
 * C ABI (extern "C", plain pointers and sizes).  The entry points are the NLP oracle surface the
 * MPC's IPOPT solver reaches through CasADi in the reference:
 *
 *   reference: ct.nlpsol('solver', 'ipopt', {'x': V, 'p': p, 'f': f, 'g': g_fun(V, P_fun(p))})
 *              awebox/pmpc.py:193-217, called per MPC step at pmpc.py:252-270 with
 *              p = [x0, ref, u_ref, Q, R, P] (pmpc.py:166-186)
 *
 *   awempc_eval_nlp      <->  nlp_grad_f + nlp_jac_g fused (f, g, grad f, J_g values)
 *   awempc_sparsity_jac  <->  Sparsity of nlp_jac_g's output (CCS: colind[n_v+1], row[nnz])
 *   awempc_eval_hess     <->  nlp_hess_l: sigma f + lam^T g, upper triangle in a fixed CCS pattern
 *                             (IPOPT's exact Hessian, awebox/opts/default.py:323, pmpc.py:193-217)
 *   awempc_sparsity_hess <->  Sparsity of nlp_hess_l's output
 *
 * Memory: V[b*n_v + i], p[b*n_p + i], g[b*n_g + i], grad_f[b*n_v + i], jac[b*nnz + i], f[b] are
 * device pointers for awempc_eval_nlp, host pointers for awempc_eval_nlp_host.  Return codes as in
 * awegpu.h (0 = OK; awempc_last_error() describes a failure; a NaN/Inf in any output of the host
 * wrapper returns AWE_ERR_NONFINITE).  One handle per host thread; `batch` MPC instances (one per
 * simulated system or per real-time iteration) are evaluated per call.
 */
#ifndef AWEMPC_H
#define AWEMPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- node-variable layout (awebox/mdl/system.py:42-230, kite_dof 3, tether control dddl_t):
 *      x = [q10(3) dq10(3) coeff10(2) l_t dl_t ddl_t], xdot = d<x>, u = [f_fict10(3) dcoeff10(2)
 *      dddl_t], z = [lambda10], theta = [diam_t t_f] */
#define K3_NX 11
#define K3_NU 6
#define K3_NZ 1
#define K3_NTH 2
#define K3_NW 31
#define K3_N_EQ 12
#define K3_N_INEQ 2
#define K3_NPHI 7
#define K3_NXI 2

/* ---- model constants vector -- keep in sync with awebox_amd/kite3.py CONST_NAMES */
#define K3_C_N_K 0
#define K3_C_D 1
#define K3_C_G 2
#define K3_C_T_REF 3
#define K3_C_RHO_REF 4
#define K3_C_GAMMA_AIR 5
#define K3_C_R_AIR 6
#define K3_C_Z_REF 7
#define K3_C_Z0_AIR 8
#define K3_C_KAPPA 9
#define K3_C_RHO_TETHER 10
#define K3_C_CD_TETHER 11
#define K3_C_STRESS_MAX 12
#define K3_C_M_K 13
#define K3_C_S_REF 14
#define K3_C_AR 15
#define K3_C_CD0 16
#define K3_C_ACC_MAX 17
#define K3_C_SCALING_LENGTH 18
#define K3_C_SCALING_DIAM 19
#define K3_C_G_SCALING 20
#define K3_C_Q_SCALING_MEAN 21
#define K3_C_LAMBDA_SCALING 22
#define K3_C_N_ELEMENTS 23
#define K3_C_SCALING 24 /* [31] */
#define K3_NCONST 55

typedef struct awempc_handle_s* awempc_handle;

/* Build the evaluator for horizon n_k, d radau nodes, `batch` instances per call. */
int awempc_create(int n_k, int d, const double* consts, int n_consts, int batch, awempc_handle* out);
int awempc_destroy(awempc_handle h);
const char* awempc_last_error(void);

/* n_v = 22 + n_k (2 nx + nu + nz + d (nx + nz)), n_g = nx + n_k (n_eq + n_ineq + d n_eq + nx),
 * n_p = n_v + 2 nx + nu + nx + 1 */
int awempc_sizes(awempc_handle h, int* n_v, int* n_g, int* n_p, int* nnz_jac);
int awempc_sparsity_jac(awempc_handle h, int* colind, int* row);
/* the same pattern without a device; colind = row = NULL returns *nnz */
int awempc_sparsity_jac_static(int n_k, int d, const double* consts, int n_consts, int* nnz, int* colind,
                               int* row);

/* device pointers, asynchronous on `stream` (NULL = default stream) */
int awempc_eval_nlp(awempc_handle h, const double* V, const double* p, double* f, double* g, double* grad_f,
                    double* jac, void* stream);
/* host pointers: copy in, evaluate, copy out, synchronise, check finiteness */
int awempc_eval_nlp_host(awempc_handle h, const double* V, const double* p, double* f, double* g,
                         double* grad_f, double* jac);
/* kernel time of the last awempc_eval_nlp (HIP events on its stream), ms */
int awempc_last_kernel_ms(awempc_handle h, float* ms_main, float* ms_finalize);

/* ---- generated instance-minor path ------------------------------------------------------------
 * The same f, g, grad f and J_g values from straight-line node code generated from the model
 * (csrc/gen/kite3_jacgen.cpp: the sparse Jacobian of each node, one lane per instance) instead of the
 * dual-number kernel of awempc_eval_nlp.  grad_f and jac are instance-minor: grad_f[i * ld + b],
 * jac[e * ld + b], ld >= batch (each J_g / gradient row of all instances contiguous, the layout the
 * batched solvers read); V, p, f, g as above.  Device pointers, asynchronous on `stream`.
 * awempc_gen_status sets *available = 0 (awempc_last_error() says why) when the model constants do
 * not have the integer structure the code was generated for. */
int awempc_gen_status(awempc_handle h, int* available);
int awempc_eval_nlp_im(awempc_handle h, const double* V, const double* p, double* f, double* g, double* grad_f,
                       double* jac, size_t ld, void* stream);
/* kernel times of the last awempc_eval_nlp_im: input transposition, node kernel, finalize (ms) */
int awempc_last_kernel_ms_im(awempc_handle h, float* ms_in, float* ms_node, float* ms_finalize);

/* ---- the simulation plant ---------------------------------------------------------------------
 * sim.py's plant (sim.py:72-78): rk4root over n_steps sampling times of length ts [s], n_fe RK4 steps
 * each, the control of a sampling time held over it; at every stage, and at the end of every sampling
 * time, a Newton rootfinder solves the shooting node's 12 equalities for (xdot, z) (at most max_newton
 * solves, until max |row| < tol), warm-started from the previous one.  One launch, one lane per loop.
 * x0[B][11], u[B][n_steps][6] (scaled), z0[B][12] = rootfinder guess (xdot(11), lambda), par[B][4] =
 * theta.diam_t, theta.t_f, phi.gamma (scaled), u_ref.  Out: xf[B][n_steps][11], zf[B][12] at the last
 * xf, qf[B][n_steps] = the power integral of each sampling time [J], res[B] = the largest rootfinder
 * residual at exit.  B = the handle's batch.  Device pointers, asynchronous on `stream`. */
int awempc_plant_rk4root(awempc_handle h, const double* x0, const double* u, const double* z0, const double* par,
                         double ts, int n_fe, int n_steps, int max_newton, double tol, double* xf, double* zf,
                         double* qf, double* res, void* stream);
/* the same core on the host, no device and no handle (as the *_static sparsity calls): host pointers */
int awempc_plant_rk4root_cpu(const double* consts, int n_consts, int batch, const double* x0, const double* u,
                             const double* z0, const double* par, double ts, int n_fe, int n_steps, int max_newton,
                             double tol, double* xf, double* zf, double* qf, double* res);
/* kernel time of the last awempc_plant_rk4root (HIP events on its stream), ms */
int awempc_last_plant_ms(awempc_handle h, float* ms);

/* ---- the reference generator ------------------------------------------------------------------
 * Pmpc's reference windows (pmpc.py:408-550: get_reference on the interpolated periodic solution): a
 * periodic trajectory, given as piecewise polynomials, evaluated at every time of a loop's horizon
 * (reduced as t - T floor(t / T)) and written as the loop's V-shaped window.  One launch for all loops,
 * one thread per (loop, time point).
 * A table is three grids, in this order: the states (K3_NX channels), the algebraic variables (K3_NZ)
 * and what an interval holds (K3_NU + K3_NX + K3_NZ: u, then the shooting node's xdot and z).  Grid g
 * has pieces[g] pieces of degree[g]; brk = the grids' breakpoints one after another (pieces[g] + 1
 * each, strictly ascending from 0 to the period), coef = their coefficients one after another,
 * [piece][channel][degree + 1] in s = (t - b_i) / (b_{i+1} - b_i), lowest power first.
 * offs[(n_k + 1) + n_k d + n_k]: the time offsets of the shooting, collocation (interval-major) and
 * control points from the window's start; head[K3_NTH + K3_NPHI + K3_NXI]: theta, phi, xi as written.
 * awempc_ref_set refuses (awempc_last_error() says why) a degree above 7 or more than 2048 breakpoints
 * in all: what the kernel's LDS staging holds.  The handle keeps its own device copy of the table.
 * awempc_ref_window: t0[B] and out are device pointers, out[b * ld + off + i] for i < n_v (ld = n_p,
 * off = n_x writes the `ref` entry of p in place); asynchronous on `stream`.  A NaN or infinite t0[b]
 * gives loop b a non-finite window and touches nothing else. */
int awempc_ref_set(awempc_handle h, double period, const double* offs, const double* head, const int* pieces,
                   const int* degree, const double* brk, const double* coef);
int awempc_ref_window(awempc_handle h, const double* t0, double* out, size_t ld, size_t off, void* stream);
/* the same core on the host, no device and no handle: host pointers */
int awempc_ref_window_cpu(int n_k, int d, int batch, double period, const double* offs, const double* head,
                          const int* pieces, const int* degree, const double* brk, const double* coef,
                          const double* t0, double* out, size_t ld, size_t off);
/* kernel time of the last awempc_ref_window (HIP events on its stream), ms */
int awempc_last_ref_ms(awempc_handle h, float* ms);

/* ---- nlp_hess_l ----------------------------------------------------------------------------------
 * Hessian of sigma f + lam^T g w.r.t. V, upper triangle (row <= col), CCS over the n_v columns:
 * H[b*nnz_h + i].  sigma[b], lam[b*n_g + i].  The structure is derived on the host from the node
 * model's second-order dependencies (built on the first call). */
int awempc_hess_init(awempc_handle h, int* nnz_h);
int awempc_sparsity_hess(awempc_handle h, int* colind, int* row);
/* the same pattern without a device; colind = row = NULL returns *nnz */
int awempc_sparsity_hess_static(int n_k, int d, const double* consts, int n_consts, int* nnz, int* colind,
                                int* row);
/* device pointers, asynchronous on `stream` */
int awempc_eval_hess(awempc_handle h, const double* V, const double* p, const double* sigma, const double* lam_g,
                     double* H, void* stream);
/* host pointers: copy in, evaluate, copy out, synchronise, check finiteness */
int awempc_eval_hess_host(awempc_handle h, const double* V, const double* p, const double* sigma,
                          const double* lam_g, double* H);
/* kernel time (Hessian + finalize) of the last awempc_eval_hess, ms */
int awempc_last_hess_ms(awempc_handle h, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* AWEMPC_H */
