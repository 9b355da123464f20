// awempc -- MI355X (gfx950) evaluator for the awebox tracking-MPC NLP of a 3-DOF kite
// (pmpc.py:193-217; SURVEY.md section 8 row a37, config 5: B MPC instances per launch).
//
// Execution model (same shape as the AP2 evaluator, awegpu.hip, specialised for the small node):
//   * one workgroup per (MPC instance, horizon interval), W = ceil((d+1)/2) wavefronts; the
//     interval's slice of V and the parameters it reads are staged in LDS with coalesced loads;
//   * model pass: every half-wavefront evaluates ONE node of kite3_node in forward-mode dual
//     arithmetic with one seed direction per lane -- 31 node variables + phi.gamma = 32 lanes, so
//     a wavefront produces two complete node Jacobian blocks and no colouring is needed.  The
//     collocation chain rule xdot = C X / (h tf) is folded into the seeds (kite3_tables.hpp);
//   * tracking objective (pmpc.py:304-358) and its gradient are closed-form per V column;
//   * J_g values come from a host-built gather list (one entry per CCS slot: tangent index and
//     polynomial scale, or a constant for the initial-condition and continuity rows), so the J
//     stores of one interval are contiguous; a one-wave finalize kernel per instance reduces the
//     interval objective partials in a fixed order and adds the terminal cost (no float atomics).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/awegpu.h"
#include "../../include/awempc.h"
#include "host_util.hpp"
#include "im_layout.hpp"
#include "kite3_model.hpp"
#include "kite3_nodejac.gen.hpp"
#include "kite3_noderoot.gen.hpp"
#include "kite3_tables.hpp"
#include "plant_rk4root.hpp"
#include "ref_pp.hpp"

namespace {

using namespace k3t;
using namespace hostu;

struct MArgs {
    int n_k, d, n_v, n_g, n_p, nnz, stride;
    const double* V;
    const double* P;
    double* f;
    double* g;
    double* grad;
    double* jac;
    const double* cst;
    const awt::DevColl* coll;
    const int* goff;
    const int* gslot;
    const uint32_t* gcode;
    double* fpart;       // [B][n_k]
};

struct LaneIn {
    const double* w;     // node values (scaled), [32]
    const double* nc;    // LDS: C[n][n] / (h tf) at a Radau node (0 at the shooting node), 1 / tf
    int lane;
    __device__ __forceinline__ awe::Dual operator()(int i) const {
        double t = (i == lane) ? 1.0 : 0.0;
        if (i >= K3_NX && i < 2 * K3_NX) {
            // re-read at each use (volatile): two fewer live doubles per lane in the model pass
            const volatile double* vn = nc;
            if (lane == i - K3_NX) t = vn[0];
            if (lane == kDirTf) t = -w[i] * vn[1];
        }
        return awe::Dual(w[i], t);
    }
};

struct LaneSink {
    double* tang;        // node base: [row][32]
    double* gval;        // node base: [16]
    int lane;
    __device__ __forceinline__ void eq_row(int r, const awe::Dual& v) {
        tang[r * kLanes + lane] = v.d;
        if (lane == 0) gval[r] = v.v;
    }
    __device__ __forceinline__ void ineq_row(int r, const awe::Dual& v) { eq_row(K3_N_EQ + r, v); }
};

// Main-tether drag preaccumulated per node (K3InlineDrag's element sum): values and partials
// w.r.t. the scaled node variables q0..2, dq0..2, diam_t; pr = D[3] | dD/d(var j)[7][3].
constexpr int kDragDirs = 7, kDragStride = 24;
__device__ __forceinline__ int drag_var(int j) { return j < 6 ? j : awe::k3::TH_DIAM; }

struct LdsDrag {
    const double* pr;
    int lane;
    __device__ __forceinline__ void operator()(const awe::Dual*, const awe::Dual*, const awe::Dual&, double,
                                               const double*, awe::Dual D[3]) const {
        // lane = direction (uncompressed seeds): its tangent is the partial along its own variable
        const int j = lane < 6 ? lane : (lane == awe::k3::TH_DIAM ? 6 : -1);
#pragma unroll
        for (int i = 0; i < 3; ++i) D[i] = awe::Dual(pr[i], j >= 0 ? pr[3 + 3 * j + i] : 0.0);
    }
};

template <int D>
constexpr int waves_for() { return (D + 2) / 2; }

template <int D>
// 3 waves per SIMD (168 VGPRs, 15 spilled): four 3-wave workgroups per CU; 0.190 -> 0.146 ms at B = 256
// against 225 VGPRs and two workgroups (tools/mpc_variants.py)
__global__ __launch_bounds__(64 * waves_for<D>(), 3) void mpc_interval_kernel(MArgs a) {
    constexpr int NN = D + 1;
    constexpr int NT = 64 * waves_for<D>();
    constexpr int STRIDE = K3_NX + K3_NU + K3_NX + K3_NZ + D * (K3_NX + K3_NZ);
    constexpr int NLOC = 9 + STRIDE + K3_NX;
    __shared__ double vloc[NLOC];                  // theta, phi, x[k], u, xdot, z, coll.., x[k+1]
    __shared__ double rloc[STRIDE + K3_NX];        // p.ref slice of the same block
    __shared__ double wts[K3_NX + K3_NZ + K3_NU];  // Q, Z(=1), R
    __shared__ double wn[NN][kLanes];
    __shared__ double tang[NN * kRowsPerNode * kLanes];
    __shared__ double gval[NN][16];
    __shared__ double fterm[STRIDE];
    __shared__ double pre[NN][kDragStride];
    __shared__ double nodec[NN][2];

    const int b = blockIdx.x / a.n_k, k = blockIdx.x % a.n_k;
    const int tid = threadIdx.x;
    const double* V = a.V + (size_t)b * a.n_v;
    const double* P = a.P + (size_t)b * a.n_p;
    const int base = 9 + 2 + k * STRIDE;            // v_int0 = 11
    // ---- stage ---------------------------------------------------------------------------
    for (int i = tid; i < NLOC; i += NT) vloc[i] = i < 9 ? V[i] : V[base + (i - 9)];
    const double* pref = P + K3_NX;                 // p.ref (V-shaped)
    for (int i = tid; i < STRIDE + K3_NX; i += NT) rloc[i] = pref[base + i];
    const double u_ref = P[K3_NX + a.n_v];
    const double* pQ = P + K3_NX + a.n_v + 1;
    for (int i = tid; i < K3_NX + K3_NZ + K3_NU; i += NT)
        wts[i] = i < K3_NX ? pQ[i] : (i == K3_NX ? 1.0 : pQ[K3_NX + (i - K3_NX - 1)]);
    __syncthreads();

    const double tf = vloc[1];
    const double inv_h_tf = (double)a.n_k / tf;
    const double* C = a.coll->C;                    // C[j*(d+1)+r] = l_j'(tau_r)
    const double* xk = vloc + 9;
    const double* uk = xk + K3_NX;
    const double* xdk = uk + K3_NU;
    const double* zk = xdk + K3_NX;
    const double* coll = zk + K3_NZ;
    const double* xk1 = coll + D * (K3_NX + K3_NZ);
    auto Xv = [&](int r, int i) -> double { return r == 0 ? xk[i] : coll[(r - 1) * (K3_NX + K3_NZ) + i]; };

    // ---- node values -----------------------------------------------------------------------
    for (int t = tid; t < NN * kLanes; t += NT) {
        const int n = t / kLanes, i = t % kLanes;
        double val;
        if (i < K3_NX) val = Xv(n, i);
        else if (i < 2 * K3_NX) {
            if (n == 0) val = xdk[i - K3_NX];
            else {
                double s = 0.0;
                for (int r = 0; r < NN; ++r) s += C[r * NN + n] * Xv(r, i - K3_NX);
                val = s * inv_h_tf;
            }
        } else if (i < 2 * K3_NX + K3_NU) val = uk[i - 2 * K3_NX];
        else if (i == 2 * K3_NX + K3_NU) val = n == 0 ? zk[0] : coll[(n - 1) * (K3_NX + K3_NZ) + K3_NX];
        else if (i < K3_NW) val = vloc[i - (2 * K3_NX + K3_NU + K3_NZ)];
        else val = vloc[2];                         // phi.gamma
        wn[n][i] = val;
    }
    __syncthreads();

    if (tid < NN) {
        nodec[tid][0] = tid > 0 ? C[tid * NN + tid] * inv_h_tf : 0.0;
        nodec[tid][1] = tid > 0 ? 1.0 / tf : 0.0;     // the t_f direction acts at Radau nodes only
    }
    // ---- tether drag, one (node, direction) per thread: the element sum in the model's order --
    for (int t = tid; t < NN * kDragDirs; t += NT) {
        const int n = t / kDragDirs, j = t - n * kDragDirs, vj = drag_var(j);
        const double* s = a.cst + K3_C_SCALING;
        awe::Dual q[3], v[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            q[i] = awe::Dual(wn[n][awe::k3::Q + i], vj == awe::k3::Q + i ? 1.0 : 0.0) * s[awe::k3::Q + i];
            v[i] = awe::Dual(wn[n][awe::k3::DQ + i], vj == awe::k3::DQ + i ? 1.0 : 0.0) * s[awe::k3::DQ + i];
        }
        const awe::Dual diam = awe::Dual(wn[n][awe::k3::TH_DIAM], vj == awe::k3::TH_DIAM ? 1.0 : 0.0) * s[awe::k3::TH_DIAM];
        awe::Dual Dt[3];
        awe::K3InlineDrag()(q, v, diam, u_ref, a.cst, Dt);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (j == 0) pre[n][i] = Dt[i].v;
            pre[n][3 + 3 * j + i] = Dt[i].d;
        }
    }
    __syncthreads();

    // ---- model pass: half-wave = node, lane = direction --------------------------------------
    {
        const int n = tid / kLanes, lane = tid % kLanes;
        if (n < NN) {
            LaneIn in{wn[n], nodec[n], lane};
            LaneSink sink{tang + n * kRowsPerNode * kLanes, gval[n], lane};
            awe::Dual gamma(wn[n][kDirGamma], lane == kDirGamma ? 1.0 : 0.0);
            awe::kite3_node<awe::Dual>(in, gamma, u_ref, a.cst, sink, n == 0, LdsDrag{pre[n], lane});
        }
    }
    // ---- tracking objective: per local column (pmpc.py:304-358) -----------------------------
    double* grad = a.grad + (size_t)b * a.n_v + base;
    const double* w = a.coll->w;
    const double invN = 1.0 / a.n_k;
    for (int c = tid; c < STRIDE; c += NT) {
        double gr = 0.0, ft = 0.0;
        if (c >= K3_NX && c < K3_NX + K3_NU) {                       // u[k], zero-order hold
            const int i = c - K3_NX;
            const double e = vloc[9 + c] - rloc[c], W = wts[K3_NX + K3_NZ + i];
            double sw = 0.0;
            for (int j = 0; j < D; ++j) sw += w[j];
            gr = 2.0 * sw * W * e * invN;
            ft = sw * W * e * e;
        } else if (c >= 2 * K3_NX + K3_NU + K3_NZ) {                 // coll_var[k][j] = {x, z}
            const int q = c - (2 * K3_NX + K3_NU + K3_NZ);
            const int j = q / (K3_NX + K3_NZ), e_ = q % (K3_NX + K3_NZ);
            const double e = vloc[9 + c] - rloc[c], W = wts[e_];
            gr = 2.0 * w[j] * W * e * invN;
            ft = w[j] * W * e * e;
        }
        grad[c] = gr;
        fterm[c] = ft;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int c = 0; c < STRIDE; ++c) s += fterm[c];
        a.fpart[(size_t)b * a.n_k + k] = s * invN;
    }

    // ---- g ---------------------------------------------------------------------------------------
    double* g = a.g + (size_t)b * a.n_g;
    const int row0 = K3_NX + k * (K3_N_EQ + K3_N_INEQ + D * K3_N_EQ + K3_NX);
    constexpr int ROWS = K3_N_EQ + K3_N_INEQ + D * K3_N_EQ + K3_NX;
    const double* Dc = a.coll->D;
    for (int r = tid; r < ROWS; r += NT) {
        double val;
        if (r < K3_N_EQ + K3_N_INEQ) val = gval[0][r];
        else if (r < K3_N_EQ + K3_N_INEQ + D * K3_N_EQ) {
            const int q = r - (K3_N_EQ + K3_N_INEQ);
            val = gval[1 + q / K3_N_EQ][q % K3_N_EQ];
        } else {
            const int i = r - (K3_N_EQ + K3_N_INEQ + D * K3_N_EQ);
            double s = 0.0;
            for (int rr = 0; rr < NN; ++rr) s += Dc[rr] * Xv(rr, i);
            val = xk1[i] - s;
        }
        g[row0 + r] = val;
    }
    if (k == 0)
        for (int i = tid; i < K3_NX; i += NT) g[i] = xk[i] - P[i];     // initial conditions

    // ---- J_g values through the gather list ------------------------------------------------------
    double* jac = a.jac + (size_t)b * a.nnz;
    const int e0 = a.goff[k], e1 = a.goff[k + 1];
    for (int e = e0 + tid; e < e1; e += NT) {
        const uint32_t cd = a.gcode[e];
        const uint32_t kind = cd >> 29;
        const int rr = (cd >> 25) & 15, n = (cd >> 21) & 15, idx = cd & ((1u << 21) - 1u);
        double val;
        if (kind == kKindTang) val = tang[idx];
        else if (kind == kKindTangPoly) val = tang[idx] * (C[rr * NN + n] * inv_h_tf);
        else if (kind == kKindOne) val = 1.0;
        else val = -Dc[rr];
        __builtin_nontemporal_store(val, &jac[a.gslot[e]]);  // written once (as the AP2 path's J_g)
    }
}

// one wave per instance: objective partials in a fixed order, terminal cost, global gradient
__global__ __launch_bounds__(64) void mpc_finalize_kernel(MArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* V = a.V + (size_t)b * a.n_v;
    const double* P = a.P + (size_t)b * a.n_p;
    const double* ref = P + K3_NX;
    const double* pP = P + K3_NX + a.n_v + 1 + K3_NX + K3_NU;
    double* grad = a.grad + (size_t)b * a.n_v;
    const int xN = 11 + a.n_k * a.stride;
    double term = 0.0;
    if (lane < K3_NX) {
        const double e = V[xN + lane] - ref[xN + lane];
        grad[xN + lane] = 2.0 * pP[lane] * e;
        term = pP[lane] * e * e;
    }
    if (lane < 11) grad[lane] = 0.0;                     // theta, phi, xi
    __shared__ double tt[64];
    tt[lane] = term;
    __syncthreads();
    if (lane == 0) {
        double s = 0.0;
        for (int k = 0; k < a.n_k; ++k) s += a.fpart[(size_t)b * a.n_k + k];
        for (int i = 0; i < K3_NX; ++i) s += tt[i];
        a.f[b] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// nlp_hess_l: sigma f + lam^T g (kite3_tables.hpp, build_hess_tables)
// ---------------------------------------------------------------------------------------------
struct HArgs {
    MArgs a;
    const double* sigma;     // [B]
    const double* lam;       // [B][n_g]
    double* H;               // [B][hnnz]
    double* gpart;           // [B][n_k][ng]
    const int* task;         // p | q << 8
    int ntask0, ntask1, npair1, hnnz, ng, hd_total;
    const int* slot0;
    const int* nslot;
    const int* ent_off;
    const int* term_off;
    const unsigned* terms;
    const int* gslot;
    const int* xnslot;
};

constexpr int kHessThreads = 256;

// hyper-dual node variable i: e1 along direction p, e2 along direction q (the first-order seeds)
struct LaneHIn {
    const double* w;
    int p, q;
    double cxx, inv_tf;      // C[n][n] / (h tf) and 1 / tf at a Radau node, 0 at the shooting node
    __device__ __forceinline__ double seed(int dir, int i) const {
        double t = (i == dir) ? 1.0 : 0.0;
        if (i >= K3_NX && i < 2 * K3_NX) {
            if (dir == i - K3_NX) t += cxx;
            if (dir == kDirTf) t += -w[i] * inv_tf;
        }
        return t;
    }
    __device__ __forceinline__ awe::HDual operator()(int i) const {
        return awe::HDual(w[i], seed(p, i), q == kGTask ? 0.0 : seed(q, i), 0.0);
    }
};

// sum_r mu_r d2F_r / de1 de2 (pair task) or sum_r mu_r dF_r / de1 (first-order task)
struct LaneHSink {
    const double* mu;
    bool first;
    double acc;
    __device__ __forceinline__ void eq_row(int r, const awe::HDual& v) { acc += mu[r] * (first ? v.a : v.ab); }
    __device__ __forceinline__ void ineq_row(int r, const awe::HDual& v) { eq_row(K3_N_EQ + r, v); }
};

template <int D>
__global__ __launch_bounds__(kHessThreads) void mpc_hess_kernel(HArgs ha) {
    const MArgs& a = ha.a;
    constexpr int NN = D + 1;
    constexpr int NT = kHessThreads;
    constexpr int STRIDE = K3_NX + K3_NU + K3_NX + K3_NZ + D * (K3_NX + K3_NZ);
    constexpr int NLOC = 9 + STRIDE + K3_NX;
    __shared__ double vloc[NLOC];
    __shared__ double wn[NN][kLanes];
    __shared__ double mu[NN][kRowsPerNode];
    __shared__ double wq[K3_NX + K3_NU];                  // Q, R tracking weights
    __shared__ double scl[1 + NN * NN];
    extern __shared__ double hd[];                        // [hd_total]: per node, its tasks' values

    const int b = blockIdx.x / a.n_k, k = blockIdx.x % a.n_k;
    const int tid = threadIdx.x;
    const double* V = a.V + (size_t)b * a.n_v;
    const double* P = a.P + (size_t)b * a.n_p;
    const double* lam = ha.lam + (size_t)b * a.n_g;
    const double sigma = ha.sigma[b];
    const int base = 9 + 2 + k * STRIDE;
    for (int i = tid; i < NLOC; i += NT) vloc[i] = i < 9 ? V[i] : V[base + (i - 9)];
    const double* pQ = P + K3_NX + a.n_v + 1;
    for (int i = tid; i < K3_NX + K3_NU; i += NT) wq[i] = pQ[i];
    const double u_ref = P[K3_NX + a.n_v];
    const int row0 = K3_NX + k * (K3_N_EQ + K3_N_INEQ + D * K3_N_EQ + K3_NX);
    for (int t = tid; t < NN * kRowsPerNode; t += NT) {
        const int n = t / kRowsPerNode, r = t % kRowsPerNode;
        double m = 0.0;
        if (n == 0) m = lam[row0 + r];
        else if (r < K3_N_EQ) m = lam[row0 + K3_N_EQ + K3_N_INEQ + (n - 1) * K3_N_EQ + r];
        mu[n][r] = m;
    }
    __syncthreads();
    const double tf = vloc[1];
    const double inv_h_tf = (double)a.n_k / tf, inv_tf = 1.0 / tf;
    const double* C = a.coll->C;
    for (int i = tid; i < 1 + NN * NN; i += NT) scl[i] = i == 0 ? 1.0 : C[i - 1] * inv_h_tf;
    const double* xk = vloc + 9;
    const double* uk = xk + K3_NX;
    const double* xdk = uk + K3_NU;
    const double* zk = xdk + K3_NX;
    const double* coll = zk + K3_NZ;
    auto Xv = [&](int r, int i) -> double { return r == 0 ? xk[i] : coll[(r - 1) * (K3_NX + K3_NZ) + i]; };
    for (int t = tid; t < NN * kLanes; t += NT) {
        const int n = t / kLanes, i = t % kLanes;
        double val;
        if (i < K3_NX) val = Xv(n, i);
        else if (i < 2 * K3_NX) {
            if (n == 0) val = xdk[i - K3_NX];
            else {
                double s = 0.0;
                for (int r = 0; r < NN; ++r) s += C[r * NN + n] * Xv(r, i - K3_NX);
                val = s * inv_h_tf;
            }
        } else if (i < 2 * K3_NX + K3_NU) val = uk[i - 2 * K3_NX];
        else if (i == 2 * K3_NX + K3_NU) val = n == 0 ? zk[0] : coll[(n - 1) * (K3_NX + K3_NZ) + K3_NX];
        else if (i < K3_NW) val = vloc[i - (2 * K3_NX + K3_NU + K3_NZ)];
        else val = vloc[2];                               // phi.gamma
        wn[n][i] = val;
    }
    __syncthreads();

    // ---- second-order pass: one (node, direction pair) per thread --------------------------------
    const int nt0 = ha.ntask0, nt1 = ha.ntask1;
    for (int t = tid; t < nt0 + D * nt1; t += NT) {
        const int n = t < nt0 ? 0 : 1 + (t - nt0) / nt1;
        const int ti = n == 0 ? t : (t - nt0) % nt1;
        const int pq = ha.task[(n == 0 ? 0 : nt0) + ti];
        LaneHIn in{wn[n], pq & 0xff, pq >> 8, n > 0 ? C[n * NN + n] * inv_h_tf : 0.0, n > 0 ? inv_tf : 0.0};
        LaneHSink sink{mu[n], in.q == kGTask, 0.0};
        const awe::HDual gamma(wn[n][kDirGamma], in.p == kDirGamma ? 1.0 : 0.0,
                               in.q == kDirGamma ? 1.0 : 0.0, 0.0);
        awe::kite3_node<awe::HDual>(in, gamma, u_ref, a.cst, sink, n == 0);
        hd[(n == 0 ? 0 : nt0 + (n - 1) * nt1) + ti] = sink.acc;
    }
    __syncthreads();

    // ---- V-space entries: the interval's contiguous local slots, then its global partials ---------
    const int nloc = ha.nslot[k];
    const int e0 = ha.ent_off[k];
    const double* w = a.coll->w;
    const double invN = 1.0 / a.n_k;
    double sw = 0.0;
    for (int j = 0; j < D; ++j) sw += w[j];
    double* Hb = ha.H + (size_t)b * ha.hnnz + ha.slot0[k];
    double* gp = ha.gpart + ((size_t)b * a.n_k + k) * ha.ng;
    auto hoff = [&](int n) { return n == 0 ? 0 : nt0 + (n - 1) * nt1; };
    for (int e = tid; e < nloc + ha.ng; e += NT) {
        double v = 0.0;
        for (int t = ha.term_off[e0 + e]; t < ha.term_off[e0 + e + 1]; ++t) {
            const unsigned term = ha.terms[t];
            const int type = term >> 30, n = (term >> 27) & 7;
            if (type == kHTA) {
                v += scl[(term >> 7) & 127] * scl[term & 127] * hd[hoff(n) + ((term >> 14) & 8191)];
            } else if (type == kHTB) {
                const int i = (term >> 22) & 31, r = (term >> 19) & 7;
                v += hd[hoff(n) + ha.npair1 + i] * (-C[r * NN + n] * inv_h_tf * inv_tf);
            } else if (type == kHTC) {
                const int i = (term >> 22) & 31;
                v += hd[hoff(n) + ha.npair1 + i] * (2.0 * wn[n][K3_NX + i] * inv_tf * inv_tf);
            } else {
                const int sub = (term >> 22) & 3, i = (term >> 17) & 31;
                const double wt = sub == 0 ? w[n - 1] * wq[i] : (sub == 1 ? w[n - 1] : sw * wq[K3_NX + i]);
                v += sigma * 2.0 * wt * invN;
            }
        }
        if (e < nloc) Hb[e] = v;
        else gp[e - nloc] = v;
    }
}

// global-global entries (sums of the interval partials, fixed order) and the terminal cost
__global__ __launch_bounds__(64) void mpc_hess_finalize_kernel(HArgs ha) {
    const MArgs& a = ha.a;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane < ha.ng) {
        double v = 0.0;
        for (int k = 0; k < a.n_k; ++k) v += ha.gpart[((size_t)b * a.n_k + k) * ha.ng + lane];
        ha.H[(size_t)b * ha.hnnz + ha.gslot[lane]] = v;
    }
    if (lane < K3_NX) {
        const double* pP = a.P + (size_t)b * a.n_p + K3_NX + a.n_v + 1 + K3_NX + K3_NU;
        ha.H[(size_t)b * ha.hnnz + ha.xnslot[lane]] = ha.sigma[b] * 2.0 * pP[lane];
    }
}


// ---------------------------------------------------------------------------------------------
// Generated instance-minor path (awempc_eval_nlp_im): one lane per MPC instance.
//   mpc_gen_in (im::transpose_in_kernel): V, p -> VT[i * ld + b], PT[i * ld + b]
//   mpc_gen_node_kernel: three kinds of tiles in one launch, so that they run side by side --
//     Radau and shooting tiles: lane = instance, one wavefront per node, the node in the straight-line
//     code generated from kite3_node (kite3_nodejac.gen.hpp: the node's rows and the values of its
//     J_g pattern entries, no dual numbers, no zero tangents); each tangent slot goes straight to its
//     J_g entries (1, or the d polynomial columns X_r, r != n, of a Radau xdot direction, scaled by
//     C[r][n] / (h t_f)) through the node's destination row staged in LDS;
//     interval tiles: the interval's tracking-cost gradient and partial sum, continuity rows and
//     constant J_g entries, every load of the interval issued at once.
//   At the config-5 batch (256 instances) the launch is one round of wavefronts, so it takes as long
//   as its longest wavefront: in separate launches, with the interval work behind the shooting node
//   in a loop that waited on each column's loads, 0.070 ms; merged and unrolled 0.029 ms
//   (profiles/r05/mpc_ab/: direction strips on separate wavefronts and preloaded node inputs measured
//   no faster, outputs bitwise equal).
//   mpc_gen_finalize_kernel: objective (fixed order), terminal cost, global gradient rows.
// J_g and grad f leave instance-minor (jac[e * ldj + b]), every store one 512-byte row; g stays
// per-instance (g[b * n_g + i]) as the solver reads it.
// ---------------------------------------------------------------------------------------------
// the tangent slots of kite3_nodejac.gen.hpp (im_tables.hpp)
using GenSlots = im::SlotTraits<awe_k3gen::kTanIdx, awe_k3gen::kNTan, K3_NX, 128>;
template <int D, int KIND>
using GenJSink = im::JSink<GenSlots, D, KIND>;

struct GenArgs {
    awt::DevColl coll;
    int n_k, batch, n_v, n_g, n_p, stride, v_int0, rows, nib, dstride;
    unsigned ld8;                // bytes between VT / PT / fpart rows
    unsigned ldj8;               // bytes between J_g / grad rows
    double kconst[8];            // constant J_g values: 1, -D[0..d]
};

// node inputs of node n of interval k (first column c0) from VT; n = 0 the shooting node
template <int D>
struct GenIn {
    const double* v;
    unsigned ld8, lb;
    int c0, n;
    double inv_h_tf;
    const double* C;
    __device__ __forceinline__ double at(int col) const { return im::at(v, (unsigned)col, ld8, lb); }
    __device__ __forceinline__ double operator()(int i) const {
        constexpr int NN = D + 1;
        constexpr int CO = 2 * K3_NX + K3_NU + K3_NZ;          // x, u, xdot, z of the interval
        if (n > 0) {
            const int xc = c0 + CO + (n - 1) * (K3_NX + K3_NZ);
            if (i < K3_NX) return at(xc + i);
            if (i < 2 * K3_NX) {                               // xdot from the collocation polynomial
                const int s = i - K3_NX;
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < NN; ++r)
                    acc += C[r * NN + n] * at(r == 0 ? c0 + s : c0 + CO + (r - 1) * (K3_NX + K3_NZ) + s);
                return acc * inv_h_tf;
            }
            if (i == 2 * K3_NX + K3_NU) return at(xc + K3_NX);
        } else {
            if (i < K3_NX) return at(c0 + i);
            if (i < 2 * K3_NX) return at(c0 + K3_NX + K3_NU + (i - K3_NX));
            if (i == 2 * K3_NX + K3_NU) return at(c0 + 2 * K3_NX + K3_NU);
        }
        if (i < 2 * K3_NX + K3_NU) return at(c0 + K3_NX + (i - 2 * K3_NX));   // u[k], zero-order hold
        if (i < K3_NW) return at(i - (2 * K3_NX + K3_NU + K3_NZ));             // theta: diam_t, t_f
        return at(K3_NTH + 0);                                                 // phi.gamma
    }
};

// node inputs preloaded into registers: every load of the node issued at once (one memory latency)
// instead of at the generated code's first use of each input (one exposed latency per input)
template <int D>
struct GenInPre {
    double w[K3_NW + 1];
    __device__ __forceinline__ explicit GenInPre(const GenIn<D>& in) {
#pragma unroll
        for (int i = 0; i <= K3_NW; ++i) w[i] = in(i);
    }
    __device__ __forceinline__ double operator()(int i) const { return w[i]; }
};

#ifndef AWE_MPC_PRELOAD
#define AWE_MPC_PRELOAD 1
#endif
#ifndef AWE_MPC_STRIP_WAVES
#define AWE_MPC_STRIP_WAVES 1
#endif

// calls f(std::integral_constant<int, s>) for the direction strip s == sg of the generated code
template <int S, int I = 0, class F>
__device__ __forceinline__ void gen_strip(int sg, const F& f) {
    if constexpr (I < S) {
        if (sg == I) f(std::integral_constant<int, I>{});
        else gen_strip<S, I + 1>(sg, f);
    }
}

// Strip groups: with AWE_MPC_STRIP_WAVES the kNStrips direction strips of a node run in separate
// workgroups side by side (each recomputes the values it needs: more, shorter wavefronts -- at the
// config-5 batch of 256 instances one node per wavefront leaves most SIMDs idle and the kernel is the
// latency of one wavefront); otherwise one wavefront runs the strips of its node in turn.
constexpr int kGenStripGroups = AWE_MPC_STRIP_WAVES ? awe_k3gen::kNStrips : 1;
constexpr int kGenNodeWaves = 4;
constexpr int kGenShootWaves = kGenNodeWaves;
template <int D>
constexpr int gen_radau_waves() { return D < kGenNodeWaves ? D : kGenNodeWaves; }

template <int D>
__device__ __forceinline__ void gen_radau_tile(int t, unsigned* ldt, const double* __restrict__ VT,
                                               const double* __restrict__ PT, const double* __restrict__ cst,
                                               const unsigned* __restrict__ dtab, double* __restrict__ g,
                                               double* __restrict__ jac, const GenArgs& a) {
    constexpr int NN = D + 1;
    constexpr int W = gen_radau_waves<D>();
    constexpr int T1 = im::kSlots<GenSlots, D>.total[1];
    const int sg = t % kGenStripGroups, tk = t / kGenStripGroups;
    const int ib = tk / a.n_k, k = tk - ib * a.n_k;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int m = 1; m < NN; ++m)
        im::stage_offsets<64 * kGenNodeWaves>(ldt + (m - 1) * T1, dtab + (size_t)(k * NN + m) * a.dstride, T1,
                                              a.ldj8, tid);
    __syncthreads();
    const int b = ib * 64 + lane;
    if (wave >= W || b >= a.batch) return;
    const unsigned lb = 8u * (unsigned)b, ld8 = a.ld8;
    const int c0 = a.v_int0 + k * a.stride;
    const double* C = a.coll.C;
    const double tf = im::at(VT, 1u, ld8, lb);
    const double inv_h_tf = (double)a.n_k / tf;
    const double u_ref = im::at(PT, (unsigned)(K3_NX + a.n_v), ld8, lb);
    double* gb = g + (size_t)b * a.n_g + K3_NX + k * a.rows + K3_N_EQ + K3_N_INEQ;
    for (int n = 1 + wave; n < NN; n += W) {
        double xs[D];                                 // C[r][n] / (h t_f) of the columns X_r, r != n
#pragma unroll
        for (int q = 0; q < D; ++q) xs[q] = C[(q < n ? q : q + 1) * NN + n] * inv_h_tf;
        const GenIn<D> gin{VT, ld8, lb, c0, n, inv_h_tf, C};
#if AWE_MPC_PRELOAD
        const GenInPre<D> in(gin);
#else
        const GenIn<D>& in = gin;
#endif
        GenJSink<D, 1> js{jac, lb, ldt + (n - 1) * T1, xs};
        const double cxx = C[n * NN + n] * inv_h_tf, itf = 1.0 / tf;
        auto run = [&](auto st) {
            awe_k3gen::k3_node_radau<1, decltype(st)::value>(in, u_ref, cxx, itf, cst, gb + (n - 1) * K3_N_EQ, js);
        };
        if constexpr (kGenStripGroups > 1) {
            gen_strip<awe_k3gen::kNStrips>(sg, run);
        } else {
            gen_strip<awe_k3gen::kNStrips>(0, run);
            if constexpr (awe_k3gen::kNStrips > 1) gen_strip<awe_k3gen::kNStrips, 1>(1, run);
            if constexpr (awe_k3gen::kNStrips > 2) gen_strip<awe_k3gen::kNStrips, 2>(2, run);
            if constexpr (awe_k3gen::kNStrips > 3) gen_strip<awe_k3gen::kNStrips, 3>(3, run);
            static_assert(awe_k3gen::kNStrips <= 4, "strip loop");
        }
    }
}

#ifndef AWE_MPC_EXTRA_TILES
#define AWE_MPC_EXTRA_TILES 1
#endif
template <int D>
__device__ __forceinline__ void gen_interval_extras(int k, int b, const double* __restrict__ VT,
                                                    const double* __restrict__ PT, const unsigned* __restrict__ ctab,
                                                    const int* __restrict__ coff, double* __restrict__ g,
                                                    double* __restrict__ grad, double* __restrict__ jac,
                                                    double* __restrict__ fpart, const GenArgs& a);

// shooting nodes: one wavefront per interval (kGenShootWaves intervals of one instance block per
// workgroup); strip group 0 then writes the interval's tracking-cost gradient and partial sum,
// continuity rows, initial conditions and constant J_g entries
template <int D>
__device__ __forceinline__ void gen_shoot_tile(int t, unsigned* ldt, const double* __restrict__ VT,
                                               const double* __restrict__ PT, const double* __restrict__ cst,
                                               const unsigned* __restrict__ dtab, const unsigned* __restrict__ ctab,
                                               const int* __restrict__ coff, double* __restrict__ g,
                                               double* __restrict__ grad, double* __restrict__ jac,
                                               double* __restrict__ fpart, const GenArgs& a) {
    constexpr int NN = D + 1;
    constexpr int T0 = im::kSlots<GenSlots, D>.total[0];
    const int nk4 = (a.n_k + kGenShootWaves - 1) / kGenShootWaves;
    const int sg = t % kGenStripGroups, tk = t / kGenStripGroups;
    const int ib = tk / nk4, k0 = (tk - ib * nk4) * kGenShootWaves;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int w = 0; w < kGenShootWaves && k0 + w < a.n_k; ++w)
        im::stage_offsets<64 * kGenNodeWaves>(ldt + w * T0, dtab + (size_t)((k0 + w) * NN) * a.dstride, T0, a.ldj8,
                                              tid);
    __syncthreads();
    const int k = k0 + wave;
    const int b = ib * 64 + lane;
    if (k >= a.n_k || b >= a.batch) return;
    const unsigned lb = 8u * (unsigned)b, ld8 = a.ld8;
    const int c0 = a.v_int0 + k * a.stride;
    const double* C = a.coll.C;
    const double tf = im::at(VT, 1u, ld8, lb);
    const double inv_h_tf = (double)a.n_k / tf;
    const double u_ref = im::at(PT, (unsigned)(K3_NX + a.n_v), ld8, lb);
    double* gb = g + (size_t)b * a.n_g;
    const int row0 = K3_NX + k * a.rows;
    {
        const GenIn<D> gin{VT, ld8, lb, c0, 0, inv_h_tf, C};
#if AWE_MPC_PRELOAD
        const GenInPre<D> in(gin);
#else
        const GenIn<D>& in = gin;
#endif
        GenJSink<D, 0> js{jac, lb, ldt + wave * T0, nullptr};
        auto run = [&](auto st) { awe_k3gen::k3_node_shoot<1, decltype(st)::value>(in, u_ref, cst, gb + row0, js); };
        if constexpr (kGenStripGroups > 1) {
            gen_strip<awe_k3gen::kNStrips>(sg, run);
        } else {
            gen_strip<awe_k3gen::kNStrips>(0, run);
            if constexpr (awe_k3gen::kNStrips > 1) gen_strip<awe_k3gen::kNStrips, 1>(1, run);
            if constexpr (awe_k3gen::kNStrips > 2) gen_strip<awe_k3gen::kNStrips, 2>(2, run);
            if constexpr (awe_k3gen::kNStrips > 3) gen_strip<awe_k3gen::kNStrips, 3>(3, run);
        }
    }
    if (AWE_MPC_EXTRA_TILES || sg != 0) return;
    gen_interval_extras<D>(k, b, VT, PT, ctab, coff, g, grad, jac, fpart, a);
}

// the interval's tracking-cost gradient and partial sum, continuity rows, initial conditions and
// constant J_g entries (lane b = instance)
template <int D>
__device__ __forceinline__ void gen_interval_extras(int k, int b, const double* __restrict__ VT,
                                                    const double* __restrict__ PT, const unsigned* __restrict__ ctab,
                                                    const int* __restrict__ coff, double* __restrict__ g,
                                                    double* __restrict__ grad, double* __restrict__ jac,
                                                    double* __restrict__ fpart, const GenArgs& a) {
    constexpr int NN = D + 1;
    constexpr int STRIDE = K3_NX + K3_NU + K3_NX + K3_NZ + D * (K3_NX + K3_NZ);
    const unsigned lb = 8u * (unsigned)b, ld8 = a.ld8;
    const int c0 = a.v_int0 + k * a.stride;
    double* gb = g + (size_t)b * a.n_g;
    const int row0 = K3_NX + k * a.rows;
    auto V = [&](int col) { return im::at(VT, (unsigned)col, ld8, lb); };
    auto Pp = [&](int row) { return im::at(PT, (unsigned)row, ld8, lb); };
    // tracking objective of the interval's columns (pmpc.py:304-358), as mpc_interval_kernel
    const double* w = a.coll.w;
    const double invN = 1.0 / a.n_k;
    double sw = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) sw += w[j];
    const int pref = K3_NX + c0;                       // p.ref row of column c0
    const int pq = K3_NX + a.n_v + 1;                  // Q, then R
    double fs = 0.0;
#pragma unroll
    for (int c = 0; c < STRIDE; ++c) {
        double gr = 0.0, ft = 0.0;
        if (c >= K3_NX && c < K3_NX + K3_NU) {
            const int i = c - K3_NX;
            const double e = V(c0 + c) - Pp(pref + c), W = Pp(pq + K3_NX + i);
            gr = 2.0 * sw * W * e * invN;
            ft = sw * W * e * e;
        } else if (c >= 2 * K3_NX + K3_NU + K3_NZ) {
            const int q = c - (2 * K3_NX + K3_NU + K3_NZ);
            const int j = q / (K3_NX + K3_NZ), e_ = q % (K3_NX + K3_NZ);
            const double e = V(c0 + c) - Pp(pref + c), W = e_ < K3_NX ? Pp(pq + e_) : 1.0;
            gr = 2.0 * w[j] * W * e * invN;
            ft = w[j] * W * e * e;
        }
        __builtin_nontemporal_store(gr, &im::at(grad, (unsigned)(c0 + c), a.ldj8, lb));
        fs += ft;
    }
    im::at(fpart, (unsigned)k, ld8, lb) = fs * invN;
    // continuity x[k+1] - sum_r D_r X_{k,r} (collocation.py:319-336) and the initial conditions
    const int gc = row0 + K3_N_EQ + K3_N_INEQ + D * K3_N_EQ;
    constexpr int CO = 2 * K3_NX + K3_NU + K3_NZ;
#pragma unroll
    for (int i = 0; i < K3_NX; ++i) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < NN; ++r) s += a.coll.D[r] * V(r == 0 ? c0 + i : c0 + CO + (r - 1) * (K3_NX + K3_NZ) + i);
        gb[gc + i] = V(c0 + a.stride + i) - s;
    }
    if (k == 0)
        for (int i = 0; i < K3_NX; ++i) gb[i] = V(c0 + i) - Pp(i);
    // the interval's constant J_g entries (initial-condition and continuity rows)
    for (int q = coff[k]; q < coff[k + 1]; ++q) {
        const unsigned e = ctab[q];
        __builtin_nontemporal_store(a.kconst[e >> 24], &im::at(jac, e & 0xffffffu, a.ldj8, lb));
    }
}

// The node kernel: the Radau tiles (instance block, interval, strip group) and the shooting tiles
// (instance block, kGenShootWaves intervals, strip group) in one launch, so that the two node kinds
// run side by side; one wavefront per SIMD (the node code keeps 100-150 values live)
template <int D>
constexpr int gen_radau_tiles(const GenArgs& a) { return a.nib * a.n_k * kGenStripGroups; }
template <int D>
__global__ __launch_bounds__(64 * kGenNodeWaves) __attribute__((amdgpu_waves_per_eu(1)))
void mpc_gen_node_kernel(const double* __restrict__ VT, const double* __restrict__ PT,
                         const double* __restrict__ cst, const unsigned* __restrict__ dtab,
                         const unsigned* __restrict__ ctab, const int* __restrict__ coff, double* __restrict__ g,
                         double* __restrict__ grad, double* __restrict__ jac, double* __restrict__ fpart, GenArgs a) {
    constexpr int T0 = im::kSlots<GenSlots, D>.total[0], T1 = im::kSlots<GenSlots, D>.total[1];
    constexpr int NLDT = D * T1 > kGenShootWaves * T0 ? D * T1 : kGenShootWaves * T0;
    __shared__ unsigned ldt[NLDT];
    const int nr = gen_radau_tiles<D>(a);
    const int nk4 = (a.n_k + kGenShootWaves - 1) / kGenShootWaves;
    const int ns = a.nib * nk4 * kGenStripGroups;
    const int ne = AWE_MPC_EXTRA_TILES ? a.nib * nk4 : 0;
    const int t = im::xcd_tile(ne + nr + ns);
    if (t >= ne + nr + ns) return;
    if (t < ne) {                        // first: the extras tiles are short and latency-bound
        const int ib = t / nk4, k = (t - ib * nk4) * kGenShootWaves + (int)(threadIdx.x >> 6);
        const int b = ib * 64 + (int)(threadIdx.x & 63);
        if (k < a.n_k && b < a.batch) gen_interval_extras<D>(k, b, VT, PT, ctab, coff, g, grad, jac, fpart, a);
    } else if (t < ne + nr) {
        gen_radau_tile<D>(t - ne, ldt, VT, PT, cst, dtab, g, jac, a);
    } else {
        gen_shoot_tile<D>(t - ne - nr, ldt, VT, PT, cst, dtab, ctab, coff, g, grad, jac, fpart, a);
    }
}

// one lane per instance: objective partials in a fixed order, terminal cost, global gradient rows
__global__ __launch_bounds__(64) void mpc_gen_finalize_kernel(const double* __restrict__ VT,
                                                             const double* __restrict__ PT,
                                                             const double* __restrict__ fpart, double* __restrict__ f,
                                                             double* __restrict__ grad, GenArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.batch) return;
    const unsigned lb = 8u * (unsigned)b;
    double s = 0.0;
    int k = 0;
    for (; k + 8 <= a.n_k; k += 8) {                   // 8 loads in flight, the sum in interval order
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = im::at(fpart, (unsigned)(k + u), a.ld8, lb);
#pragma unroll
        for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; k < a.n_k; ++k) s += im::at(fpart, (unsigned)k, a.ld8, lb);
    const int xN = a.v_int0 + a.n_k * a.stride;
    const int pP = K3_NX + a.n_v + 1 + K3_NX + K3_NU;
    for (int i = 0; i < K3_NX; ++i) {
        const double e = im::at(VT, (unsigned)(xN + i), a.ld8, lb) - im::at(PT, (unsigned)(K3_NX + xN + i), a.ld8, lb);
        const double W = im::at(PT, (unsigned)(pP + i), a.ld8, lb);
        im::at(grad, (unsigned)(xN + i), a.ldj8, lb) = 2.0 * W * e;
        s += W * e * e;
    }
    for (int i = 0; i < a.v_int0; ++i) im::at(grad, (unsigned)i, a.ldj8, lb) = 0.0;   // theta, phi, xi
    f[b] = s;
}

// ---------------------------------------------------------------------------------------------
// The reference's simulation plant (sim.py:72-78 -> rk4root, tools/integrator_routines.py:32-96):
// plant_rk4root.hpp instantiated on the generated rootfinder node code (kite3_noderoot.gen.hpp).
//   mpc_plant_rk4root_kernel: one lane per loop, one launch for all n_steps sampling times, no
//   cross-lane operation.  A lane's 12 x 12 matrix and right-hand side sit in LDS lane-minor (entry e
//   of lane l at [e * 64 + l]: every lane of a ds_read_b64 / ds_write_b64 in its own bank pair whatever
//   row it pivots on), 72 + 6 KiB, so one wavefront per workgroup; the constants and the xdot / x
//   scaling ratios are staged once behind them.  awempc_plant_rk4root_cpu runs the same core on the host.
// ---------------------------------------------------------------------------------------------
constexpr int kPlantN = awe_k3root::kNUnk;               // 12 unknowns (xdot, z) = 12 rows
constexpr int kPlantPar = 4;                             // theta.diam_t, theta.t_f, phi.gamma, u_ref
static_assert(awe_k3root::kNRows == kPlantN && kPlantN == K3_NX + K3_NZ, "square rootfinder system");

// node inputs of the generated code from the stage state, the unknowns, the applied control and par
struct PlantIn {
    const double* x;
    const double* y;
    const double* u;
    const double* par;
    AWE_HD double operator()(int i) const {
        if (i < K3_NX) return x[i];
        if (i < 2 * K3_NX) return y[i - K3_NX];
        if (i < 2 * K3_NX + K3_NU) return u[i - 2 * K3_NX];
        if (i == awe::k3::Z_LAMBDA) return y[K3_NX];
        return par[i - (awe::k3::Z_LAMBDA + 1)];          // theta.diam_t, theta.t_f, phi.gamma
    }
};

template <class Sys>
struct PlantRows {
    Sys& sys;
    AWE_HD double& operator[](int r) const { return sys.r(r); }
};
template <class Sys>
struct PlantSlots {
    Sys& sys;
    AWE_HD double& operator[](int s) const {
        return sys.a(awe_k3root::kEntry[s] / kPlantN, awe_k3root::kEntry[s] % kPlantN);
    }
};

// plant_rk4root.hpp's Node for the 3-DOF kite; cst: the model constants followed by the K3_NX ratios
// s[xdot_i] / s[x_i], u: the loop's controls [n_steps][K3_NU], par: its kPlantPar parameters
struct K3PlantNode {
    const double* cst;
    const double* u_seq;
    double par[kPlantPar];
    double u[K3_NU];
    AWE_HD void begin(int step) {
#pragma unroll
        for (int i = 0; i < K3_NU; ++i) u[i] = u_seq[(size_t)step * K3_NU + i];
    }
    template <class Sys>
    AWE_HD void eval(int, const double* x, const double* y, Sys& sys) const {
#pragma unroll
        for (int r = 0; r < kPlantN; ++r)
#pragma unroll
            for (int j = 0; j < kPlantN; ++j)
                if (awe_k3root::kSlot[r][j] < 0) sys.a(r, j) = 0.0;      // the LU fills in: rewritten every time
        awe_k3root::k3_node_root<1>(PlantIn{x, y, u, par}, par[3], cst, PlantRows<Sys>{sys}, PlantSlots<Sys>{sys});
    }
    template <class Sys>
    AWE_HD void solve(Sys& sys, double* y) const { awe::rk4root_solve_update<kPlantN>(sys, y); }
    // the power integral's integrand lambda l_t dl_t in SI units (dynamics.py:318-330)
    AWE_HD double integrand(int, const double* x, const double* y) const {
        const double* s = cst + K3_C_SCALING;
        return (y[K3_NX] * s[awe::k3::Z_LAMBDA]) * (x[awe::k3::LT] * s[awe::k3::LT]) * (x[awe::k3::DLT] * s[awe::k3::DLT]);
    }
    AWE_HD double rate(int i, double xdot_scaled) const { return xdot_scaled * cst[K3_NCONST + i]; }
};

struct PlantLdsSys {       // both pointers already at the lane's column
    double* A;
    double* b;
    __device__ __forceinline__ double& a(int i, int j) const { return A[(i * kPlantN + j) * 64]; }
    __device__ __forceinline__ double& r(int i) const { return b[i * 64]; }
};
struct PlantHostSys {
    double A[kPlantN * kPlantN], b[kPlantN];
    double& a(int i, int j) { return A[i * kPlantN + j]; }
    double& r(int i) { return b[i]; }
};

struct PlantArgs {
    const double* x0;     // [B][K3_NX]
    const double* u;      // [B][n_steps][K3_NU]
    const double* z0;     // [B][kPlantN]
    const double* par;    // [B][kPlantPar]
    const double* cst;    // [K3_NCONST]
    double ts, tol;
    int n_fe, n_steps, max_newton, batch;
    double* xf;           // [B][n_steps][K3_NX]
    double* zf;           // [B][kPlantN]
    double* qf;           // [B][n_steps]
    double* res;          // [B]
};

// one instance of the plant; shared by the kernel's lanes and the host loop
template <class Sys>
AWE_HD void plant_instance(const PlantArgs& a, size_t b, const double* cst_ratio, Sys& sys) {
    K3PlantNode node{cst_ratio, a.u + b * (size_t)a.n_steps * K3_NU, {}, {}};
    double x[K3_NX], y[kPlantN];
#pragma unroll
    for (int i = 0; i < kPlantPar; ++i) node.par[i] = a.par[b * kPlantPar + i];
#pragma unroll
    for (int i = 0; i < K3_NX; ++i) x[i] = a.x0[b * K3_NX + i];
#pragma unroll
    for (int i = 0; i < kPlantN; ++i) y[i] = a.z0[b * kPlantN + i];
    double* xf = a.xf + b * (size_t)a.n_steps * K3_NX;
    double* qf = a.qf + b * (size_t)a.n_steps;
    const double res = awe::rk4root_run<K3_NX, kPlantN>(
        node, sys, x, y, a.ts, a.n_fe, a.n_steps, a.max_newton, a.tol,
        [xf](int s, int i, double v) { xf[(size_t)s * K3_NX + i] = v; }, [qf](int s, double v) { qf[s] = v; });
#pragma unroll
    for (int i = 0; i < kPlantN; ++i) a.zf[b * kPlantN + i] = y[i];
    a.res[b] = res;
}

__global__ __launch_bounds__(64) void mpc_plant_rk4root_kernel(PlantArgs a) {
    __shared__ double A[kPlantN * kPlantN * 64];
    __shared__ double rhs[kPlantN * 64];
    __shared__ double cs[K3_NCONST + K3_NX];
    const int lane = threadIdx.x;
    if (lane < K3_NCONST) cs[lane] = a.cst[lane];
    static_assert(K3_NCONST <= 64, "one wavefront stages the constants");
    __syncthreads();
    if (lane < K3_NX) cs[K3_NCONST + lane] = cs[K3_C_SCALING + K3_NX + lane] / cs[K3_C_SCALING + lane];
    __syncthreads();
    const size_t b = (size_t)blockIdx.x * 64 + lane;
    if (b >= (size_t)a.batch) return;
    PlantLdsSys sys{A + lane, rhs + lane};
    plant_instance(a, b, cs, sys);
}

// ---------------------------------------------------------------------------------------------
// The MPC's reference generator (pmpc.py:408-550): ref_pp.hpp, one thread per (loop, time point).
//   mpc_ref_window_kernel: the N + 1 shooting, N d collocation and N control points of a loop on
//   consecutive threads; the three grids' breakpoints staged in LDS (the piece search reads them
//   log2(pieces) times per point), the coefficients read piece-major from global memory (a point's
//   channels are contiguous).  Every entry of the window is written here, the constant ones included.
//   No cross-lane operation: a loop's window does not depend on the batch.
//   awempc_ref_window_cpu runs the same core on the host.
// ---------------------------------------------------------------------------------------------
constexpr int kRefBlock = 256;

__global__ __launch_bounds__(kRefBlock) void mpc_ref_window_kernel(awe::RefArgs a, const double* brk, int n_brk) {
    __shared__ double sb[awe::kRefMaxBrk];
    for (int i = threadIdx.x; i < n_brk && i < awe::kRefMaxBrk; i += kRefBlock) sb[i] = brk[i];
    __syncthreads();
    const int n_pt = awe::ref_points(a.n_k, a.d);
    const size_t idx = (size_t)blockIdx.x * kRefBlock + threadIdx.x;
    if (idx >= (size_t)a.batch * (size_t)n_pt) return;
    const size_t b = idx / (size_t)n_pt;
    awe::ref_point(a, sb, b, (int)(idx - b * (size_t)n_pt));
}

}  // namespace

struct awempc_handle_s {
    Tables t;
    int batch = 0;
    std::vector<double> consts;
    DevBuf<double> d_cst;
    DevBuf<awt::DevColl> d_coll;
    DevBuf<int> d_goff, d_gslot;
    DevBuf<uint32_t> d_gcode;
    DevBuf<double> d_fpart;
    DevBuf<double> d_V, d_P, d_f, d_g, d_grad, d_jac;   // staging of the host entry points
    Event ev[3];
    bool timed = false;
    // Hessian (built on first use: awempc_hess_init)
    HessTables ht;
    bool hess_ready = false;
    int hd_total = 0;
    DevBuf<int> d_task, d_slot0, d_nslot, d_ent_off, d_term_off, d_hgslot, d_xnslot;
    DevBuf<unsigned> d_terms;
    DevBuf<double> d_gpart;
    DevBuf<double> d_hsig, d_hlam, d_H;
    Event hev[2];
    bool htimed = false;
    // generated instance-minor path (awempc_eval_nlp_im)
    bool gen_ok = false;
    std::string gen_why;
    int gen_dstride = 0;
    size_t gen_ld = 0;                       // row length of VT / PT / fpart
    DevBuf<unsigned> d_gdtab, d_gctab;
    DevBuf<int> d_gcoff;
    DevBuf<double> d_VT, d_PT, d_gfpart;
    double gen_kconst[8] = {};
    Event gev[4];
    bool gtimed = false;
    // rk4root plant (awempc_plant_rk4root)
    Event pev[2];
    bool ptimed = false;
    // reference generator (awempc_ref_set, awempc_ref_window)
    bool ref_ready = false;
    awe::RefArgs ref{};                      // grids, period, offsets and head: device pointers
    int ref_nbrk = 0;
    DevBuf<double> d_ref_brk, d_ref_coef, d_ref_offs, d_ref_head;
    Event rev[2];
    bool rtimed = false;
};

namespace {

int unsupported_d() { return fail(AWE_ERR_ARG, "unsupported d"); }

// destination tables of the generated path from the gather list of build_tables: per (interval k,
// node n) a row of CCS positions in slot order (slot s of the node's generated code, then its
// d polynomial columns for a Radau xdot direction), and per interval the constant entries
// (position | value index << 24, values 1, -D[r])
int build_gen(awempc_handle_s* h) {
    const Tables& T = h->t;
    const int n_k = T.lay.n_k, d = T.lay.d, NN = d + 1;
    if ((int)h->consts[K3_C_N_ELEMENTS] != awe_k3gen::kNElements) {
        h->gen_why = "the generated node code has " + std::to_string(awe_k3gen::kNElements) +
                     " tether elements, the constants " + std::to_string((int)h->consts[K3_C_N_ELEMENTS]);
        return AWE_OK;
    }
    if ((size_t)T.row.size() >= (1u << 24)) { h->gen_why = "J_g too large for the constant table"; return AWE_OK; }
    im::DestTables<GenSlots> tabs(n_k, d);
    for (int k = 0; k < n_k; ++k) {
        for (int e = T.goff[k]; e < T.goff[k + 1]; ++e) {
            const unsigned pos = (unsigned)T.gslot[e];
            const uint32_t cd = T.gcode[e];
            const uint32_t kind = cd >> 29;
            const int rr = (cd >> 25) & 15, idx = (int)(cd & ((1u << 21) - 1u));
            if (kind == kKindOne || kind == kKindMinusD) {
                tabs.add_const(k, pos, kind == kKindOne ? 0u : 1u + (unsigned)rr);
                continue;
            }
            const int n = idx / (kRowsPerNode * kLanes), r = (idx / kLanes) % kRowsPerNode, l = idx % kLanes;
            const int kd = n > 0 ? 1 : 0;
            const int s = awe_k3gen::kTanIdx[kd][r][l];
            if (s < 0) return fail(AWE_ERR_ARG, "internal: J_g entry without a generated tangent");
            const int q = kind == kKindTangPoly ? (rr < n ? rr : rr - 1) : 0;
            if (const char* why = tabs.place(k, n, kd, s, q, pos)) return fail(AWE_ERR_ARG, why);
        }
        tabs.close_interval(k);
    }
    if (const char* why = tabs.finish()) return fail(AWE_ERR_ARG, why);
    h->gen_kconst[0] = 1.0;
    for (int r = 0; r < NN; ++r) h->gen_kconst[1 + r] = -h->t.coll.D[r];
    h->gen_dstride = tabs.dstride;
    h->gen_ld = (size_t)h->batch;
    HIP_TRY(h->d_gdtab.upload(tabs.dtab));
    HIP_TRY(h->d_gctab.upload(tabs.ctab));
    HIP_TRY(h->d_gcoff.upload(tabs.coff));
    HIP_TRY(h->d_VT.alloc(h->gen_ld * T.lay.n_v));
    HIP_TRY(h->d_PT.alloc(h->gen_ld * T.lay.n_p));
    HIP_TRY(h->d_gfpart.alloc(h->gen_ld * n_k));
    for (auto& e : h->gev) HIP_TRY(e.create());
    h->gen_ok = true;
    return AWE_OK;
}

}  // namespace

extern "C" {

const char* awempc_last_error(void) { return g_err.c_str(); }

int awempc_sparsity_jac_static(int n_k, int d, const double* consts, int n_consts, int* nnz, int* colind, int* row) {
    if (!consts || !nnz) return fail(AWE_ERR_ARG, "null argument");
    Tables T;
    std::string err;
    if (build_tables(n_k, d, consts, n_consts, T, err)) return fail(AWE_ERR_ARG, err);
    copy_ccs(nnz, colind, row, T.colind, T.row);
    return AWE_OK;
}

int awempc_create(int n_k, int d, const double* consts, int n_consts, int batch, awempc_handle* out) {
    if (!consts || !out || batch < 1) return fail(AWE_ERR_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(AWE_ERR_NODEVICE, "no HIP device");
    if (d < 2 || d > 5) return fail(AWE_ERR_ARG, "the MPC kernel is instantiated for 2 <= d <= 5");
    auto h = std::make_unique<awempc_handle_s>();   // freed, with all it owns, by every early return
    std::string err;
    if (build_tables(n_k, d, consts, n_consts, h->t, err)) return fail(AWE_ERR_ARG, err);
    if (consts[K3_C_N_K] != (double)n_k || consts[K3_C_D] != (double)d)
        return fail(AWE_ERR_ARG, "consts[K3_C_N_K], consts[K3_C_D] disagree with n_k, d");
    h->batch = batch;
    h->consts.assign(consts, consts + n_consts);
    awt::DevColl dc{};
    const int NN = d + 1;
    for (int j = 0; j < NN; ++j) {
        for (int r = 0; r < NN; ++r) dc.C[j * NN + r] = h->t.coll.C[j][r];
        dc.D[j] = h->t.coll.D[j];
    }
    for (int j = 0; j < d; ++j) dc.w[j] = h->t.coll.w[j];
    const Tables& T = h->t;
    HIP_TRY(h->d_cst.upload(consts, n_consts));
    HIP_TRY(h->d_coll.upload(&dc, 1));
    HIP_TRY(h->d_goff.upload(T.goff));
    HIP_TRY(h->d_gslot.upload(T.gslot));
    HIP_TRY(h->d_gcode.upload(T.gcode));
    HIP_TRY(h->d_fpart.alloc((size_t)batch * n_k));
    for (auto& e : h->ev) HIP_TRY(e.create());
    for (auto& e : h->pev) HIP_TRY(e.create());
    for (auto& e : h->rev) HIP_TRY(e.create());
    if (int rc = build_gen(h.get())) return rc;
    *out = h.release();
    return AWE_OK;
}

int awempc_destroy(awempc_handle h) {
    delete h;   // the members free their device memory and events
    return AWE_OK;
}

int awempc_sizes(awempc_handle h, int* n_v, int* n_g, int* n_p, int* nnz) {
    if (!h) return fail(AWE_ERR_ARG, "null handle");
    if (n_v) *n_v = h->t.lay.n_v;
    if (n_g) *n_g = h->t.lay.n_g;
    if (n_p) *n_p = h->t.lay.n_p;
    if (nnz) *nnz = (int)h->t.row.size();
    return AWE_OK;
}

int awempc_sparsity_jac(awempc_handle h, int* colind, int* row) {
    if (!h || !colind || !row) return fail(AWE_ERR_ARG, "null argument");
    copy_ccs(nullptr, colind, row, h->t.colind, h->t.row);
    return AWE_OK;
}

int awempc_eval_nlp(awempc_handle h, const double* V, const double* p, double* f, double* g, double* grad_f,
                    double* jac, void* stream) {
    if (!h || !V || !p || !f || !g || !grad_f || !jac) return fail(AWE_ERR_ARG, "null argument");
    const Tables& T = h->t;
    hipStream_t s = (hipStream_t)stream;
    MArgs a{T.lay.n_k, T.lay.d, T.lay.n_v, T.lay.n_g, T.lay.n_p, (int)T.row.size(), T.lay.stride,
            V, p, f, g, grad_f, jac, h->d_cst, h->d_coll, h->d_goff, h->d_gslot, h->d_gcode, h->d_fpart};
    const dim3 grid((unsigned)(h->batch * T.lay.n_k));
    HIP_TRY(hipEventRecord(h->ev[0], s));
    if (int rc = for_degree<2>(T.lay.d, [&](auto dc) -> int {
            constexpr int D = decltype(dc)::value;
            mpc_interval_kernel<D><<<grid, 64 * waves_for<D>(), 0, s>>>(a);
            return AWE_OK;
        }, unsupported_d)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[1], s));
    mpc_finalize_kernel<<<dim3((unsigned)h->batch), 64, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[2], s));
    h->timed = true;
    return AWE_OK;
}

int awempc_gen_status(awempc_handle h, int* available) {
    if (!h || !available) return fail(AWE_ERR_ARG, "null argument");
    *available = h->gen_ok ? 1 : 0;
    if (!h->gen_ok) g_err = h->gen_why;
    return AWE_OK;
}

int awempc_eval_nlp_im(awempc_handle h, const double* V, const double* p, double* f, double* g, double* grad_f,
                       double* jac, size_t ld, void* stream) {
    if (!h || !V || !p || !f || !g || !grad_f || !jac) return fail(AWE_ERR_ARG, "null argument");
    if (!h->gen_ok) return fail(AWE_ERR_ARG, "generated path unavailable: " + h->gen_why);
    const Tables& T = h->t;
    const int B = h->batch;
    if (ld < (size_t)B) return fail(AWE_ERR_ARG, "ld must be >= batch");
    const size_t nrows = std::max((size_t)T.row.size(), (size_t)T.lay.n_v);
    if (nrows * ld * 8 >= ((size_t)1 << 32)) return fail(AWE_ERR_ARG, "instance-minor J_g must stay below 4 GiB");
    if ((size_t)std::max(T.lay.n_v, T.lay.n_p) * h->gen_ld * 8 >= ((size_t)1 << 32))
        return fail(AWE_ERR_ARG, "instance-minor inputs must stay below 4 GiB");
    hipStream_t s = (hipStream_t)stream;
    GenArgs a{};
    const int NN = T.lay.d + 1;
    for (int j = 0; j < NN; ++j) {
        for (int r = 0; r < NN; ++r) a.coll.C[j * NN + r] = T.coll.C[j][r];
        a.coll.D[j] = T.coll.D[j];
    }
    for (int j = 0; j < T.lay.d; ++j) a.coll.w[j] = T.coll.w[j];
    a.n_k = T.lay.n_k;
    a.batch = B;
    a.n_v = T.lay.n_v;
    a.n_g = T.lay.n_g;
    a.n_p = T.lay.n_p;
    a.stride = T.lay.stride;
    a.v_int0 = T.lay.v_int0;
    a.rows = T.lay.rows;
    a.nib = (B + 63) / 64;
    a.dstride = h->gen_dstride;
    a.ld8 = (unsigned)(8 * h->gen_ld);
    a.ldj8 = (unsigned)(8 * ld);
    for (int i = 0; i < 8; ++i) a.kconst[i] = h->gen_kconst[i];
    HIP_TRY(hipEventRecord(h->gev[0], s));
    const dim3 tgrid((unsigned)((T.lay.n_v + T.lay.n_p + 63) / 64), (unsigned)a.nib);
    im::transpose_in_kernel<<<tgrid, 256, 0, s>>>(V, p, h->d_VT, h->d_PT, B, T.lay.n_v, T.lay.n_p, (int)h->gen_ld);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->gev[1], s));
    const int n_tiles = a.nib * (a.n_k + (a.n_k + kGenShootWaves - 1) / kGenShootWaves) * kGenStripGroups +
                        (AWE_MPC_EXTRA_TILES ? a.nib * ((a.n_k + kGenShootWaves - 1) / kGenShootWaves) : 0);
    const dim3 ngrid((unsigned)im::xcd_grid(n_tiles));
    if (int rc = for_degree<2>(T.lay.d, [&](auto dc) -> int {
            mpc_gen_node_kernel<decltype(dc)::value><<<ngrid, 64 * kGenNodeWaves, 0, s>>>(
                h->d_VT, h->d_PT, h->d_cst, h->d_gdtab, h->d_gctab, h->d_gcoff, g, grad_f, jac, h->d_gfpart, a);
            return AWE_OK;
        }, unsupported_d)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->gev[2], s));
    mpc_gen_finalize_kernel<<<dim3((unsigned)a.nib), 64, 0, s>>>(h->d_VT, h->d_PT, h->d_gfpart, f, grad_f, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->gev[3], s));
    h->gtimed = true;
    return AWE_OK;
}

int awempc_last_kernel_ms_im(awempc_handle h, float* ms_in, float* ms_node, float* ms_fin) {
    if (!h || !h->gtimed) return fail(AWE_ERR_ARG, "no timed instance-minor evaluation yet");
    HIP_TRY(hipEventSynchronize(h->gev[3]));
    if (ms_in) HIP_TRY(hipEventElapsedTime(ms_in, h->gev[0], h->gev[1]));
    if (ms_node) HIP_TRY(hipEventElapsedTime(ms_node, h->gev[1], h->gev[2]));
    if (ms_fin) HIP_TRY(hipEventElapsedTime(ms_fin, h->gev[2], h->gev[3]));
    return AWE_OK;
}

int awempc_last_kernel_ms(awempc_handle h, float* ms_main, float* ms_fin) {
    if (!h || !h->timed) return fail(AWE_ERR_ARG, "no timed evaluation yet");
    HIP_TRY(hipEventSynchronize(h->ev[2]));
    if (ms_main) HIP_TRY(hipEventElapsedTime(ms_main, h->ev[0], h->ev[1]));
    if (ms_fin) HIP_TRY(hipEventElapsedTime(ms_fin, h->ev[1], h->ev[2]));
    return AWE_OK;
}

int awempc_eval_nlp_host(awempc_handle h, const double* V, const double* p, double* f, double* g, double* grad_f,
                         double* jac) {
    if (!h || !V || !p || !f || !g || !grad_f || !jac) return fail(AWE_ERR_ARG, "null argument");
    const Tables& T = h->t;
    const size_t nb = (size_t)h->batch, nnz = T.row.size();
    return host_round_trip(
        {{h->d_V, V, nb * T.lay.n_v}, {h->d_P, p, nb * T.lay.n_p}},
        {{h->d_f, f, nb}, {h->d_g, g, nb * T.lay.n_g}, {h->d_grad, grad_f, nb * T.lay.n_v}, {h->d_jac, jac, nb * nnz}},
        [&] { return awempc_eval_nlp(h, h->d_V, h->d_P, h->d_f, h->d_g, h->d_grad, h->d_jac, nullptr); },
        "non-finite output");
}

// ---- rk4root plant ---------------------------------------------------------------------------
static int plant_check(const double* consts, int n_consts, const void* const* ptrs, int n_ptrs, int batch, int n_fe,
                       int n_steps, int max_newton) {
    if (n_consts != K3_NCONST) return fail(AWE_ERR_ARG, "expected " + std::to_string(K3_NCONST) + " model constants");
    if (batch < 1) return fail(AWE_ERR_ARG, "batch must be >= 1");
    if (n_fe < 1) return fail(AWE_ERR_ARG, "n_fe must be >= 1");
    if (n_steps < 1) return fail(AWE_ERR_ARG, "n_steps must be >= 1");
    if (max_newton < 0) return fail(AWE_ERR_ARG, "max_newton must be >= 0");
    for (int i = 0; i < n_ptrs; ++i)
        if (!ptrs[i]) return fail(AWE_ERR_ARG, "null argument");
    if ((int)consts[K3_C_N_ELEMENTS] != awe_k3root::kNElements)
        return fail(AWE_ERR_ARG, "the generated rootfinder code has " + std::to_string(awe_k3root::kNElements) +
                                     " tether elements, the constants " + std::to_string((int)consts[K3_C_N_ELEMENTS]));
    return AWE_OK;
}

int awempc_plant_rk4root(awempc_handle h, const double* x0, const double* u, const double* z0, const double* par,
                         double ts, int n_fe, int n_steps, int max_newton, double tol, double* xf, double* zf,
                         double* qf, double* res, void* stream) {
    if (!h) return fail(AWE_ERR_ARG, "null handle");
    const void* ptrs[] = {x0, u, z0, par, xf, zf, qf, res};
    if (int rc = plant_check(h->consts.data(), (int)h->consts.size(), ptrs, 8, h->batch, n_fe, n_steps, max_newton))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    PlantArgs a{x0, u, z0, par, h->d_cst, ts, tol, n_fe, n_steps, max_newton, h->batch, xf, zf, qf, res};
    HIP_TRY(hipEventRecord(h->pev[0], s));
    mpc_plant_rk4root_kernel<<<dim3((unsigned)((h->batch + 63) / 64)), 64, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->pev[1], s));
    h->ptimed = true;
    return AWE_OK;
}

int awempc_plant_rk4root_cpu(const double* consts, int n_consts, int batch, const double* x0, const double* u,
                             const double* z0, const double* par, double ts, int n_fe, int n_steps, int max_newton,
                             double tol, double* xf, double* zf, double* qf, double* res) {
    const void* ptrs[] = {consts, x0, u, z0, par, xf, zf, qf, res};
    if (!consts) return fail(AWE_ERR_ARG, "null argument");
    if (int rc = plant_check(consts, n_consts, ptrs, 9, batch, n_fe, n_steps, max_newton)) return rc;
    double cs[K3_NCONST + K3_NX];
    for (int i = 0; i < K3_NCONST; ++i) cs[i] = consts[i];
    for (int i = 0; i < K3_NX; ++i) cs[K3_NCONST + i] = cs[K3_C_SCALING + K3_NX + i] / cs[K3_C_SCALING + i];
    PlantArgs a{x0, u, z0, par, cs, ts, tol, n_fe, n_steps, max_newton, batch, xf, zf, qf, res};
    PlantHostSys sys;
    for (int b = 0; b < batch; ++b) plant_instance(a, (size_t)b, cs, sys);
    return AWE_OK;
}

int awempc_last_plant_ms(awempc_handle h, float* ms) {
    if (!h || !h->ptimed) return fail(AWE_ERR_ARG, "no timed plant call yet");
    HIP_TRY(hipEventSynchronize(h->pev[1]));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, h->pev[0], h->pev[1]));
    return AWE_OK;
}

// ---- reference generator ---------------------------------------------------------------------
// the grids of a table over `coef`, or why not
static int ref_grids(int n_k, int d, double period, const int* pieces, const int* degree, const double* brk,
                     const double* coef, awe::RefArgs& a) {
    if (n_k < 1 || d < 1) return fail(AWE_ERR_ARG, "n_k and d must be >= 1");
    if (const char* why = awe::ref_check(pieces, degree, brk, period)) return fail(AWE_ERR_ARG, why);
    const int channels[awe::kRefGrids] = {K3_NX, K3_NZ, K3_NU + K3_NX + K3_NZ};
    int b0 = 0;
    size_t c0 = 0;
    for (int g = 0; g < awe::kRefGrids; ++g) {
        a.g[g] = awe::RefGrid{b0, pieces[g], degree[g], channels[g], coef ? coef + c0 : nullptr};
        b0 += pieces[g] + 1;
        c0 += (size_t)pieces[g] * channels[g] * (degree[g] + 1);
    }
    a.period = period;
    a.n_k = n_k, a.d = d, a.n_head = K3_NTH + K3_NPHI + K3_NXI, a.nx = K3_NX, a.nu = K3_NU, a.nz = K3_NZ;
    return AWE_OK;
}

static size_t ref_ncoef(const awe::RefArgs& a) {
    size_t n = 0;
    for (const awe::RefGrid& g : a.g) n += (size_t)g.pieces * g.channels * (g.degree + 1);
    return n;
}

int awempc_ref_set(awempc_handle h, double period, const double* offs, const double* head, const int* pieces,
                   const int* degree, const double* brk, const double* coef) {
    if (!h) return fail(AWE_ERR_ARG, "null handle");
    if (!offs || !head || !coef) return fail(AWE_ERR_ARG, "null argument");
    awe::RefArgs a{};
    if (int rc = ref_grids(h->t.lay.n_k, h->t.lay.d, period, pieces, degree, brk, nullptr, a)) return rc;
    h->ref_ready = false;
    const int n_brk = a.g[2].brk0 + a.g[2].pieces + 1;
    HIP_TRY(h->d_ref_brk.upload(brk, (size_t)n_brk));
    HIP_TRY(h->d_ref_coef.upload(coef, ref_ncoef(a)));
    HIP_TRY(h->d_ref_offs.upload(offs, (size_t)awe::ref_points(a.n_k, a.d)));
    HIP_TRY(h->d_ref_head.upload(head, (size_t)a.n_head));
    if (int rc = ref_grids(a.n_k, a.d, period, pieces, degree, brk, h->d_ref_coef, a)) return rc;
    a.offs = h->d_ref_offs, a.head = h->d_ref_head, a.batch = h->batch;
    h->ref = a;
    h->ref_nbrk = n_brk;
    h->ref_ready = true;
    return AWE_OK;
}

int awempc_ref_window(awempc_handle h, const double* t0, double* out, size_t ld, size_t off, void* stream) {
    if (!h) return fail(AWE_ERR_ARG, "null handle");
    if (!h->ref_ready) return fail(AWE_ERR_ARG, "no reference tables: call awempc_ref_set first");
    if (!t0 || !out) return fail(AWE_ERR_ARG, "null argument");
    if (ld < off + (size_t)h->t.lay.n_v) return fail(AWE_ERR_ARG, "ld must be >= off + n_v");
    hipStream_t s = (hipStream_t)stream;
    awe::RefArgs a = h->ref;
    a.t0 = t0, a.out = out, a.ld = ld, a.off = off;
    const size_t n = (size_t)h->batch * (size_t)awe::ref_points(a.n_k, a.d);
    HIP_TRY(hipEventRecord(h->rev[0], s));
    mpc_ref_window_kernel<<<dim3((unsigned)((n + kRefBlock - 1) / kRefBlock)), kRefBlock, 0, s>>>(a, h->d_ref_brk,
                                                                                                   h->ref_nbrk);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->rev[1], s));
    h->rtimed = true;
    return AWE_OK;
}

int awempc_ref_window_cpu(int n_k, int d, int batch, double period, const double* offs, const double* head,
                          const int* pieces, const int* degree, const double* brk, const double* coef,
                          const double* t0, double* out, size_t ld, size_t off) {
    if (!offs || !head || !coef || !t0 || !out) return fail(AWE_ERR_ARG, "null argument");
    if (batch < 1) return fail(AWE_ERR_ARG, "batch must be >= 1");
    awe::RefArgs a{};
    if (int rc = ref_grids(n_k, d, period, pieces, degree, brk, coef, a)) return rc;
    const int n_v = a.n_head + n_k * (2 * K3_NX + K3_NU + K3_NZ + d * (K3_NX + K3_NZ)) + K3_NX;
    if (ld < off + (size_t)n_v) return fail(AWE_ERR_ARG, "ld must be >= off + n_v");
    a.offs = offs, a.head = head, a.batch = batch, a.t0 = t0, a.out = out, a.ld = ld, a.off = off;
    const int n_pt = awe::ref_points(n_k, d);
    for (int b = 0; b < batch; ++b)
        for (int q = 0; q < n_pt; ++q) awe::ref_point(a, brk, (size_t)b, q);
    return AWE_OK;
}

int awempc_last_ref_ms(awempc_handle h, float* ms) {
    if (!h || !h->rtimed) return fail(AWE_ERR_ARG, "no timed reference window yet");
    HIP_TRY(hipEventSynchronize(h->rev[1]));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, h->rev[0], h->rev[1]));
    return AWE_OK;
}

// ---- nlp_hess_l ------------------------------------------------------------------------------
int awempc_sparsity_hess_static(int n_k, int d, const double* consts, int n_consts, int* nnz, int* colind, int* row) {
    if (!consts || !nnz) return fail(AWE_ERR_ARG, "null argument");
    Tables T;
    HessTables H;
    std::string err;
    if (build_tables(n_k, d, consts, n_consts, T, err) || build_hess_tables(T, consts, H, err))
        return fail(AWE_ERR_ARG, err);
    copy_ccs(nnz, colind, row, H.colind, H.row);
    return AWE_OK;
}

int awempc_hess_init(awempc_handle h, int* nnz) {
    if (!h) return fail(AWE_ERR_ARG, "null handle");
    if (!h->hess_ready) {
        std::string err;
        if (build_hess_tables(h->t, h->consts.data(), h->ht, err)) return fail(AWE_ERR_ARG, err);
        const HessTables& H = h->ht;
        h->hd_total = H.ntask[0] + h->t.lay.d * H.ntask[1];
        if ((size_t)h->hd_total * sizeof(double) > 60 * 1024) return fail(AWE_ERR_ARG, "Hessian tasks exceed the LDS budget");
        if ((int)H.gslot.size() > 64) return fail(AWE_ERR_ARG, "too many global Hessian entries");
        HIP_TRY(h->d_task.upload(H.task));
        HIP_TRY(h->d_slot0.upload(H.slot0));
        HIP_TRY(h->d_nslot.upload(H.nslot));
        HIP_TRY(h->d_ent_off.upload(H.ent_off));
        HIP_TRY(h->d_term_off.upload(H.term_off));
        HIP_TRY(h->d_terms.upload(H.terms));
        HIP_TRY(h->d_hgslot.upload(H.gslot));
        HIP_TRY(h->d_xnslot.upload(H.xnslot));
        HIP_TRY(h->d_gpart.alloc((size_t)h->batch * h->t.lay.n_k * std::max<size_t>(1, H.gslot.size())));
        for (auto& e : h->hev) HIP_TRY(e.create());
        h->hess_ready = true;
    }
    if (nnz) *nnz = h->ht.nnz;
    return AWE_OK;
}

int awempc_sparsity_hess(awempc_handle h, int* colind, int* row) {
    if (!h || !colind || !row) return fail(AWE_ERR_ARG, "null argument");
    int rc = awempc_hess_init(h, nullptr);
    if (rc) return rc;
    copy_ccs(nullptr, colind, row, h->ht.colind, h->ht.row);
    return AWE_OK;
}

int awempc_eval_hess(awempc_handle h, const double* V, const double* p, const double* sigma, const double* lam_g,
                     double* H, void* stream) {
    if (!h || !V || !p || !sigma || !lam_g || !H) return fail(AWE_ERR_ARG, "null argument");
    int rc = awempc_hess_init(h, nullptr);
    if (rc) return rc;
    const Tables& T = h->t;
    const HessTables& HT = h->ht;
    hipStream_t s = (hipStream_t)stream;
    MArgs a{T.lay.n_k, T.lay.d, T.lay.n_v, T.lay.n_g, T.lay.n_p, (int)T.row.size(), T.lay.stride,
            V, p, nullptr, nullptr, nullptr, nullptr, h->d_cst, h->d_coll, h->d_goff, h->d_gslot, h->d_gcode, h->d_fpart};
    HArgs ha{a, sigma, lam_g, H, h->d_gpart, h->d_task, HT.ntask[0], HT.ntask[1], HT.npair1, HT.nnz,
             (int)HT.gslot.size(), h->hd_total, h->d_slot0, h->d_nslot, h->d_ent_off, h->d_term_off, h->d_terms,
             h->d_hgslot, h->d_xnslot};
    const dim3 grid((unsigned)(h->batch * T.lay.n_k));
    const size_t lds = sizeof(double) * (size_t)h->hd_total;
    HIP_TRY(hipEventRecord(h->hev[0], s));
    if (int rc = for_degree<2>(T.lay.d, [&](auto dc) -> int {
            mpc_hess_kernel<decltype(dc)::value><<<grid, kHessThreads, lds, s>>>(ha);
            return AWE_OK;
        }, unsupported_d)) return rc;
    HIP_TRY(hipGetLastError());
    mpc_hess_finalize_kernel<<<dim3((unsigned)h->batch), 64, 0, s>>>(ha);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->hev[1], s));
    h->htimed = true;
    return AWE_OK;
}

int awempc_last_hess_ms(awempc_handle h, float* ms) {
    if (!h || !h->htimed) return fail(AWE_ERR_ARG, "no timed Hessian evaluation yet");
    HIP_TRY(hipEventSynchronize(h->hev[1]));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, h->hev[0], h->hev[1]));
    return AWE_OK;
}

int awempc_eval_hess_host(awempc_handle h, const double* V, const double* p, const double* sigma, const double* lam_g,
                          double* H) {
    if (!h || !V || !p || !sigma || !lam_g || !H) return fail(AWE_ERR_ARG, "null argument");
    int rc = awempc_hess_init(h, nullptr);
    if (rc) return rc;
    const Tables& T = h->t;
    const size_t nb = (size_t)h->batch, hnnz = h->ht.nnz;
    return host_round_trip(
        {{h->d_V, V, nb * T.lay.n_v}, {h->d_P, p, nb * T.lay.n_p}, {h->d_hsig, sigma, nb},
         {h->d_hlam, lam_g, nb * T.lay.n_g}},
        {{h->d_H, H, nb * hnnz}},
        [&] { return awempc_eval_hess(h, h->d_V, h->d_P, h->d_hsig, h->d_hlam, h->d_H, nullptr); },
        "non-finite Hessian");
}

}  // extern "C"
