// Instance-minor kit shared by the evaluators' generated paths (awegpu.hip, awempc.hip,
// awedual_gen.hip): addressing, tile order, the input transpose, the staging of a node's destination
// row and the tangent sink of the generated node code.  The slot table and the host builder of the
// destination tables are in im_tables.hpp.
//
// An instance-minor buffer holds row i of every instance side by side: X[i * ld + b].  A wavefront
// with lane = instance then reads or writes one 512-byte row per access.  Rows are addressed as a
// uniform byte offset row * ld8 (32-bit; the hosts keep every such buffer below 4 GiB) plus the
// lane's constant offset lb = 8 b, so an access is one scalar base (SGPR) plus the lane's constant
// vector offset -- no per-access 64-bit address arithmetic in the vector registers.
#pragma once

#include <hip/hip_runtime.h>

#include "im_tables.hpp"

namespace im {

__device__ __forceinline__ const double& at(const double* x, unsigned row, unsigned ld8, unsigned lb) {
    return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(x) + row * ld8 + lb);
}
__device__ __forceinline__ double& at(double* x, unsigned row, unsigned ld8, unsigned lb) {
    return *reinterpret_cast<double*>(reinterpret_cast<char*>(x) + row * ld8 + lb);
}
__device__ __forceinline__ double& at_byte(double* x, unsigned off) {
    return *reinterpret_cast<double*>(reinterpret_cast<char*>(x) + off);
}

// blockIdx.x -> tile: consecutive tiles to the same XCD (blocks are dealt to the 8 XCDs round robin),
// so that the tiles of one instance block share that XCD's L2
__device__ __forceinline__ int xcd_tile(int total) {
    const int per = (total + 7) / 8;
    return (blockIdx.x & 7) * per + (blockIdx.x >> 3);
}
__host__ __device__ constexpr int xcd_grid(int total) { return ((total + 7) / 8) * 8; }

// A [batch][na] and B [batch][nb] (per-instance rows) -> AT[i * ld + b], BT[i * ld + b], 64 x 64 tiles
// through LDS; grid (ceil((na + nb) / 64), ceil(batch / 64)), 256 threads.  NONTEMPORAL: the stores
// bypass L2 (for outputs beyond it, which the next kernel reads back from HBM anyway).  The kernel
// with plain stores is a plain function of this header, so every library that includes the header
// carries it: 2 KiB of code that awegpu.hip, which launches its own wrapper, does not use
template <bool NONTEMPORAL>
__device__ __forceinline__ void transpose_in(const double* __restrict__ A, const double* __restrict__ B,
                                             double* __restrict__ AT, double* __restrict__ BT, int batch, int na,
                                             int nb, int ld) {
    __shared__ double tile[64][65];
    const int ncol = na + nb;
    const int c0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
    const int tid = threadIdx.x;
    double r[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int e = tid + it * 256, bl = e >> 6, cl = e & 63;
        const int bc = min(b0 + bl, batch - 1), cc = min(c0 + cl, ncol - 1);   // unconditional loads
        r[it] = cc < na ? A[(size_t)bc * na + cc] : B[(size_t)bc * nb + (cc - na)];
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int e = tid + it * 256;
        tile[e >> 6][e & 63] = r[it];
    }
    __syncthreads();
    auto put = [](double v, double* p) {
        if (NONTEMPORAL) __builtin_nontemporal_store(v, p);
        else *p = v;
    };
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int e = tid + it * 256, cl = e >> 6, bl = e & 63;
        const int b = b0 + bl, c = c0 + cl;
        if (b < batch && c < ncol) {
            if (c < na) put(tile[bl][cl], &AT[(size_t)c * ld + b]);
            else put(tile[bl][cl], &BT[(size_t)(c - na) * ld + b]);
        }
    }
}
__global__ __launch_bounds__(256) void transpose_in_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                           double* __restrict__ AT, double* __restrict__ BT,
                                                           int batch, int na, int nb, int ld) {
    transpose_in<false>(A, B, AT, BT, batch, na, nb, ld);
}

// stages n destination-table entries into LDS as byte offsets (pos * row8), 8 loads in flight per thread
template <int NT>
__device__ __forceinline__ void stage_offsets(unsigned* dst, const unsigned* src, int n, unsigned row8, int tid) {
    for (int base = tid; base < n; base += NT * 8) {
        unsigned r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = src[base + u * NT < n ? base + u * NT : n - 1];   // unconditional
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (base + u * NT < n) dst[base + u * NT] = r[u] * row8;
    }
}

template <class Traits, int D>
constexpr SlotTab<Traits> kSlots{D};

// tan[s] = v  ->  the J_g entries of slot s.  dt: the node's destination row in LDS, as byte offsets
// pos * 8 ldj (staged by the workgroup with stage_offsets; reading the table with scalar loads left
// every wave of the AP2 node kernels waiting on scalar-cache misses for 58 % of its cycles); the d
// destinations of an xdot direction (polynomial columns X_r, r != n, in r order) take
// v x C[r][n] / (h t_f), the lane's xs[q] -- the AP2 gather kernel's scl[sc] * tangent, bitwise.
template <class Traits, int D, int KIND>
struct JSink {
    double* jac;
    unsigned lb;
    const unsigned* dt;
    const double* xs;
    struct Ref {
        const JSink* s;
        int slot;
        __device__ __forceinline__ void operator=(double v) const { s->put(slot, v); }
    };
    __device__ __forceinline__ Ref operator[](int slot) const { return Ref{this, slot}; }
    __device__ __forceinline__ void put(int slot, double v) const {
        const int f = kSlots<Traits, D>.first[KIND][slot], c = kSlots<Traits, D>.cnt[KIND][slot];
        // non-temporal: J_g is written once and read by nobody in this launch; allocating its
        // lines in L2 evicted the staged inputs and the interval pass's rows (AP2 at B = 2048:
        // 0.58 -> 0.50 ms node kernels, 0.146 -> 0.116 ms interval kernel, tools/gpu_soa_ab.sh)
        if (c == 1) {
            __builtin_nontemporal_store(v, &at_byte(jac, dt[f] + lb));
            return;
        }
#pragma unroll
        for (int q = 0; q < D; ++q) __builtin_nontemporal_store(xs[q] * v, &at_byte(jac, dt[f + q] + lb));
    }
};

}  // namespace im
