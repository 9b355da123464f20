// Host-side plumbing shared by the model libraries (awegpu.hip, awedual.hip + awedual_gen.hip,
// awempc.hip): owners of device allocations, events and streams, the thread-local error string
// behind each library's *_last_error, and the host round trip of the *_host entry points.
// Host only: nothing here is __global__ or __device__.  Every name has hidden visibility, so each
// shared library keeps its own error string and exports nothing from this header.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/awegpu.h"

#pragma GCC visibility push(hidden)
namespace hostu {

// ---- errors ------------------------------------------------------------------------------------
inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess)                                                                       \
            return hostu::fail(AWE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
    } while (0)

// ---- owners ------------------------------------------------------------------------------------
// One hipMalloc allocation of n elements of T; move-only, freed by the destructor.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    hipError_t alloc(size_t n) {
        reset();
        return hipMalloc((void**)&p_, sizeof(T) * n);
    }
    hipError_t upload(const T* src, size_t n) {
        hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemcpy(p_, src, sizeof(T) * n, hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
};

// A hipEvent_t / hipStream_t created on demand and destroyed with its owner.
class Event {
public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e_) (void)hipEventDestroy(e_);
    }
    hipError_t create() { return hipEventCreate(&e_); }
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e_, flags); }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

class Stream {
public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s_) (void)hipStreamDestroy(s_);
    }
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s_, flags); }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

// ---- helpers -----------------------------------------------------------------------------------
// The CCS pattern out of a sparsity entry point: the count, and the arrays where asked for.
inline void copy_ccs(int* nnz, int* colind, int* row, const std::vector<int>& c, const std::vector<int>& r) {
    if (nnz) *nnz = (int)r.size();
    if (colind) std::memcpy(colind, c.data(), sizeof(int) * c.size());
    if (row) std::memcpy(row, r.data(), sizeof(int) * r.size());
}

inline bool all_finite(const double* x, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return false;
    return true;
}

// The collocation degree as a compile-time constant: f(std::integral_constant<int, D>{}) for the D in
// LO..5 that equals the run-time d, and its result; for any other d, unsupported() and its result.
template <int LO = 1, class F, class U>
auto for_degree(int d, F&& f, U&& unsupported) -> decltype(unsupported()) {
    if constexpr (LO > 5) return unsupported();
    else if (d == LO) return f(std::integral_constant<int, LO>{});
    else return for_degree<LO + 1>(d, f, unsupported);
}

// One array of a host round trip: the handle's staging buffer, the caller's array and its length.
struct HostIn {
    DevBuf<double>& buf;
    const double* src;
    size_t n;
};
struct HostOut {
    DevBuf<double>& buf;
    double* dst;
    size_t n;
};

// The host entry points: staging buffers allocated on first use, inputs copied in, `launch` (which
// enqueues on the null stream and returns an AWE code), a device synchronisation, outputs copied
// back and scanned: a non-finite value is AWE_ERR_NONFINITE with `nonfinite` as the message.
template <class Launch>
int host_round_trip(std::initializer_list<HostIn> ins, std::initializer_list<HostOut> outs, Launch&& launch,
                    const char* nonfinite) {
    for (const HostIn& i : ins)
        if (!i.buf) HIP_TRY(i.buf.alloc(i.n));
    for (const HostOut& o : outs)
        if (!o.buf) HIP_TRY(o.buf.alloc(o.n));
    for (const HostIn& i : ins) HIP_TRY(hipMemcpy(i.buf, i.src, sizeof(double) * i.n, hipMemcpyHostToDevice));
    if (int rc = launch()) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (const HostOut& o : outs) HIP_TRY(hipMemcpy(o.dst, o.buf, sizeof(double) * o.n, hipMemcpyDeviceToHost));
    for (const HostOut& o : outs)
        if (!all_finite(o.dst, o.n)) return fail(AWE_ERR_NONFINITE, nonfinite);
    return AWE_OK;
}

}  // namespace hostu
#pragma GCC visibility pop
