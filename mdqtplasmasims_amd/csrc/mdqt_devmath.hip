// mdqt_device_math (include/mdqt.h): the device math functions of the QT, pair and observables kernels, evaluated
// one element per thread through the same inline functions the kernels call, so that a test can hold
// each of them to its stated error against an extended-precision value (tests/test_gpu_device_math.py).
// No shared state; the two tables are read from their __constant__ arrays (the kernels stage the same
// values in LDS).
#include "mdqt_devbuf.hpp"
#include "mdqt_device.hpp"
#include "mdqt_error.hpp"
#include "mdqt_pairs.hpp"

#include "mdqt.h"

namespace mdqt {

enum DevMathFn : int {
    DM_SINCOS_TAB = 0,    // sincos_tab(x, kSinCos64): |x| < 2^20
    DM_SINCOS_FAST = 1,   // sincos_fast(x): |x| < 2^20
    DM_SINCOS_Q2 = 2,     // sincos_q2(x, kSinCos64): the table form, the library for |x| >= 2^20
    DM_RSQ3 = 3,          // rsq3(x)
    DM_EXP_NEG = 4,       // exp_neg(x), x <= 0
    DM_EXP2_TAB = 5,      // exp2_neg_cut_tab(x, true, kExp2Tab64) = 2^(x/64), x <= 0
    DM_EXP_LIB = 6,       // exp(x): the math library's, as the velocity distributions call it (kde_chunk)
    DM_NFN
};

__global__ __launch_bounds__(256) void k_device_math(int fn, const double* __restrict__ x, int n,
                                                     double* __restrict__ out0, double* __restrict__ out1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double a = 0., b = 0.;
    switch (fn) {
    case DM_SINCOS_TAB: sincos_tab(v, kSinCos64, a, b); break;
    case DM_SINCOS_FAST: sincos_fast(v, a, b); break;
    case DM_SINCOS_Q2: sincos_q2(v, kSinCos64, a, b); break;
    case DM_RSQ3: a = rsq3(v); break;
    case DM_EXP_NEG: a = exp_neg(v); break;
    case DM_EXP_LIB: a = exp(v); break;
    default: a = exp2_neg_cut_tab(v, true, kExp2Tab64); break;
    }
    out0[i] = a;
    if (out1) out1[i] = b;
}

}  // namespace mdqt

extern "C" int mdqt_device_math(int fn, const double* x, int n, double* out0, double* out1, int device) {
    using namespace mdqt;
    if (fn < 0 || fn >= DM_NFN) return set_error("mdqt_device_math: unknown function %d", fn);
    if (n < 1 || !x || !out0) return set_error("mdqt_device_math: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error("no HIP device available");
    hipError_t e = hipSuccess;
    if (device >= 0 && (e = hipSetDevice(device)) != hipSuccess)
        return set_error("mdqt_device_math: hipSetDevice: %s", hipGetErrorString(e));
    const size_t bytes = (size_t)n * sizeof(double);
    DevBuf<double> dx, d0, d1;
    auto run = [&]() -> hipError_t {
        hipError_t r;
        if ((r = dx.alloc((size_t)n)) != hipSuccess) return r;
        if ((r = d0.alloc((size_t)n)) != hipSuccess) return r;
        if (out1 && (r = d1.alloc((size_t)n)) != hipSuccess) return r;
        if ((r = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice)) != hipSuccess) return r;
        hipLaunchKernelGGL(k_device_math, dim3((n + 255) / 256), dim3(256), 0, 0, fn, (const double*)dx, n, (double*)d0,
                           (double*)d1);
        if ((r = hipGetLastError()) != hipSuccess) return r;
        if ((r = hipMemcpy(out0, d0, bytes, hipMemcpyDeviceToHost)) != hipSuccess) return r;
        if (out1 && (r = hipMemcpy(out1, d1, bytes, hipMemcpyDeviceToHost)) != hipSuccess) return r;
        return hipSuccess;
    };
    e = run();
    if (e != hipSuccess) return set_error("mdqt_device_math: %s", hipGetErrorString(e));
    return 0;
}
