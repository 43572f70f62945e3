// The error plumbing every host source of the three engines shares (MDQT, MC + MD, three-level cooling): the C
// ABI's error message, the check of a HIP call, and two host constants that came with them.  Host code only (the
// one .hip file that includes it, mdqt_devmath.hip, does so for its own C ABI entry point).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// mdqt::set_error (mdqt_engine.cpp) records the calling thread's message for mdqt_last_error, mdmc_last_error
// and mdlc_last_error, and returns -1
#define HIPCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess)                                                         \
            return mdqt::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

namespace mdqt {

// error message of the C ABI (mdqt_last_error), shared by the mdmc_* and mdlc_* entry points
int set_error(const char* fmt, ...);
// the reference's "(unsigned)(x)" printed with %d (x86-64 runtime behaviour):
// the directory names of every program's main()
inline int ref_udcast(double x) { return (int)(uint32_t)(int64_t)x; }

// Timing events only measure: no system-scope release/acquire when they complete.  With the
// default flags every timed launch ended in an L2 write-back + invalidate that cost the MD step
// ~20 us (kernel trace of the driver's bench command: gaps of 6.5 / 8.9 / 4.8 us around each
// timed pair of launches, none elsewhere).
constexpr unsigned kTimingEventFlags = hipEventDisableSystemFence;

}  // namespace mdqt
