// The step kernel of a three-level laser-cooling scan (mdlc_create_sweep: parameter points x replicas), in a
// translation unit — hence a code object — of its own: mdlc_kernels.hip's stays what it is without the scan.
// The kernel wraps lc_steps_body (mdlc_device.hpp), the body k_lc_steps runs.  Built with mdlc_kernels.hip's
// flags.
//
// A member's workgroups read its point's three constants (Im M11 at v = 0, the coupling, the optical kick's
// scale) once, before the step loop, at a workgroup-uniform address: three scalar loads into the SGPRs where
// k_lc_steps holds the same kernel arguments.  Everything else of LCArgs is fixed across a scan.  The table is
// written once, at create.
#include "mdlc_device.hpp"

namespace mdqt {

__global__ __launch_bounds__(kLCBlock) void k_lc_steps_sweep(LCArgs a, const LCPoint* __restrict__ pts, int R) {
    const int member = blockIdx.x / a.B;
    const int point = member / R;
    const LCPoint p = pts[point];
    // the three loads are waited for here, not at their first use inside the step loop (an empty statement that
    // takes the values in SGPRs)
    asm volatile("" ::"s"(p.mi0), "s"(p.cim), "s"(p.ks));
    lc_steps_body(a, member, a.job0 + (uint32_t)(member - point * R), p.mi0, p.cim, p.ks);
}

hipError_t launch_lc_steps_sweep(const LCArgs& a, const LCPoint* pts, int R, int J, hipStream_t s, hipEvent_t ev0,
                                 hipEvent_t ev1) {
    if (!pts || R < 1 || J < 1 || J % R) return hipErrorInvalidValue;
    launch_timed(k_lc_steps_sweep, dim3((unsigned)J * (unsigned)a.B), dim3(kLCBlock), s, ev0, ev1, a, pts, R);
    return hipGetLastError();
}

}  // namespace mdqt
