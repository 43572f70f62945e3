// Three-level laser cooling without plasma: qstep() of laserCoolNoPlasmaThreeState.cpp ("LC3",
// :140-293) for an ensemble of independent jobs, one ion per thread, many steps per launch.
//
// The ions do not interact, so an ion's whole state — psi (6 doubles), vx, tPart — is loaded once,
// stepped nsteps times in registers and stored once.  Arithmetic follows the qt_math 2 form of
// mdqt_qtfast.hip: each row of M = I - i dt H is one fixed FMA chain (row 0: two coupling slots,
// rows 1 and 2: the diagonal and one slot; the couplings i dt Om/2 are purely imaginary and M00
// is exactly 1, so the FMAs that would add +-0 y are not issued), the 3/8-rule stages (:212-271) run
// on d = s - y with s = M y / sqrt(1 - dp(y)), and the prefactor is rsq3.  No phase, no sincos, no
// table: this program's H is constant in time.  Only the two excited diagonals depend on the
// thread (through vx); the rest of M comes in as launch-uniform kernel arguments.
//
// Random numbers: the Philox stream of mdqt_device.hpp, counter (ion, qstep index), key (seed,
// job); u1 is draw 0 and randDir draw 1 of the same call.
//
// Limit: a launch of one job is 16 waves on a 1,024-SIMD part, so its length is one wave's time
// for nsteps steps, not throughput.  A step is 198 FP64 instructions (286 vector instructions with
// the Philox call and the uniform conversion) in four stages, each a chain norm -> rsq3 -> rows ->
// update with six-fold parallelism inside.  Measured: 0.554 us per step, about 1,330 cycles per
// wave against 286 x 4 = 1,144 cycles of vector issue for a wave alone on its SIMD — the launch
// sits under the wave's own instruction issue, the dependent FP64 chain (FMA: 4 cycles issue, 6
// dependent, tools/ubench_f64.hip) adds the rest; 0.7 % of the FP64 roof for one job.  An ensemble
// fills the idle SIMDs at nearly the same launch length until every SIMD holds a wave: 64 jobs
// take 1.12 x one job's launch, 42 % of the roof (docs/PROGRAMS.md).
//
// EkinX (output(), :309-316) is deterministic: each wave sums its lanes' 0.5 vx^2 by a fixed xor
// tree, the workgroup adds its four waves in order and stores one partial, and k_lc_ekin adds a
// job's partials in a fixed order.  No floating-point atomics.
#include "mdlc_device.hpp"

namespace mdqt {

// the step body, with the laser's constants from the kernel arguments: lc_steps_body (mdlc_device.hpp), shared
// with k_lc_steps_sweep (mdlc_sweep_kernels.hip)
__global__ __launch_bounds__(kLCBlock) void k_lc_steps(LCArgs a) {
    const int job = blockIdx.x / a.B;
    lc_steps_body(a, job, a.job0 + (uint32_t)job, a.mi0, a.cim, a.ks);
}

// one wave per job: lane l adds partials l, l + 64, ... in ascending order, then the xor tree
__global__ __launch_bounds__(64) void k_lc_ekin(const double* __restrict__ part, int B, int N0,
                                                double* __restrict__ out) {
    const double* p = part + (size_t)blockIdx.x * B;
    double e = 0.;
    for (int b = threadIdx.x; b < B; b += 64) e = e + p[b];
    e = lc_wave_sum(e);
    if (threadIdx.x == 0) out[blockIdx.x] = e / (double)N0;                   // :316
}

hipError_t launch_lc_steps(const LCArgs& a, int J, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    launch_timed(k_lc_steps, dim3((unsigned)J * (unsigned)a.B), dim3(kLCBlock), s, ev0, ev1, a);
    return hipGetLastError();
}

hipError_t launch_lc_ekin(const double* part, int J, int B, int N0, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_lc_ekin, dim3(J), dim3(64), 0, s, part, B, N0, out);
    return hipGetLastError();
}

}  // namespace mdqt
