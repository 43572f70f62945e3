// The three-level laser-cooling program's interface between its host engine (mdlc_engine.cpp) and its kernels
// (mdlc_kernels.hip, mdlc_sweep_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdqt {

// ---- three-level laser cooling without plasma (mdlc_kernels.hip; laserCoolNoPlasmaThreeState.cpp, "LC3") ----
// An ensemble of J independent jobs of N0 ions: job k's ions sit at [k S, k S + N0) of every array,
// S = N0 padded to whole workgroups (kLCBlock threads), so that no workgroup straddles two jobs.
constexpr int kLCBlock = 256;
struct LCArgs {
    double* vx;         // [J][S] V[0][i] (LC3:170: the only velocity row qstep() reads)
    double* psi;        // [6][J S] component-major (re0, im0, re1, im1, re2, im2)
    double* tPart;      // [J S]
    double* part;       // [J][B] out: each workgroup's sum of 0.5 vx^2 after the launch's last step
    int N0, S, B;       // ions per job, padded stride, workgroups per job (S / kLCBlock)
    int nsteps;         // qstep() x nsteps (0: the partial sums only)
    uint64_t q0;        // qstep index of the first step (Philox counter)
    uint32_t seed, job0;   // Philox key of job k: (seed, job0 + k)
    int applyForce;     // LC3:63, :287
    // M = I - i dt H (LC3:192-208, :223): M00 = 1, M11 = mre + i (mi0 - dt v), M22 = mre + i (mi0 + dt v),
    // M01 = M02 = M10 = M20 = i cim
    double dt, mre, mi0, cim;
    double ks;          // vKick Om dt: the optical kick's scale (LC3:189)
    double vKick;       // LC3:88, :279-284
};
hipError_t launch_lc_steps(const LCArgs& a, int J, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// A parameter scan (mdlc_create_sweep; mdlc_sweep_kernels.hip): what differs between the points in LCArgs.  The J
// members are npoints x R, point-major: member m is point m / R, its Philox key (seed, job0 + m % R); a's mi0, cim
// and ks are not read
struct LCPoint {
    double mi0, cim, ks;
};
hipError_t launch_lc_steps_sweep(const LCArgs& a, const LCPoint* pts, int R, int J, hipStream_t s,
                                 hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// out[k] = (fixed-order sum of job k's B workgroup partials) / N0: output()'s EkinX (LC3:309-316)
hipError_t launch_lc_ekin(const double* part, int J, int B, int N0, double* out, hipStream_t s);

}  // namespace mdqt
