// The batched kernels of an ensemble of optical-pumping jobs (include/mdqt.h "ensembles of the
// optical-pumping programs"; host: mdqt_pump_ensemble.cpp), in a translation unit — hence a code object —
// of their own, so that the single-job kernels' code objects stay what they are.  Every kernel takes a
// device array of per-member argument blocks indexed by a grid axis and runs its single-job kernel's body
// (lane_substeps of mdqt_qtfast.hpp; leapfrog_kick, leapfrog_drift, tag_spin_up_ion, tagged_kde_chunk and
// tagged_kde_reduce_1 of mdqt_pump_device.hpp; the canonical slot sum of mdqt_math.hpp — slot_sum16's
// chains and tree16_sum, loaded in rounds: pump_settled_forces) on the member's own arguments: bit-identical
// to the member on its own.  Workgroups past a member's last ion, 16-ion group
// or chunk leave at once — a condition on blockIdx and the block, uniform over the workgroup, before any
// barrier or cross-lane operation.  The blocks' pointers come from memory, so the accesses are flat.
// Built with mdqt_qtfast.hip's flags (Makefile QTSCHED) and, as everything here, -ffp-contract=off:
// v += kick * f stays a product and a sum.
#include "mdqt_ens_args.hpp"
#include "mdqt_qtfast.hpp"
#include "mdqt_pump_device.hpp"

namespace mdqt {

// ---- QT: the pump models' lane instance (k_substeps_lanes_r<false, FAST>) over members; the FastTab is
// shared (same model and parameters) ----
template <bool FAST>
__global__ __launch_bounds__(256) void k_substeps_lanes_pump_ens(const SubstepArgs* __restrict__ jobs,
                                                                 const FastTab* __restrict__ tab) {
    const SubstepArgs& a = jobs[blockIdx.y];
    if ((int)blockIdx.x * kLaneIons >= a.n) return;
    lane_substeps<false, FAST, false>(a, tab, blockIdx.x);
}

hipError_t launch_substeps_pump_ens(const SubstepArgs* jobs, const SubstepArgs& a, int njobs, int max_n,
                                    const FastTab* tab, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int* instance) {
    if (njobs <= 0 || max_n <= 0 || a.nsub <= 0) return hipSuccess;
    if (!jobs || njobs > 65535 || a.nsub > MAXSUB || a.qc.model < 1 || a.qc.model >= NMODELS || a.arrive || a.U)
        return hipErrorInvalidValue;
    const dim3 gl((max_n + kLaneIons - 1) / kLaneIons, njobs), bl(kLaneWG);
    const FastTab* lt = tab + 1;                      // by lane
    const QTKernel inst = lane_qt_instance(a);
    switch (inst) {
    case QTK_LANES_R_PUMP_FAST: launch_timed(k_substeps_lanes_pump_ens<true>, gl, bl, s, ev0, ev1, jobs, lt); break;
    case QTK_LANES_R_PUMP: launch_timed(k_substeps_lanes_pump_ens<false>, gl, bl, s, ev0, ev1, jobs, lt); break;
    default: return hipErrorInvalidValue;             // (model 1-3, checked above: none of model 0's instances)
    }
    if (instance) *instance = inst;
    return hipGetLastError();
}

// ---- step(): one thread per ion of a member; F of a member with pending partials = their canonical sum
// (k_reduce_segments' value), written back ----
// slot_sum16 as written (k_reduce_segments) walks its sixteen strided chains one load at a time — each add
// waits for its load before the next is issued — and with the three components in one thread that is 3 nseg
// dependent memory round trips (measured: 43.7 us for one job of 3,523 ions and 56 slots, where the whole
// four-launch step of a context takes 33.8).  Here the same sum is evaluated in rounds, as the lane QT kernel
// evaluates it: a round loads slots s0 .. s0 + 15 of all three components at once (a slot past nseg: a clamped,
// in-range load replaced by +0), then q_k = q_k + p[s0 + k] — the chains' own operations in the chains' own
// order — and tree16_sum combines them.  The +0 terms change nothing: a chain starts at +0 and a sum in
// round-to-nearest is never -0 unless both terms are, so q_k is never -0 and q_k + 0 = q_k exactly.  Every
// load comes before the first store, since the compiler cannot know that the blocks' pointers do not alias.
__device__ __forceinline__ void pump_settled_forces(const PumpStepArgs& a, int i, double f[3]) {
    const int nseg = a.nseg, S = a.S;
    if (nseg <= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = a.F[(size_t)c * S + i];
        return;
    }
    const size_t plane = (size_t)3 * S;
    double q[3][16];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 16; ++k) q[c][k] = 0.;
    for (int s0 = 0; s0 < nseg; s0 += 16) {
        double t[3][16];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const double x = a.Fpart[(size_t)min(s0 + k, nseg - 1) * plane + (size_t)c * S + i];
                t[c][k] = s0 + k < nseg ? x : 0.;
            }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 16; ++k) q[c][k] = q[c][k] + t[c][k];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = tree16_sum(q[c]);
}

__global__ __launch_bounds__(256) void k_pump_drift_ens(const PumpStepArgs* __restrict__ jobs, double DT, double DT2,
                                                        int moving) {
    const PumpStepArgs& a = jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    double f[3], r[3];
    pump_settled_forces(a, i, f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t k = (size_t)c * a.S + i;
        r[c] = leapfrog_drift(a.R[k], a.V[k], f[c], a.L, DT, DT2, moving);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t k = (size_t)c * a.S + i;
        if (a.nseg > 1) a.F[k] = f[c];
        a.R[k] = r[c];
    }
}

__global__ __launch_bounds__(256) void k_pump_kick_ens(const PumpStepArgs* __restrict__ jobs, double DT, double DT2,
                                                       int moving, double kick, int fold) {
    const PumpStepArgs& a = jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    double f[3], v[3], r[3];
    pump_settled_forces(a, i, f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t k = (size_t)c * a.S + i;
        v[c] = leapfrog_kick(a.V[k], f[c], kick);                              // step_V(dt)
        r[c] = leapfrog_drift(a.R[k], v[c], f[c], a.L, DT, DT2, moving);       // step_R(dt/2)
        if (fold) r[c] = leapfrog_drift(r[c], v[c], f[c], a.L, DT, DT2, 1);    // the next step's step_R(dt/2), t > 0
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t k = (size_t)c * a.S + i;
        if (a.nseg > 1) a.F[k] = f[c];
        a.V[k] = v[c];
        a.R[k] = r[c];
    }
}

hipError_t launch_pump_drift_ens(const PumpStepArgs* jobs, int njobs, int max_n, double DT, double DT2, int moving,
                                 hipStream_t s) {
    if (njobs <= 0 || max_n <= 0) return hipSuccess;
    if (!jobs || njobs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pump_drift_ens, dim3((max_n + 255) / 256, njobs), dim3(256), 0, s, jobs, DT, DT2, moving);
    return hipGetLastError();
}

hipError_t launch_pump_kick_ens(const PumpStepArgs* jobs, int njobs, int max_n, double DT, double DT2, int moving,
                                double kick, int fold, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0 || max_n <= 0) return hipSuccess;
    if (!jobs || njobs > 65535 || kick == 0.) return hipErrorInvalidValue;
    launch_timed(k_pump_kick_ens, dim3((max_n + 255) / 256, njobs), dim3(256), s, ev0, ev1, jobs, DT, DT2, moving, kick,
                 fold);
    return hipGetLastError();
}

// ---- measureSpinUps of every member ----
__global__ __launch_bounds__(256) void k_tag_spin_up_ens(const PumpTagArgs* __restrict__ jobs) {
    const PumpTagArgs& a = jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    tag_spin_up_ion(a.psi, i, a.S, a.gid0, a.q, a.qc, a.tags);
}

hipError_t launch_tag_spin_up_ens(const PumpTagArgs* jobs, int njobs, int max_n, hipStream_t s) {
    if (njobs <= 0 || max_n <= 0) return hipSuccess;
    if (!jobs || njobs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tag_spin_up_ens, dim3((max_n + 255) / 256, njobs), dim3(256), 0, s, jobs);
    return hipGetLastError();
}

// ---- the tagged distribution of every member: chunk partials, then each member's chunks in chunk order ----
__global__ __launch_bounds__(256) void k_tagged_kde_ens(const PumpKdeArgs* __restrict__ jobs) {
    __shared__ double sv[3][TKDE_CHUNK];
    __shared__ int st[TKDE_CHUNK];
    const PumpKdeArgs& a = jobs[blockIdx.z];
    if ((int)blockIdx.y * TKDE_CHUNK >= a.N) return;               // past this member's last chunk
    tagged_kde_chunk(a.V, a.tags, a.N, a.S, a.bin0, a.part, blockIdx.x, blockIdx.y, sv, st);
}

__global__ __launch_bounds__(256) void k_tagged_kde_reduce_ens(const PumpKdeArgs* __restrict__ jobs) {
    const PumpKdeArgs& a = jobs[blockIdx.y];
    const int k = blockIdx.x * 256 + threadIdx.x;                  // c * TKDE_BINS + j
    if (k >= 3 * TKDE_BINS) return;
    tagged_kde_reduce_1(a.part, (a.N + TKDE_CHUNK - 1) / TKDE_CHUNK, a.out, k);
}

hipError_t launch_tagged_kde_ens(const PumpKdeArgs* jobs, int njobs, int max_N, hipStream_t s) {
    if (njobs <= 0 || max_N <= 0) return hipSuccess;
    if (!jobs || njobs > 65535) return hipErrorInvalidValue;
    const int nch = (max_N + TKDE_CHUNK - 1) / TKDE_CHUNK;
    hipLaunchKernelGGL(k_tagged_kde_ens, dim3((TKDE_BINS + 255) / 256, nch, njobs), dim3(256), 0, s, jobs);
    hipLaunchKernelGGL(k_tagged_kde_reduce_ens, dim3((3 * TKDE_BINS + 255) / 256, njobs), dim3(256), 0, s, jobs);
    return hipGetLastError();
}

}  // namespace mdqt
