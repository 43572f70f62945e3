// The batched MD-stage kernels of an ensemble of Monte-Carlo + MD jobs (mdmc_ensemble.cpp, md_batch 1): one
// launch steps or reduces every member.  Each kernel runs the single-job kernel's body (mdmc_device.hpp,
// mdqt_pairs.hpp n3_tile) on jobs[blockIdx.<job axis>], the member's own argument block in device memory —
// one body, two callers, which is why a member's bits are those of its own launches.  A translation unit,
// hence a code object, of its own: mdmc_kernels.hip's and mdqt_ensemble_forces.hip's stay what they are
// without it.  Built with mdqt_forces.hip's flags (Makefile FORCESFLAGS), as every caller of n3_tile is.
//
// The blocks are copied into registers at entry — wave-uniform loads of memory the launch never writes,
// ahead of every loop — so the loop constants sit in scalar registers as a by-value argument's do.
#include "mdmc_device.hpp"
#include "mdqt_pairs_ens.hpp"

namespace mdqt {

// grid (ceil(max N / 64), 3, J), 512 threads: k_vv_step on jobs[blockIdx.z].  A workgroup past its member's
// last tile sums nothing and leaves after the barrier, as the ragged lanes of a single launch do.
__global__ __launch_bounds__(512) void k_vv_step_ens(const VVArgs* __restrict__ jobs) {
    __shared__ double acc[8][64];
    const VVArgs a = jobs[blockIdx.z];
    vv_step_body(a, blockIdx.x, blockIdx.y, acc);
}

// grid (ceil(max nhits / 64), J), 64 threads: k_collide on jobs[blockIdx.y]; h >= a.nhits leaves (a member
// without a hit this step: every workgroup of its row)
__global__ __launch_bounds__(64) void k_collide_ens(const VVArgs* __restrict__ jobs) {
    const VVArgs a = jobs[blockIdx.y];
    collide_body(a, blockIdx.x);
}

// one workgroup per member; k = the step of the stage: the member's sums go to its row k
__global__ __launch_bounds__(RBT) void k_temperatures_ens(const MDObsArgs* __restrict__ jobs, int k) {
    __shared__ double sp[4][RBT / 64];
    const MDObsArgs a = jobs[blockIdx.x];
    temperatures_body(a.V, a.N, a.S, a.temp + (size_t)4 * k, sp);
}

__global__ __launch_bounds__(RBT) void k_tag_moments_ens(const MDObsArgs* __restrict__ jobs, int k) {
    __shared__ double sp[kTagMomentSums][RBT / 64];
    const MDObsArgs a = jobs[blockIdx.x];
    tag_moments_body(a.V, a.tags, a.N, a.mom + (size_t)kTagMomentSums * k, sp);
}

// grid (ceil(max N / 256), J)
__global__ __launch_bounds__(256) void k_store_velocities_ens(const MDObsArgs* __restrict__ jobs, int t) {
    const MDObsArgs a = jobs[blockIdx.y];
    store_velocities_body(a.V, a.N, a.S, a.T, t, a.vs, blockIdx.x);
}

// calculateAccelerations of every member: variant 2 (force_kernel 1) or 0, never guarded (mdmc_engine.cpp
// n3_args)
hipError_t launch_forces_n3_mdmc_ens(const N3Args* jobs, int njobs, int max_npairs, int variant, hipStream_t s,
                                     hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0 || max_npairs <= 0) return hipSuccess;
    if (!jobs || njobs > 65535 || (variant != 0 && variant != 2)) return hipErrorInvalidValue;
    const dim3 grid(max_npairs, njobs), blk(64 * N3W);
    if (variant == 2) launch_timed(k_pairs_n3_ens<2, false>, grid, blk, s, ev0, ev1, jobs);
    else launch_timed(k_pairs_n3_ens<0, false>, grid, blk, s, ev0, ev1, jobs);
    return hipGetLastError();
}

hipError_t launch_vv_step_ens(const VVArgs* jobs, int njobs, int max_N, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0 || max_N <= 0) return hipSuccess;
    if (!jobs || njobs > 65535) return hipErrorInvalidValue;
    launch_timed(k_vv_step_ens, dim3((max_N + 63) / 64, 3, njobs), dim3(512), s, ev0, ev1, jobs);
    return hipGetLastError();
}

hipError_t launch_collide_ens(const VVArgs* jobs, int njobs, int max_nhits, hipStream_t s) {
    if (njobs <= 0 || max_nhits <= 0) return hipSuccess;
    if (!jobs || njobs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_collide_ens, dim3((max_nhits + 63) / 64, njobs), dim3(64), 0, s, jobs);
    return hipGetLastError();
}

hipError_t launch_temperatures_ens(const MDObsArgs* jobs, int njobs, int k, hipStream_t s) {
    if (njobs <= 0) return hipSuccess;
    if (!jobs || k < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_temperatures_ens, dim3(njobs), dim3(RBT), 0, s, jobs, k);
    return hipGetLastError();
}

hipError_t launch_tag_moments_ens(const MDObsArgs* jobs, int njobs, int k, hipStream_t s) {
    if (njobs <= 0) return hipSuccess;
    if (!jobs || k < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tag_moments_ens, dim3(njobs), dim3(RBT), 0, s, jobs, k);
    return hipGetLastError();
}

hipError_t launch_store_velocities_ens(const MDObsArgs* jobs, int njobs, int max_N, int t, hipStream_t s) {
    if (njobs <= 0 || max_N <= 0) return hipSuccess;
    if (!jobs || njobs > 65535 || t < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_store_velocities_ens, dim3((max_N + 255) / 256, njobs), dim3(256), 0, s, jobs, t);
    return hipGetLastError();
}

}  // namespace mdqt
