// The X distribution of the tagged ions of every member of an ensemble of QT tagging jobs (mdmc_ensemble.cpp,
// "batched QT"): recordTaggedParticleMoments writes the X row only (QTT:1128-1136), so a recorded step of the
// ensemble evaluates that row alone, for all members, in two launches.  The kernels run k_tagged_kde's and
// k_tagged_kde_reduce's bodies (mdqt_pump_device.hpp) with one component instead of three: the same ascending
// order within a chunk, the same wave-ballot skip — decided per component, so component 0's decisions are the
// three-component kernel's — and the same chunk-order reduce; the 4,001 values are the bits of row 0 of
// launch_tagged_kde.  The partials are [chunks][1][TKDE_BINS], in the member's own partial buffer.  A code
// object of its own, built with mdmc_kernels.hip's flags (the Makefile's defaults), as the single-job
// instance of the body is.
//
// The argument blocks are per member, in device memory, and are copied to registers at entry; a workgroup
// past its member's last chunk returns before any barrier or LDS use (a condition on blockIdx and the block).
#include "mdmc_kernels.hpp"
#include "mdqt_pump_device.hpp"

namespace mdqt {

// grid (ceil(TKDE_BINS / 256), ceil(max N / TKDE_CHUNK), J)
__global__ __launch_bounds__(256) void k_tagged_kde_x_ens(const MDKdeXArgs* __restrict__ jobs) {
    __shared__ double sv[1][TKDE_CHUNK];
    __shared__ int st[TKDE_CHUNK];
    const MDKdeXArgs a = jobs[blockIdx.z];
    if ((int)blockIdx.y * TKDE_CHUNK >= a.N) return;               // past this member's last chunk
    tagged_kde_chunk<1>(a.V, a.tags, a.N, a.S, -2000, a.part, blockIdx.x, blockIdx.y, sv, st);
}

// grid (ceil(TKDE_BINS / 256), J): member k's chunks in chunk order into rows[k][TKDE_BINS]
__global__ __launch_bounds__(256) void k_tagged_kde_x_reduce_ens(const MDKdeXArgs* __restrict__ jobs,
                                                                 double* __restrict__ rows) {
    const MDKdeXArgs a = jobs[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= TKDE_BINS) return;
    tagged_kde_reduce_1<1>(a.part, (a.N + TKDE_CHUNK - 1) / TKDE_CHUNK, rows + (size_t)blockIdx.y * TKDE_BINS, j);
}

// rows: [njobs][TKDE_BINS]; ev0 / ev1 (or null) take the chunk kernel's own timestamps (the reduce is 16 J
// workgroups of at most six adds a thread)
hipError_t launch_tagged_kde_x_ens(const MDKdeXArgs* jobs, int njobs, int max_N, double* rows, hipStream_t s,
                                   hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0 || max_N <= 0) return hipSuccess;
    if (!jobs || !rows || njobs > 65535) return hipErrorInvalidValue;
    const int nch = (max_N + TKDE_CHUNK - 1) / TKDE_CHUNK;
    launch_timed(k_tagged_kde_x_ens, dim3((TKDE_BINS + 255) / 256, nch, njobs), dim3(256), s, ev0, ev1, jobs);
    hipLaunchKernelGGL(k_tagged_kde_x_reduce_ens, dim3((TKDE_BINS + 255) / 256, njobs), dim3(256), 0, s, jobs, rows);
    return hipGetLastError();
}

}  // namespace mdqt
