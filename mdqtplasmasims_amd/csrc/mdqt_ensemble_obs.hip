// The batched output() / Epotential() kernels of an ensemble of SpeedUp jobs (mdqt_ensemble_output,
// mdqt_ensemble_observables, mdqt_ensemble_epotential; host: mdqt_ensemble_output.cpp), in a translation unit
// — hence a code object — of their own, so that the single-job kernels' code objects stay what they are.
// Every kernel takes a device array of per-member argument blocks indexed by a grid axis and runs its
// single-job kernel's body on the member's own arguments: n3_pot_pair and reduce_segments_row of
// mdqt_pairs.hpp (k_pairs_n3_pot, k_reduce_segments), the bodies of mdqt_obs_device.hpp (k_sum_vx,
// k_energy_sums, k_kde, k_kde_reduce, k_output_pack) — bit-identical to the member on its own.  The block is
// read into registers at entry (it is uniform over the workgroup: scalar loads); a workgroup past its
// member's last tile pair, ion, chunk or bin leaves at once — a condition on blockIdx and the block, uniform
// over the workgroup (the per-thread ion and bin tests of the kernels without barriers aside), before any
// barrier, LDS use or cross-lane operation.  The blocks' pointers come from memory, so the accesses are flat.
// Built with mdqt_forces.hip's flags (Makefile FORCESFLAGS: the pair kernel's), and, as everything here,
// -ffp-contract=off; the flag only keeps the vectorizer from packing operations and changes no value.
#include "mdqt_ens_args.hpp"
#include "mdqt_obs_device.hpp"
#include "mdqt_pairs.hpp"

namespace mdqt {

// ---- Epotential(): k_pairs_n3_pot over members, grid (largest npairs, J), x fastest (a member's tile
// pairs are consecutive workgroups) ----
template <int VARIANT, bool GUARD>
__global__ __launch_bounds__(64 * N3W) void k_pairs_n3_pot_ens(const N3Args* __restrict__ jobs) {
    __shared__ double pj[3][128];
    __shared__ double accj[N3W][3][128];
    __shared__ double ia[N3W][3][64];
    __shared__ double mj[128];
    const N3Args a = jobs[blockIdx.y];
    if ((int)blockIdx.x >= a.npairs) return;
    n3_pot_pair<VARIANT, GUARD>(a, blockIdx.x, pj, accj, mj, ia);
}

hipError_t launch_potential_n3_ens(const N3Args* jobs, int njobs, int max_npairs, int variant, bool guard, hipStream_t s,
                                   hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0 || max_npairs <= 0) return hipSuccess;
    if (!jobs || njobs > 65535 || variant < 0 || variant > 1) return hipErrorInvalidValue;
    const dim3 grid(max_npairs, njobs), blk(64 * N3W);
    by_variant_guard<2>(variant, guard, [&](auto V, auto G) {
        launch_timed(k_pairs_n3_pot_ens<decltype(V)::value, decltype(G)::value>, grid, blk, s, ev0, ev1, jobs);
    });
    return hipGetLastError();
}

// ---- the potential slots' canonical sum per ion: k_reduce_segments (component 0, plane S), grid
// (ceil(largest N / 256), J) ----
__global__ __launch_bounds__(256) void k_reduce_segments_ens(const EnsObsArgs* __restrict__ jobs) {
    const EnsObsArgs a = jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    reduce_segments_row(a.Upart, a.Urow, a.nslots, a.S, (size_t)a.S, i, 0);
}

// ---- k_sum_vx, then k_energy_sums with its <vx>, one 1,024-thread workgroup per member: the same strided
// sums and block_sums in the same order, avg the same IEEE division (every thread holds r) ----
__global__ __launch_bounds__(RT) void k_energy_sums_ens(const EnsObsArgs* __restrict__ jobs) {
    __shared__ double sh[RT];
    const EnsObsArgs a = jobs[blockIdx.x];
    const double r = sum_vx_body(a.V, a.N, sh);
    const double avg = a.N > 0 ? r / (double)a.N : 0.;
    if (threadIdx.x == 0) { a.scr[0] = r; a.scr[8] = avg; }
    energy_sums_body(a.V, a.N, a.S, avg, a.Urow, a.scr + 16, sh);
}

hipError_t launch_potential_sums_ens(const EnsObsArgs* jobs, int njobs, int max_N, hipStream_t s) {
    if (njobs <= 0 || max_N <= 0) return hipSuccess;
    if (!jobs || njobs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_reduce_segments_ens, dim3((max_N + 255) / 256, njobs), dim3(256), 0, s, jobs);
    hipLaunchKernelGGL(k_energy_sums_ens, dim3(njobs), dim3(RT), 0, s, jobs);
    return hipGetLastError();
}

// ---- k_kde over members: grid (bin blocks x 3 components, largest nch, J) — the component folded into x
// (kKdeBlocks is a power of two: a shift and a mask) ----
constexpr int kKdeBlocks = (NBINS + KT - 1) / KT;
static_assert((kKdeBlocks & (kKdeBlocks - 1)) == 0, "component and bin block from blockIdx.x by shift and mask");

__global__ __launch_bounds__(KT) void k_kde_ens(const EnsObsArgs* __restrict__ jobs) {
    __shared__ double sv[KT];
    const EnsObsArgs a = jobs[blockIdx.z];
    const int z = blockIdx.y;
    if (z >= a.nch) return;
    const int c = blockIdx.x / kKdeBlocks, jb = blockIdx.x % kKdeBlocks;
    kde_chunk(a.V, a.N, a.S, (c == 0) ? a.scr[8] : 0., a.kde, a.chunk, jb, c, z, sv);
}

__global__ __launch_bounds__(256) void k_kde_reduce_ens(const EnsObsArgs* __restrict__ jobs) {
    const EnsObsArgs a = jobs[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= 3 * NBINS) return;
    kde_reduce_bin(a.kde, a.nch, a.scr + 64, j);
}

hipError_t launch_kde_ens(const EnsObsArgs* jobs, int njobs, int max_nch, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0 || max_nch <= 0) return hipSuccess;
    if (!jobs || njobs > 65535 || max_nch > 65535) return hipErrorInvalidValue;
    launch_timed(k_kde_ens, dim3(3 * kKdeBlocks, max_nch, njobs), dim3(KT), s, ev0, ev1, jobs);
    hipLaunchKernelGGL(k_kde_reduce_ens, dim3((3 * NBINS + 255) / 256, njobs), dim3(256), 0, s, jobs);
    return hipGetLastError();
}

// ---- k_output_pack over members, grid (ceil(largest N / 256), J) ----
__global__ __launch_bounds__(256) void k_output_pack_ens(const EnsObsArgs* __restrict__ jobs) {
    const EnsObsArgs a = jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    output_pack_ion(a.V, a.psi, i, a.N, a.S, a.model, a.pack);
}

hipError_t launch_output_pack_ens(const EnsObsArgs* jobs, int njobs, int max_N, hipStream_t s) {
    if (njobs <= 0 || max_N <= 0) return hipSuccess;
    if (!jobs || njobs > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_output_pack_ens, dim3((max_N + 255) / 256, njobs), dim3(256), 0, s, jobs);
    return hipGetLastError();
}

}  // namespace mdqt
