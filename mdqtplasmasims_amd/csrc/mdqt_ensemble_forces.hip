// The batched force kernel of an ensemble of jobs (mdqt_ensemble_forces), in a translation unit — hence a
// code object — of its own: mdqt_forces.hip's, which holds the single-job kernels, stays byte for byte what
// it is without the ensemble (a larger code object cost the single-job QT launch 0.2 us of 18.5, measured).
// Built with mdqt_forces.hip's flags (Makefile FORCESFLAGS).
#include "mdqt_internal.hpp"
#include "mdqt_pairs.hpp"

namespace mdqt {

// forces() of an ensemble of independent jobs in one launch (mdqt_ensemble_forces): grid (max npairs,
// jobs), x fastest, so consecutive workgroups are one job's tile pairs (its positions and slots stay
// close in time for L2).  Each job's argument block — its own pairs table (split or plain), slots and
// one-slot case — lives in device memory; the body is k_pairs_n3's without arrival counts, so a job's
// F is bit for bit what its own launch gives.  Workgroups past a job's last tile pair leave before
// any LDS use or barrier.
template <int VARIANT, bool GUARD>
__global__ __launch_bounds__(64 * N3W) void k_pairs_n3_ens(const N3Args* __restrict__ jobs) {
    __shared__ double pj[3][128];
    __shared__ double accj[N3W][3][128];
    __shared__ double ia[N3W][3][64];
    __shared__ double mj[128];
    __shared__ double etab[64];
    const N3Args& a = jobs[blockIdx.y];
    if ((int)blockIdx.x >= a.npairs) return;
    stage_exp_tab(etab);
    const int2 IJ = a.pairs[blockIdx.x];
    const PairC c = {a.L, a.micT, a.micGuard, a.Rcut, a.lDeb, a.invlDeb, 1. / a.L, a.rc2, etab};
    const bool rag = (a.N & 63) && IJ.y == a.ntiles - 1;
    if (rag) n3_tile<VARIANT, GUARD, true, false>(a, c, IJ.x, IJ.y, pj, accj, mj, ia);
    else n3_tile<VARIANT, GUARD, false, false>(a, c, IJ.x, IJ.y, pj, accj, mj, ia);
}

hipError_t launch_forces_n3_ens(const N3Args* jobs, int njobs, int max_npairs, int variant, bool guard, hipStream_t s,
                                hipEvent_t ev0, hipEvent_t ev1) {
    if (njobs <= 0 || max_npairs <= 0) return hipSuccess;
    if (!jobs || njobs > 65535 || variant < 0 || variant > 1) return hipErrorInvalidValue;
    const dim3 grid(max_npairs, njobs), blk(64 * N3W);
    if (variant == 1) {
        if (guard) launch_timed(k_pairs_n3_ens<1, true>, grid, blk, s, ev0, ev1, jobs);
        else launch_timed(k_pairs_n3_ens<1, false>, grid, blk, s, ev0, ev1, jobs);
    } else {
        if (guard) launch_timed(k_pairs_n3_ens<0, true>, grid, blk, s, ev0, ev1, jobs);
        else launch_timed(k_pairs_n3_ens<0, false>, grid, blk, s, ev0, ev1, jobs);
    }
    return hipGetLastError();
}

}  // namespace mdqt
