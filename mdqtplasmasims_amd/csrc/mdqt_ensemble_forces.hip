// The batched force kernel of an ensemble of jobs (mdqt_ensemble_forces), in a translation unit — hence a
// code object — of its own: mdqt_forces.hip's, which holds the single-job kernels, stays byte for byte what
// it is without the ensemble (a larger code object cost the single-job QT launch 0.2 us of 18.5, measured).
// Built with mdqt_forces.hip's flags (Makefile FORCESFLAGS).  The kernel template is mdqt_pairs_ens.hpp's;
// this unit holds the SpeedUp ensemble's instances (variants 0 and 1).
#include "mdqt_ens_args.hpp"
#include "mdqt_pairs_ens.hpp"

namespace mdqt {

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
