// The batched QT kernels of an ensemble of jobs (mdqt_ensemble_substeps), in a translation unit — hence a
// code object — of their own: mdqt_qtfast.hip's, which holds the single-job kernels, stays byte for byte
// what it is without the ensemble (a larger code object cost the single-job QT launch 0.2 us of 18.5,
// measured).  The kernels wrap lane_substeps (mdqt_qtfast.hpp).  Built with mdqt_qtfast.hip's flags
// (Makefile QTSCHED).
#include "mdqt_ens_args.hpp"
#include "mdqt_qtfast.hpp"

namespace mdqt {

// ------------------------------------------------------------------------------------------
// The same kernels over an ensemble of independent jobs (mdqt_ensemble_substeps): grid (max over jobs of
// their workgroups, jobs); the jobs share the parameters, t and the table, each has its own argument
// block in device memory (its arrays, n, nseg), which lane_substeps indexes in place (a.t[k],
// a.expDet[k]: scalar loads, no copy in registers).  Workgroups past a job's last ion leave at once
// (uniform: before any cross-lane operation).  Same body as the single-job kernels: bit-identical.
// The _w3 set is compiled for three waves per SIMD (168 VGPRs; the production instance then spills 20
// bytes of scratch per lane and its launch is 7 % shorter at 8 jobs of N0 = 3500: Ensemble option
// "qt_waves" 3, A/B in docs/PROGRAMS.md; four waves per SIMD, 128 VGPRs and 176 bytes, was 57 % longer
// and is not built).  The default set keeps the single-job kernels' budget and has no scratch.
#define LANE_ENS_KERNELS(SUFFIX, ATTR, JUNI)                                                                        \
    template <bool DPPX, bool FAST>                                                                                 \
    __global__ __launch_bounds__(256) ATTR void k_substeps_lanes_r_ens##SUFFIX(const SubstepArgs* __restrict__ jobs, \
                                                                               const FastTab* __restrict__ tab) {   \
        const SubstepArgs& a = jobs[blockIdx.y];                                                                    \
        if ((int)blockIdx.x * kLaneIons >= a.n) return;                                                             \
        lane_substeps<DPPX, FAST, false, false, false, false, JUNI>(a, tab, blockIdx.x);                            \
    }                                                                                                               \
    template <bool DPPX, bool EDZ, bool NORN = false>                                                               \
    __global__ __launch_bounds__(256) ATTR void k_substeps_lanes_im_ens##SUFFIX(const SubstepArgs* __restrict__ jobs, \
                                                                                const FastTab* __restrict__ tab) {  \
        const SubstepArgs& a = jobs[blockIdx.y];                                                                    \
        if ((int)blockIdx.x * kLaneIons >= a.n) return;                                                             \
        lane_substeps<DPPX, true, false, true, EDZ, NORN, JUNI>(a, tab, blockIdx.x);                                \
    }
LANE_ENS_KERNELS(, , true)
LANE_ENS_KERNELS(_w3, __attribute__((amdgpu_waves_per_eu(3, 3))), false)   // (lane_substeps: JUNI)
#undef LANE_ENS_KERNELS

// The lane kernels of launch_substeps_r's mode 2, model 0, over an ensemble: `jobs` is the device array of
// the njobs argument blocks, `a` the host copy of one of them — every job has the same nsub, do_step,
// do_qt, movmask, expdet_zero and qc, so the instance chosen for it (lane_qt_instance, mdqt_qtfast.hpp) is
// every job's.  max_n = the largest a.n; wpe = the production instance's register budget (0, 3:
// LANE_ENS_KERNELS; the other instances keep the single-job budget).
hipError_t launch_substeps_r_ens(const SubstepArgs* jobs, const SubstepArgs& a, int njobs, int max_n, const FastTab* tab,
                                 int wpe, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int* instance) {
    if (njobs <= 0 || max_n <= 0 || a.nsub <= 0) return hipSuccess;
    if (!jobs || njobs > 65535 || a.nsub > MAXSUB || a.qc.model != 0 || a.arrive || a.U) return hipErrorInvalidValue;
    if (wpe != 0 && wpe != 3) return hipErrorInvalidValue;
    const dim3 gl((max_n + kLaneIons - 1) / kLaneIons, njobs), bl(kLaneWG);
    const FastTab* lt = tab + 1;                      // by lane
    const QTKernel inst = lane_qt_instance(a);
    switch (inst) {
    case QTK_LANES_IM_EDZ:                            // the production launch: the register budget asked for
        if (wpe == 3) launch_timed(k_substeps_lanes_im_ens_w3<true, true, true>, gl, bl, s, ev0, ev1, jobs, lt);
        else launch_timed(k_substeps_lanes_im_ens<true, true, true>, gl, bl, s, ev0, ev1, jobs, lt);
        break;
    case QTK_LANES_IM_EDZ_RN: launch_timed(k_substeps_lanes_im_ens<true, true>, gl, bl, s, ev0, ev1, jobs, lt); break;
    case QTK_LANES_IM: launch_timed(k_substeps_lanes_im_ens<true, false>, gl, bl, s, ev0, ev1, jobs, lt); break;
    case QTK_LANES_R_FAST: launch_timed(k_substeps_lanes_r_ens<true, true>, gl, bl, s, ev0, ev1, jobs, lt); break;
    case QTK_LANES_R: launch_timed(k_substeps_lanes_r_ens<true, false>, gl, bl, s, ev0, ev1, jobs, lt); break;
    default: return hipErrorInvalidValue;             // (model 0, checked above: none of the pump instances)
    }
    if (instance) *instance = inst;
    return hipGetLastError();
}

}  // namespace mdqt
