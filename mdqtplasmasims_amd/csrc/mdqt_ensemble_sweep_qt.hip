// The batched QT kernels of a sweep ensemble (mdqt_ensemble_create_sweep: parameter points x replicas), in a
// translation unit — hence a code object — of their own: mdqt_ensemble_qt.hip's and mdqt_qtfast.hip's stay
// byte for byte what they are without the sweep.  The kernels wrap lane_substeps (mdqt_qtfast.hpp).  Built
// with mdqt_qtfast.hip's flags (Makefile QTSCHED).
#include "mdqt_ens_args.hpp"
#include "mdqt_qtfast.hpp"

namespace mdqt {

// ------------------------------------------------------------------------------------------
// mdqt_ensemble_qt.hip's kernels with the by-lane table per member: grid (max over members of their
// workgroups, members); `tabs` holds one by-lane FastTab per parameter point, point[member] says which is the
// member's.  The index is one scalar load per workgroup and the table's address SGPR arithmetic; each lane then
// reads its own entries from that base, as with the shared table.  The laser's other constants (QTConst, expDet[])
// were per member already: they sit in the member's argument block.  Same body as the single-job kernels on
// the member's own arguments and table: bit-identical to the member run alone.
// The _w3 set: three waves per SIMD for the production instance (Ensemble option "qt_waves" 3), as
// LANE_ENS_KERNELS has it.
#define LANE_SWEEP_KERNELS(SUFFIX, ATTR, JUNI)                                                                         \
    template <bool DPPX, bool FAST>                                                                                    \
    __global__ __launch_bounds__(256) ATTR void k_substeps_lanes_r_sweep##SUFFIX(const SubstepArgs* __restrict__ jobs, \
                                                                                 const FastTab* __restrict__ tabs,     \
                                                                                 const int* __restrict__ point) {      \
        const SubstepArgs& a = jobs[blockIdx.y];                                                                       \
        if ((int)blockIdx.x * kLaneIons >= a.n) return;                                                                \
        lane_substeps<DPPX, FAST, false, false, false, false, JUNI>(a, tabs + point[blockIdx.y], blockIdx.x);          \
    }                                                                                                                  \
    template <bool DPPX, bool EDZ, bool NORN = false>                                                                  \
    __global__ __launch_bounds__(256) ATTR void k_substeps_lanes_im_sweep##SUFFIX(const SubstepArgs* __restrict__ jobs, \
                                                                                  const FastTab* __restrict__ tabs,    \
                                                                                  const int* __restrict__ point) {     \
        const SubstepArgs& a = jobs[blockIdx.y];                                                                       \
        if ((int)blockIdx.x * kLaneIons >= a.n) return;                                                                \
        lane_substeps<DPPX, true, false, true, EDZ, NORN, JUNI>(a, tabs + point[blockIdx.y], blockIdx.x);              \
    }
LANE_SWEEP_KERNELS(, , true)
LANE_SWEEP_KERNELS(_w3, __attribute__((amdgpu_waves_per_eu(3, 3))), false)   // (lane_substeps: JUNI)
#undef LANE_SWEEP_KERNELS

// launch_substeps_r_ens for a sweep ensemble: `h` = the host copies of all njobs blocks.  One instance serves
// the whole launch, so every member's block must agree with member 0's on what the choice reads
// (sweep_choice_differs, beside lane_qt_instance in mdqt_qtfast.hpp); where one does not, nothing is launched,
// *differs = that member's index and the result is hipErrorInvalidValue (*differs = -1 for any other refusal).
hipError_t launch_substeps_r_sweep(const SubstepArgs* jobs, const SubstepArgs* h, int njobs, int max_n, const FastTab* tabs,
                                   const int* point, int wpe, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int* instance,
                                   int* differs) {
    if (differs) *differs = -1;
    if (njobs <= 0 || max_n <= 0) return hipSuccess;
    if (!jobs || !h || !tabs || !point || njobs > 65535) return hipErrorInvalidValue;
    const SubstepArgs& a = h[0];
    if (a.nsub <= 0) return hipSuccess;
    if (a.nsub > MAXSUB || a.qc.model != 0 || a.arrive || a.U) return hipErrorInvalidValue;
    if (wpe != 0 && wpe != 3) return hipErrorInvalidValue;
    for (int k = 1; k < njobs; ++k)
        if (sweep_choice_differs(a, h[k])) {
            if (differs) *differs = k;
            return hipErrorInvalidValue;
        }
    const dim3 gl((max_n + kLaneIons - 1) / kLaneIons, njobs), bl(kLaneWG);
    const QTKernel inst = lane_qt_instance(a);
    switch (inst) {
    case QTK_LANES_IM_EDZ:                            // the production launch: the register budget asked for
        if (wpe == 3) launch_timed(k_substeps_lanes_im_sweep_w3<true, true, true>, gl, bl, s, ev0, ev1, jobs, tabs, point);
        else launch_timed(k_substeps_lanes_im_sweep<true, true, true>, gl, bl, s, ev0, ev1, jobs, tabs, point);
        break;
    case QTK_LANES_IM_EDZ_RN: launch_timed(k_substeps_lanes_im_sweep<true, true>, gl, bl, s, ev0, ev1, jobs, tabs, point); break;
    case QTK_LANES_IM: launch_timed(k_substeps_lanes_im_sweep<true, false>, gl, bl, s, ev0, ev1, jobs, tabs, point); break;
    case QTK_LANES_R_FAST: launch_timed(k_substeps_lanes_r_sweep<true, true>, gl, bl, s, ev0, ev1, jobs, tabs, point); break;
    case QTK_LANES_R: launch_timed(k_substeps_lanes_r_sweep<true, false>, gl, bl, s, ev0, ev1, jobs, tabs, point); break;
    default: return hipErrorInvalidValue;             // (model 0, checked above: none of the pump instances)
    }
    if (instance) *instance = inst;
    return hipGetLastError();
}

}  // namespace mdqt
