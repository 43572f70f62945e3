// The MDQT ensembles' interface between their host sources (mdqt_ensemble.hpp and its sources) and their batched
// kernels (mdqt_ensemble_*.hip, mdqt_pump_ensemble_kernels.hip): the members' argument blocks that only a batched
// launch takes, and the batched launchers.  A member's N3Args, SubstepArgs and tables are mdqt_internal.hpp's.
#pragma once
#include "mdqt_internal.hpp"

namespace mdqt {

// An ensemble of independent jobs in one launch (mdqt_ensemble_*): `jobs` = device array of the jobs'
// argument blocks; grid (largest job's workgroups, njobs).  Forces: max_npairs = the largest a.npairs,
// guard = any job's.  Substeps: `a` = host copy of one job's block (selects the instance, as
// launch_substeps_r mode 2 does: model 0 only), max_n the largest a.n, tab[1] the by-lane table the jobs
// share, wpe the production instance's register budget in waves per SIMD (0 = the single-job kernel's, or 3).
hipError_t launch_forces_n3_ens(const N3Args* jobs, int njobs, int max_npairs, int variant, bool guard, hipStream_t s,
                                hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_substeps_r_ens(const SubstepArgs* jobs, const SubstepArgs& a, int njobs, int max_n, const FastTab* tab,
                                 int wpe, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                                 int* instance = nullptr);
// A sweep ensemble's substeps (mdqt_ensemble_sweep_qt.hip): members with different laser parameters in one
// launch.  `h` = the host copies of all njobs blocks, `tabs` the device array of the points' by-lane tables,
// `point` the device array of the members' point indices.  The instance is launch_substeps_r_ens's choice, made
// only if every block agrees on what it reads (sweep_choice_differs, defined beside the choice itself in
// mdqt_qtfast.hpp); otherwise nothing is launched, *differs = the first member that differs from member 0 and the
// result is hipErrorInvalidValue (*differs = -1 for any other refusal).
hipError_t launch_substeps_r_sweep(const SubstepArgs* jobs, const SubstepArgs* h, int njobs, int max_n, const FastTab* tabs,
                                   const int* point, int wpe, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int* instance,
                                   int* differs);
// An ensemble of optical-pumping jobs in batched launches (mdqt_pump_ensemble_kernels.hip; host:
// mdqt_pump_ensemble.cpp): `jobs` = device array of the members' argument blocks, grid (largest member's
// workgroups, njobs); every kernel runs its single-job kernel's body (mdqt_pump_device.hpp, lane_substeps).
struct PumpStepArgs {   // one member's leapfrog half (step() :377-394)
    double *R, *V, *F;  // [3][S]
    const double* Fpart;// nseg > 1: the pending force partials [nseg][3][S]; F = their canonical sum
    int nseg;           //   (slot_sum16, as k_reduce_segments), written back before it is used
    int n, S;
    double L;
};
struct PumpTagArgs {    // one member's measureSpinUps (k_tag_spin_up's arguments)
    const double* psi;
    int n, S;
    uint64_t gid0, q;
    int* tags;
    QTConst qc;
};
struct PumpKdeArgs {    // one member's tagged distribution (launch_tagged_kde's arguments)
    const double* V;
    const int* tags;
    int N, S, bin0;
    double* part;       // [chunks][3][TKDE_BINS]
    double* out;        // [3][TKDE_BINS]
};
// the pump models' lane QT instance (launch_substeps_r's mode 2, model 1-3) over members: `a` = host copy of
// one member's block (every member has the same nsub, do_step, do_qt, movmask and model)
hipError_t launch_substeps_pump_ens(const SubstepArgs* jobs, const SubstepArgs& a, int njobs, int max_n,
                                    const FastTab* tab, hipStream_t s, hipEvent_t ev0 = nullptr,
                                    hipEvent_t ev1 = nullptr, int* instance = nullptr);
// the leading half drift of step(): k_leapfrog_half (kick 0) of every member, after settling pending forces
hipError_t launch_pump_drift_ens(const PumpStepArgs* jobs, int njobs, int max_n, double DT, double DT2, int moving,
                                 hipStream_t s);
// the second half of step(): F = the canonical slot sum (written back), k_leapfrog_half's kick and half drift,
// and with fold != 0 the next step's leading half drift (t > 0 form) as a second, separately rounded update
hipError_t launch_pump_kick_ens(const PumpStepArgs* jobs, int njobs, int max_n, double DT, double DT2, int moving,
                                double kick, int fold, hipStream_t s, hipEvent_t ev0 = nullptr,
                                hipEvent_t ev1 = nullptr);
hipError_t launch_tag_spin_up_ens(const PumpTagArgs* jobs, int njobs, int max_n, hipStream_t s);
hipError_t launch_tagged_kde_ens(const PumpKdeArgs* jobs, int njobs, int max_N, hipStream_t s);
// output() / Epotential() of an ensemble of SpeedUp jobs in batched launches (mdqt_ensemble_obs.hip; host:
// mdqt_ensemble_output.cpp): `jobs` = device array of the members' argument blocks, grid (largest member's
// workgroups, njobs); every kernel runs its single-job kernel's body (mdqt_pairs.hpp n3_pot_pair and
// reduce_segments_row, mdqt_obs_device.hpp).
constexpr int kObsRow = 64 + 3 * NBINS;   // a member's scratch row, dScr's layout: [0] sum vx, [8] <vx>,
                                          // [16..19] the energy sums, [64..] the KDE bins
struct EnsObsArgs {     // one member's observables
    const double* V;    // [3][S]
    const double* psi;  // [24][S]
    const double* Upart;// [nslots][S] the potential launch's slots (component 0)
    double* Urow;       // [S] their canonical sum per ion
    double* kde;        // [nch][3][NBINS] the KDE partials
    double* scr;        // [kObsRow] the member's row of the ensemble's scratch
    double* pack;       // [4][N] the member's part of the ensemble's column buffer
    int N, S, nslots;
    int nch, chunk;     // KDE chunks clamp(N / 32, 1, kdeChunks) and their length ceil(N / nch)
    int model;          // qt_model (k_output_pack's populations)
};
// k_pairs_n3_pot of every member: max_npairs = the largest a.npairs, guard = any member's
hipError_t launch_potential_n3_ens(const N3Args* jobs, int njobs, int max_npairs, int variant, bool guard, hipStream_t s,
                                   hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// k_reduce_segments (one component, plane S) into Urow, then k_sum_vx + k_energy_sums in one workgroup per
// member: scr[0] = sum vx, scr[8] = <vx>, scr[16..19] the sums
hipError_t launch_potential_sums_ens(const EnsObsArgs* jobs, int njobs, int max_N, hipStream_t s);
// k_kde and k_kde_reduce of every member into scr[64..] (max_nch = the largest nch; reads scr[8])
hipError_t launch_kde_ens(const EnsObsArgs* jobs, int njobs, int max_nch, hipStream_t s, hipEvent_t ev0 = nullptr,
                          hipEvent_t ev1 = nullptr);
hipError_t launch_output_pack_ens(const EnsObsArgs* jobs, int njobs, int max_N, hipStream_t s);
// The pooled output() of an ensemble (mdqt_ensemble_pool.hip; option "pool"): the velocity-resolved populations of
// each parameter point over all ions of its replicas.  kPopSlots slots: 0 .. 1000 have the centres (slot - 500) *
// 0.01 (the KDE's +-5 range), 1001 is "outside"; kPopPlanes planes per slot: the count (a 64-bit integer in the
// double's place), sum S, sum P, sum D.
constexpr int kPopSlots = 1002;
constexpr int kPopPlanes = 4;
static_assert(kPopPlanes * kPopSlots <= 3 * NBINS, "a chunk's slot partials fit its spent KDE partials (EnsObsArgs::kde)");
// k_popv_ens over the npoints x R blocks at `jobs` (point-major; after launch_kde_ens and launch_output_pack_ens:
// it reads pack and overwrites kde), then k_popv_pool into out [npoints][kPopPlanes][kPopSlots]; the launches'
// timestamps to (ev0, ev1) and (ev2, ev3)
hipError_t launch_popv_ens(const EnsObsArgs* jobs, int npoints, int R, int max_nch, double* out, hipStream_t s,
                           hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, hipEvent_t ev2 = nullptr,
                           hipEvent_t ev3 = nullptr);

}  // namespace mdqt
