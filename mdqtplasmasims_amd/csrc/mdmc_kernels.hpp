// The Monte-Carlo + MD program's interface between its host engine (mdmc_ctx.hpp and its sources) and its kernels
// (mdmc_kernels.hip, mdmc_ensemble_kernels.hip, mdmc_ensemble_qt_kernels.hip).  What the program shares with MDQT
// (N3Args, the QT tables, launch_tagged_kde and TKDE_BINS) is mdqt_internal.hpp's.
#pragma once
#include "mdqt_internal.hpp"

namespace mdqt {

// ---- Monte-Carlo + MD analytics program (mdmc_kernels.hip) ----
struct MCArgs {
    double* R;          // [3][S]
    double* U;          // [N] per-particle potential energies (MCMD:123)
    double* D;          // [N] scratch: the candidate U'
    uint32_t* mt;       // [625]: std::mt19937 state words + position (in/out)
    unsigned long long* accepted;   // in/out
    int N, S, nsteps;
    double L, kappa, rCut, maxRStep, Gamma;
    double micT;        // smallest d with fl(d / L) >= 0.5: round(d/L) without a division, |d| < 1.25 L
    int fast;           // 1: reciprocal pair energy values (rsq, exp_neg; <= 2 ulp per pair), 0: the reference's ops;
                        //    both keep the reference's pair set: exact image, cutoff as r2 < rc2
    double rc2;         // smallest double x with sqrt(x) >= rCut
};
struct VVArgs {
    double* V;
    double* A;          // in: a(t) ; out: a(t + dt) = the canonical sum of the force slots
    const double* slots;   // [nslots][3][S] Newton-3 tile partials of a(t + dt)
    int nslots;
    const double* R;    // r(t + dt)
    double* Rn;         // out: r(t + 2 dt) = stepPositions of the next MDStep (pre-advanced)
    double L;
    const double* hits;        // [nhits][4] = (i, vx, vy, vz): this step's collisions (host-drawn)
    int nhits;
    int N, S, laser, oneAxis;
    double dt, p6, beta, sqrtn; // p6 = pow(10, -6), sqrtn = sqrt(n) (MCMD:491-496)
};
hipError_t launch_particle_potentials(const double* R, int N, int S, double L, double kappa, double rCut, double* U,
                                      hipStream_t s);
hipError_t launch_monte_carlo(const MCArgs& a, hipStream_t s);
// njobs chains in one launch (grid njobs; N <= 6144): dev_jobs on the device, `one` a member's block on the host;
// ev0 / ev1 (or null) take the launch's own timestamps
hipError_t launch_monte_carlo_ens(const MCArgs* dev_jobs, const MCArgs& one, int njobs, hipStream_t s,
                                  hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_vv_positions(const double* R, const double* V, const double* A, double* Rn, int N, int S, double dt,
                               double L, hipStream_t s);
hipError_t launch_vv_velocities(const VVArgs& a, hipStream_t s);   // + the collision scatter when nhits > 0
hipError_t launch_pair_hist(const double* R, int N, int S, double L, double step, int nbins, unsigned* hist,
                            hipStream_t s);
int autocorr_blocks(int N);
hipError_t launch_autocorr(const double* vs, int N, int T, double c2, double c4, double* part, double* out,
                           hipStream_t s);
hipError_t launch_temperatures(const double* V, int N, int S, double* out, hipStream_t s);
// out[kTagMomentSums]: (sum v, v^2, v^3, v^4, count) of the four tag sets
constexpr int kTagMomentSums = 20;
hipError_t launch_tag_moments(const double* V, const int* tags, int N, double* out, hipStream_t s);
hipError_t launch_anisotropize(double* V, int N, int S, double tpd, hipStream_t s);
hipError_t launch_store_velocities(const double* V, int N, int S, int T, int t, double* vs, hipStream_t s);
// The MD stages of an ensemble of MC + MD jobs in batched launches (mdmc_ensemble_kernels.hip): `jobs` = device
// array of the members' argument blocks, one launch for all njobs.  Forces: variant 2 or 0, never guarded;
// ev0 / ev1 (or null) take the force and velocity-Verlet launches' own timestamps.  The collision scatter is a
// launch of its own, only when a member has a hit (max_nhits > 0).
struct MDObsArgs {      // a member's per-step observables: row k of temp / mom, column t of vs
    const double* V;
    const int* tags;    // [4][N]
    int N, S, T;
    double* temp;       // [steps][4]
    double* mom;        // [steps][kTagMomentSums]
    double* vs;         // [3][N][T]
};
hipError_t launch_forces_n3_mdmc_ens(const N3Args* jobs, int njobs, int max_npairs, int variant, hipStream_t s,
                                     hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_vv_step_ens(const VVArgs* jobs, int njobs, int max_N, hipStream_t s, hipEvent_t ev0 = nullptr,
                              hipEvent_t ev1 = nullptr);
hipError_t launch_collide_ens(const VVArgs* jobs, int njobs, int max_nhits, hipStream_t s);
hipError_t launch_temperatures_ens(const MDObsArgs* jobs, int njobs, int k, hipStream_t s);
hipError_t launch_tag_moments_ens(const MDObsArgs* jobs, int njobs, int k, hipStream_t s);
hipError_t launch_store_velocities_ens(const MDObsArgs* jobs, int njobs, int max_N, int t, hipStream_t s);
// The X row of the tagged distribution of every member of an ensemble of QT tagging jobs
// (mdmc_ensemble_qt_kernels.hip): launch_tagged_kde's component 0, bit for bit, member k's 4,001 values into
// rows[k][TKDE_BINS]; two launches; ev0 / ev1 (or null) take the chunk kernel's own timestamps
struct MDKdeXArgs {
    const double* V;
    const int* tags;    // [N] tag set 0
    int N, S;
    double* part;       // [chunks][1][TKDE_BINS]: the member's own partial buffer
};
hipError_t launch_tagged_kde_x_ens(const MDKdeXArgs* jobs, int njobs, int max_N, double* rows, hipStream_t s,
                                   hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

}  // namespace mdqt
