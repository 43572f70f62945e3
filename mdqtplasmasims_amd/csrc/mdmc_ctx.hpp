// Internal header of the Monte-Carlo + MD host engine: the context behind include/mdmc.h's opaque mdmc_ctx,
// an ensemble of them (struct mdmc_ensemble), and what crosses between mdmc_engine.cpp (the context), mdmc_run.cpp
// (main() by stage) and mdmc_ensemble.cpp (namespace mdmc).  Not installed: the C ABI sees both structs as opaque.
#pragma once

#include <random>
#include <string>
#include <vector>

#include "../../include/mdmc.h"
#include "mdmc_kernels.hpp"
#include "mdqt_batch.hpp"    // PinRing, LaunchTimer
#include "mdqt_devbuf.hpp"
#include "mdqt_error.hpp"    // HIPCHK, mdqt::set_error
#include "mdqt_internal.hpp" // QTConst, FastTab, N3Args, SubstepArgs: shared with MDQT
#include "mdqt_mt32.hpp"   // Mt32: the reference's std::mt19937 with the state in plain view

struct mdmc_ctx {
    mdmc_params p;
    int N = 0, S = 0, nbins = 0, T = 0, nt = 0, npairs = 0;
    double L = 0., rCut = 0.;
    double collisionFreq = 0.;
    int addLaserForce = 0;
    // the reference's RNG (MCMD:52-55, :87)
    mdqt::Mt32 rng;
    std::uniform_real_distribution<double> uni{0., 1.};
    std::normal_distribution<double> vd;
    int dev = 0;
    hipStream_t st = nullptr;
    mdqt::DevBuf<double> dR, dV, dA, dU, dD;
    mdqt::DevBuf<double> dRn;       // positions of the next MDStep, pre-advanced by k_vv_step
    bool rnValid = false;           // dRn == stepPositions(dR, dV, dA): cleared by every other writer
    mdqt::DevBuf<double> dSlots, dVS, dPart, dOut;
    mdqt::DevBuf<double> dTemp, dMom;   // per-step observables of the run (4 / 20 per step)
    int temp_rows() const { return (int)(dTemp.capacity() / 4); }   // steps they hold
    mdqt::DevBuf<int2> dPairs;
    mdqt::DevBuf<unsigned> dHist;
    mdqt::DevBuf<int> dTags;
    mdqt::DevBuf<uint32_t> dMT;
    mdqt::DevBuf<unsigned long long> dAcc;
    mdqt::PinBuf<double> hHits;    // pinned ring of collision entries (i, vx, vy, vz), read by k_collide
    int hitCap = 0, hitOff = 0;
    // pinned landing area of the run's per-step read-backs: [0, 20) moment sums, [20, 24) temperature sums,
    // [24, 24 + 3 TKDE_BINS) tagged distributions (QT only), then the g(r) histogram (unsigned [nbins]);
    // evDrain is recorded behind the copies into it, so the host waits for those and not for the MD step
    // queued after them
    mdqt::PinBuf<unsigned> hStageMem;
    double* hStage = nullptr;          // views of hStageMem: the doubles,
    unsigned* hStageHist = nullptr;    // the histogram behind them
    hipEvent_t evDrain = nullptr;
    std::string saveDir;
    // QT tagging variants (qt_model 1..3)
    int qt = 0;
    double dtQ = 0., gamToE = 0., pv2q = 0., decayRatio = 0.;
    int qtRatio = 0, pumpSteps = 0;
    mdqt::QTConst qc;
    mdqt::FastTab ftab;
    mdqt::DevBuf<mdqt::FastTab> dFTab;   // [2]: by state, by lane (the same for the pumping models)
    mdqt::DevBuf<double> dPsi;     // [24][S] component-major (re0, im0, re1, ...), as include/mdqt.h's engine
    mdqt::DevBuf<double> dTp;      // [S] tPart
    mdqt::DevBuf<int> dFlags;
    mdqt::DevBuf<double> dKdePart, dKde;
    uint64_t qidx = 0;
    unsigned short x48[3] = {0x330E, 0xABCD, 0x1234};   // drand48's default state (no srand48 in QTT)
};

// J contexts (job + k, seed + k) annealed by one launch (mdmc_ensemble.cpp).  Every member keeps its own
// stream for everything that is its own; the ensemble's stream carries the batched anneal, the batched MD
// steps and per-step observables (md_batch 1), and their argument blocks.
struct mdmc_ensemble {
    std::vector<mdmc_ctx*> jobs;
    int dev = 0;
    hipStream_t stream = nullptr;
    mdqt::DevBuf<mdqt::MCArgs> dArgs;  // [J] the blocks the next launch reads
    mdqt::PinBuf<mdqt::MCArgs> hArgs;  // pinned [2][J]: the blocks of a full chunk, of a call's last chunk
    mdqt::PinBuf<uint32_t> hMT;        // pinned [J][625]: the chains' mt19937 states coming back
    mdqt::PinBuf<unsigned long long> hAcc;   // pinned [J]
    bool timing = false;
    mdqt::LaunchTimer annealTimer;     // the anneal launches' own timestamps
    // wall time of the last run's stages (ms, with timing on): anneal, pre-record MD, QT pump, recorded MD,
    // autocorrelations, the rest
    static constexpr int kStages = 6;
    double stage_ms[kStages] = {};
    // ---- batched MD (mdmc_ensemble.cpp, "batched MD stretches") ----
    int mdBatch = 0;                   // mdmc_ensemble_set_md_batch: 0 member by member, 1 batched
    unsigned long long mdLaunches = 0; // kernel launches the batched path has issued
    // device blocks of a stretch, one allocation: N3Args [2][J], VVArgs [2][J] (the two buffer parities of
    // the collisionless step), MDObsArgs [J], MDKdeXArgs [J], then VVArgs [J] of a step with collision draws
    mdqt::DevBuf<char> dBlocks;
    mdqt::N3Args* dN3 = nullptr;       // views of dBlocks, these five
    mdqt::VVArgs* dVV = nullptr;
    mdqt::MDObsArgs* dObs = nullptr;
    mdqt::MDKdeXArgs* dKdeX = nullptr;
    mdqt::VVArgs* dVVc = nullptr;
    size_t hdrBytes = 0;               // of the first four
    mdqt::PinRing hdrRing, vvRing;     // a stretch's blocks (4 slots); a collisional step's VVArgs [J] (64 slots)
    bool open = false;                 // inside a stretch: the members' streams are fenced behind `stream`
    int parity = 0;                    // which of the two block sets the next step takes
    int obsCap = 0;                    // rows of the members' dTemp / dMom at the stretch's start
    std::vector<char> coll;            // [J] the member draws collisions in this stretch
    std::vector<unsigned long long> skip;   // [J] mt19937 words of collisionless steps still to discard
    std::vector<hipEvent_t> evMember;  // [J] fences: a member's stream -> `stream`
    hipEvent_t evEns = nullptr;        // `stream` -> the members' streams
    mdqt::LaunchTimer forceTimer, vvTimer;   // the batched force / velocity-Verlet launches' timestamps
    // ---- batched QT (mdmc_ensemble.cpp, "batched QT"; members with qt_model 1..3 only) ----
    static constexpr int kDistSlots = 4;   // recorded steps whose X distributions may be on their way at once
    unsigned long long qtLaunches = 0; // kernel launches the batched QT, tagging and distribution paths have issued
    mdqt::DevBuf<char> dQt;            // [J] SubstepArgs of a QT chunk, or PumpTagArgs of the tagging: the next launch's
    mdqt::PinRing qtRing;              // their way over, in stream order
    mdqt::DevBuf<double> dDist;        // [kDistSlots][J][TKDE_BINS]: the reduce's rows
    mdqt::PinBuf<double> hDist;        // pinned, the same shape: one copy per slot brings all members' rows
    mdqt::PinBuf<double> hMom;         // pinned [J][kTagMomentSums]: mdmc_ensemble_tagged_moments_qt's sums
    hipEvent_t evDist[kDistSlots] = {};   // behind the copy into a slot of hDist
    mdqt::LaunchTimer qtTimer, distTimer;   // the batched QT launches'; the distribution's chunk kernel's
};

namespace mdmc {

constexpr int kAnnealChunk = 10000;    // Metropolis steps per launch (bounded launches)
constexpr int kBatchedMaxN = 6144;     // positions in LDS: k_monte_carlo_lds<6>

// mdmc_engine.cpp
void mc_args(const mdmc_ctx* c, mdqt::MCArgs& a);   // the anneal's argument block (nsteps left to the caller)
int md_step_async(mdmc_ctx* c);                     // one MDStep() queued on the member's stream
// the pieces of md_step_async, shared with the batched step: the force and velocity-Verlet argument blocks
// of the member's current buffers, and the step's collision rolls and Maxwellians from the member's rng into
// its pinned ring (`drain`: the stream whose queued launches read the ring)
void n3_args(const mdmc_ctx* c, mdqt::N3Args& a);
void vv_args(const mdmc_ctx* c, const double* hits, int nhits, mdqt::VVArgs& v);
int collision_draws(mdmc_ctx* c, hipStream_t drain, double** hits, int* nhits);
int pair_corr_queue(mdmc_ctx* c);                   // g(r) of the member queued on its stream, evDrain behind the copy
int qsteps_async(mdmc_ctx* c, int n);
// a launch of m <= MAXSUB QT substeps of the member from its qstep index: qsteps_async's block, shared with the
// batched launch (the caller advances qidx)
void substep_args(const mdmc_ctx* c, int m, mdqt::SubstepArgs& a);
// the sums of k_tag_moments' tag set 0 -> recordTaggedParticleMoments' four moments (QTT:1106-1109)
void moments_qt_from_sums(const double* m, double* out4);
FILE* open_in(const mdmc_ctx* c, const char* name, const char* mode);   // fopen in the member's save directory
void pair_corr_finish(const mdmc_ctx* c, std::vector<double>& g);       // g(r) from the landed histogram (:627-635)
int autocorr_queue(mdmc_ctx* c, double* out);                           // the four autocorrelations [4][T] and their copy, queued
void temps_from_sums(const mdmc_ctx* c, const double* s, double* out4);      // k_temperatures' sums -> T, Tx, Ty, Tz
void moments_from_sums(const mdmc_ctx* c, const double* m, double* out16);   // k_tag_moments' sums -> the four tag sets' moments
int tagged_moments_qt_queue(mdmc_ctx* c, double* sums_dev, bool dist);       // tag set 0's sums (+ the three-component KDE), queued
// mdmc_run.cpp: main() of the program for J contexts in lockstep: J = 1 without an ensemble is mdmc_run
int run_members(mdmc_ctx* const* cs, int J, mdmc_ensemble* ens, int verbose);

// mdmc_ensemble.cpp: nsteps Metropolis steps of every member, chunked launches on the ensemble's stream
int ensemble_anneal(mdmc_ensemble* e, int nsteps, long long* accepted);
// batched MD stretches (md_batch 1): begin fences `stream` behind every member's stream and uploads the
// members' blocks; a step is one force and one velocity-Verlet launch for all members (+ one collision
// scatter when a member has a hit); the observables of step k are one launch per kind; end fences the
// members' streams behind `stream` and settles the members' rng
int ensemble_md_begin(mdmc_ensemble* e);
int ensemble_md_step(mdmc_ensemble* e);
int ensemble_md_end(mdmc_ensemble* e);
int ensemble_md_temperatures(mdmc_ensemble* e, int k);
int ensemble_tag_moments(mdmc_ensemble* e, int k, bool qt);   // row k of dMom; charges qt_launches() (qt) or md_launches()
int ensemble_md_store_velocities(mdmc_ensemble* e, int t);
int ensemble_md_pair_corr_queue(mdmc_ensemble* e);   // every member's g(r) on its own stream, fenced both ways
// batched QT (md_batch 1), queued on the ensemble's stream inside a stretch: n qsteps of every member in
// ceil(n / MAXSUB) launches; the spin-up tagging in one; the X distribution into slot `slot` of the distribution
// ring and its copy to the pinned ring
int ensemble_qt_steps(mdmc_ensemble* e, int n);
int ensemble_qt_tag(mdmc_ensemble* e);
int ensemble_qt_dist_x(mdmc_ensemble* e, int slot);
// waits for slot's copy: [J][TKDE_BINS], valid until the slot is queued again (NULL: error)
const double* ensemble_qt_dist_rows(mdmc_ensemble* e, int slot);

// What a stage queues a step on: one member on its own stream (c), or the whole ensemble in batched launches
// (e, md_batch 1).  Exactly one of the two is set; every method is the member's call or its batched twin.
struct MdLane {
    mdmc_ctx* c;
    mdmc_ensemble* e;
    int begin() const { return e ? ensemble_md_begin(e) : 0; }
    int end() const { return e ? ensemble_md_end(e) : 0; }
    int md_step() const { return e ? ensemble_md_step(e) : md_step_async(c); }
    int temperatures(int k) const {
        if (e) return ensemble_md_temperatures(e, k);
        HIPCHK(mdqt::launch_temperatures(c->dV, c->N, c->S, c->dTemp + (size_t)4 * k, c->st));
        return 0;
    }
    int tag_moments(int k) const {
        if (e) return ensemble_tag_moments(e, k, false);
        HIPCHK(mdqt::launch_tag_moments(c->dV, c->dTags, c->N, c->dMom + (size_t)20 * k, c->st));
        return 0;
    }
    int store_velocities(int k) const { return e ? ensemble_md_store_velocities(e, k) : mdmc_record_velocities(c, k); }
    int pair_corr_queue() const { return e ? ensemble_md_pair_corr_queue(e) : mdmc::pair_corr_queue(c); }
    int qt_steps(int n) const { return e ? ensemble_qt_steps(e, n) : qsteps_async(c, n); }
    int qt_tag() const { return e ? ensemble_qt_tag(e) : mdmc_tag_qt(c, nullptr, nullptr); }
};
// a run's lanes: one ensemble lane under md_batch 1, else J member lanes in job order (mdmc_run: J = 1, no ensemble)
inline std::vector<MdLane> md_lanes(mdmc_ctx* const* cs, int J, mdmc_ensemble* ens) {
    if (ens && ens->mdBatch == 1) return {MdLane{nullptr, ens}};
    std::vector<MdLane> l;
    for (int j = 0; j < J; ++j) l.push_back(MdLane{cs[j], nullptr});
    return l;
}

}  // namespace mdmc
