// Internal header of the Monte-Carlo + MD host engine: the context behind include/mdmc.h's opaque mdmc_ctx,
// an ensemble of them (struct mdmc_ensemble), and the functions of mdmc_engine.cpp that mdmc_ensemble.cpp
// drives (namespace mdmc).  Not installed: the C ABI sees both structs as opaque.
#pragma once

#include <random>
#include <string>
#include <vector>

#include "../../include/mdmc.h"
#include "mdqt_ctx.hpp"    // HIPCHK, mdqt::set_error, mdqt::take_events
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
    double *dR = nullptr, *dV = nullptr, *dA = nullptr, *dU = nullptr, *dD = nullptr;
    double* dRn = nullptr;          // positions of the next MDStep, pre-advanced by k_vv_step
    bool rnValid = false;           // dRn == stepPositions(dR, dV, dA): cleared by every other writer
    double *dSlots = nullptr, *dVS = nullptr, *dPart = nullptr, *dOut = nullptr;
    double *dTemp = nullptr, *dMom = nullptr;   // per-step observables of the run (4 / 20 per step)
    int capTemp = 0;
    int2* dPairs = nullptr;
    unsigned* dHist = nullptr;
    int* dTags = nullptr;
    uint32_t* dMT = nullptr;
    unsigned long long* dAcc = nullptr;
    double* hHits = nullptr;       // pinned ring of collision entries (i, vx, vy, vz), read by k_collide
    int hitCap = 0, hitOff = 0;
    // pinned landing area of the run's per-step read-backs: [0, 20) moment sums, [20, 24) temperature sums,
    // [24, 24 + 3 TKDE_BINS) tagged distributions (QT only), then the g(r) histogram (unsigned [nbins]);
    // evDrain is recorded behind the copies into it, so the host waits for those and not for the MD step
    // queued after them
    double* hStage = nullptr;
    unsigned* hStageHist = nullptr;
    hipEvent_t evDrain = nullptr;
    std::string saveDir;
    // QT tagging variants (qt_model 1..3)
    int qt = 0;
    double dtQ = 0., gamToE = 0., pv2q = 0., decayRatio = 0.;
    int qtRatio = 0, pumpSteps = 0;
    mdqt::QTConst qc;
    mdqt::FastTab ftab;
    mdqt::FastTab* dFTab = nullptr;   // [2]: by state, by lane (the same for the pumping models)
    double* dPsi = nullptr;        // [24][S] component-major (re0, im0, re1, ...), as include/mdqt.h's engine
    double* dTp = nullptr;         // [S] tPart
    int* dFlags = nullptr;
    double *dKdePart = nullptr, *dKde = nullptr;
    uint64_t qidx = 0;
    unsigned short x48[3] = {0x330E, 0xABCD, 0x1234};   // drand48's default state (no srand48 in QTT)
};

// J contexts (job + k, seed + k) annealed by one launch (mdmc_ensemble.cpp).  Every member keeps its own
// stream for everything else; the ensemble's stream carries the batched anneal and its argument blocks.
struct mdmc_ensemble {
    std::vector<mdmc_ctx*> jobs;
    int dev = 0;
    hipStream_t stream = nullptr;
    mdqt::MCArgs* dArgs = nullptr;     // [J] the blocks the next launch reads
    mdqt::MCArgs* hArgs = nullptr;     // pinned [2][J]: the blocks of a full chunk, of a call's last chunk
    uint32_t* hMT = nullptr;           // pinned [J][625]: the chains' mt19937 states coming back
    unsigned long long* hAcc = nullptr;   // pinned [J]
    bool timing = false;
    std::vector<hipEvent_t> evpool;    // the anneal launches' own timestamps (pairs)
    int evused = 0;
    // wall time of the last run's stages (ms, with timing on): anneal, pre-record MD, QT pump, recorded MD,
    // autocorrelations, the rest
    static constexpr int kStages = 6;
    double stage_ms[kStages] = {};
};

namespace mdmc {

constexpr int kAnnealChunk = 10000;    // Metropolis steps per launch (bounded launches)
constexpr int kBatchedMaxN = 6144;     // positions in LDS: k_monte_carlo_lds<6>

// mdmc_engine.cpp
void mc_args(const mdmc_ctx* c, mdqt::MCArgs& a);   // the anneal's argument block (nsteps left to the caller)
int md_step_async(mdmc_ctx* c);                     // one MDStep() queued on the member's stream
int qsteps_async(mdmc_ctx* c, int n);
// main() of the program for J contexts in lockstep: J = 1 without an ensemble is mdmc_run
int run_members(mdmc_ctx* const* cs, int J, mdmc_ensemble* ens, int verbose);

// mdmc_ensemble.cpp: nsteps Metropolis steps of every member, chunked launches on the ensemble's stream
int ensemble_anneal(mdmc_ensemble* e, int nsteps, long long* accepted);

}  // namespace mdmc
