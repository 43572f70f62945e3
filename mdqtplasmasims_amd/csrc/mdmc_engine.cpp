// Host engine of the Monte-Carlo + MD analytics program: the C ABI of
// include/mdmc.h.  Owns the device-resident state (R, V, A, U, stored velocities), keeps the
// reference's std::mt19937 stream (its Metropolis part runs inside the device MC kernel, the
// state handed over both ways), drives the gfx950 kernels of mdmc_kernels.hip and the
// Newton-3 force kernel; main()'s stages and files are mdmc_run.cpp.  Every function cites the
// lines of MonteCarloFollowedByMDAndTempAnisotropy.cpp ("MCMD") it stands in for.
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "mdmc_ctx.hpp"   // struct mdmc_ctx; HIPCHK, mdqt::set_error, Mt32

using namespace mdqt;

namespace {

double sqrt_threshold(double rc) {   // smallest x with sqrt(x) >= rc: sqrt(r2) < rc iff r2 < x
    double x = rc * rc;
    while (x > 0 && sqrt(x) >= rc) x = nextafter(x, 0.);
    while (sqrt(x) < rc) x = nextafter(x, INFINITY);
    return x;
}

double mic_threshold(double L) {   // smallest d with fl(d / L) >= 0.5 (Newton-3 kernel, exact variant)
    double d = 0.5 * L;
    while (d > 0 && d / L >= 0.5) d = nextafter(d, 0.);
    while (d / L < 0.5) d = nextafter(d, INFINITY);
    return d;
}

// the rng state to / from the device MC kernel (the same [624 words, position] layout)
int rng_to_device(mdmc_ctx* c) {
    HIPCHK(hipMemcpyAsync(c->dMT, c->rng.x, sizeof c->rng.x, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}
int rng_from_device(mdmc_ctx* c) {
    HIPCHK(hipMemcpyAsync(c->rng.x, c->dMT, sizeof c->rng.x, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (c->rng.x[624] > 624) return set_error("device MC kernel returned a bad mt19937 position");
    return 0;
}

// calculateAccelerations (:387-448): the Newton-3 tile kernel (lDeb = 1/kappa); its slots are
// summed into A by k_vv_step
int accelerations(mdmc_ctx* c) {
    N3Args a;
    mdmc::n3_args(c, a);
    // force_kernel 1: variant 2 (fast values, the reference's exact pair set), 0: exact
    HIPCHK(launch_forces_n3(a, c->p.force_kernel == 1 ? 2 : 0, c->st));
    return 0;
}

int mkdir_p(const char* d) {
    if (mkdir(d, 0777) != 0 && errno != EEXIST) return set_error("mkdir %s: %s", d, strerror(errno));
    return 0;
}

}  // namespace

FILE* mdmc::open_in(const mdmc_ctx* c, const char* name, const char* mode) {
    std::string f = c->saveDir + name;
    return fopen(f.c_str(), mode);
}

extern "C" void mdmc_default_params(mdmc_params* p) {                 // MCMD:62-107
    memset(p, 0, sizeof *p);
    p->N = 4096; p->kappa = 0.5; p->Gamma = 3; p->n = 0.4; p->collisionFreq = 0.25;
    p->monteCarloSteps = 200000; p->maxRStep = 0.3; p->pairPairStep = 0.05; p->timeStep = 0.005;
    p->numPreRecordMDSteps = 200; p->numVelAutoCorrsSteps = 2500; p->numInstantaneousAnisotropySteps = 2500;
    p->numReestablishEquilSteps = 500; p->tempPercentDiff = 0.15; p->applyForceAlongOneAxisOnly = 0;
    p->beta = 26000; p->anisotropyEstablishmentTime = 10; p->anisotropyFromForcesRelaxSteps = 2000;
    p->seed = 12345; p->job = 1; p->device = -1; p->force_kernel = 1;
    p->qt_model = 0; p->tpumpreal = 0.0000002; p->detuning = -2.5; p->Om = 0.7;   // QTT 408 linear :85-87
    strcpy(p->saveDirectory, "data/");
}

extern "C" int mdmc_default_params_qt(mdmc_params* p, int model) {   // QTT:75-121
    if (!p) return set_error("mdmc_default_params_qt: NULL argument");
    if (model < 1 || model > 3) return set_error("mdmc_default_params_qt: model must be 1, 2 or 3");
    mdmc_default_params(p);
    p->n = 2;                                       // :82
    p->monteCarloSteps = 100000;                    // :98
    p->numVelAutoCorrsSteps = 1500;                 // :109
    p->qt_model = model;
    static const double tp[4] = {0, 0.0000002, 0.0000001, 0.00000005};   // 408Linear :85, 408Quad :114, 422 :85
    static const double det[4] = {0, -2.5, 0, -1}, om[4] = {0, 0.7, 2, 1.3};
    static const char* dir[4] = {"", "data408/", "dataSpinTagQuad/", "data422/"};
    p->tpumpreal = tp[model]; p->detuning = det[model]; p->Om = om[model];
    strcpy(p->saveDirectory, dir[model]);
    return 0;
}

extern "C" void mdmc_destroy(mdmc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->dev);
    if (c->st) (void)hipStreamSynchronize(c->st);
    if (c->evDrain) (void)hipEventDestroy(c->evDrain);
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
}

extern "C" int mdmc_create(const mdmc_params* p, mdmc_ctx** out) {
    if (!p || !out) return set_error("mdmc_create: NULL argument");
    *out = nullptr;
    if (p->N < 2) return set_error("N must be >= 2");
    if (p->numVelAutoCorrsSteps < 1 || p->numVelAutoCorrsSteps > 4096)
        return set_error("numVelAutoCorrsSteps must be in [1, 4096]");
    if (p->kappa <= 0 || p->Gamma <= 0 || p->timeStep <= 0 || p->pairPairStep <= 0)
        return set_error("kappa, Gamma, timeStep and pairPairStep must be positive");
    if (p->force_kernel != 0 && p->force_kernel != 1) return set_error("force_kernel must be 0 or 1");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) return set_error("no HIP device available (%s)", hipGetErrorString(e));
    std::unique_ptr<mdmc_ctx, void (*)(mdmc_ctx*)> guard(new mdmc_ctx(), mdmc_destroy);
    mdmc_ctx* c = guard.get();
    c->p = *p;
    c->p.saveDirectory[sizeof(c->p.saveDirectory) - 1] = 0;
    if (p->device >= 0) {
        if (p->device >= ndev) return set_error("device %d >= device count %d", p->device, ndev);
        c->dev = p->device;
    } else {
        (void)hipGetDevice(&c->dev);
    }
    if (hipSetDevice(c->dev) != hipSuccess || hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess)
        return set_error("cannot create a HIP stream on device %d", p->device);
    const int N = p->N;
    c->N = N;
    c->S = ((N + 63) / 64) * 64;
    c->T = p->numVelAutoCorrsSteps;
    c->L = pow(N * 4. * M_PI / 3., 1. / 3);                         // :73
    c->rCut = c->L / 2.;                                            // :74
    c->nbins = (int)((c->L / 2) / p->pairPairStep);                 // :83, :616
    c->collisionFreq = p->collisionFreq;
    c->rng.seed(p->seed);                                           // :53 (seed instead of random_device)
    (void)c->uni(c->rng);                                           // :55 auto random_double = uni(rng)
    c->vd = std::normal_distribution<double>(0, sqrt(1 / p->Gamma));   // :87
    c->nt = (N + 63) / 64;
    c->npairs = c->nt * (c->nt + 1) / 2;
    const size_t S = c->S, sz = S * sizeof(double);
    const int nblk = autocorr_blocks(N);
    bool ok = c->dR.alloc(3 * S) == hipSuccess && c->dV.alloc(3 * S) == hipSuccess &&
              c->dA.alloc(3 * S) == hipSuccess && c->dRn.alloc(3 * S) == hipSuccess &&
              c->dU.alloc(S) == hipSuccess && c->dD.alloc(S) == hipSuccess &&
              c->dSlots.alloc(3 * S * c->nt) == hipSuccess &&
              c->dVS.alloc((size_t)3 * N * c->T) == hipSuccess &&
              c->dPart.alloc((size_t)nblk * 4 * c->T) == hipSuccess &&
              // dOut: the autocorrelations [4][T], the temperature sums and k_tag_moments' sums
              c->dOut.alloc((size_t)std::max(4 * c->T, kTagMomentSums)) == hipSuccess &&
              c->dPairs.alloc((size_t)c->npairs) == hipSuccess &&
              c->dHist.alloc((size_t)(c->nbins > 0 ? c->nbins : 1)) == hipSuccess &&
              c->dTags.alloc((size_t)4 * N) == hipSuccess &&
              c->dMT.alloc(625) == hipSuccess &&
              c->dAcc.alloc(1) == hipSuccess;
    if (!ok) return set_error("mdmc_create: device allocation failed");
    // the reference's globals start at zero (R, V, A, U; MCMD:110-123)
    ok = hipMemsetAsync(c->dR, 0, 3 * sz, c->st) == hipSuccess && hipMemsetAsync(c->dV, 0, 3 * sz, c->st) == hipSuccess &&
         hipMemsetAsync(c->dA, 0, 3 * sz, c->st) == hipSuccess && hipMemsetAsync(c->dU, 0, sz, c->st) == hipSuccess &&
         hipMemsetAsync(c->dVS, 0, (size_t)3 * N * c->T * sizeof(double), c->st) == hipSuccess &&
         hipMemsetAsync(c->dTags, 0, (size_t)4 * N * sizeof(int), c->st) == hipSuccess;
    std::vector<int2> h;
    h.reserve(c->npairs);
    for (int I = 0; I < c->nt; ++I)
        for (int J = I; J < c->nt; ++J) h.push_back(make_int2(I, J));
    ok = ok && hipMemcpyAsync(c->dPairs, h.data(), h.size() * sizeof(int2), hipMemcpyHostToDevice, c->st) == hipSuccess &&
         hipStreamSynchronize(c->st) == hipSuccess;
    if (!ok) return set_error("mdmc_create: device initialisation failed");
    c->hitCap = 4 * 65536;
    if (c->hHits.alloc((size_t)c->hitCap * 4) != hipSuccess)
        return set_error("mdmc_create: pinned allocation failed");
    const size_t stageD = 24 + (p->qt_model != 0 ? (size_t)3 * TKDE_BINS : 0);
    if (c->hStageMem.alloc(2 * stageD + (size_t)(c->nbins > 0 ? c->nbins : 1)) != hipSuccess ||
        hipEventCreateWithFlags(&c->evDrain, hipEventDisableTiming) != hipSuccess)
        return set_error("mdmc_create: pinned allocation failed");
    c->hStage = reinterpret_cast<double*>(c->hStageMem.get());
    c->hStageHist = c->hStageMem + 2 * stageD;
    c->saveDir = c->p.saveDirectory;
    if (p->qt_model != 0) {
        // the QT tagging program's constants: 408 (QTT408Linear:115-121) / 422 (QTT422Linear:115-121)
        const int m = p->qt_model;
        if (m < 1 || m > 3) return set_error("mdmc_create: qt_model must be 0 .. 3");
        const double nn = p->n;
        c->qt = m;
        c->gamToE = m == 3 ? 174.07 * .894 / sqrt(nn) : 174.07 / sqrt(nn);
        c->qtRatio = m == 3 ? (int)round(87 * .894 / sqrt(nn)) : (int)round(87 / sqrt(nn));
        c->dtQ = p->timeStep / c->qtRatio;
        c->pv2q = m == 3 ? 1.1821 * pow(nn, 1. / 6) * .967 : 1.1821 * pow(nn, 1. / 6);
        c->decayRatio = m == 3 ? 0.0753 : 0.0617;
        const double tpump = p->tpumpreal * 813490 * sqrt(nn);
        c->pumpSteps = (int)round(tpump / p->timeStep);
        if (c->qtRatio < 1) return set_error("mdmc_create: QT substep ratio < 1");
        build_pump_program(m, p->detuning, p->Om, c->dtQ, c->gamToE, c->pv2q, c->decayRatio, p->seed, p->job, c->qc,
                           c->ftab);
        const int nch = (N + 255) / 256;
        ok = c->dFTab.alloc(2) == hipSuccess && c->dPsi.alloc((size_t)24 * S) == hipSuccess &&
             c->dTp.alloc(S) == hipSuccess && c->dFlags.alloc(1) == hipSuccess &&
             c->dKdePart.alloc((size_t)nch * 3 * TKDE_BINS) == hipSuccess &&
             c->dKde.alloc((size_t)3 * TKDE_BINS) == hipSuccess;
        if (!ok) return set_error("mdmc_create: QT allocation failed");
        ok = hipMemcpyAsync(c->dFTab, &c->ftab, sizeof(FastTab), hipMemcpyHostToDevice, c->st) == hipSuccess &&
             hipMemcpyAsync(c->dFTab + 1, &c->ftab, sizeof(FastTab), hipMemcpyHostToDevice, c->st) == hipSuccess &&
             hipMemsetAsync(c->dPsi, 0, (size_t)24 * S * sizeof(double), c->st) == hipSuccess &&
             hipMemsetAsync(c->dTp, 0, (size_t)S * sizeof(double), c->st) == hipSuccess &&
             hipMemsetAsync(c->dFlags, 0, sizeof(int), c->st) == hipSuccess &&
             hipStreamSynchronize(c->st) == hipSuccess;
        if (!ok) return set_error("mdmc_create: QT initialisation failed");
    }
    *out = guard.release();
    return 0;
}

extern "C" double mdmc_get_const(const mdmc_ctx* c, const char* n) {
    if (!c || !n) return NAN;
    if (!strcmp(n, "N")) return c->N;
    if (!strcmp(n, "L")) return c->L;
    if (!strcmp(n, "rCut")) return c->rCut;
    if (!strcmp(n, "nbins")) return c->nbins;
    if (!strcmp(n, "collisionFreq")) return c->collisionFreq;
    if (c->qt) {
        if (!strcmp(n, "plasmaToQuantumTimestepRatio")) return c->qtRatio;
        if (!strcmp(n, "quantumTimestep")) return c->dtQ;
        if (!strcmp(n, "gamToEinsteinFreq")) return c->gamToE;
        if (!strcmp(n, "plasVelToQuantVel")) return c->pv2q;
        if (!strcmp(n, "decayRatio")) return c->decayRatio;
        if (!strcmp(n, "pumpMDTimeSteps")) return c->pumpSteps;
    }
    return NAN;
}

// init() :173-203 (cubic lattice + Maxwell-Boltzmann velocities from the reference's rng),
// then calculatePotentialEnergyForParticles() :207-245
extern "C" int mdmc_init(mdmc_ctx* c) {
    if (!c) return set_error("NULL context");
    c->rnValid = false;
    const int N = c->N, S = c->S;
    const double L = c->L;
    std::vector<double> R((size_t)3 * S, 0.), V((size_t)3 * S, 0.);
    std::vector<double> psi(c->qt ? (size_t)24 * S : 0, 0.);
    int N0 = 0;
    for (int i = 0; i < round(pow(N, 1. / 3)); i++)
        for (int j = 0; j < round(pow(N, 1. / 3)); j++)
            for (int k = 0; k < round(pow(N, 1. / 3)); k++) {
                if (N0 >= N) return set_error("mdmc_init: N = %d is not a perfect cube (lattice init :182-201)", N);
                R[N0] = i * L / pow(N, 1 / 3.) + 0.5;               // :189-191
                R[S + N0] = j * L / pow(N, 1 / 3.) + 0.5;
                R[2 * S + N0] = k * L / pow(N, 1 / 3.) + 0.5;
                V[N0] = c->vd(c->rng);                              // :193-195
                V[S + N0] = c->vd(c->rng);
                V[2 * S + N0] = c->vd(c->rng);
                if (c->qt) {                                         // QTT:224-239: random S superposition
                    const double rand1 = erand48(c->x48), rand2 = erand48(c->x48);
                    const double rand3 = erand48(c->x48);
                    const double sign = rand3 < 0.5 ? -1 : 1;
                    const double rand4 = erand48(c->x48);
                    const double sign2 = rand4 < 0.5 ? -1 : 1;
                    psi[(size_t)0 * S + N0] = sqrt(rand1);                                    // re, state 0
                    psi[(size_t)2 * S + N0] = sign2 * sqrt(1 - rand1) * sqrt(rand2);          // re, state 1
                    psi[(size_t)3 * S + N0] = sign * sqrt(1 - rand1) * sqrt(1 - rand2);       // im, state 1
                }
                N0++;
            }
    if (N0 != N) return set_error("mdmc_init: N = %d is not a perfect cube (lattice init :182-201)", N);
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemcpyAsync(c->dR, R.data(), R.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->dV, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemsetAsync(c->dA, 0, (size_t)3 * S * sizeof(double), c->st));
    HIPCHK(launch_particle_potentials(c->dR, N, S, L, c->p.kappa, c->rCut, c->dU, c->st));
    if (c->qt) {
        HIPCHK(hipMemcpyAsync(c->dPsi, psi.data(), psi.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemsetAsync(c->dTp, 0, (size_t)S * sizeof(double), c->st));
        c->qidx = 0;
    }
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

void mdmc::mc_args(const mdmc_ctx* c, MCArgs& a) {
    memset(&a, 0, sizeof a);
    a.R = c->dR; a.U = c->dU; a.D = c->dD; a.mt = c->dMT; a.accepted = c->dAcc;
    a.N = c->N; a.S = c->S;
    a.L = c->L; a.kappa = c->p.kappa; a.rCut = c->rCut; a.maxRStep = c->p.maxRStep; a.Gamma = c->p.Gamma;
    a.micT = mic_threshold(c->L);
    a.fast = c->p.force_kernel == 1;
    a.rc2 = sqrt_threshold(c->rCut);
}

// MonteCarloStep() x nsteps (:315-382) on the device with the reference's mt19937 stream
extern "C" int mdmc_monte_carlo(mdmc_ctx* c, int nsteps, long long* accepted) {
    if (!c) return set_error("NULL context");
    c->rnValid = false;
    if (nsteps < 0) return set_error("nsteps < 0");
    HIPCHK(hipSetDevice(c->dev));
    if (rng_to_device(c)) return -1;
    HIPCHK(hipMemsetAsync(c->dAcc, 0, sizeof(unsigned long long), c->st));
    MCArgs a;
    mdmc::mc_args(c, a);
    for (int done = 0; done < nsteps;) {                      // bounded launches
        a.nsteps = std::min(mdmc::kAnnealChunk, nsteps - done);
        HIPCHK(launch_monte_carlo(a, c->st));
        done += a.nsteps;
    }
    unsigned long long acc = 0;
    HIPCHK(hipMemcpyAsync(&acc, c->dAcc, sizeof acc, hipMemcpyDeviceToHost, c->st));
    if (rng_from_device(c)) return -1;
    if (accepted) *accepted = (long long)acc;
    return 0;
}

// One MDStep() (:504-511) queued on the stream: stepPositions, calculateAccelerations,
// stepVelocities.  The collision rolls and Maxwellian draws of the step are state-independent,
// so the host makes them (the reference's rng, its order :474-482) while the device runs.
int mdmc::md_step_async(mdmc_ctx* c) {
    const int N = c->N;
    const double dt = c->p.timeStep;
    if (!c->rnValid)                                                                          // :452-467
        HIPCHK(launch_vv_positions(c->dR, c->dV, c->dA, c->dRn, N, c->S, dt, c->L, c->st));
    std::swap(c->dR, c->dRn);
    if (accelerations(c)) return -1;                                                          // :508
    int nh = 0;
    double* hits = nullptr;
    if (dt * c->collisionFreq <= 0) {
        // every roll misses (uni >= 0): each is one generate_canonical, i.e. two mt19937 words
        c->rng.discard(2ull * N);
    } else if (collision_draws(c, c->st, &hits, &nh)) {
        return -1;
    }
    VVArgs v;
    vv_args(c, hits, nh, v);
    HIPCHK(launch_vv_velocities(v, c->st));                                                   // :469-502
    c->rnValid = true;
    return 0;
}

// calculateAccelerations' argument block on the member's current positions (:387-448; lDeb = 1/kappa)
void mdmc::n3_args(const mdmc_ctx* c, N3Args& a) {
    memset(&a, 0, sizeof a);
    a.R = c->dR; a.P = c->dSlots; a.pairs = c->dPairs;
    a.N = c->N; a.S = c->S; a.ntiles = c->nt; a.npairs = c->npairs;
    a.L = c->L; a.lDeb = 1. / c->p.kappa; a.Rcut = c->rCut; a.invlDeb = c->p.kappa;
    a.micT = mic_threshold(c->L); a.micGuard = 1.25 * c->L; a.guard = 0;
    a.rc2 = sqrt_threshold(c->rCut);
}

// stepVelocities' argument block (:469-502) on the member's current buffers, laser force and collision list
void mdmc::vv_args(const mdmc_ctx* c, const double* hits, int nhits, VVArgs& v) {
    memset(&v, 0, sizeof v);
    v.V = c->dV; v.A = c->dA; v.slots = c->dSlots; v.nslots = c->nt; v.R = c->dR; v.Rn = c->dRn; v.L = c->L;
    v.hits = hits; v.nhits = nhits; v.N = c->N; v.S = c->S;
    v.laser = c->addLaserForce; v.oneAxis = c->p.applyForceAlongOneAxisOnly;
    v.dt = c->p.timeStep; v.p6 = pow(10, -6); v.beta = c->p.beta; v.sqrtn = sqrt(c->p.n);
}

// the collision rolls and Maxwellians of one step (:474-482, the reference's order) into the member's pinned
// ring; `drain` is the stream whose queued launches read the ring
int mdmc::collision_draws(mdmc_ctx* c, hipStream_t drain, double** hits_out, int* nhits) {
    const int N = c->N;
    const double dt = c->p.timeStep;
    if (c->hitOff + N > c->hitCap) {           // ring wrap: the queued readers must be done
        HIPCHK(hipStreamSynchronize(drain));
        c->hitOff = 0;
    }
    double* hits = c->hHits + (size_t)4 * c->hitOff;
    int nh = 0;
    for (int i = 0; i < N; i++) {
        const double collRoll = c->uni(c->rng);
        if (collRoll < dt * c->collisionFreq) {
            double* e = hits + 4 * (size_t)nh++;
            e[0] = i;
            e[1] = c->vd(c->rng);
            e[2] = c->vd(c->rng);
            e[3] = c->vd(c->rng);
        }
    }
    c->hitOff += nh;
    *hits_out = hits;
    *nhits = nh;
    return 0;
}

extern "C" int mdmc_md_steps(mdmc_ctx* c, int nsteps) {
    if (!c) return set_error("NULL context");
    HIPCHK(hipSetDevice(c->dev));
    for (int k = 0; k < nsteps; ++k)
        if (mdmc::md_step_async(c)) return -1;
    HIPCHK(hipStreamSynchronize(c->st));
    c->hitOff = 0;
    return 0;
}

extern "C" int mdmc_set_collision_freq(mdmc_ctx* c, double f) {
    if (!c) return set_error("NULL context");
    c->collisionFreq = f;
    return 0;
}
extern "C" int mdmc_set_laser_force(mdmc_ctx* c, int on) {
    if (!c) return set_error("NULL context");
    c->addLaserForce = on ? 1 : 0;
    return 0;
}

// recordPairPairCorr (:584-635): the histogram on the device (queued, read back into the pinned landing
// area, evDrain behind the copy), the normalisation here once the copy has landed
int mdmc::pair_corr_queue(mdmc_ctx* c) {
    const int nb = c->nbins;
    if (nb > 0) {
        HIPCHK(hipMemsetAsync(c->dHist, 0, nb * sizeof(unsigned), c->st));
        HIPCHK(launch_pair_hist(c->dR, c->N, c->S, c->L, c->p.pairPairStep, nb, c->dHist, c->st));
        HIPCHK(hipMemcpyAsync(c->hStageHist, c->dHist, nb * sizeof(unsigned), hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(hipEventRecord(c->evDrain, c->st));
    return 0;
}
void mdmc::pair_corr_finish(const mdmc_ctx* c, std::vector<double>& g) {
    const int nb = c->nbins;
    g.assign(nb > 0 ? nb : 0, 0.);
    const unsigned* h = c->hStageHist;
    const int N = c->N;
    const double ps = c->p.pairPairStep;
    for (int i = 0; i < nb; i++) {                               // :627-635
        if (i == 0) g[i] = (double)h[i] / (N * 4 / 3 * M_PI * ps * ps * ps);
        else g[i] = (double)h[i] / (N * 3 * ps * ps * ps * i * i);
    }
}

extern "C" int mdmc_pair_corr(mdmc_ctx* c, double* g, int cap, int* nbins) {
    if (!c) return set_error("NULL context");
    HIPCHK(hipSetDevice(c->dev));
    if (mdmc::pair_corr_queue(c)) return -1;
    HIPCHK(hipEventSynchronize(c->evDrain));
    std::vector<double> v;
    mdmc::pair_corr_finish(c, v);
    if (nbins) *nbins = (int)v.size();
    if (g) {
        if (cap < (int)v.size()) return set_error("mdmc_pair_corr: buffer holds %d < %d bins", cap, (int)v.size());
        memcpy(g, v.data(), v.size() * sizeof(double));
    }
    return 0;
}

extern "C" int mdmc_record_velocities(mdmc_ctx* c, int k) {      // :513-523
    if (!c) return set_error("NULL context");
    if (k < 0 || k >= c->T) return set_error("mdmc_record_velocities: step %d outside [0, %d)", k, c->T);
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(launch_store_velocities(c->dV, c->N, c->S, c->T, k, c->dVS, c->st));
    return 0;
}

extern "C" int mdmc_set_velocity_store(mdmc_ctx* c, const double* vs) {
    if (!c || !vs) return set_error("mdmc_set_velocity_store: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemcpyAsync(c->dVS, vs, (size_t)3 * c->N * c->T * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// recordVAF, recordLongViscAutoCorr, recordVCubeAutoCorr, recordVFourthAutoCorr (:655-807)
int mdmc::autocorr_queue(mdmc_ctx* c, double* out) {
    const double G = c->p.Gamma;
    const double c2 = 3 / (G * G), c4 = 3 * 9 / (G * G * G * G);   // :710, :785
    HIPCHK(launch_autocorr(c->dVS, c->N, c->T, c2, c4, c->dPart, c->dOut, c->st));
    HIPCHK(hipMemcpyAsync(out, c->dOut, (size_t)4 * c->T * sizeof(double), hipMemcpyDeviceToHost, c->st));
    return 0;
}
extern "C" int mdmc_autocorrelations(mdmc_ctx* c, double* out) {
    if (!c || !out) return set_error("mdmc_autocorrelations: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    if (mdmc::autocorr_queue(c, out)) return -1;
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

void mdmc::temps_from_sums(const mdmc_ctx* c, const double* s, double* out4) {
    out4[0] = s[0] / (c->N * 3);                                 // recordTemperature :535-543
    out4[1] = s[1] / c->N;                                       // recordTempForEachAxis :567-576
    out4[2] = s[2] / c->N;
    out4[3] = s[3] / c->N;
}

extern "C" int mdmc_temperatures(mdmc_ctx* c, double out4[4]) {
    if (!c || !out4) return set_error("mdmc_temperatures: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    double s[4];
    HIPCHK(launch_temperatures(c->dV, c->N, c->S, c->dOut, c->st));
    HIPCHK(hipMemcpyAsync(s, c->dOut, sizeof s, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    mdmc::temps_from_sums(c, s, out4);
    return 0;
}

extern "C" int mdmc_anisotropize(mdmc_ctx* c) {                  // :548-558
    if (!c) return set_error("NULL context");
    c->rnValid = false;
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(launch_anisotropize(c->dV, c->N, c->S, c->p.tempPercentDiff, c->st));
    return 0;
}

// tagParticles (:810-921): needs vx only, consumes the reference's rng on the host
extern "C" int mdmc_tag_particles(mdmc_ctx* c, int* tags4) {
    if (!c) return set_error("NULL context");
    HIPCHK(hipSetDevice(c->dev));
    const int N = c->N;
    std::vector<double> vx(N);
    std::vector<int> t((size_t)4 * N);
    HIPCHK(hipMemcpyAsync(vx.data(), c->dV, N * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    const double Gamma = c->p.Gamma;
    const double vT = sqrt(1 / Gamma);                           // :814
    double roll;
    for (int i = 0; i < N; i++) {
        const double currVx = vx[i];
        int one, two, three, four;
        if (currVx < -3 * vT) one = 0;                           // :819-838
        else if (currVx > 3 * vT) one = 1;
        else { roll = c->uni(c->rng); one = roll < (.5 + currVx / vT / 6); }
        const double c2 = .5 / 9 / vT / vT;                      // :840-864
        roll = c->uni(c->rng);
        if (currVx < -3 * vT || currVx > 3 * vT) two = !(roll < .5);
        else two = roll < (c2 * currVx * currVx);
        const double c3 = .5 / 27 / vT / vT / vT;                // :868-888
        if (currVx < -3 * vT) three = 0;
        else if (currVx > 3 * vT) three = 1;
        else { roll = c->uni(c->rng); three = roll < (.5 + c3 * currVx * currVx * currVx); }
        const double c4 = .5 / 81 / vT / vT / vT / vT;           // :892-916
        roll = c->uni(c->rng);
        if (currVx < -3 * vT || currVx > 3 * vT) four = !(roll < .5);
        else four = roll < (c4 * currVx * currVx * currVx * currVx);
        t[i] = one; t[(size_t)N + i] = two; t[(size_t)2 * N + i] = three; t[(size_t)3 * N + i] = four;
    }
    HIPCHK(hipMemcpyAsync(c->dTags, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (tags4) memcpy(tags4, t.data(), t.size() * sizeof(int));
    return 0;
}

void mdmc::moments_from_sums(const mdmc_ctx* c, const double* m, double* out16) {   // :972-998
    const double G = c->p.Gamma;
    for (int t = 0; t < 4; ++t) {
        const unsigned num = (unsigned)m[5 * t + 4];
        out16[4 * t] = m[5 * t] / num;
        out16[4 * t + 1] = m[5 * t + 1] / num;
        out16[4 * t + 1] -= 1 / (G);
        out16[4 * t + 2] = m[5 * t + 2] / num;
        out16[4 * t + 3] = m[5 * t + 3] / num;
        out16[4 * t + 3] -= 3 / (G * G);
    }
}

extern "C" int mdmc_tagged_moments(mdmc_ctx* c, double out16[16]) {
    if (!c || !out16) return set_error("mdmc_tagged_moments: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    double m[kTagMomentSums];
    HIPCHK(launch_tag_moments(c->dV, c->dTags, c->N, c->dOut, c->st));
    HIPCHK(hipMemcpyAsync(m, c->dOut, sizeof m, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    mdmc::moments_from_sums(c, m, out16);
    return 0;
}

extern "C" int mdmc_get_state(mdmc_ctx* c, double* R, double* V, double* A, double* U) {
    if (!c) return set_error("NULL context");
    HIPCHK(hipSetDevice(c->dev));
    const int N = c->N, S = c->S;
    double* src[3] = {c->dR, c->dV, c->dA};
    double* dst[3] = {R, V, A};
    for (int q = 0; q < 3; ++q) {
        if (!dst[q]) continue;
        for (int k = 0; k < 3; ++k)
            HIPCHK(hipMemcpyAsync(dst[q] + (size_t)k * N, src[q] + (size_t)k * S, N * sizeof(double),
                                  hipMemcpyDeviceToHost, c->st));
    }
    if (U) HIPCHK(hipMemcpyAsync(U, c->dU, N * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

extern "C" int mdmc_set_state(mdmc_ctx* c, const double* R, const double* V, const double* A, const double* U) {
    if (!c) return set_error("NULL context");
    c->rnValid = false;
    HIPCHK(hipSetDevice(c->dev));
    const int N = c->N, S = c->S;
    if (R)   // the kernels' division-free minimum image needs |dx| < 1.25 L: the box of :262-271, :459-464
        for (size_t k = 0; k < (size_t)3 * N; ++k)
            if (!(R[k] >= 0 && R[k] <= c->L)) return set_error("mdmc_set_state: position %zu = %g outside [0, L]", k, R[k]);
    double* dst[3] = {c->dR, c->dV, c->dA};
    const double* src[3] = {R, V, A};
    for (int q = 0; q < 3; ++q) {
        if (!src[q]) continue;
        for (int k = 0; k < 3; ++k)
            HIPCHK(hipMemcpyAsync(dst[q] + (size_t)k * S, src[q] + (size_t)k * N, N * sizeof(double),
                                  hipMemcpyHostToDevice, c->st));
    }
    if (U) HIPCHK(hipMemcpyAsync(c->dU, U, N * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// ---- QT tagging variants ----
static int need_qt(const mdmc_ctx* c, const char* what) {
    if (!c) return set_error("NULL context");
    if (!c->qt) return set_error("%s: the context has no QT (qt_model 0)", what);
    return 0;
}

// qstep() x n (QTT:555-756): the pumping model's fused QT substeps on this system's velocities
// (no drift: the MD steps move the ions), in launches of up to MAXSUB substeps
void mdmc::substep_args(const mdmc_ctx* c, int m, SubstepArgs& a) {
    memset(&a, 0, sizeof a);
    a.R = c->dR; a.V = c->dV; a.F = c->dA; a.Fpart = nullptr; a.nseg = 1;
    a.psi = c->dPsi; a.tPart = c->dTp; a.oor = c->dFlags;
    a.n = c->N; a.S = c->S; a.gid0 = 0; a.q0 = c->qidx;
    a.nsub = m; a.do_step = 0; a.do_qt = 1; a.U = nullptr;
    a.L = c->L;
    a.qc = c->qc;
}

int mdmc::qsteps_async(mdmc_ctx* c, int n) {
    while (n > 0) {
        const int m = n < MAXSUB ? n : MAXSUB;
        SubstepArgs a;
        substep_args(c, m, a);
        HIPCHK(launch_substeps_r(a, c->dFTab, 0, c->st));
        c->qidx += (uint64_t)m;
        n -= m;
    }
    return 0;
}

extern "C" int mdmc_qsteps(mdmc_ctx* c, int n) {
    if (need_qt(c, "mdmc_qsteps")) return -1;
    HIPCHK(hipSetDevice(c->dev));
    if (mdmc::qsteps_async(c, n)) return -1;
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// tagParticles (QTT:1022-1067 / 422:992-1034): the spin-up measurement of include/mdqt.h's
// k_tag_spin_up (Philox draws 6, 7 of the current qstep index); the tags drive the moments
extern "C" int mdmc_tag_qt(mdmc_ctx* c, int* tags, int* n_up) {
    if (need_qt(c, "mdmc_tag_qt")) return -1;
    HIPCHK(hipSetDevice(c->dev));
    const int N = c->N;
    HIPCHK(launch_tag_spin_up(c->dPsi, N, c->S, 0, c->qidx, c->qc, c->dTags, c->st));
    std::vector<int> h((size_t)N);
    HIPCHK(hipMemcpyAsync(h.data(), c->dTags, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    int cnt = 0;
    for (int i = 0; i < N; ++i) cnt += h[i];
    if (tags) memcpy(tags, h.data(), (size_t)N * sizeof(int));
    if (n_up) *n_up = cnt;
    return 0;
}

// recordTaggedParticleMoments (QTT:1069-1138): moments from the device sums of tag set 0,
// distributions from k_tagged_kde (queued; dist == NULL skips them)
int mdmc::tagged_moments_qt_queue(mdmc_ctx* c, double* sums_dev, bool dist) {
    HIPCHK(launch_tag_moments(c->dV, c->dTags, c->N, sums_dev, c->st));
    if (dist) HIPCHK(launch_tagged_kde(c->dV, c->dTags, c->N, c->S, c->dKdePart, c->dKde, c->st));
    return 0;
}
void mdmc::moments_qt_from_sums(const double* m, double* out4) {   // :1106-1109
    const unsigned num = (unsigned)m[4];
    out4[0] = m[0] / num; out4[1] = m[1] / num; out4[2] = m[2] / num; out4[3] = m[3] / num;
}

extern "C" int mdmc_tagged_moments_qt(mdmc_ctx* c, double out4[4], double* dist) {
    if (need_qt(c, "mdmc_tagged_moments_qt")) return -1;
    if (!out4) return set_error("mdmc_tagged_moments_qt: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    if (mdmc::tagged_moments_qt_queue(c, c->dOut, dist != nullptr)) return -1;
    double m[kTagMomentSums];
    HIPCHK(hipMemcpyAsync(m, c->dOut, sizeof m, hipMemcpyDeviceToHost, c->st));
    if (dist) HIPCHK(hipMemcpyAsync(dist, c->dKde, (size_t)3 * TKDE_BINS * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    mdmc::moments_qt_from_sums(m, out4);
    return 0;
}

extern "C" int mdmc_get_psi(mdmc_ctx* c, double* psi) {             // [N][12][2]
    if (need_qt(c, "mdmc_get_psi")) return -1;
    if (!psi) return set_error("mdmc_get_psi: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    const int N = c->N, S = c->S;
    std::vector<double> h((size_t)24 * S);
    HIPCHK(hipMemcpyAsync(h.data(), c->dPsi, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < 24; ++k) psi[(size_t)24 * i + k] = h[(size_t)k * S + i];
    return 0;
}

extern "C" int mdmc_set_psi(mdmc_ctx* c, const double* psi) {
    if (need_qt(c, "mdmc_set_psi")) return -1;
    if (!psi) return set_error("mdmc_set_psi: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    const int N = c->N, S = c->S;
    std::vector<double> h((size_t)24 * S, 0.);
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < 24; ++k) h[(size_t)k * S + i] = psi[(size_t)24 * i + k];
    HIPCHK(hipMemcpyAsync(c->dPsi, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

extern "C" int mdmc_setup_directories(mdmc_ctx* c) {            // main() :1037-1058
    if (!c) return set_error("NULL context");
    std::string d = c->p.saveDirectory;
    if (mkdir_p(d.c_str())) return -1;
    char nb[256];
    if (c->qt)                                                     // QTT:1153
        snprintf(nb, sizeof nb, "Gamma%dKappa%dNumIons%dPumpTime%dDet%dOm%dDensity%d", (unsigned)(c->p.Gamma * 100),
                 (unsigned)(c->p.kappa * 100), (unsigned)(c->N), (unsigned)(1000000000. * c->p.tpumpreal),
                 (unsigned)(100. * fabs(c->p.detuning)), (unsigned)(100. * c->p.Om), (unsigned)(10. * c->p.n));
    else
        snprintf(nb, sizeof nb, "Gamma%dKappa%dNumIons%d", (unsigned)(c->p.Gamma * 100), (unsigned)(c->p.kappa * 100),
                 (unsigned)(c->N));
    d += nb;
    if (mkdir_p(d.c_str())) return -1;
    snprintf(nb, sizeof nb, "/job%d/", c->p.job);
    d += nb;
    if (mkdir_p(d.c_str())) return -1;
    c->saveDir = d;
    return 0;
}

extern "C" const char* mdmc_save_directory(const mdmc_ctx* c) { return c ? c->saveDir.c_str() : ""; }
