// Host engine of the three-level laser-cooling program (laserCoolNoPlasmaThreeState.cpp, "LC3"):
// the C ABI of include/mdlc.h.  Owns the device-resident state of an ensemble of jobs (vx, psi,
// tPart), draws init()'s velocities from the reference's std::mt19937 stream, drives the gfx950
// kernels of mdlc_kernels.hip and reproduces main()'s loop, directories and energies.dat.  A parameter scan
// (mdlc_create_sweep) is the same context over npoints x R members, stepped by mdlc_sweep_kernels.hip.
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/mdlc.h"
#include "mdlc_kernels.hpp"
#include "mdqt_batch.hpp"    // LaunchTimer
#include "mdqt_devbuf.hpp"
#include "mdqt_error.hpp"    // HIPCHK, mdqt::set_error
#include "mdqt_lgtext.hpp"   // LgText: energies.dat's "%lg" rows
#include "mdqt_mt32.hpp"
#include "mdqt_sweep.hpp"

using namespace mdqt;

struct mdlc_ctx {
    mdlc_params p;                     // point 0: the fixed fields of every member
    std::vector<mdlc_params> pts;      // [npoints] the parameter points (an ordinary context: p alone)
    int npoints = 1, R = 0;            // members: npoints x R, point-major (member k: point k / R, job p.job + k % R)
    bool sweep = false;                // made by mdlc_create_sweep: stepped by k_lc_steps_sweep
    DevBuf<LCPoint> dPts;              // [npoints] the points' laser constants, written once at create
    int N0 = 0, J = 0, S = 0, B = 0;   // J: the members
    int dev = 0;
    hipStream_t st = nullptr;
    DevBuf<double> dVx, dPsi, dTp, dPart, dEk;
    PinBuf<double> hEk;                // pinned: a chunk of the run's EkinX values [kChunk][J]
    std::vector<double> hVyz;          // [J][2][N0]: V[1], V[2] (drawn by init(), never read by qstep())
    uint64_t qidx = 0;
    std::vector<std::string> dirs;     // [J]
};

namespace {

constexpr int kMaxLaunchSteps = 8192;  // steps per launch (a few ms): a launch's length never follows tmax
constexpr int kChunk = 512;            // output intervals between two host synchronisations of mdlc_run

constexpr long long kMaxGrid = 0x7fffffffLL;   // workgroups of one launch

// what is wrong with p (nullptr: nothing)
const char* params_refusal(const mdlc_params* p) {
    if (p->N0 < 1) return "N0 must be >= 1";
    if (p->njobs < 1) return "njobs must be >= 1";
    if (!(p->dt > 0)) return "dt must be positive";
    if (p->sampleFreq < 1) return "sampleFreq must be >= 1";
    if (!(p->temperature >= 0)) return "temperature must be >= 0";
    const long long S = ((long long)p->N0 + kLCBlock - 1) / kLCBlock * kLCBlock;
    if (S * p->njobs / kLCBlock > kMaxGrid) return "N0 x njobs is too large for one launch grid";
    return nullptr;
}

int check_params(const mdlc_params* p) {
    const char* r = params_refusal(p);
    return r ? set_error("%s", r) : 0;
}

// The swept fields (mdqt_sweep.hpp; the reference's directory name has a level for each, LC3:371-375, with these
// scales: directory_levels), and the name of the first other field in which b differs from a (nullptr: none).
// Field by field: the struct has padding.
const SweepField<mdlc_params> kSweep[] = {{"detuning", &mdlc_params::detuning, 100},
                                          {"Om", &mdlc_params::Om, 100},
                                          {"temperature", &mdlc_params::temperature, 1000000}};
const char* fixed_field_differs(const mdlc_params& a, const mdlc_params& b) {
#define FIXED(name) if (memcmp(&a.name, &b.name, sizeof a.name)) return #name;
    FIXED(N0) FIXED(tmax) FIXED(applyForce) FIXED(sampleFreq) FIXED(vKick) FIXED(dt) FIXED(seed) FIXED(job)
    FIXED(device) FIXED(njobs)
#undef FIXED
    if (strncmp(a.saveDirectory, b.saveDirectory, sizeof a.saveDirectory)) return "saveDirectory";
    return nullptr;
}

// mdlc_create_sweep's refusals: host arithmetic only
int sweep_validate(const mdlc_params* pts, int npoints, const char* what) {
    if (!pts) return set_error("%s: NULL argument", what);
    if (npoints < 1) return set_error("%s: npoints must be >= 1", what);
    for (int q = 0; q < npoints; ++q) {
        if (const char* r = params_refusal(pts + q)) return set_error("%s: point %d: %s", what, q, r);
        if (sweep_refuse_fixed(kSweep, q, fixed_field_differs(pts[0], pts[q]),
                               "the others fix the stride, the loop counts, the outputs and the Philox keys of every member; "
                               "the directory name has no level for vKick", what))
            return -1;
    }
    if (sweep_refuse_same(kSweep, pts, npoints, what)) return -1;
    const long long B = ((long long)pts[0].N0 + kLCBlock - 1) / kLCBlock;
    if (B * pts[0].njobs * npoints > kMaxGrid)
        return set_error("%s: npoints x njobs x workgroups per job = %d x %d x %lld is too large for one launch grid", what,
                         npoints, pts[0].njobs, B);
    return 0;
}

// what differs between the points in LCArgs
LCPoint laser_point(const mdlc_params& p) {
    LCPoint l;
    l.mi0 = p.dt * p.detuning;             // Im M11, M22 at v = 0: -dt (-detuning) (:192-193)
    l.cim = p.dt * (p.Om / 2);             // -i dt (-Om/2) (:194)
    l.ks = 1 * p.vKick * p.Om * p.dt;      // :189
    return l;
}

LCArgs make_args(const mdlc_ctx* c, int nsteps) {
    const mdlc_params& p = c->p;
    const LCPoint l = laser_point(p);      // (a scan's kernel reads its points' instead)
    LCArgs a;
    memset(&a, 0, sizeof a);
    a.vx = c->dVx; a.psi = c->dPsi; a.tPart = c->dTp; a.part = c->dPart;
    a.N0 = c->N0; a.S = c->S; a.B = c->B; a.nsteps = nsteps;
    a.q0 = c->qidx; a.seed = p.seed; a.job0 = p.job; a.applyForce = p.applyForce ? 1 : 0;
    a.dt = p.dt;
    a.mre = 1. - p.dt * 0.5;               // Re M11 = Re M22: 1 + dt Im(hamDecayTerm) (:203, :223)
    a.mi0 = l.mi0; a.cim = l.cim; a.ks = l.ks;
    a.vKick = p.vKick;
    return a;
}

// one launch of nsteps qsteps (0: the partial sums only) for every member
hipError_t launch_steps(const mdlc_ctx* c, int nsteps, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
    if (c->npoints > 1 || c->sweep) return launch_lc_steps_sweep(make_args(c, nsteps), c->dPts, c->R, c->J, c->st, ev0, ev1);
    return launch_lc_steps(make_args(c, nsteps), c->J, c->st, ev0, ev1);
}

// member k's point and job number
const mdlc_params& member_point(const mdlc_ctx* c, int k) { return c->pts[(size_t)(k / c->R)]; }
uint32_t member_job(const mdlc_ctx* c, int k) { return c->p.job + (uint32_t)(k % c->R); }

// qstep() x n on the stream, in launches of at most kMaxLaunchSteps
int qsteps_async(mdlc_ctx* c, long long n) {
    while (n > 0) {
        const int k = (int)(n < kMaxLaunchSteps ? n : kMaxLaunchSteps);
        HIPCHK(launch_steps(c, k));
        c->qidx += (uint64_t)k;
        n -= k;
    }
    return 0;
}

// EkinX of every job into dst[J] (device), from the last launch's workgroup partials
int ekin_async(mdlc_ctx* c, double* dst, bool fresh) {
    if (!fresh) HIPCHK(launch_steps(c, 0));
    HIPCHK(launch_lc_ekin(c->dPart, c->J, c->B, c->N0, dst, c->st));
    return 0;
}

// main() :364-380: the directory levels of job `job`, innermost last
void directory_levels(const mdlc_params* p, uint32_t job, std::string lv[4]) {
    char sd[sizeof p->saveDirectory + 1];
    memcpy(sd, p->saveDirectory, sizeof p->saveDirectory);
    sd[sizeof p->saveDirectory] = 0;
    char b[128];
    lv[0] = sd;
    snprintf(b, sizeof b, "Om%d/", ref_udcast(p->Om * 100));                                   // :371
    lv[1] = lv[0] + b;
    snprintf(b, sizeof b, "Det%dNumIons%dInitialTemp%duK", ref_udcast(p->detuning * 100),      // :374
             ref_udcast((double)p->N0), ref_udcast(p->temperature * 1000000));
    lv[2] = lv[1] + b;
    snprintf(b, sizeof b, "/job%d/", (int)job);                                                // :378
    lv[3] = lv[2] + b;
}

// main()'s loop (:392-407) without its body: the t of every output() and the number of qsteps
void main_loop_counts(const mdlc_params& p, std::vector<double>* touts, long long* iterations) {
    double t = 0;
    long long c0 = 0;
    while (t <= p.tmax) {
        t += p.dt;                                                  // repeated addition, as the reference
        if ((c0 + 1) % p.sampleFreq == 0 && touts) touts->push_back(t);
        c0++;
    }
    *iterations = c0;
}

}  // namespace

extern "C" void mdlc_default_params(mdlc_params* p) {                 // LC3:54-88, :393
    memset(p, 0, sizeof *p);
    p->N0 = 1000; p->detuning = -0.5; p->Om = 0.5; p->tmax = 45000; p->applyForce = 1;
    p->sampleFreq = 1000; p->temperature = 0.01; p->vKick = 0.0012076; p->dt = 0.01;
    p->seed = 12345; p->job = 1; p->device = -1; p->njobs = 1;
    strcpy(p->saveDirectory, "dataLaserCoolTestDoppShift/");
}

extern "C" int mdlc_sample_velocities(uint32_t seed, int N0, double temperature, double* V) {
    if (!V || N0 < 1) return set_error("mdlc_sample_velocities: bad argument");
    Mt32 rng;
    rng.seed(seed);                                                   // :46 (seed instead of random_device)
    std::uniform_real_distribution<double> uni(0, 1);                 // :47
    (void)uni(rng);                                                   // :48 auto random_double = uni(rng)
    std::normal_distribution<double> velocityDistribution(0, 1.0508 * sqrt(temperature));   // :83
    for (int i = 0; i < N0; ++i) {                                    // :119-124
        V[i] = velocityDistribution(rng);
        V[(size_t)N0 + i] = velocityDistribution(rng);
        V[(size_t)2 * N0 + i] = velocityDistribution(rng);
    }
    return 0;
}

extern "C" int mdlc_format_directory(const mdlc_params* p, uint32_t job, char* out, size_t cap) {
    if (!p || !out) return set_error("mdlc_format_directory: NULL argument");
    std::string lv[4];
    directory_levels(p, job, lv);
    if (lv[3].size() + 1 > cap) return set_error("mdlc_format_directory: buffer holds %zu < %zu bytes", cap, lv[3].size() + 1);
    memcpy(out, lv[3].c_str(), lv[3].size() + 1);
    return 0;
}

extern "C" void mdlc_destroy(mdlc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->dev);
    if (c->st) (void)hipStreamSynchronize(c->st);
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
}

namespace {

// mdlc_create (one point, its njobs jobs) and mdlc_create_sweep (the caller has validated the points)
int create(const mdlc_params* p, int npoints, bool sweep, mdlc_ctx** out) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) return set_error("no HIP device available (%s)", hipGetErrorString(e));
    std::unique_ptr<mdlc_ctx, void (*)(mdlc_ctx*)> guard(new mdlc_ctx(), mdlc_destroy);
    mdlc_ctx* c = guard.get();
    c->pts.assign(p, p + npoints);
    for (auto& q : c->pts) q.saveDirectory[sizeof(q.saveDirectory) - 1] = 0;
    c->p = c->pts[0];
    c->npoints = npoints;
    c->sweep = sweep;
    if (p->device >= 0) {
        if (p->device >= ndev) return set_error("device %d >= device count %d", p->device, ndev);
        c->dev = p->device;
    } else {
        (void)hipGetDevice(&c->dev);
    }
    if (hipSetDevice(c->dev) != hipSuccess || hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess)
        return set_error("cannot create a HIP stream on device %d", p->device);
    c->N0 = p->N0;
    c->R = p->njobs;
    c->J = npoints * c->R;
    c->B = (p->N0 + kLCBlock - 1) / kLCBlock;
    c->S = c->B * kLCBlock;
    const size_t n = (size_t)c->J * c->S, sz = n * sizeof(double);
    bool ok = c->dVx.alloc(n) == hipSuccess && c->dPsi.alloc(6 * n) == hipSuccess && c->dTp.alloc(n) == hipSuccess &&
              c->dPart.alloc((size_t)c->J * c->B) == hipSuccess && c->dEk.alloc((size_t)kChunk * c->J) == hipSuccess;
    if (sweep) {
        std::vector<LCPoint> l;
        for (const auto& q : c->pts) l.push_back(laser_point(q));
        ok = ok && c->dPts.alloc((size_t)npoints) == hipSuccess &&
             hipMemcpyAsync(c->dPts, l.data(), l.size() * sizeof(LCPoint), hipMemcpyHostToDevice, c->st) == hipSuccess &&
             hipStreamSynchronize(c->st) == hipSuccess;
    }
    if (!ok) return set_error("mdlc_create: device allocation failed");
    // the reference's globals start at zero (V, tPart, LC3:84, :91); psi gets its value in init()
    ok = hipMemsetAsync(c->dVx, 0, sz, c->st) == hipSuccess && hipMemsetAsync(c->dPsi, 0, 6 * sz, c->st) == hipSuccess &&
         hipMemsetAsync(c->dTp, 0, sz, c->st) == hipSuccess && hipStreamSynchronize(c->st) == hipSuccess;
    if (!ok) return set_error("mdlc_create: device initialisation failed");
    if (c->hEk.alloc((size_t)kChunk * c->J) != hipSuccess)
        return set_error("mdlc_create: pinned allocation failed");
    c->hVyz.assign((size_t)c->J * 2 * c->N0, 0.);
    c->dirs.resize(c->J);
    for (int k = 0; k < c->J; ++k) {
        std::string lv[4];
        directory_levels(&member_point(c, k), member_job(c, k), lv);
        c->dirs[k] = lv[3];
    }
    *out = guard.release();
    return 0;
}

}  // namespace

extern "C" int mdlc_create(const mdlc_params* p, mdlc_ctx** out) {
    if (!p || !out) return set_error("mdlc_create: NULL argument");
    *out = nullptr;
    if (check_params(p)) return -1;
    return create(p, 1, false, out);
}

// member k of a scan: point k / R, replica k % R (R = points[0].njobs), as the single job job + r
extern "C" int mdlc_sweep_params(const mdlc_params* points, int npoints, int k, mdlc_params* out) {
    if (!points || !out) return set_error("mdlc_sweep_params: NULL argument");
    if (sweep_validate(points, npoints, "mdlc_sweep_params")) return -1;
    int q, r;
    if (sweep_member(npoints, points[0].njobs, k, "member", "mdlc_sweep_params", &q, &r)) return -1;
    *out = points[q];
    out->job += (uint32_t)r;
    out->njobs = 1;
    return 0;
}

extern "C" int mdlc_create_sweep(const mdlc_params* points, int npoints, mdlc_ctx** out) {
    if (!points || !out) return set_error("mdlc_create_sweep: NULL argument");
    *out = nullptr;
    if (sweep_validate(points, npoints, "mdlc_create_sweep")) return -1;
    return create(points, npoints, true, out);
}

extern "C" double mdlc_get_const(const mdlc_ctx* c, const char* n) {
    if (!c || !n) return NAN;
    if (!strcmp(n, "N0")) return c->N0;
    if (!strcmp(n, "njobs")) return c->R;
    if (!strcmp(n, "npoints")) return c->npoints;
    if (!strcmp(n, "members")) return c->J;
    if (!strcmp(n, "dt")) return c->p.dt;
    if (!strcmp(n, "stride")) return c->S;
    if (!strcmp(n, "qstep_index")) return (double)c->qidx;
    if (!strcmp(n, "iterations") || !strcmp(n, "outputs")) {
        long long it = 0;
        main_loop_counts(c->p, nullptr, &it);
        return !strcmp(n, "iterations") ? (double)it : (double)(it / c->p.sampleFreq);
    }
    return NAN;
}

extern "C" int mdlc_set_state(mdlc_ctx* c, const double* V, const double* psi, const double* tPart,
                              const uint64_t* qstep) {
    if (!c) return set_error("NULL context");
    HIPCHK(hipSetDevice(c->dev));
    const int N0 = c->N0, J = c->J;
    const size_t S = c->S, n = (size_t)J * S;
    std::vector<double> h;
    if (V) {
        h.assign(n, 0.);
        for (int k = 0; k < J; ++k) {
            const double* Vk = V + (size_t)k * 3 * N0;
            memcpy(&h[k * S], Vk, N0 * sizeof(double));
            memcpy(&c->hVyz[(size_t)k * 2 * N0], Vk + N0, (size_t)2 * N0 * sizeof(double));
        }
        HIPCHK(hipMemcpyAsync(c->dVx, h.data(), n * sizeof(double), hipMemcpyHostToDevice, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    if (psi) {
        h.assign(6 * n, 0.);
        for (int k = 0; k < J; ++k)
            for (int i = 0; i < N0; ++i)
                for (int q = 0; q < 6; ++q) h[q * n + k * S + i] = psi[((size_t)k * N0 + i) * 6 + q];
        HIPCHK(hipMemcpyAsync(c->dPsi, h.data(), 6 * n * sizeof(double), hipMemcpyHostToDevice, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    if (tPart) {
        h.assign(n, 0.);
        for (int k = 0; k < J; ++k) memcpy(&h[k * S], tPart + (size_t)k * N0, N0 * sizeof(double));
        HIPCHK(hipMemcpyAsync(c->dTp, h.data(), n * sizeof(double), hipMemcpyHostToDevice, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    if (qstep) c->qidx = *qstep;
    return 0;
}

extern "C" int mdlc_get_state(mdlc_ctx* c, double* V, double* psi, double* tPart, uint64_t* qstep) {
    if (!c) return set_error("NULL context");
    HIPCHK(hipSetDevice(c->dev));
    const int N0 = c->N0, J = c->J;
    const size_t S = c->S, n = (size_t)J * S;
    std::vector<double> h;
    if (V) {
        h.resize(n);
        HIPCHK(hipMemcpyAsync(h.data(), c->dVx, n * sizeof(double), hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        for (int k = 0; k < J; ++k) {
            double* Vk = V + (size_t)k * 3 * N0;
            memcpy(Vk, &h[k * S], N0 * sizeof(double));
            memcpy(Vk + N0, &c->hVyz[(size_t)k * 2 * N0], (size_t)2 * N0 * sizeof(double));
        }
    }
    if (psi) {
        h.resize(6 * n);
        HIPCHK(hipMemcpyAsync(h.data(), c->dPsi, 6 * n * sizeof(double), hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        for (int k = 0; k < J; ++k)
            for (int i = 0; i < N0; ++i)
                for (int q = 0; q < 6; ++q) psi[((size_t)k * N0 + i) * 6 + q] = h[q * n + k * S + i];
    }
    if (tPart) {
        h.resize(n);
        HIPCHK(hipMemcpyAsync(h.data(), c->dTp, n * sizeof(double), hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        for (int k = 0; k < J; ++k) memcpy(tPart + (size_t)k * N0, &h[k * S], N0 * sizeof(double));
    }
    if (qstep) *qstep = c->qidx;
    return 0;
}

// init() :115-131 for every member: job number j's velocities from mt19937(seed + j) at its point's temperature,
// psi = (1, 0, 0), tPart = 0
extern "C" int mdlc_init(mdlc_ctx* c) {
    if (!c) return set_error("NULL context");
    const int N0 = c->N0, J = c->J;
    std::vector<double> V((size_t)J * 3 * N0), psi((size_t)J * N0 * 6, 0.), tp((size_t)J * N0, 0.);
    for (int k = 0; k < J; ++k)
        if (mdlc_sample_velocities(c->p.seed + member_job(c, k), N0, member_point(c, k).temperature, &V[(size_t)k * 3 * N0]))
            return -1;
    for (size_t i = 0; i < (size_t)J * N0; ++i) psi[6 * i] = 1.;          // :125
    const uint64_t q0 = 0;
    return mdlc_set_state(c, V.data(), psi.data(), tp.data(), &q0);
}

extern "C" int mdlc_qsteps(mdlc_ctx* c, long long n) {
    if (!c) return set_error("NULL context");
    if (n < 0) return set_error("mdlc_qsteps: n < 0");
    HIPCHK(hipSetDevice(c->dev));
    if (qsteps_async(c, n)) return -1;
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

extern "C" int mdlc_time_qsteps(mdlc_ctx* c, int nsteps, int warmup, int launches, double* ms) {
    if (!c || !ms) return set_error("mdlc_time_qsteps: NULL argument");
    if (nsteps < 1 || nsteps > kMaxLaunchSteps || warmup < 0 || launches < 1)
        return set_error("mdlc_time_qsteps: nsteps must be in [1, %d], warmup >= 0, launches >= 1", kMaxLaunchSteps);
    HIPCHK(hipSetDevice(c->dev));
    if (qsteps_async(c, (long long)warmup * nsteps)) return -1;
    std::vector<hipEvent_t> ev((size_t)2 * launches, nullptr);
    int rc = 0;
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) rc = set_error("mdlc_time_qsteps: cannot create an event");
    for (int l = 0; l < launches && !rc; ++l) {
        if (launch_steps(c, nsteps, ev[2 * l], ev[2 * l + 1]) != hipSuccess)
            rc = set_error("mdlc_time_qsteps: launch failed");
        else
            c->qidx += (uint64_t)nsteps;
    }
    if (hipStreamSynchronize(c->st) != hipSuccess && !rc) rc = set_error("mdlc_time_qsteps: synchronisation failed");
    for (int l = 0; l < launches && !rc; ++l) {
        float t = 0;
        if (hipEventElapsedTime(&t, ev[2 * l], ev[2 * l + 1]) != hipSuccess) rc = set_error("mdlc_time_qsteps: no event time");
        ms[l] = t;
    }
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

extern "C" int mdlc_ekin_x(mdlc_ctx* c, double* out) {
    if (!c || !out) return set_error("mdlc_ekin_x: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    if (ekin_async(c, c->dEk, false)) return -1;
    HIPCHK(hipMemcpyAsync(c->hEk, c->dEk, (size_t)c->J * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    memcpy(out, c->hEk, (size_t)c->J * sizeof(double));
    return 0;
}

extern "C" int mdlc_setup_directories(mdlc_ctx* c) {            // main() :364-380
    if (!c) return set_error("NULL context");
    for (int k = 0; k < c->J; ++k) {
        std::string lv[4];
        directory_levels(&member_point(c, k), member_job(c, k), lv);
        for (int l = 0; l < 4; ++l) (void)mkdir(lv[l].c_str(), 0777);   // the reference ignores mkdir's result
        struct stat sb;
        if (stat(lv[3].c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode))
            return set_error("cannot create output directory %s", lv[3].c_str());
    }
    return 0;
}

extern "C" const char* mdlc_save_directory(const mdlc_ctx* c, int k) {
    if (!c || k < 0 || k >= c->J) return nullptr;
    return c->dirs[k].c_str();
}

// main() :356-408.  One launch per output interval (sampleFreq - 1 steps before the first
// output(), sampleFreq between two, the remainder after the last); each interval's EkinX goes to
// a device buffer that the host drains every kChunk intervals into the jobs' energies.dat.
extern "C" int mdlc_run(mdlc_ctx* c, int verbose) {
    if (!c) return set_error("NULL context");
    HIPCHK(hipSetDevice(c->dev));
    if (mdlc_setup_directories(c)) return -1;
    if (mdlc_init(c)) return -1;                                    // :391
    std::vector<double> touts;
    long long iterations = 0;
    main_loop_counts(c->p, &touts, &iterations);
    const int J = c->J;
    const long long sf = c->p.sampleFreq, nout = (long long)touts.size();
    long long done = 0, drained = 0;
    auto drain = [&](long long upto) -> int {                      // outputs [drained, upto) sit in dEk
        const long long m = upto - drained;
        if (m <= 0) return 0;
        HIPCHK(hipMemcpyAsync(c->hEk, c->dEk, (size_t)m * J * sizeof(double), hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        for (int k = 0; k < J; ++k) {
            const std::string path = c->dirs[k] + "energies.dat";
            FILE* fa = fopen(path.c_str(), "a");                    // :321
            if (!fa) return set_error("cannot open %s: %s", path.c_str(), strerror(errno));
            bool ok;
            {
                LgText tx(fa);
                for (long long o = 0; o < m; ++o) {                 // :322 "%lg\t%lg\n"
                    tx.num(touts[drained + o]); tx.ch('\t'); tx.num(c->hEk[(size_t)o * J + k]); tx.ch('\n');
                }
                tx.spill();
                ok = tx.ok();
            }
            if (fclose(fa) != 0 || !ok) return set_error("write error on %s", path.c_str());
        }
        if (verbose) {
            printf("mdlc: t = %g  (%lld of %lld outputs)  EkinX[job %u] = %g\n", touts[upto - 1], upto, nout,
                   c->p.job, c->hEk[(size_t)(m - 1) * J]);
            fflush(stdout);
        }
        drained = upto;
        return 0;
    };
    for (long long o = 0; o < nout; ++o) {
        const long long target = (o + 1) * sf - 1;                  // qsteps before output o (:399-406)
        const bool stepped = target > done;
        if (qsteps_async(c, target - done)) return -1;
        done = target;
        if (ekin_async(c, c->dEk + (size_t)(o - drained) * J, stepped)) return -1;
        if (o + 1 - drained == kChunk && drain(o + 1)) return -1;
    }
    if (drain(nout)) return -1;
    if (qsteps_async(c, iterations - done)) return -1;              // the steps after the last output()
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}
