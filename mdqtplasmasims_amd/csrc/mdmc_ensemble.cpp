// mdmc_ensemble — J independent jobs of the Monte-Carlo + MD programs in one process (include/mdmc.h,
// "ensembles").  The reference runs them as a Slurm array (exampleSlurmFile.slurm:3,16, `srun tagQuad
// $SLURM_ARRAY_TASK_ID`); a single job's Metropolis anneal is one workgroup on one CU, because the chain is
// sequential, so the array's anneals run here as ONE launch of J workgroups (k_monte_carlo_lds_ens: the
// single-job kernel's body on each member's own argument block, which is the bit-identity argument).  The MD
// stages queue every member's own launches on its own stream, one host thread, so they overlap on the chip;
// they are the single context's code on the single context's arguments.
#include <algorithm>
#include <memory>

#include "mdmc_ctx.hpp"

using namespace mdqt;

namespace {

constexpr int kEnsembleMaxJobs = 1024;

int sync_members(mdmc_ensemble* e) {
    for (mdmc_ctx* c : e->jobs) HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

}  // namespace

extern "C" int mdmc_ensemble_job_params(const mdmc_params* base, int k, mdmc_params* out) {
    if (!base || !out) return set_error("mdmc_ensemble_job_params: NULL argument");
    if (k < 0 || k >= kEnsembleMaxJobs) return set_error("mdmc_ensemble_job_params: job index %d outside [0, %d)", k, kEnsembleMaxJobs);
    mdmc_params p = *base;
    p.job = base->job + (uint32_t)k;               // the array index, MCMD:1035
    p.seed = base->seed + (uint32_t)k;             // the reference: std::random_device per job, MCMD:52-53
    *out = p;
    return 0;
}

extern "C" void mdmc_ensemble_destroy(mdmc_ensemble* e) {
    if (!e) return;
    (void)hipSetDevice(e->dev);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (size_t k = e->jobs.size(); k-- > 0;) mdmc_destroy(e->jobs[k]);
    if (e->dArgs) (void)hipFree(e->dArgs);
    if (e->hArgs) (void)hipHostFree(e->hArgs);
    if (e->hMT) (void)hipHostFree(e->hMT);
    if (e->hAcc) (void)hipHostFree(e->hAcc);
    for (hipEvent_t ev : e->evpool) (void)hipEventDestroy(ev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

extern "C" int mdmc_ensemble_create(const mdmc_params* p, int njobs, mdmc_ensemble** out) {
    if (!p || !out) return set_error("mdmc_ensemble_create: NULL argument");
    *out = nullptr;
    if (njobs < 1 || njobs > kEnsembleMaxJobs) return set_error("mdmc_ensemble_create: njobs must be 1 .. %d", kEnsembleMaxJobs);
    if (p->N > mdmc::kBatchedMaxN)
        return set_error("mdmc_ensemble_create: N = %d: the batched anneal keeps the positions in LDS (N <= %d)", p->N,
                         mdmc::kBatchedMaxN);
    std::unique_ptr<mdmc_ensemble, void (*)(mdmc_ensemble*)> e(new (std::nothrow) mdmc_ensemble(), mdmc_ensemble_destroy);
    if (!e) return set_error("mdmc_ensemble_create: out of memory");
    try {
        e->jobs.reserve((size_t)njobs);
    } catch (const std::exception& x) {
        return set_error("mdmc_ensemble_create: %s", x.what());
    }
    for (int k = 0; k < njobs; ++k) {
        mdmc_params pk;
        mdmc_ctx* c = nullptr;
        if (mdmc_ensemble_job_params(p, k, &pk) || mdmc_create(&pk, &c)) {
            const std::string why = mdqt_last_error();
            return set_error("mdmc_ensemble_create: job index %d: %s", k, why.c_str());   // e frees jobs 0 .. k-1
        }
        e->jobs.push_back(c);
        if (k == 0) e->dev = c->dev;
    }
    HIPCHK(hipSetDevice(e->dev));
    const size_t J = (size_t)njobs;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&e->dArgs, J * sizeof(MCArgs)) != hipSuccess ||
        hipHostMalloc((void**)&e->hArgs, 2 * J * sizeof(MCArgs), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&e->hMT, J * 625 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&e->hAcc, J * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
        return set_error("mdmc_ensemble_create: allocating the argument blocks of %d jobs failed", njobs);
    *out = e.release();
    return 0;
}

extern "C" int mdmc_ensemble_size(const mdmc_ensemble* e) { return e ? (int)e->jobs.size() : -1; }

extern "C" mdmc_ctx* mdmc_ensemble_job(mdmc_ensemble* e, int k) {
    if (!e || k < 0 || k >= (int)e->jobs.size()) {
        set_error("mdmc_ensemble_job: job index %d outside the ensemble", k);
        return nullptr;
    }
    return e->jobs[(size_t)k];
}

extern "C" int mdmc_ensemble_init(mdmc_ensemble* e) {            // init() of every job, MCMD:173-245
    if (!e) return set_error("NULL ensemble");
    for (mdmc_ctx* c : e->jobs)
        if (mdmc_init(c)) return -1;
    return 0;
}

// mdmc_monte_carlo for every member: each chain's mt19937 state to its own dMT, its dAcc zeroed (on its own
// stream, then waited for), the chunks on the ensemble's stream with the argument blocks copied in stream
// order before each, and everything back with one synchronisation.  The chains share nothing and need no
// lockstep: a member annealed or stepped on its own in between simply carries its state.
int mdmc::ensemble_anneal(mdmc_ensemble* e, int nsteps, long long* accepted) {
    const size_t J = e->jobs.size();
    for (mdmc_ctx* c : e->jobs) c->rnValid = false;
    if (nsteps < 0) return set_error("nsteps < 0");
    HIPCHK(hipSetDevice(e->dev));
    for (mdmc_ctx* c : e->jobs) {
        HIPCHK(hipMemcpyAsync(c->dMT, c->rng.x, sizeof c->rng.x, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemsetAsync(c->dAcc, 0, sizeof(unsigned long long), c->st));
    }
    if (sync_members(e)) return -1;
    // a call has two kinds of chunk: full ones and its last; the pinned area holds the blocks of both, written
    // here while nothing is in flight (every ensemble call ends synchronised)
    const int last = nsteps % mdmc::kAnnealChunk;
    for (size_t k = 0; k < J; ++k) {
        MCArgs a;
        mdmc::mc_args(e->jobs[k], a);
        a.nsteps = mdmc::kAnnealChunk;
        e->hArgs[k] = a;
        a.nsteps = last;
        e->hArgs[J + k] = a;
    }
    for (int done = 0; done < nsteps;) {
        const int n = std::min(mdmc::kAnnealChunk, nsteps - done);
        const MCArgs* h = e->hArgs + (n == mdmc::kAnnealChunk ? 0 : J);
        HIPCHK(hipMemcpyAsync(e->dArgs, h, J * sizeof(MCArgs), hipMemcpyHostToDevice, e->stream));
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (e->timing && take_events(e->evpool, e->evused, &e0, &e1)) return -1;
        HIPCHK(launch_monte_carlo_ens(e->dArgs, h[0], (int)J, e->stream, e0, e1));
        done += n;
    }
    for (size_t k = 0; k < J; ++k) {
        mdmc_ctx* c = e->jobs[k];
        HIPCHK(hipMemcpyAsync(e->hMT + 625 * k, c->dMT, 625 * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(e->hAcc + k, c->dAcc, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t k = 0; k < J; ++k) {
        mdmc_ctx* c = e->jobs[k];
        memcpy(c->rng.x, e->hMT + 625 * k, sizeof c->rng.x);
        if (c->rng.x[624] > 624) return set_error("device MC kernel returned a bad mt19937 position for job index %zu", k);
        if (accepted) accepted[k] = (long long)e->hAcc[k];
    }
    return 0;
}

extern "C" int mdmc_ensemble_monte_carlo(mdmc_ensemble* e, int nsteps, long long* accepted) {   // MonteCarloStep() x n
    if (!e) return set_error("NULL ensemble");
    return mdmc::ensemble_anneal(e, nsteps, accepted);
}

// MDStep() x n of every member (:504-511): each step queued member by member on the members' own streams
extern "C" int mdmc_ensemble_md_steps(mdmc_ensemble* e, int nsteps) {
    if (!e) return set_error("NULL ensemble");
    HIPCHK(hipSetDevice(e->dev));
    for (int k = 0; k < nsteps; ++k)
        for (mdmc_ctx* c : e->jobs)
            if (mdmc::md_step_async(c)) return -1;
    if (sync_members(e)) return -1;
    for (mdmc_ctx* c : e->jobs) c->hitOff = 0;
    return 0;
}

// main() of every job in lockstep (:1030-1167; QTT:1140-1254): the stages of mdmc_run
extern "C" int mdmc_ensemble_run(mdmc_ensemble* e, int verbose) {
    if (!e) return set_error("NULL ensemble");
    HIPCHK(hipSetDevice(e->dev));
    std::fill(e->stage_ms, e->stage_ms + mdmc_ensemble::kStages, 0.);
    if (mdmc::run_members(e->jobs.data(), (int)e->jobs.size(), e, verbose)) return -1;
    return sync_members(e);
}

extern "C" int mdmc_ensemble_enable_timing(mdmc_ensemble* e, int on) {
    if (!e) return set_error("NULL ensemble");
    e->timing = on > 0;
    e->evused = 0;
    return 0;
}

// the anneal launches' own durations (their dispatch timestamps) since the last call: out[0..5) = sum (ms),
// launches, median, minimum, maximum (ms); out[5..11) = wall time (ms) of the last run's stages: anneal,
// pre-record MD, QT pump, recorded MD, autocorrelations, the rest.  Fills what n holds (n >= 3); resets the
// launch list
extern "C" int mdmc_ensemble_kernel_times(mdmc_ensemble* e, double* out, int n) {
    if (!e || !out) return set_error("mdmc_ensemble_kernel_times: NULL argument");
    if (n < 3) return set_error("mdmc_ensemble_kernel_times: need at least 3 doubles");
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<double> ms;
    double tot = 0.;
    for (int i = 0; i + 1 < e->evused; i += 2) {
        float x = 0.f;
        HIPCHK(hipEventElapsedTime(&x, e->evpool[i], e->evpool[i + 1]));
        ms.push_back(x);
        tot += x;
    }
    std::sort(ms.begin(), ms.end());
    double v[5 + mdmc_ensemble::kStages] = {tot, (double)ms.size(), ms.empty() ? 0. : ms[ms.size() / 2],
                                            ms.empty() ? 0. : ms.front(), ms.empty() ? 0. : ms.back()};
    std::copy(e->stage_ms, e->stage_ms + mdmc_ensemble::kStages, v + 5);
    for (int i = 0; i < n && i < 5 + mdmc_ensemble::kStages; ++i) out[i] = v[i];
    e->evused = 0;
    return 0;
}
