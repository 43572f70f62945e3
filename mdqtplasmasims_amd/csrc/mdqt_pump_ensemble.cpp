// mdqt_pump_ensemble — J independent jobs of an optical-pumping program (randomFrozenStartTag408Linear.cpp,
// 408Quad, 422Linear; qt_model 1-3) stepped in batched launches (include/mdqt.h, "ensembles of the
// optical-pumping programs").  It owns an mdqt_ensemble for the members (ordinary contexts on one stream), the
// pinned argument ring, the lockstep check (ens_check), the QT chunk loop (ens_qt_chunks), the batched force launch
// (ens_forces: k_pairs_n3_ens over the members on the Newton-3 tiles, a row member's own small launch), the range
// flags and the writer pool, and adds the pump programs' kernels over members (mdqt_pump_ensemble_kernels.hip).  Each member's arguments come from the helpers its own path uses
// (n3_force_args / n3_forces_pending inside ens_forces, substep_args(s, a, m, 0, 1, 1), mdqt_tag_spin_up's lo,
// qstep index and qc) and the kernels run the single-job kernels' bodies: every member's state and files are
// those of the job on its own, bit for bit.
//
// One MD step (step() :377-394) of every member at t > 0 is two launches: the batched force launch and
// k_pump_kick_ens (the canonical slot sum, the kick, the trailing half drift and — when nothing reads R, V or F
// before the next step — that step's leading half drift).  A step whose leading drift was not folded into the
// launch before it (the first of a call, the one after an output or the measurement, the t == 0 step with its
// forces() first) starts with k_pump_drift_ens.  In a run the time loop decides which steps lead and fold
// (mdqt_main_loops.hpp: pump_loop, mdqt_run_pump's too); mdqt_pump_ensemble_run's driver hands that to pump_step.
// The step blocks change only with a member's size or pending state: they are uploaded when they differ from
// what the device holds; the QT and tagging blocks go through the pinned ring.

#include <algorithm>

#include "mdqt_ensemble.hpp"

using namespace mdqt;

static_assert(sizeof(PumpTagArgs) <= sizeof(SubstepArgs) && sizeof(PumpKdeArgs) <= sizeof(SubstepArgs) &&
                  sizeof(PumpStepArgs) <= sizeof(SubstepArgs),
              "a ring slot holds one block per member of every kind");

namespace {

// the base ensemble's check (mdqt_ensemble.cpp: ens_check) with the tagged / untagged flag compared as well
int pump_check(const mdqt_pump_ensemble* pe, const char* what) { return ens_check(pe ? pe->base : nullptr, what, true); }

// the members' leapfrog blocks from their pending-force state, uploaded to dStep[which] when they differ
int step_blocks(mdqt_pump_ensemble* pe, int which, int* max_n) {
    mdqt_ensemble* e = pe->base;
    const int J = (int)e->jobs.size();
    std::vector<PumpStepArgs> h((size_t)J);
    int mx = 0;
    for (int k = 0; k < J; ++k) {
        const mdqt_ctx* s = e->jobs[k];
        PumpStepArgs& a = h[k];
        memset(&a, 0, sizeof a);
        a.R = s->dR; a.V = s->dV; a.F = s->dF; a.Fpart = s->dFpart;
        a.nseg = s->f_pending ? s->pend_nseg : 1;
        a.n = s->nloc; a.S = s->S; a.L = s->L;
        mx = std::max(mx, a.n);
    }
    *max_n = mx;
    return e->ring.send_if_changed(h, pe->step_held[which], pe->dStep[which], e->stream);
}

// step() of every member at the members' t (:377-394).  lead: the leading half drift is still to be done (it
// was not folded into the launch before); fold: append the next step's leading half drift (the caller knows
// that nothing reads R, V or F before it and that it is a t > 0 step)
int pump_step(mdqt_pump_ensemble* pe, bool lead, bool fold) {
    mdqt_ensemble* e = pe->base;
    const int J = (int)e->jobs.size();
    const mdqt_ctx* a = e->jobs[0];
    const double dt = a->dtQ * a->ratio;                         // :389 dt=quantumTimestep*ratio
    const double DT = 0.5 * dt, DT2 = DT * DT;
    const int moving = a->t > 0 ? 1 : 0;
    if (!moving && !lead) return set_error("mdqt_pump_ensemble: the t == 0 step has forces() before its leading drift");
    int max_n = 0;
    if (!moving && ens_forces(e)) return -1;                     // :331 forces() before the first drift
    if (lead) {
        if (step_blocks(pe, 0, &max_n)) return -1;               // settles what the t == 0 forces() left pending
        HIPCHK(launch_pump_drift_ens(pe->dStep[0], J, max_n, DT, DT2, moving, e->stream));
        pe->launches++;
        for (mdqt_ctx* s : e->jobs) s->f_pending = false;
    }
    if (ens_forces(e)) return -1;                                // step_V: forces() :361
    if (step_blocks(pe, 1, &max_n)) return -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e->timing && pe->kick_timer.take(&e0, &e1)) return -1;
    HIPCHK(launch_pump_kick_ens(pe->dStep[1], J, max_n, DT, DT2, moving, dt, fold ? 1 : 0, e->stream, e0, e1));
    pe->launches++;
    for (mdqt_ctx* s : e->jobs) s->f_pending = false;
    return 0;
}

// n x qstep() of every member (QT only: run_substeps(s, n, 0, 1, 1)), chunks of at most MAXSUB
int pump_qsteps(mdqt_pump_ensemble* pe, int n) {
    return ens_qt_chunks(pe->base, n, 0, [pe](const SubstepArgs* h, int maxn, hipEvent_t e0, hipEvent_t e1, int* inst) {
        mdqt_ensemble* e = pe->base;
        HIPCHK(launch_substeps_pump_ens(e->dSub, h[0], (int)e->jobs.size(), maxn, e->jobs[0]->dFTab, e->stream, e0, e1, inst));
        pe->launches++;
        return 0;
    });
}

// a member's tag array and tagged-distribution buffers at the member's present size
int member_buffers(mdqt_pump_ensemble* pe, int k) {
    mdqt_ensemble* e = pe->base;
    mdqt_ctx* s = e->jobs[k];
    const int nch = std::max(1, (s->N + 255) / 256);
    const size_t kde = ((size_t)nch + 1) * 3 * TKDE_BINS;
    if (s->dTkde.capacity() < kde || s->dSpinUp.capacity() < (size_t)s->capS) HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(s->dTkde.reserve(kde));
    if (s->dSpinUp.capacity() < (size_t)s->capS) {
        HIPCHK(s->dSpinUp.reserve((size_t)s->capS));
        HIPCHK(hipMemsetAsync(s->dSpinUp, 0, (size_t)s->capS * sizeof(int), e->stream));
        if ((int)s->spinUp.size() >= s->N && tagged(s))
            HIPCHK(hipMemcpyAsync(s->dSpinUp, s->spinUp.data(), (size_t)s->N * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));                 // spinUp may change before the copy would run
    }
    return 0;
}

// measureSpinUps() :600-665 of every member but its file: one launch writes every member's device tags, the
// host lists follow with one synchronisation
int pump_tag(mdqt_pump_ensemble* pe) {
    mdqt_ensemble* e = pe->base;
    const int J = (int)e->jobs.size();
    char* slot = nullptr;
    int idx = 0;
    if (e->ring.take(&slot, &idx)) return -1;
    PumpTagArgs* h = reinterpret_cast<PumpTagArgs*>(slot);
    int maxn = 0;
    for (int k = 0; k < J; ++k) {
        if (member_buffers(pe, k)) return -1;
        mdqt_ctx* s = e->jobs[k];
        PumpTagArgs& a = h[k];
        memset(&a, 0, sizeof a);
        a.psi = s->dPsi; a.n = s->nloc; a.S = s->S;
        a.gid0 = (uint64_t)s->lo; a.q = s->qidx; a.tags = s->dSpinUp; a.qc = s->qc;
        maxn = std::max(maxn, a.n);
    }
    if (e->ring.send(idx, pe->dTag, (size_t)J * sizeof(PumpTagArgs), e->stream)) return -1;
    HIPCHK(launch_tag_spin_up_ens(pe->dTag, J, maxn, e->stream));
    pe->launches++;
    for (mdqt_ctx* s : e->jobs) {
        s->spinUp.assign((size_t)(s->N > 0 ? s->N : 1), 0);
        HIPCHK(hipMemcpyAsync(s->spinUp.data(), s->dSpinUp, (size_t)s->nloc * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    for (mdqt_ctx* s : e->jobs) {
        int cnt = 0;
        for (int i = 0; i < s->nloc; ++i) cnt += s->spinUp[i];
        s->nSpinUp = cnt;
    }
    return 0;
}

// output() :799-935 (and, vaf >= 0, Zfunc(vaf) + printVAF) of every member: the velocity read-backs and the
// batched tagged distribution queued on the ensemble's stream, one synchronisation, then each member's host
// sums and files by output_pump's own code (pump_output_host, pump_vaf_host; Epotential() each member's call, or with option output_batch 1 the base
// ensemble's three batched launches under the same synchronisation)
int pump_output(mdqt_pump_ensemble* pe, int vaf) {
    mdqt_ensemble* e = pe->base;
    const int J = (int)e->jobs.size();
    char* slot = nullptr;
    int idx = 0;
    if (e->ring.take(&slot, &idx)) return -1;
    PumpKdeArgs* h = reinterpret_cast<PumpKdeArgs*>(slot);
    int maxN = 0;
    std::vector<std::vector<double>> Vs((size_t)J), Ps((size_t)J);
    for (int k = 0; k < J; ++k) {
        if (member_buffers(pe, k)) return -1;
        mdqt_ctx* s = e->jobs[k];
        PumpKdeArgs& a = h[k];
        memset(&a, 0, sizeof a);
        a.V = s->dV; a.tags = s->dSpinUp; a.N = s->N; a.S = s->S; a.bin0 = s->pumpBin0;
        a.part = s->dTkde + (size_t)3 * TKDE_BINS; a.out = s->dTkde;
        maxN = std::max(maxN, a.N);
        Vs[k].assign((size_t)3 * s->S, 0.);
        Ps[k].assign((size_t)3 * TKDE_BINS, 0.);
        HIPCHK(hipMemcpyAsync(Vs[k].data(), s->dV, Vs[k].size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    }
    if (e->ring.send(idx, pe->dKde, (size_t)J * sizeof(PumpKdeArgs), e->stream)) return -1;
    HIPCHK(launch_tagged_kde_ens(pe->dKde, J, maxN, e->stream));
    pe->launches += 2;
    for (int k = 0; k < J; ++k)
        HIPCHK(hipMemcpyAsync(Ps[k].data(), e->jobs[k]->dTkde, Ps[k].size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    // option output_batch 1: Epotential() of the members on the tile potential in the ensemble's three batched
    // launches (mdqt_ensemble_output.cpp), read back under the same synchronisation
    std::vector<int> batched;
    const double* rows = nullptr;
    if (e->output_batch && ens_epotential_queue(e, batched, &rows)) return -1;
    if (!batched.empty()) pe->launches += 3;
    HIPCHK(hipStreamSynchronize(e->stream));
    size_t q = 0;
    for (int k = 0; k < J; ++k) {
        mdqt_ctx* s = e->jobs[k];
        const int N = s->N, S = s->S;
        std::vector<double> V((size_t)3 * N);                    // [3][N], as mdqt_get_state gives it
        for (int c = 0; c < 3; ++c) std::copy_n(Vs[k].begin() + (size_t)c * S, N, V.begin() + (size_t)c * N);
        double epot = 0.;
        const bool have = q < batched.size() && batched[q] == k;
        if (have) epot = ens_epot_of(s, rows + 64 * q++);
        if (pump_output_host(s, V, Ps[k], nullptr, e->writer.get(), have ? &epot : nullptr)) return -1;
        if (vaf >= 0 && pump_vaf_host(s, V, vaf)) return -1;
    }
    return 0;
}

int pump_md_steps(mdqt_pump_ensemble* pe, int n) {
    const bool moving = pe->base->jobs[0]->t > 0;
    for (int k = 0; k < n; ++k) {
        // t stays: at t > 0 every step but the call's last takes the next one's leading drift along
        if (pump_step(pe, !moving || k == 0, moving && k + 1 < n)) return -1;
        for (mdqt_ctx* s : pe->base->jobs) s->c0++;
    }
    return 0;
}

}  // namespace

extern "C" void mdqt_pump_ensemble_destroy(mdqt_pump_ensemble* pe) {
    if (!pe) return;
    if (pe->base) {
        (void)hipSetDevice(pe->base->dev);
        if (pe->base->stream) (void)hipStreamSynchronize(pe->base->stream);
    }
    mdqt_ensemble_destroy(pe->base);
    delete pe;
}

extern "C" int mdqt_pump_ensemble_create(const mdqt_params* p, int njobs, mdqt_pump_ensemble** out) {
    if (!p || !out) return set_error("mdqt_pump_ensemble_create: NULL argument");
    *out = nullptr;
    std::unique_ptr<mdqt_pump_ensemble, void (*)(mdqt_pump_ensemble*)> pe(new (std::nothrow) mdqt_pump_ensemble(),
                                                                         mdqt_pump_ensemble_destroy);
    if (!pe) return set_error("mdqt_pump_ensemble_create: out of memory");
    if (ensemble_create(p, 1, njobs, &pe->base, "mdqt_pump_ensemble_create", true)) return -1;
    HIPCHK(hipSetDevice(pe->base->dev));
    if (pe->dStep[0].alloc((size_t)njobs) != hipSuccess || pe->dStep[1].alloc((size_t)njobs) != hipSuccess ||
        pe->dTag.alloc((size_t)njobs) != hipSuccess || pe->dKde.alloc((size_t)njobs) != hipSuccess)
        return set_error("mdqt_pump_ensemble_create: allocating the argument blocks of %d jobs failed", njobs);
    *out = pe.release();
    return 0;
}

// the members are the base ensemble's (its "qt_waves" picks an instance of the SpeedUp QT kernel: the pump
// kernels do not read it)
extern "C" int mdqt_pump_ensemble_size(const mdqt_pump_ensemble* pe) { return mdqt_ensemble_size(pe ? pe->base : nullptr); }

extern "C" mdqt_ctx* mdqt_pump_ensemble_job(mdqt_pump_ensemble* pe, int k) { return mdqt_ensemble_job(pe ? pe->base : nullptr, k); }

extern "C" int mdqt_pump_ensemble_set_option(mdqt_pump_ensemble* pe, const char* name, int value) {
    return mdqt_ensemble_set_option(pe ? pe->base : nullptr, name, value);
}

extern "C" int mdqt_pump_ensemble_init(mdqt_pump_ensemble* pe) {       // init() of every job
    if (!pe) return set_error("NULL ensemble");
    for (mdqt_ctx* s : pe->base->jobs) {
        if (mdqt_init(s)) return -1;
        s->spinUp.clear();
        s->nSpinUp = 0;
    }
    return 0;
}

extern "C" int mdqt_pump_ensemble_md_steps(mdqt_pump_ensemble* pe, int n) {   // n x (step(); c0++) of every job
    if (pump_check(pe, "mdqt_pump_ensemble_md_steps")) return -1;
    if (n < 0) return set_error("negative step count");
    HIPCHK(hipSetDevice(pe->base->dev));
    return pump_md_steps(pe, n);
}

extern "C" int mdqt_pump_ensemble_qsteps(mdqt_pump_ensemble* pe, int n) {     // n x qstep() of every job
    if (pump_check(pe, "mdqt_pump_ensemble_qsteps")) return -1;
    if (n < 0) return set_error("negative step count");
    HIPCHK(hipSetDevice(pe->base->dev));
    return pump_qsteps(pe, n);
}

extern "C" int mdqt_pump_ensemble_tag_spin_up(mdqt_pump_ensemble* pe) {       // measureSpinUps() of every job
    if (pump_check(pe, "mdqt_pump_ensemble_tag_spin_up")) return -1;
    HIPCHK(hipSetDevice(pe->base->dev));
    return pump_tag(pe);
}

extern "C" int mdqt_pump_ensemble_output(mdqt_pump_ensemble* pe) {            // output() of every job
    if (pump_check(pe, "mdqt_pump_ensemble_output")) return -1;
    HIPCHK(hipSetDevice(pe->base->dev));
    if (pump_output(pe, -1)) return -1;
    return flush_files(pe->base->jobs[0]);
}

extern "C" int mdqt_pump_ensemble_synchronize(mdqt_pump_ensemble* pe) {
    if (!pe) return set_error("NULL ensemble");
    return mdqt_ensemble_synchronize(pe->base);     // every member that raised the range flag is marked
}

extern "C" unsigned long long mdqt_pump_ensemble_launches(const mdqt_pump_ensemble* pe) {
    return pe && pe->base ? pe->launches + pe->base->force_launches : 0;
}

// main() :981-1076 for every member at once; the time loop itself is mdqt_run_pump's, pump_loop
// (mdqt_main_loops.hpp): the members are in lockstep, so member 0's t and c0 drive it
extern "C" int mdqt_pump_ensemble_run(mdqt_pump_ensemble* pe) {
    if (!pe) return set_error("NULL ensemble");
    mdqt_ensemble* e = pe->base;
    for (mdqt_ctx* s : e->jobs) {
        if (pump_setup_directories(s)) return -1;
        s->spinUp.clear();
        s->nSpinUp = 0;
        s->pumpBin0 = -2000;
    }
    const int recorded = e->jobs[0]->p.newRun == 1 ? 0 : 1;      // recordedSpinUps :81
    for (mdqt_ctx* s : e->jobs)                                  // :1036-1046
        if (recorded ? pump_read_conditions(s, s->p.c0) : mdqt_init(s)) return -1;
    if (pump_check(pe, "mdqt_pump_ensemble_run")) return -1;
    HIPCHK(hipSetDevice(e->dev));
    struct {                                                     // the loop's driver: one batched call over the members
        mdqt_pump_ensemble* pe;
        std::vector<mdqt_ctx*>& jobs;
        double t() const { return jobs[0]->t; }
        int c0() const { return jobs[0]->c0; }
        int qsteps(int n) { return pump_qsteps(pe, n); }         // qstep() x n :396-598
        int measure() {
            if (pump_tag(pe)) return -1;
            for (mdqt_ctx* s : jobs)
                if (pump_spin_ups_file(s)) return -1;
            return 0;
        }
        int output(int vaf) { return pump_output(pe, vaf); }
        int md_step(bool lead, bool fold) {
            if (pump_step(pe, lead, fold)) return -1;
            for (mdqt_ctx* s : jobs) s->c0++;
            return 0;
        }
        int idle() { for (mdqt_ctx* s : jobs) s->t += s->dtQ; return 0; }
        int fail(const char* what) { return set_error("mdqt_pump_ensemble_run: %s", what); }
    } d{pe, e->jobs};
    if (pump_loop(pump_schedule(e->jobs[0]), recorded, d)) return -1;
    if (flush_files(e->jobs[0])) return -1;                      // the shared pool: every member's files
    for (mdqt_ctx* s : e->jobs)
        if (pump_write_conditions(s, s->c0)) return -1;          // :1084
    return 0;
}

extern "C" int mdqt_pump_ensemble_enable_timing(mdqt_pump_ensemble* pe, int on) {
    if (!pe) return set_error("NULL ensemble");
    pe->kick_timer.reset();
    return mdqt_ensemble_enable_timing(pe->base, on);
}

// the batched kernels' own durations (their dispatch timestamps) since the last call: out[9] = force ms (sum),
// force launches, QT ms, QT launches, kick launch ms, kick launches, then the medians of the three (ms); resets
extern "C" int mdqt_pump_ensemble_kernel_times(mdqt_pump_ensemble* pe, double* out, int n) {
    if (!pe || !out) return set_error("mdqt_pump_ensemble_kernel_times: NULL argument");
    if (n < 9) return set_error("mdqt_pump_ensemble_kernel_times: need 9 doubles");
    double b[6];
    if (mdqt_ensemble_kernel_times(pe->base, b, 6)) return -1;
    double kick[5];
    if (pe->kick_timer.stats(kick)) return -1;
    out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; out[3] = b[3];
    out[4] = kick[0]; out[5] = kick[1];
    out[6] = b[4]; out[7] = b[5]; out[8] = kick[2];
    return 0;
}
