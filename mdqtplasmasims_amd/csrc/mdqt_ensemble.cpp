// mdqt_ensemble — J independent jobs of the SpeedUp program stepped by ONE force launch and ONE QT launch
// per MD step (include/mdqt.h, "ensembles").  It works on mdqt_ctx's internals (mdqt_ctx.hpp) and on
// the argument helpers the single-job path uses (mdqt_step.cpp: n3_force_args, substep_args), so a member's launch arguments are the ones its own mdqt_forces / mdqt_substeps
// would pass — which is the whole bit-identity argument: the batched kernels run the single-job
// kernels' bodies on those arguments (mdqt_forces.hip k_pairs_n3_ens, mdqt_ensemble_qt.hip LANE_ENS_KERNELS).
//
// The reference runs this program as a Slurm array of 99 independent jobs (exampleSlurmFile.slurm:3,
// srand48(time + job), SpeedUp:1219); one job of N0 = 3500 does not fill an MI355X.
//
// Argument hand-off.  The force blocks (N3Args) do not change from step to step: they are uploaded
// when they differ from what the device holds (after init, a resize, an option, the range guard).  The
// QT blocks (SubstepArgs: t[], q0, nseg change every launch) are built in a slot of the pinned ring
// (mdqt_batch.hpp: PinRing, 8 slots) and copied in stream order before the launches that read them; a slot
// is reused after the event behind its copy has completed.  mdqt_ensemble_substeps and mdqt_ensemble_run copy one launch's blocks just
// before it; mdqt_ensemble_md_steps builds the blocks of up to 64 MD steps ahead and copies them at once
// (ens_md_steps has the reason and the numbers).  mdqt_ensemble_run: mdqt_run's time loop (mdqt_main_loops.hpp) on a batched driver.

#include <algorithm>

#include "mdqt_ensemble.hpp"
#include "mdqt_qtfast.hpp"   // sweep_choice_differs (the host part)
#include "mdqt_sweep.hpp"

using namespace mdqt;

namespace {
constexpr int kRingSlots = 8;   // launches (or md_steps' batches of launches) whose blocks may be on their way at once
}  // namespace

// Every batched call: the members still are what the batched kernels cover, and still in lockstep — t
// (bitwise), the qstep index, c0 and, for the pump programs, the tagged / untagged flag.  Nothing is
// launched before this has passed.
// The pending-force state is NOT compared: it is per job by design (a one-tile job never has pending
// slots; mdqt_get_state on a member settles that member's) and each QT block takes its own nseg.
int mdqt::ens_check(const mdqt_ensemble* e, const char* what, bool pump) {
    if (!e) return set_error("%s: NULL ensemble", what);
    const mdqt_ctx* a = e->jobs[0];
    for (size_t k = 0; k < e->jobs.size(); ++k) {
        const mdqt_ctx* s = e->jobs[k];
        if (s->stream != e->stream) return set_error("%s: job index %zu was moved to another stream", what, k);
        if (s->overlap_opt || s->fused_opt)
            return set_error("%s: job index %zu has the option overlap / fused_step set (one system per launch)", what, k);
        if (s->qt_math != 2) return set_error("%s: job index %zu has qt_math %d (the batched QT kernels are qt_math 2)", what, k, s->qt_math);
        if (s->substep_mode == 1) return set_error("%s: job index %zu has substep_kernel 1 (the batched QT kernels are the lane kernels)", what, k);
        if (s->N < 1) return set_error("%s: job index %zu has no ions (the ensemble's init or mdqt_set_state first)", what, k);
        if (s->use_n3b || s->N > 65536)
            return set_error("%s: job index %zu has N = %d: beyond the Newton-3 tile scheme (N <= 65,536)", what, k, s->N);
        if (s->force_arrive || s->sub_stream || !s->local.empty()) return set_error("%s: job index %zu is part of another scheme", what, k);
        if (memcmp(&s->t, &a->t, sizeof(double)) || s->qidx != a->qidx || s->c0 != a->c0 || (pump && tagged(s) != tagged(a))) {
            char tags[32] = "";
            if (pump) snprintf(tags, sizeof tags, ", tagged %d / %d", (int)tagged(s), (int)tagged(a));
            return set_error("%s: job index %zu is out of step with job index 0 (t %.17g / %.17g, qstep %llu / %llu, c0 %d / %d%s): "
                             "a member stepped on its own ends the ensemble's stepping",
                             what, k, s->t, a->t, (unsigned long long)s->qidx, (unsigned long long)a->qidx, s->c0, a->c0, tags);
        }
    }
    return 0;
}

namespace {

// The force blocks of the members on the Newton-3 tiles (packed, in job order), uploaded when they differ
// from what the device holds
struct EnsForce {
    std::vector<N3Args> h;
    int maxp = 0, variant = -1;
    bool guard = false;
};

int ens_force_blocks(mdqt_ensemble* e, EnsForce& f) {
    const int J = (int)e->jobs.size();
    f.h.reserve(J);
    for (int k = 0; k < J; ++k) {
        mdqt_ctx* s = e->jobs[k];
        if (!s->use_n3) continue;
        N3Args a;
        if (n3_force_args(s, a)) return -1;
        if (f.variant >= 0 && f.variant != s->force_variant) return set_error("mdqt_ensemble_forces: job index %d has another force_kernel", k);
        f.variant = s->force_variant;
        f.guard = f.guard || a.guard;
        f.maxp = std::max(f.maxp, a.npairs);
        f.h.push_back(a);
    }
    return e->ring.send_if_changed(f.h, e->force_held, e->dForce, e->stream);
}

int ens_force_launch(mdqt_ensemble* e, const EnsForce& f) {
    if (f.h.empty()) return 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e->timing && e->timers[0].take(&e0, &e1)) return -1;
    HIPCHK(launch_forces_n3_ens(e->dForce, (int)f.h.size(), f.maxp, f.variant, f.guard, e->stream, e0, e1));
    e->force_launches++;
    return 0;
}

}  // namespace

// forces() of every member: one launch over the members on the Newton-3 tiles; a member below 128 ions
// (owner-computes rows by default, as on its own) gets its own small launch
int mdqt::ens_forces(mdqt_ensemble* e) {
    EnsForce f;
    if (ens_force_blocks(e, f) || ens_force_launch(e, f)) return -1;
    size_t q = 0;
    for (mdqt_ctx* s : e->jobs) {
        if (s->use_n3) n3_forces_pending(s, f.h[q++]);
        else if (mdqt_forces(s)) return -1;
        else e->force_launches++;
    }
    return 0;
}

// run_substeps(s, n, do_step, 1, 1) of every member: chunks of at most MAXSUB, one launch per chunk
int mdqt::ens_qt_chunks(mdqt_ensemble* e, int n, int do_step, const EnsQtLaunch& launch) {
    const int J = (int)e->jobs.size();
    const int do_qt = e->jobs[0]->p.qt_enabled ? 1 : 0;
    while (n > 0) {
        const int m = n < MAXSUB ? n : MAXSUB;
        char* slot = nullptr;
        int idx = 0;
        if (e->ring.take(&slot, &idx)) return -1;
        SubstepArgs* h = reinterpret_cast<SubstepArgs*>(slot);
        double t = 0.;
        int maxn = 0;
        for (int k = 0; k < J; ++k) {
            mdqt_ctx* s = e->jobs[k];
            t = substep_args(s, h[k], m, do_step, do_qt, 1);
            maxn = std::max(maxn, h[k].n);
        }
        if (e->ring.send(idx, e->dSub, (size_t)J * sizeof(SubstepArgs), e->stream)) return -1;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (e->timing && e->timers[1].take(&e0, &e1)) return -1;
        int inst = 0;
        if (launch(h, maxn, e0, e1, &inst)) return -1;
        for (int k = 0; k < J; ++k) {
            mdqt_ctx* s = e->jobs[k];
            s->f_pending = false;
            s->last_qt_kernel = inst;
            s->last_qt_nseg = h[k].nseg;
            s->t = t;
            s->qidx += (uint64_t)m;
        }
        n -= m;
    }
    return 0;
}

// check_range_flag of every member with one synchronisation (drain), or, inside the MD-step loops, the
// members' words as they stand (host loads: what completed launches raised)
int mdqt::ens_range_flags(mdqt_ensemble* e, bool drain) {
    const int J = (int)e->jobs.size();
    if (drain) HIPCHK(hipStreamSynchronize(e->stream));
    int first = -1;
    for (int k = 0; k < J; ++k)                    // each member's own host-mapped word (mdqt_ctx::hFlags)
        if (e->jobs[k]->hFlags[0] && !e->jobs[k]->guard) {
            e->jobs[k]->guard = true;
            if (first < 0) first = k;
        }
    return first >= 0 ? range_flag_error(first) : 0;
}

namespace {

// A sweep ensemble's QT launch serves members with different parameters by ONE kernel instance, so before a
// call changes anything the members' blocks of its first launch (m substeps) must agree on what the choice of
// the instance reads (launch_substeps_r_sweep checks every launch again).  mdqt_ensemble_create_sweep's
// fracOfSig rule keeps expdet_zero in step; an option set on one member only (qt_im01) ends up here.
int sweep_check(mdqt_ensemble* e, int m, const char* what) {
    const int J = (int)e->jobs.size();
    const int do_qt = e->jobs[0]->p.qt_enabled ? 1 : 0;
    if (m <= 0) return 0;
    SubstepArgs a0, a;
    substep_args(e->jobs[0], a0, m, 1, do_qt, 1);
    for (int k = 1; k < J; ++k) {
        substep_args(e->jobs[k], a, m, 1, do_qt, 1);
        if (const char* field = sweep_choice_differs(a0, a))
            return set_error("%s: job index %d differs from job index 0 in %s: one QT launch (one kernel instance) serves every "
                             "member of a sweep ensemble; nothing was launched", what, k, field);
    }
    return 0;
}

// one sweep QT launch over the blocks at `dev` (host copies: h)
int sweep_launch(mdqt_ensemble* e, const SubstepArgs* dev, const SubstepArgs* h, int maxn, hipEvent_t e0, hipEvent_t e1, int* inst) {
    int differs = -1;
    const hipError_t r = launch_substeps_r_sweep(dev, h, (int)e->jobs.size(), maxn, e->dTabs, e->dPoint, e->qt_waves, e->stream,
                                                 e0, e1, inst, &differs);
    if (differs >= 0)
        return set_error("the sweep ensemble's QT launch: job index %d differs from job index 0 in %s: one kernel instance "
                         "serves every member; the launch was not issued", differs, sweep_choice_differs(h[0], h[differs]));
    HIPCHK(r);
    return 0;
}

// n x (step(); qstep()) of every member
int ens_substeps(mdqt_ensemble* e, int n) {
    if (e->sweep) {
        if (sweep_check(e, std::min(n, MAXSUB), "mdqt_ensemble_substeps")) return -1;
        return ens_qt_chunks(e, n, 1, [e](const SubstepArgs* h, int maxn, hipEvent_t e0, hipEvent_t e1, int* inst) {
            return sweep_launch(e, e->dSub, h, maxn, e0, e1, inst);
        });
    }
    return ens_qt_chunks(e, n, 1, [e](const SubstepArgs* h, int maxn, hipEvent_t e0, hipEvent_t e1, int* inst) {
        HIPCHK(launch_substeps_r_ens(e->dSub, h[0], (int)e->jobs.size(), maxn, e->jobs[0]->dFTab, e->qt_waves, e->stream, e0, e1, inst));
        return 0;
    });
}

// n MD steps without the argument hand-off inside them.  A copy between two launches costs more than
// its bytes (the launch before it ends in a cache write-back for the copy engine: measured 28 us per MD
// step at 8 jobs of N0 = 3500, docs/PROGRAMS.md), and everything in the QT blocks is known in advance: t
// and the qstep index advance by fixed amounts, nseg is each job's slot count after its force launch.  So
// the blocks of up to 64 MD steps are built at once — by the same helpers, on the members' host state
// stepped forward exactly as the launches will leave it — and uploaded in one copy; the launches then
// follow back to back.  Members off the Newton-3 tiles (their own force launch sets their pending state
// when it is issued) take the step-by-step route.
int ens_md_steps(mdqt_ensemble* e, int n) {
    const int J = (int)e->jobs.size();
    const int ratio = e->jobs[0]->ratio, per_step = (ratio + MAXSUB - 1) / MAXSUB;
    const int do_qt = e->jobs[0]->p.qt_enabled ? 1 : 0;
    if (e->sweep && n > 0 && sweep_check(e, std::min(ratio, MAXSUB), "mdqt_ensemble_md_steps")) return -1;   // before the forces
    bool tiles = true;
    for (const mdqt_ctx* s : e->jobs) tiles = tiles && s->use_n3;
    const int ahead = tiles ? std::min(64, e->sub_blocks / (J * per_step)) : 0;
    if (ahead < 2) {
        for (int k = 0; k < n; ++k) {
            if (ens_range_flags(e, false)) return -1;
            if (ens_forces(e)) return -1;
            for (mdqt_ctx* s : e->jobs) s->c0++;
            if (ens_substeps(e, ratio)) return -1;
        }
        return 0;
    }
    for (int k = 0; k < n;) {
        if (ens_range_flags(e, false)) return -1;
        const int b = std::min(std::min(n - k, ahead), 64 - k % 64);
        EnsForce f;
        if (ens_force_blocks(e, f)) return -1;
        char* slot = nullptr;
        int idx = 0;
        if (e->ring.take(&slot, &idx)) return -1;
        SubstepArgs* h = reinterpret_cast<SubstepArgs*>(slot);
        int nl = 0, maxn = 0;
        for (int st = 0; st < b; ++st) {
            for (int j = 0; j < J; ++j) {
                n3_forces_pending(e->jobs[j], f.h[j]);
                e->jobs[j]->c0++;
            }
            for (int rem = ratio; rem > 0; ++nl) {
                const int m = rem < MAXSUB ? rem : MAXSUB;
                for (int j = 0; j < J; ++j) {
                    mdqt_ctx* s = e->jobs[j];
                    SubstepArgs& a = h[(size_t)nl * J + j];
                    s->t = substep_args(s, a, m, 1, do_qt, 1);
                    s->qidx += (uint64_t)m;
                    s->f_pending = false;
                    maxn = std::max(maxn, a.n);
                }
                rem -= m;
            }
        }
        if (e->ring.send(idx, e->dSub, (size_t)nl * J * sizeof(SubstepArgs), e->stream)) return -1;
        int inst = 0;
        for (int st = 0, l = 0; st < b; ++st) {
            if (ens_force_launch(e, f)) return -1;
            for (int c = 0; c < per_step; ++c, ++l) {
                hipEvent_t e0 = nullptr, e1 = nullptr;
                if (e->timing && e->timers[1].take(&e0, &e1)) return -1;
                if (e->sweep) {
                    if (sweep_launch(e, e->dSub + (size_t)l * J, h + (size_t)l * J, maxn, e0, e1, &inst)) return -1;
                } else {
                    HIPCHK(launch_substeps_r_ens(e->dSub + (size_t)l * J, h[(size_t)l * J], J, maxn, e->jobs[0]->dFTab,
                                                 e->qt_waves, e->stream, e0, e1, &inst));
                }
            }
        }
        for (int j = 0; j < J; ++j) {
            e->jobs[j]->last_qt_kernel = inst;
            e->jobs[j]->last_qt_nseg = h[(size_t)(nl - 1) * J + j].nseg;
        }
        k += b;
    }
    return 0;
}

}  // namespace

extern "C" int mdqt_ensemble_job_params(const mdqt_params* base, int k, mdqt_params* out) {
    if (!base || !out) return set_error("mdqt_ensemble_job_params: NULL argument");
    if (k < 0 || k >= kEnsembleMaxJobs) return set_error("mdqt_ensemble_job_params: job index %d outside [0, %d)", k, kEnsembleMaxJobs);
    mdqt_params p = *base;
    p.job = base->job + (uint32_t)k;               // the array index, SpeedUp:1145
    p.seed = base->seed + (uint32_t)k;             // srand48(time + job), SpeedUp:1219
    *out = p;
    return 0;
}

namespace {

// what mdqt_ensemble_create refuses in the parameters themselves (before any context or HIP call)
int refuse_params(const mdqt_params* p, const char* what, bool pump) {
    if (p->world_size != 1) return set_error("%s: world_size must be 1 (an ensemble's jobs are whole systems on one device)", what);
    if (p->rng_mode != 1)
        return set_error("%s: rng_mode must be 1 (Philox): the drand48 order needs one substep per launch "
                         "and a resolve kernel per job", what);
    if (!pump && p->qt_model != 0)
        return set_error("%s: qt_model must be 0 (the SpeedUp program; the pump programs have mdqt_pump_ensemble_create)", what);
    if (pump && (p->qt_model < 1 || p->qt_model > 3))
        return set_error("%s: qt_model must be 1, 2 or 3 (the optical-pumping programs)", what);
    return 0;
}

// The swept fields (mdqt_sweep.hpp; mdqt_setup_directories' name holds each x 100), and the name of the first
// other field in which b differs from a (nullptr: none).  Field by field: the struct has padding.
const SweepField<mdqt_params> kSweep[] = {{"detuning", &mdqt_params::detuning, 100},
                                          {"detuningDP", &mdqt_params::detuningDP, 100},
                                          {"Om", &mdqt_params::Om, 100},
                                          {"OmDP", &mdqt_params::OmDP, 100},
                                          {"fracOfSig", &mdqt_params::fracOfSig, 100}};
const char* fixed_field_differs(const mdqt_params& a, const mdqt_params& b) {
#define FIXED(name) if (memcmp(&a.name, &b.name, sizeof a.name)) return #name;
    FIXED(Ge) FIXED(tmax) FIXED(density) FIXED(sig0) FIXED(Te) FIXED(N0) FIXED(newRun) FIXED(c0) FIXED(sampleFreq)
    FIXED(reNormalizewvFns) FIXED(qt_enabled) FIXED(rng_mode) FIXED(seed) FIXED(job) FIXED(device) FIXED(world_size)
    FIXED(rank) FIXED(force_segments) FIXED(qt_model) FIXED(tpumpreal) FIXED(tstartV0)
#undef FIXED
    if (strncmp(a.saveDirectory, b.saveDirectory, sizeof a.saveDirectory)) return "saveDirectory";
    return nullptr;
}

// mdqt_ensemble_create_sweep's refusals: host arithmetic only
int sweep_validate(const mdqt_params* pts, int npoints, int njobs, const char* what) {
    if (!pts) return set_error("%s: NULL argument", what);
    if (npoints < 1) return set_error("%s: npoints must be >= 1", what);
    if (njobs < 1) return set_error("%s: njobs must be >= 1", what);
    if ((long long)npoints * njobs > kEnsembleMaxJobs)
        return set_error("%s: npoints x njobs = %lld members, more than %d", what, (long long)npoints * njobs, kEnsembleMaxJobs);
    if (refuse_params(pts, what, false)) return -1;
    for (int q = 1; q < npoints; ++q) {
        if (sweep_refuse_fixed(kSweep, q, fixed_field_differs(pts[0], pts[q]),
                               "the others fix the box, the substep ratio, t and the outputs of every member", what))
            return -1;
        if ((pts[q].fracOfSig == 0.) != (pts[0].fracOfSig == 0.))
            return set_error("%s: point %d has fracOfSig %g and point 0 has %g: a point with fracOfSig == 0 runs the QT kernel "
                             "instance without the expansion detuning, one with fracOfSig != 0 cannot, and one launch is one "
                             "instance (splitting a launch by instance is not supported: run the two groups as two ensembles)",
                             what, q, pts[q].fracOfSig, pts[0].fracOfSig);
    }
    return sweep_refuse_same(kSweep, pts, npoints, what);
}

// the points' tables and the members' point indices, uploaded when they differ from what the device holds
int sweep_upload(mdqt_ensemble* e) {
    const int J = (int)e->jobs.size(), R = J / e->npoints;
    std::vector<FastTab> tabs((size_t)e->npoints);
    std::vector<int> point((size_t)J);
    for (int q = 0; q < e->npoints; ++q) tabs[(size_t)q] = e->jobs[(size_t)q * R]->ftabL;
    for (int k = 0; k < J; ++k) point[(size_t)k] = k / R;
    return e->ring.send_if_changed(tabs, e->tabs_held, e->dTabs, e->stream) ||
           e->ring.send_if_changed(point, e->point_held, e->dPoint, e->stream);
}

}  // namespace

extern "C" void mdqt_ensemble_destroy(mdqt_ensemble* e) {
    if (!e) return;
    (void)hipSetDevice(e->dev);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->writer) (void)e->writer->flush(nullptr);
    for (size_t k = e->jobs.size(); k-- > 0;) {        // jobs[0] owns the shared stream: last
        e->jobs[k]->shared_writer = nullptr;
        mdqt_destroy(e->jobs[k]);
    }
    delete e;
}

// mdqt_ensemble_create, and the same members and machinery for mdqt_pump_ensemble_create (pump: qt_model 1-3)
// The members are the points' replicas, point-major (one point: the jobs of mdqt_ensemble_create); sweep: the
// caller has validated the points (sweep_validate).
int mdqt::ensemble_create(const mdqt_params* p, int npoints, int replicas, mdqt_ensemble** out, const char* what, bool pump,
                          bool sweep) {
    if (!p || !out) return set_error("%s: NULL argument", what);
    *out = nullptr;
    if (replicas < 1 || replicas > kEnsembleMaxJobs) return set_error("%s: njobs must be 1 .. %d", what, kEnsembleMaxJobs);
    if (npoints < 1 || (long long)npoints * replicas > kEnsembleMaxJobs)
        return set_error("%s: npoints x njobs must be 1 .. %d", what, kEnsembleMaxJobs);
    if (refuse_params(p, what, pump)) return -1;
    const int njobs = npoints * replicas;
    std::unique_ptr<mdqt_ensemble, void (*)(mdqt_ensemble*)> e(new (std::nothrow) mdqt_ensemble(), mdqt_ensemble_destroy);
    if (!e) return set_error("%s: out of memory", what);
    e->npoints = npoints;
    e->sweep = sweep;
    e->pump = pump;
    try {
        e->jobs.reserve((size_t)njobs);
        e->writer.reset(new FileWriter(std::min(16, 4 * njobs)));
    } catch (const std::exception& x) {
        return set_error("%s: %s", what, x.what());
    }
    for (int k = 0; k < njobs; ++k) {
        mdqt_params pk;
        mdqt_ctx* s = nullptr;
        if (mdqt_ensemble_job_params(p + k / replicas, k % replicas, &pk) || mdqt_create(&pk, &s)) return -1;
        e->jobs.push_back(s);
        s->shared_writer = e->writer.get();
        if (k == 0) { e->dev = s->dev; e->stream = s->own; }
        if (s->qt_math != 2) return set_error("%s: qt_math must be 2", what);
        if (s->overlap_opt || s->fused_opt) return set_error("%s: the options overlap / fused_step are one system per launch", what);
        mdqt_set_stream(s, (void*)e->stream);
    }
    HIPCHK(hipSetDevice(e->dev));
    e->sub_blocks = std::max(njobs, 1024);
    size_t slot_bytes = std::max((size_t)e->sub_blocks * sizeof(SubstepArgs), (size_t)njobs * sizeof(N3Args));
    if (sweep) slot_bytes = std::max(slot_bytes, (size_t)npoints * sizeof(FastTab));   // (the point indices are smaller)
    if (e->dForce.alloc((size_t)njobs) != hipSuccess || e->dSub.alloc((size_t)e->sub_blocks) != hipSuccess)
        return set_error("%s: allocating the argument blocks of %d jobs failed", what, njobs);
    if (e->ring.create(slot_bytes, kRingSlots, hipEventDisableTiming | hipEventDisableSystemFence)) return -1;
    if (sweep) {
        if (e->dTabs.alloc((size_t)npoints) != hipSuccess || e->dPoint.alloc((size_t)njobs) != hipSuccess)
            return set_error("%s: allocating the tables of %d points failed", what, npoints);
        if (sweep_upload(e.get())) return -1;
    }
    *out = e.release();
    return 0;
}

extern "C" int mdqt_ensemble_create(const mdqt_params* p, int njobs, mdqt_ensemble** out) {
    return ensemble_create(p, 1, njobs, out, "mdqt_ensemble_create", false);
}

// member k of a sweep: point k / njobs, replica k % njobs (job + r, seed + r as mdqt_ensemble_job_params)
extern "C" int mdqt_ensemble_sweep_params(const mdqt_params* points, int npoints, int njobs, int k, mdqt_params* out) {
    if (!points || !out) return set_error("mdqt_ensemble_sweep_params: NULL argument");
    if (sweep_validate(points, npoints, njobs, "mdqt_ensemble_sweep_params")) return -1;
    int q, r;
    if (sweep_member(npoints, njobs, k, "job", "mdqt_ensemble_sweep_params", &q, &r)) return -1;
    return mdqt_ensemble_job_params(points + q, r, out);
}

extern "C" int mdqt_ensemble_create_sweep(const mdqt_params* points, int npoints, int njobs, mdqt_ensemble** out) {
    if (!points || !out) return set_error("mdqt_ensemble_create_sweep: NULL argument");
    *out = nullptr;
    if (sweep_validate(points, npoints, njobs, "mdqt_ensemble_create_sweep")) return -1;
    return ensemble_create(points, npoints, njobs, out, "mdqt_ensemble_create_sweep", false, true);
}

extern "C" int mdqt_ensemble_points(const mdqt_ensemble* e) { return e ? e->npoints : -1; }

extern "C" int mdqt_ensemble_size(const mdqt_ensemble* e) { return e ? (int)e->jobs.size() : -1; }

extern "C" mdqt_ctx* mdqt_ensemble_job(mdqt_ensemble* e, int k) {
    if (!e || k < 0 || k >= (int)e->jobs.size()) {
        set_error("mdqt_ensemble_job: job index %d outside the ensemble", k);
        return nullptr;
    }
    return e->jobs[(size_t)k];
}

extern "C" int mdqt_ensemble_set_option(mdqt_ensemble* e, const char* name, int value) {
    if (!e || !name) return set_error("mdqt_ensemble_set_option: NULL argument");
    if (!strcmp(name, "qt_waves")) {
        if (value != 0 && value != 3) return set_error("qt_waves must be 0 (the single-job kernel's register budget) or 3");
        e->qt_waves = value;
        return 0;
    }
    if (!strcmp(name, "output_batch")) {
        if (value != 0 && value != 1) return set_error("output_batch must be 0 (output() member by member) or 1 (one batched pass)");
        e->output_batch = value;
        return 0;
    }
    if (!strcmp(name, "pool") || !strcmp(name, "member_files")) {    // the ensemble's own: never forwarded to the members
        if (e->pump) return set_error("%s is an option of the SpeedUp ensemble: the pump programs' output() has no pooled pass", name);
        if (value != 0 && value != 1)
            return set_error(name[0] == 'p' ? "pool must be 0 (the members' files only) or 1 (also each point's pooled files)"
                                            : "member_files must be 1 (the members' output files) or 0 (the pooled files only)");
        (name[0] == 'p' ? e->pool : e->member_files) = value;
        return 0;
    }
    for (mdqt_ctx* s : e->jobs)
        if (mdqt_set_option(s, name, value)) return -1;
    if (e->sweep) {                                 // an option may rebuild the members' tables: the points' copies follow
        HIPCHK(hipSetDevice(e->dev));
        if (sweep_upload(e)) return -1;
    }
    return 0;
}

extern "C" int mdqt_ensemble_init(mdqt_ensemble* e) {             // init() of every job, SpeedUp:289-348
    if (!e) return set_error("NULL ensemble");
    for (mdqt_ctx* s : e->jobs)                     // one after the other: a job's sampling already takes up to 16 threads
        if (mdqt_init(s)) return -1;
    return 0;
}

extern "C" int mdqt_ensemble_forces(mdqt_ensemble* e) {           // forces() of every job, SpeedUp:192-236
    if (ens_check(e, "mdqt_ensemble_forces")) return -1;
    HIPCHK(hipSetDevice(e->dev));
    return ens_forces(e);
}

extern "C" int mdqt_ensemble_substeps(mdqt_ensemble* e, int n) {  // n x (step(); qstep()), SpeedUp:1376-1377
    if (ens_check(e, "mdqt_ensemble_substeps")) return -1;
    if (n < 0) return set_error("negative substep count");
    HIPCHK(hipSetDevice(e->dev));
    return ens_substeps(e, n);
}

extern "C" int mdqt_ensemble_md_steps(mdqt_ensemble* e, int n) {  // mdqt_md_steps' plain branch for every job
    if (ens_check(e, "mdqt_ensemble_md_steps")) return -1;
    HIPCHK(hipSetDevice(e->dev));
    return ens_md_steps(e, n);
}

extern "C" int mdqt_ensemble_synchronize(mdqt_ensemble* e) {
    if (!e) return set_error("NULL ensemble");
    HIPCHK(hipSetDevice(e->dev));
    return ens_range_flags(e);
}

// main() (SpeedUp:1139-1383) for every job at once; the time loop itself is mdqt_run's, speedup_loop
// (mdqt_main_loops.hpp): the members are in lockstep, so job 0's t and c0 drive it
extern "C" int mdqt_ensemble_run(mdqt_ensemble* e) {
    if (!e) return set_error("NULL ensemble");
    for (mdqt_ctx* s : e->jobs)
        if (mdqt_setup_directories(s)) return -1;
    const bool fresh = e->jobs[0]->p.newRun == 1;
    for (mdqt_ctx* s : e->jobs)                         // one after the other, as mdqt_ensemble_init
        if (fresh ? mdqt_init(s) : mdqt_read_conditions(s, s->p.c0)) return -1;
    if (ens_check(e, "mdqt_ensemble_run")) return -1;
    if (e->sweep && sweep_check(e, std::min(e->jobs[0]->ratio, MAXSUB), "mdqt_ensemble_run")) return -1;
    if (!e->pool && !e->member_files) return set_error("mdqt_ensemble_run: member_files 0 with pool 0 would write nothing: set pool 1");
    if (e->pool && ens_pool_check(e, "mdqt_ensemble_run with pool 1")) return -1;      // before the first step, not at the first output
    HIPCHK(hipSetDevice(e->dev));
    struct {                                            // the loop's driver: one batched call over the members
        mdqt_ensemble* e;
        double t() const { return e->jobs[0]->t; }
        int c0() const { return e->jobs[0]->c0; }
        int output() { return ens_output(e); }          // one device pass and synchronisation (option output_batch)
        bool may_fuse_interval() { return false; }      // k_md_step is one system per launch
        int start_interval(bool) {
            if (ens_range_flags(e, false) || ens_forces(e)) return -1;
            for (mdqt_ctx* s : e->jobs) s->c0++;
            return 0;
        }
        int substeps(int n) { return ens_substeps(e, n); }
    } d{e};
    if (speedup_loop(speedup_schedule(e->jobs[0]), d)) return -1;
    for (mdqt_ctx* s : e->jobs)
        if (write_conditions_async(s, s->c0)) return -1;                               // :1381
    return flush_files(e->jobs[0]);                     // the shared pool: every member's files
}

extern "C" int mdqt_ensemble_enable_timing(mdqt_ensemble* e, int on) {
    if (!e) return set_error("NULL ensemble");
    e->timing = on > 0;
    for (LaunchTimer& t : e->timers) t.reset();
    for (LaunchTimer& t : e->obs_timers) t.reset();
    return 0;
}

// the two batched kernels' own durations (their dispatch timestamps) since the last call: out[6] = force
// ms (sum), force launches, QT ms (sum), QT launches, median force launch (ms), median QT launch (ms); with
// n >= 12 also the batched output's potential and KDE launches: out[6..11] = potential ms (sum), launches, KDE
// ms (sum), launches, median potential launch (ms), median KDE launch (ms); with n >= 18 also the pooled pass's two
// launches (k_popv_ens, k_popv_pool) in the same layout: out[12..17]; resets
extern "C" int mdqt_ensemble_kernel_times(mdqt_ensemble* e, double* out, int n) {
    if (!e || !out) return set_error("mdqt_ensemble_kernel_times: NULL argument");
    if (n < 6) return set_error("mdqt_ensemble_kernel_times: need 6 doubles");
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int k = 0; k < 2; ++k) {
        double v[5];
        if (e->timers[k].stats(v)) return -1;
        out[2 * k] = v[0];
        out[2 * k + 1] = v[1];
        out[4 + k] = v[2];
    }
    for (int k = 0; k < 4; ++k) {                       // 0, 1: out[6..11]; the pooled pass's 2, 3: out[12..17]
        double v[5];
        if (e->obs_timers[k].stats(v)) return -1;
        const int at = k < 2 ? 6 : 12, j = k % 2;
        if (n < at + 6) continue;
        out[at + 2 * j] = v[0];
        out[at + 1 + 2 * j] = v[1];
        out[at + 4 + j] = v[2];
    }
    return 0;
}
