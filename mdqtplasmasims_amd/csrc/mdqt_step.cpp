// The per-step hot path of the host engine: the range flags, forces() on the three schemes, the substep
// launches, the overlapped and fused MD steps, mdqt_md_steps, and the stateless pair kernels.

#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include <rccl/rccl.h>

#include "mdqt_ctx.hpp"

using namespace mdqt;

// The substep kernels raise hFlags[0] if a position leaves [-L/8, 9L/8] (an ion moving more than
// L/8 in half a substep: not a physical run).  The word lives in host-pinned memory the kernels
// store to directly, so reading it is a host load: poll_flags is called before every MD step of
// mdqt_md_steps' loops and drains nothing.  A store is certain to be visible once its kernel has
// completed, so inside a loop the poll sees what completed launches raised and lags the host's
// issue point by the launch-queue depth; check_range_flag, called where the host has synchronised
// with the stream anyway (mdqt_synchronize, the state read-backs), drains the stream first and so
// reports every excursion no later than the next host synchronisation.  From then on every pair
// is range-checked, and the call reports the event as an error.
static int poll_flags(mdqt_ctx* s) {
    if (s->hFlags[1]) return set_error("overlapped MD step: a QT launch timed out waiting for its force launch");
    if (s->hFlags[0] && !s->guard) {
        s->guard = true;
        return range_flag_error(-1);
    }
    return 0;
}
// ... and its error, for one context (job < 0) or the first member of an ensemble that raised its word
int mdqt::range_flag_error(int job) {
    char who[32] = "";
    if (job >= 0) snprintf(who, sizeof who, "job index %d: ", job);
    return set_error("%spositions left [-L/8, 9L/8] during the run (ion displacement > L/8 per half "
                     "substep); pair range checks are now on, but forces since the last sync used "
                     "the in-box minimum image", who);
}
int mdqt::check_range_flag(mdqt_ctx* s) {
    if (hipStreamSynchronize(s->stream) != hipSuccess) return set_error("reading the position-range flag failed");
    if (poll_flags(s)) return -1;
    return tail_check(s);
}
// mdqt_md_steps' loops, before MD step k: the flags every step (host loads); the Newton-3 block
// scheme's measured tail sums (a read-back: those MD steps take milliseconds) every 64 steps
static int loop_check(mdqt_ctx* s, int k) {
    if (poll_flags(s)) return -1;
    return (k > 0 && k % 64 == 0) ? tail_check(s) : 0;
}

static double expDetuning_of(const mdqt_params* p, double t) {   // :447
    return 0.0126 * p->fracOfSig * p->Te * t /
           (sqrt(p->density) * p->sig0 * sqrt(1 + 0.00014314 * t * t * p->Te / (p->density * p->sig0 * p->sig0)));
}

// forces() on the Newton-3 tiles: the launch's argument block (mdqt_forces, md_step_fused with the plain
// table, and the ensemble's batched launch: one construction, so they cannot drift apart)
int mdqt::n3_force_args(mdqt_ctx* s, N3Args& a, bool plain_table) {
    a = N3Args{};                // variant 2 (MCMD's exact pair set, rc2) is not used here
    if (s->force_variant > 1) return set_error("mdqt_forces: force_kernel must be 0 or 1");
    // one tile (N <= 64): its one slot has F's [3][S] layout, so the kernel writes F itself and
    // nothing is pending (the substep kernels read F when nseg == 1)
    const bool one_slot = s->nslots == 1 && !plain_table;
    // the split table (ensure_aux) unless the MD steps count tile arrivals (options overlap, fused_step:
    // then every force call of the context takes the plain table)
    const bool split = s->nsplit > 0 && !s->force_arrive && !one_slot && !s->overlap_opt && !s->fused_opt && !plain_table;
    a.R = s->dR; a.P = one_slot ? s->dF : s->dFpart; a.pairs = split ? s->dPairs + s->npairs : s->dPairs;
    a.N = s->N; a.S = s->S; a.ntiles = (s->N + 63) / 64; a.npairs = split ? s->nsplit_wg : s->npairs;
    ForceArgs c = force_args(s, nullptr);
    a.L = c.L; a.lDeb = c.lDeb; a.Rcut = c.Rcut; a.invlDeb = c.invlDeb; a.micT = c.micT;
    a.micGuard = c.micGuard;
    a.guard = c.guard;
    a.arrive = s->force_arrive;                // overlapped MD step: count finished workgroups
    return 0;
}
// ... and the pending-force state after a launch with that block
void mdqt::n3_forces_pending(mdqt_ctx* s, const N3Args& a) {
    const bool one_slot = a.P == s->dF, split = a.pairs != s->dPairs;
    s->f_pending = !one_slot;  // slots summed by the next substep launch (or settle_forces)
    s->pend_nseg = s->nslots + (split ? split_slots(s) : 0);
}

extern "C" int mdqt_forces(mdqt_ctx* s) {                 // forces(), SpeedUp:192-236
    if (!s) return set_error("NULL context");
    if (s->nloc == 0) return 0;
    HIPCHK(hipSetDevice(s->dev));
    const bool tm = launch_timed(s, 0);
    // timing: the Newton-3 tile kernel (one launch) records its own timestamps; the other
    // schemes (several kernels, collectives) are bracketed by events on the stream
    const bool tm_marks = tm && !s->use_n3;
    if (tm_marks && mark(s, 0)) return -1;
    if (s->use_n3) {
        N3Args a;
        if (n3_force_args(s, a)) return -1;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (tm && take_events(s, 0, &e0, &e1)) return -1;
        HIPCHK(launch_forces_n3(a, s->force_variant, s->stream, e0, e1));
        n3_forces_pending(s, a);
    } else if (s->use_n3b) {
        const bool bd = tm && (s->tkinds & 8u);    // the breakdown of this call
        mdqt_ctx::BdCall bc;
        if (bd) {
            bc.ag0 = s->bd_ag[0]; bc.ag1 = s->bd_ag[1];
            bc.m[0] = bd_event(s);
        }
        s->bd_ag[0] = s->bd_ag[1] = nullptr;
        if (n3b_balance(s)) return -1;
        N3BArgs a;
        if (n3b_args(s, a)) return -1;
        if (bd) bc.m[1] = bd_event(s);
        const int W = s->p.world_size;
        if (a.tailb) {
            HIPCHK(hipMemsetAsync(a.tailb, 0, (size_t)4 * a.T * sizeof(double), s->stream));
            HIPCHK(hipMemsetAsync(s->dTailSt + 3, 0, sizeof(unsigned long long), s->stream));
        }
        hipEvent_t e0 = nullptr, e1 = nullptr;     // timed call: the block kernel alone as well
        if (tm && take_events(s, 2, &e0, &e1)) return -1;
        hipEvent_t pm[3] = {nullptr, nullptr, nullptr};   // after the plan, the kernel, the reduction
        if (bd)
            for (auto& e : pm) {
                if (!s->bdfree.empty()) { e = s->bdfree.back(); s->bdfree.pop_back(); }
                else HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
            }
        HIPCHK(launch_forces_n3b(a, s->force_variant, W == 1 ? s->dF : s->dFr, s->stream, e0, e1, bd ? pm : nullptr));
        if (bd) { bc.m[2] = pm[0]; bc.m[3] = pm[1]; bc.m[4] = pm[2]; }
        if (a.tailb) {                  // measured tail: complete the per-tile sums, then enforce eps
            if (W > 1 && s->comm) {
                NCCLCHK(ncclAllReduce(a.tailb, a.tailb, (size_t)4 * a.T, ncclDouble, ncclSum, s->comm, s->stream));
            }
            if (W == 1 || s->comm) {
                if (tail_enforce(s, a, W == 1 ? s->dF : s->dFr)) return -1;
            } else {                    // in-process group: once every rank has its sums (local_reduce)
                s->tail_pending = true;
                s->tail_args = a;
            }
        }
        if (bd) bc.m[5] = bd_event(s);
        if (W > 1) {
            if (s->comm) {
                NCCLCHK(ncclReduceScatter(s->dFr, s->dF, (size_t)3 * s->S, ncclDouble, ncclSum, s->comm, s->stream));
            } else if (!s->local.empty()) {
                s->rs_pending = true;      // formed by local_reduce once every rank has its partials
            } else {
                return set_error("mdqt_forces: sharded Newton-3 blocks need a communicator (mdqt_comm_init)");
            }
        }
        if (bd) {
            bc.m[6] = bd_event(s);
            s->bdcalls.push_back(bc);
        }
        s->f_pending = false;
    } else if (s->nseg == 1) {
        HIPCHK(launch_forces(force_args(s, s->dF), s->stream));
    } else {
        HIPCHK(launch_forces(force_args(s, s->dFpart), s->stream));
        s->f_pending = true;       // summed by the next substep launch (or settle_forces)
        s->pend_nseg = s->nseg;
    }
    if (tm_marks && mark(s, 0)) return -1;
    return 0;
}

// The argument block of a launch of m substeps from the context's state (run_substeps, md_step_fused
// and the ensemble's batched launch); returns t after them (t itself where !advance_t).  nseg comes from
// the pending-force state, which the caller clears.
double mdqt::substep_args(const mdqt_ctx* s, SubstepArgs& a, int m, int do_step, int do_qt, int advance_t) {
    memset(&a, 0, sizeof a);
    a.R = s->dR + (size_t)s->p.rank * 3 * s->S;
    a.V = s->dV; a.F = s->dF; a.psi = s->dPsi; a.tPart = s->dTp;
    a.Fpart = s->dFpart; a.nseg = s->f_pending ? s->pend_nseg : 1;
    a.oor = s->dFlags;
    a.n = s->nloc; a.S = s->S; a.gid0 = (uint64_t)s->lo;
    a.q0 = s->qidx;
    a.nsub = m; a.do_step = do_step; a.do_qt = do_qt;
    a.L = s->L;
    a.qc = s->qc;
    double t = s->t;
    a.movmask = 0;
    a.expdet_zero = 1;
    for (int k = 0; k < m; ++k) {
        a.t[k] = t;
        a.expDet[k] = expDetuning_of(&s->p, t);
        if (t > 0) a.movmask |= 1u << k;
        if (a.expDet[k] != 0.) a.expdet_zero = 0;
        if (advance_t) t += s->dtQ;                    // qstep: t += dtQuant (:716)
    }
    return t;
}

// n substeps of (step if do_step; qstep if do_qt_flag) — t advances only when advance_t
int mdqt::run_substeps(mdqt_ctx* s, int n, int do_step, int do_qt_flag, int advance_t) {
    if (local_reduce(s)) return -1;
    HIPCHK(hipSetDevice(s->dev));
    const int do_qt = do_qt_flag && s->p.qt_enabled;
    if (do_qt && s->p.qt_model != 0 && s->qt_math != 2) return set_error("the optical-pumping qt_models need qt_math 2");
    const bool d48 = do_qt && s->p.rng_mode == 0;
    while (n > 0) {
        const int m = d48 ? 1 : (n < MAXSUB ? n : MAXSUB);   // drand48: the stream orders ions per substep
        SubstepArgs a;
        const double t = substep_args(s, a, m, do_step, do_qt, advance_t);
        if (s->sub_stream) {                            // overlapped MD step (mdqt_md_steps)
            a.arrive = s->dArrive;
            a.arrive_target = s->sub_target;
            a.spin_err = s->dSpinErr;
            a.arrive_sleep = 2;
        }
        s->f_pending = false;
        if (d48 && s->nloc > 0) {
            D48Args r;
            r.psi = s->dPsi; r.n = s->nloc; r.S = s->S;
            r.state = s->dX48; r.jA = s->dX48 + 1; r.jC = s->dX48 + 49;
            r.U = s->dU; r.qc = s->qc; r.fast = s->qt_math;
            HIPCHK(launch_d48_resolve(r, s->stream));
            a.U = s->dU;
        }
        const bool tm = launch_timed(s, 1);
        hipEvent_t e0 = nullptr, e1 = nullptr;       // timing: the kernel's own timestamps
        if (tm && (take_events(s, 1, &e0, &e1))) return -1;
        hipStream_t st = s->sub_stream ? s->sub_stream : s->stream;
        int inst = 0;
        if (s->qt_math == 2) HIPCHK(launch_substeps_r(a, s->dFTab, s->sub_stream ? 2 : s->substep_mode, st, e0, e1, &inst));
        else HIPCHK(launch_substeps(a, s->dTab, s->substep_mode, s->qt_math, s->stream, e0, e1, &inst));
        s->last_qt_kernel = inst;
        s->last_qt_nseg = a.nseg;
        if (advance_t) {
            s->t = t;
            s->qidx += (uint64_t)m;
        }
        n -= m;
    }
    return 0;
}

extern "C" int mdqt_step(mdqt_ctx* s) { return s ? run_substeps(s, 1, 1, 0, 0) : set_error("NULL context"); }
extern "C" int mdqt_qstep(mdqt_ctx* s) { return s ? run_substeps(s, 1, 0, 1, 1) : set_error("NULL context"); }
extern "C" int mdqt_substeps(mdqt_ctx* s, int n) {
    if (!s) return set_error("NULL context");
    if (n < 0) return set_error("negative substep count");
    return run_substeps(s, n, 1, 1, 1);
}

// The overlapped MD step applies to one unsharded system on the Newton-3 tile scheme with the
// lane-per-state QT kernel (qt_math 2, Philox stream), one fused launch per MD interval.
static bool overlap_applies(const mdqt_ctx* s) {
    return s->overlap_opt && s->p.world_size == 1 && s->local.empty() && s->use_n3 && s->nslots > 1 && s->qt_math == 2 &&
           s->p.qt_enabled && s->p.rng_mode == 1 && s->ratio <= MAXSUB && s->nloc > 0 &&
           (s->substep_mode == 2 || (s->substep_mode == 0 && s->nloc < kLaneKernelMaxIons));
}

// per-tile arrival counters of the overlapped / fused MD step (monotonic: a launch adds T to
// every tile's counter, the waiters compare with the running epoch)
int mdqt::arrive_setup(mdqt_ctx* s) {
    const int T = (s->N + 63) / 64;
    if (s->dArrive && s->dArrive.capacity() >= (size_t)T) return 0;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->qs) HIPCHK(hipStreamSynchronize(s->qs));
    HIPCHK(s->dArrive.alloc((size_t)T));
    HIPCHK(hipMemset(s->dArrive, 0, (size_t)T * sizeof(unsigned long long)));
    HIPCHK(hipDeviceSynchronize());
    s->arriveEpoch = 0;
    return 0;
}

static int overlap_setup(mdqt_ctx* s) {
    if (arrive_setup(s)) return -1;
    if (s->qs) return 0;
    HIPCHK(hipStreamCreateWithFlags(&s->qs, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&s->evQ, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK(hipEventCreateWithFlags(&s->evS, hipEventDisableTiming | hipEventDisableSystemFence));
    return 0;
}

// MD steps with the force and QT launches overlapped: step k's force launch (context stream)
// waits for step k-1's QT launch by an event; step k's QT launch (its own stream, in order after
// step k-1's) starts at once, issues its prologue loads and Philox draws while the forces are
// computed, and waits on the device until the tile pairs of its ions' tile have arrived.  Same
// kernels, same operations: bit-identical to the sequential order (tests/test_gpu_parity.py).
// Measured at C2 (one MI355X): 104-107 us per MD step against 45.6 sequential — the two
// cross-stream event waits cost ~17 us per step by themselves, and the resident QT waves (176
// VGPRs) leave room for 1,344 of the force launch's 1,596 workgroups, so it runs in two rounds
// (17.6 -> 52-70 us).  Kept as an option (default off) with its bit-identity test.
static int md_steps_overlapped(mdqt_ctx* s, int n) {
    if (overlap_setup(s)) return -1;
    HIPCHK(hipEventRecord(s->evS, s->stream));
    HIPCHK(hipStreamWaitEvent(s->qs, s->evS, 0));
    for (int k = 0; k < n; ++k) {
        if (k > 0) HIPCHK(hipStreamWaitEvent(s->stream, s->evQ, 0));
        if (loop_check(s, k)) return -1;
        s->force_arrive = s->dArrive;
        const int rc = mdqt_forces(s);
        s->force_arrive = nullptr;
        if (rc) return -1;
        s->arriveEpoch += (unsigned long long)((s->N + 63) / 64);   // T tile pairs touch every tile
        s->c0++;
        s->sub_stream = s->qs;
        s->sub_target = s->arriveEpoch;
        const int rq = run_substeps(s, s->ratio, 1, 1, 1);
        s->sub_stream = nullptr;
        if (rq) return -1;
        HIPCHK(hipEventRecord(s->evQ, s->qs));
    }
    HIPCHK(hipStreamWaitEvent(s->stream, s->evQ, 0));      // later work on the context stream
    return 0;
}

// One MD step as ONE launch (mdqt_qtfast.hip k_md_step): the Newton-3 tile pairs of forces() and
// the interval's fused substeps, the QT workgroups waiting on the device for the arrival counts
// of their ions' tiles instead of a kernel boundary.  Applies to one unsharded system on the tile
// scheme with the lane QT kernel's FAST instance (qt_math 2, Philox, t > 0, the whole interval in
// one launch, no range guard).  Same operations as forces() + substeps(ratio): bit-identical.
// Measured at C2 (one MI355X, per-workgroup stamps `tools/md_stamps.py`): 56-63 us per MD step
// against 43.5 for the two launches — one kernel has one VGPR count, so the tile pairs run with
// the QT part's 162 (3 waves per SIMD instead of 7), the QT workgroups dispatched while the last
// tile pairs still run take their CU slots, and the substep loops of early-complete tiles compete
// with the remaining tile pairs; the force work ends at 32-37 us instead of 18.  Kept as an option
// (default off) with its bit-identity tests.
bool mdqt::fused_applies(mdqt_ctx* s) {
    if (!(s->fused_opt && !s->overlap_opt && s->p.world_size == 1 && s->local.empty() && s->use_n3 && s->nslots > 1 &&
          s->qt_math == 2 && s->p.qt_enabled && s->p.rng_mode == 1 && s->ratio <= MAXSUB && s->nloc > 0 &&
          s->t > 0 && s->force_variant <= 1 &&
          (s->substep_mode == 2 || (s->substep_mode == 0 && s->nloc < kLaneKernelMaxIons))))
        return false;
    return !force_args(s, nullptr).guard;
}

int mdqt::md_step_fused(mdqt_ctx* s) {
    if (arrive_setup(s)) return -1;
    HIPCHK(hipSetDevice(s->dev));
    const unsigned long long T = (unsigned long long)((s->N + 63) / 64);
    N3Args f;
    if (n3_force_args(s, f, true)) return -1;          // the plain table into the slots (nslots > 1)
    f.guard = 0;
    f.arrive = s->dArrive;
    SubstepArgs a;                                     // as run_substeps(s, ratio, 1, 1, 1)
    const int m = s->ratio;
    const double t = substep_args(s, a, m, 1, 1, 1);
    a.nseg = s->nslots;
    a.arrive = s->dArrive;
    a.arrive_target = s->arriveEpoch + T;
    a.spin_err = s->dSpinErr;
    a.arrive_sleep = 2;
    if (a.movmask != (m >= 32 ? 0xFFFFFFFFu : (1u << m) - 1u)) return set_error("md_step_fused: t <= 0 in the interval");
    const bool tm = launch_timed(s, 1);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (tm && take_events(s, 1, &e0, &e1)) return -1;
    HIPCHK(launch_md_step(f, a, s->dFTab, s->force_variant, s->stream, e0, e1));
    s->last_qt_kernel = QTK_MD_STEP;
    s->last_qt_nseg = a.nseg;
    s->arriveEpoch += T;
    s->f_pending = false;                              // F written by the QT workgroups
    s->t = t;
    s->qidx += (uint64_t)m;
    return 0;
}

extern "C" int mdqt_md_steps(mdqt_ctx* s, int n) {
    if (!s) return set_error("NULL context");
    if (n > 0 && overlap_applies(s)) return md_steps_overlapped(s, n);
    for (int k = 0; k < n; ++k) {
        if (loop_check(s, k)) return -1;
        if (fused_applies(s)) {
            if (local_reduce(s) || md_step_fused(s)) return -1;
            s->last_fused = 1;
            s->c0++;
            continue;
        }
        s->last_fused = 0;
        if (mdqt_allgather_positions(s)) return -1;     // sharded: other slabs' R
        if (mdqt_forces(s)) return -1;
        s->c0++;
        if (mdqt_substeps(s, s->ratio)) return -1;
    }
    return 0;
}

// stateless pair kernels on host arrays (tests, and the MD-only programs' force seam)
static int pairs_raw(int mode, int N, double L, double lDeb, const double* R, size_t ld, double* out,
                     int nseg_req, int device, int variant) {
    if (N < 1 || !R || !out || ld < (size_t)N) return set_error("pairs_raw: bad arguments");
    if (variant < 0 || variant > 1) return set_error("pairs_raw: variant must be 0 (exact) or 1 (fast)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error("no HIP device available");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    int lo, hi, S;
    if (mdqt_slab(N, 1, 0, &lo, &hi, &S)) return -1;
    mdqt_ctx tmp;                                   // only for choose_segments
    memset(&tmp.p, 0, sizeof tmp.p);
    tmp.p.world_size = 1;
    tmp.scheme_opt = 1;
    tmp.N = N; tmp.p.force_segments = nseg_req;
    choose_segments(&tmp);
    const int nseg = tmp.nseg;
    std::vector<double> h((size_t)3 * S, 0.);
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < N; ++i) h[(size_t)c * S + i] = R[(size_t)c * ld + i];
    hipStream_t st;
    HIPCHK(hipStreamCreate(&st));
    std::unique_ptr<ihipStream_t, hipError_t (*)(hipStream_t)> st_owner(st, hipStreamDestroy);
    DevBuf<double> dR, dP, dO;
    HIPCHK(dR.alloc(h.size()));
    HIPCHK(dP.alloc((size_t)3 * S * nseg));
    HIPCHK(dO.alloc((size_t)3 * S));
    HIPCHK(hipMemcpyAsync(dR, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st));
    int oor = 0;
    for (size_t k = 0; k < (size_t)3 * N && !oor; ++k) {
        const double x = R[(k / N) * ld + k % N];
        if (!(x >= -0.125 * L && x <= 1.125 * L)) oor = 1;
    }
    ForceArgs a;
    a.Rall = dR; a.Fpart = dP; a.N = N; a.S = S; a.row_lo = 0; a.nrows = N;
    a.nseg = nseg; a.seglen = tmp.seglen;
    fill_pair_consts(a, L, lDeb, variant);
    a.guard = oor;
    HIPCHK(mode == 0 ? launch_forces(a, st) : launch_potential_rows(a, st));
    HIPCHK(launch_reduce_segments(dP, dO, nseg, N, S, mode == 0 ? 3 : 1, st));
    HIPCHK(hipMemcpyAsync(h.data(), dO, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (mode == 0) {
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < N; ++i) out[(size_t)c * ld + i] = h[(size_t)c * S + i];
    } else {
        for (int i = 0; i < N; ++i) out[i] = h[i];
    }
    return 0;
}

extern "C" int mdqt_forces_raw(int N, double L, double lDeb, const double* R, size_t ld, double* F,
                               int nseg, int device, int variant) {
    return pairs_raw(0, N, L, lDeb, R, ld, F, nseg, device, variant);
}

extern "C" int mdqt_potentials_raw(int N, double L, double lDeb, const double* R, size_t ld, double* U,
                                   int nseg, int device, int variant) {
    return pairs_raw(1, N, L, lDeb, R, ld, U, nseg, device, variant);
}
