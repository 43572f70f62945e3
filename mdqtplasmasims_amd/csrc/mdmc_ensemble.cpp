// mdmc_ensemble — J independent jobs of the Monte-Carlo + MD programs in one process (include/mdmc.h,
// "ensembles").  The reference runs them as a Slurm array (exampleSlurmFile.slurm:3,16, `srun tagQuad
// $SLURM_ARRAY_TASK_ID`); a single job's Metropolis anneal is one workgroup on one CU, because the chain is
// sequential, so the array's anneals run here as ONE launch of J workgroups (k_monte_carlo_lds_ens: the
// single-job kernel's body on each member's own argument block, which is the bit-identity argument).  The MD
// stages run one of two ways (mdmc_ensemble_set_md_batch).  Mode 0 queues every member's own launches on its
// own stream, one host thread, so they overlap on the chip: the single context's code on the single
// context's arguments.  Mode 1 steps all members with one force and one velocity-Verlet launch per step on
// the ensemble's stream ("batched MD stretches" below), again the single-job kernels' bodies on each member's
// own argument block.  For the QT tagging programs mode 1 batches the QT substeps, the tagging and the tagged
// ions' moments and X distribution the same way ("batched QT" below).  The stages themselves are mdmc_run.cpp's,
// written once on mdmc_ctx.hpp's MdLane: J member lanes in mode 0, one ensemble lane in mode 1, and the
// stepping calls here take the same lanes.  The argument blocks travel through pinned
// rings and the launches are timed by event pairs: mdqt_batch.hpp's PinRing and LaunchTimer, shared with the MDQT
// ensembles.
#include <algorithm>
#include <memory>

#include "../../include/mdqt.h"   // mdqt_last_error
#include "mdmc_ctx.hpp"
#include "mdqt_ens_args.hpp"      // the QT tagging ensemble's QT and tag launches are the pump ensemble's

using namespace mdqt;

namespace {

int sync_members(mdmc_ensemble* e) {
    for (mdmc_ctx* c : e->jobs) HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

constexpr int kHdrSlots = 4;     // stretches whose blocks may be on their way at once
constexpr int kVVSlots = 64;     // collisional steps whose blocks may be on their way at once

int md_blocks_create(mdmc_ensemble* e) {
    const size_t J = e->jobs.size();
    const size_t n3 = 2 * J * sizeof(N3Args), vv = 2 * J * sizeof(VVArgs), ob = J * sizeof(MDObsArgs);
    const size_t kx = J * sizeof(MDKdeXArgs);
    e->hdrBytes = n3 + vv + ob + kx;
    if (e->dBlocks.alloc(e->hdrBytes + J * sizeof(VVArgs)) != hipSuccess)
        return set_error("mdmc_ensemble_create: allocating the MD argument blocks of %zu jobs failed", J);
    e->dN3 = reinterpret_cast<N3Args*>(e->dBlocks.get());
    e->dVV = reinterpret_cast<VVArgs*>(e->dBlocks + n3);
    e->dObs = reinterpret_cast<MDObsArgs*>(e->dBlocks + n3 + vv);
    e->dKdeX = reinterpret_cast<MDKdeXArgs*>(e->dBlocks + n3 + vv + ob);
    e->dVVc = reinterpret_cast<VVArgs*>(e->dBlocks + e->hdrBytes);
    if (e->hdrRing.create(e->hdrBytes, kHdrSlots, hipEventDisableTiming) ||
        e->vvRing.create(J * sizeof(VVArgs), kVVSlots, hipEventDisableTiming))
        return -1;
    e->coll.assign(J, 0);
    e->skip.assign(J, 0ull);
    for (size_t k = 0; k < J; ++k) {
        hipEvent_t ev = nullptr;
        HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        e->evMember.push_back(ev);
    }
    HIPCHK(hipEventCreateWithFlags(&e->evEns, hipEventDisableTiming));
    return 0;
}

int need_open(const mdmc_ensemble* e, const char* what) {
    if (!e->open) return set_error("%s outside a batched MD stretch", what);
    return 0;
}

// the batched QT's own areas, for an ensemble of QT tagging jobs
constexpr int kQtSlots = 8;      // QT chunks / taggings whose blocks may be on their way at once

int qt_blocks_create(mdmc_ensemble* e) {
    const size_t J = e->jobs.size();
    const size_t dist = (size_t)mdmc_ensemble::kDistSlots * J * TKDE_BINS;
    if (e->dQt.alloc(J * sizeof(SubstepArgs)) != hipSuccess || e->dDist.alloc(dist) != hipSuccess ||
        e->hDist.alloc(dist) != hipSuccess || e->hMom.alloc(J * kTagMomentSums) != hipSuccess)
        return set_error("mdmc_ensemble_create: allocating the QT blocks and distribution rings of %zu jobs failed", J);
    if (e->qtRing.create(J * sizeof(SubstepArgs), kQtSlots, hipEventDisableTiming)) return -1;
    for (hipEvent_t& ev : e->evDist) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return 0;
}

// the ensemble's stream behind every member's stream
int fence_in(mdmc_ensemble* e) {
    for (size_t k = 0; k < e->jobs.size(); ++k) {
        HIPCHK(hipEventRecord(e->evMember[k], e->jobs[k]->st));
        HIPCHK(hipStreamWaitEvent(e->stream, e->evMember[k], 0));
    }
    return 0;
}

// a member's per-step observable blocks: the rows go to its dTemp / dMom (a stretch) or, scratch, its sums
// land in dOut as its own calls' do
void obs_args(const mdmc_ctx* c, bool scratch, MDObsArgs& o, MDKdeXArgs& x) {
    memset(&o, 0, sizeof o);
    o.V = c->dV; o.tags = c->dTags; o.N = c->N; o.S = c->S; o.T = c->T;
    o.temp = scratch ? c->dOut : c->dTemp; o.mom = scratch ? c->dOut : c->dMom; o.vs = c->dVS;
    memset(&x, 0, sizeof x);
    x.V = c->dV; x.tags = c->dTags; x.N = c->N; x.S = c->S; x.part = c->dKdePart;
}

static_assert(sizeof(PumpTagArgs) <= sizeof(SubstepArgs), "a QT ring slot holds one block per member of either kind");

int need_qt(const mdmc_ensemble* e, const char* what) {
    if (!e) return set_error("%s: NULL ensemble", what);
    if (!e->jobs[0]->qt) return set_error("%s: the context has no QT (qt_model 0)", what);
    if (e->open) return set_error("%s inside a batched MD stretch", what);
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// Batched MD stretches (md_batch 1).  A stretch is a run of MD steps of all members between two points where
// the members' own streams matter:
//   begin   `stream` waits on one event per member stream.  A member whose pre-advanced positions are stale
//           (rnValid false: set_state, an anneal, anisotropize) gets its own k_vv_positions on `stream`.  Then
//           every member's blocks are built by the helpers md_step_async uses — N3Args and VVArgs for BOTH
//           buffer parities (dR / dRn swap every step), MDObsArgs — and go over in one copy.  The blocks are
//           per member, so a member stepped alone an odd number of times simply has its pointers the other
//           way round.
//   step    swap every member's dR / dRn on the host; one k_pairs_n3_ens on set `parity`; the collision rolls
//           of the members that have a collision frequency, drawn per member from its own Mt32 in the
//           reference's order into its own pinned ring; one k_vv_step_ens — on the resident set when no member
//           draws, else on a fresh VVArgs [J] (one copy in stream order from the pinned ring); one
//           k_collide_ens if a member has a hit.  A collisionless member's discard(2N) is additive and
//           applied once, at the end.
//   end     the members' streams wait on one event of `stream`; the discards are applied.
// Inside a stretch nothing touches a member's stream but its g(r) (ensemble_md_pair_corr_queue).
// ------------------------------------------------------------------------------------------------------------
int mdmc::ensemble_md_begin(mdmc_ensemble* e) {
    if (e->open) return set_error("ensemble_md_begin inside a batched MD stretch");
    const size_t J = e->jobs.size();
    HIPCHK(hipSetDevice(e->dev));
    if (fence_in(e)) return -1;
    char* h = nullptr;
    int slot = 0;
    if (e->hdrRing.take(&h, &slot)) return -1;
    N3Args* n3 = reinterpret_cast<N3Args*>(h);
    VVArgs* vv = reinterpret_cast<VVArgs*>(h + 2 * J * sizeof(N3Args));
    MDObsArgs* ob = reinterpret_cast<MDObsArgs*>(h + 2 * J * (sizeof(N3Args) + sizeof(VVArgs)));
    MDKdeXArgs* kx = reinterpret_cast<MDKdeXArgs*>(ob + J);
    e->obsCap = e->jobs[0]->temp_rows();
    for (size_t k = 0; k < J; ++k) {
        mdmc_ctx* c = e->jobs[k];
        if (!c->rnValid) {                                                                    // :452-467
            HIPCHK(launch_vv_positions(c->dR, c->dV, c->dA, c->dRn, c->N, c->S, c->p.timeStep, c->L, e->stream));
            ++e->mdLaunches;
            c->rnValid = true;
        }
        for (int par = 0; par < 2; ++par) {      // set 0: the buffers as the first step sees them, after its swap
            std::swap(c->dR, c->dRn);
            mdmc::n3_args(c, n3[par * J + k]);
            mdmc::vv_args(c, nullptr, 0, vv[par * J + k]);
        }                                         // two swaps: the member's pointers are back
        obs_args(c, false, ob[k], kx[k]);
        e->obsCap = std::min(e->obsCap, c->temp_rows());
        e->coll[k] = c->p.timeStep * c->collisionFreq > 0;
        e->skip[k] = 0;
    }
    if (e->hdrRing.send(slot, e->dBlocks, e->hdrBytes, e->stream)) return -1;
    e->parity = 0;
    e->open = true;
    return 0;
}

int mdmc::ensemble_md_step(mdmc_ensemble* e) {
    if (need_open(e, "ensemble_md_step")) return -1;
    const size_t J = e->jobs.size();
    const mdmc_ctx* c0 = e->jobs[0];
    const int par = e->parity;
    for (mdmc_ctx* c : e->jobs) std::swap(c->dR, c->dRn);
    hipEvent_t f0 = nullptr, f1 = nullptr, v0 = nullptr, v1 = nullptr;
    if (e->timing && (e->forceTimer.take(&f0, &f1) || e->vvTimer.take(&v0, &v1))) return -1;
    // force_kernel 1: variant 2 (fast values, the reference's exact pair set), 0: exact            :508
    HIPCHK(launch_forces_n3_mdmc_ens(e->dN3 + par * J, (int)J, c0->npairs, c0->p.force_kernel == 1 ? 2 : 0, e->stream, f0, f1));
    ++e->mdLaunches;
    const VVArgs* blocks = e->dVV + par * J;
    int max_hits = 0;
    bool any = false;
    for (size_t k = 0; k < J; ++k) any = any || e->coll[k];
    if (any) {
        char* h = nullptr;
        int slot = 0;
        if (e->vvRing.take(&h, &slot)) return -1;
        VVArgs* vv = reinterpret_cast<VVArgs*>(h);
        for (size_t k = 0; k < J; ++k) {
            mdmc_ctx* c = e->jobs[k];
            double* hits = nullptr;
            int nh = 0;
            // every roll of a collisionless member misses (uni >= 0): one generate_canonical, two words, each
            if (!e->coll[k]) e->skip[k] += 2ull * c->N;
            else if (mdmc::collision_draws(c, e->stream, &hits, &nh)) return -1;
            mdmc::vv_args(c, hits, nh, vv[k]);
            max_hits = std::max(max_hits, nh);
        }
        if (e->vvRing.send(slot, e->dVVc, J * sizeof(VVArgs), e->stream)) return -1;
        blocks = e->dVVc;
    } else {
        for (size_t k = 0; k < J; ++k) e->skip[k] += 2ull * e->jobs[k]->N;
    }
    HIPCHK(launch_vv_step_ens(blocks, (int)J, c0->N, e->stream, v0, v1));                        // :469-502
    ++e->mdLaunches;
    if (max_hits > 0) {
        HIPCHK(launch_collide_ens(blocks, (int)J, max_hits, e->stream));
        ++e->mdLaunches;
    }
    e->parity = par ^ 1;
    return 0;
}

int mdmc::ensemble_md_end(mdmc_ensemble* e) {
    if (need_open(e, "ensemble_md_end")) return -1;
    e->open = false;
    HIPCHK(hipEventRecord(e->evEns, e->stream));
    for (size_t k = 0; k < e->jobs.size(); ++k) {
        mdmc_ctx* c = e->jobs[k];
        HIPCHK(hipStreamWaitEvent(c->st, e->evEns, 0));
        c->rng.discard(e->skip[k]);
        e->skip[k] = 0;
    }
    return 0;
}

// the per-step observables of a recorded stage, one launch per kind: row k of every member's dTemp / dMom,
// column t of its velocity store
int mdmc::ensemble_md_temperatures(mdmc_ensemble* e, int k) {
    if (need_open(e, "ensemble_md_temperatures")) return -1;
    if (k < 0 || k >= e->obsCap) return set_error("ensemble_md_temperatures: step %d outside the %d buffered", k, e->obsCap);
    HIPCHK(launch_temperatures_ens(e->dObs, (int)e->jobs.size(), k, e->stream));
    ++e->mdLaunches;
    return 0;
}

// the MC + MD program's four tag sets or, qt, the QT tagging programs' one: the same launch, charged to its own counter
int mdmc::ensemble_tag_moments(mdmc_ensemble* e, int k, bool qt) {
    const char* what = qt ? "ensemble_qt_tag_moments" : "ensemble_md_tag_moments";
    if (need_open(e, what)) return -1;
    if (k < 0 || k >= e->obsCap) return set_error("%s: step %d outside the %d buffered", what, k, e->obsCap);
    HIPCHK(launch_tag_moments_ens(e->dObs, (int)e->jobs.size(), k, e->stream));
    ++(qt ? e->qtLaunches : e->mdLaunches);
    return 0;
}

int mdmc::ensemble_md_store_velocities(mdmc_ensemble* e, int t) {                                // :513-523
    if (need_open(e, "ensemble_md_store_velocities")) return -1;
    const mdmc_ctx* c0 = e->jobs[0];
    if (t < 0 || t >= c0->T) return set_error("ensemble_md_store_velocities: step %d outside [0, %d)", t, c0->T);
    HIPCHK(launch_store_velocities_ens(e->dObs, (int)e->jobs.size(), c0->N, t, e->stream));
    ++e->mdLaunches;
    return 0;
}

// g(r) of every member inside a stretch: the histogram, its copy and evDrain stay on the member's stream,
// which waits for the batched steps so far; the next batched step overwrites the buffer the histogram reads
// (k_vv_step's Rn), so `stream` waits for every evDrain
int mdmc::ensemble_md_pair_corr_queue(mdmc_ensemble* e) {
    if (need_open(e, "ensemble_md_pair_corr_queue")) return -1;
    HIPCHK(hipEventRecord(e->evEns, e->stream));
    for (mdmc_ctx* c : e->jobs) {
        HIPCHK(hipStreamWaitEvent(c->st, e->evEns, 0));
        if (mdmc::pair_corr_queue(c)) return -1;
        HIPCHK(hipStreamWaitEvent(e->stream, c->evDrain, 0));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// Batched QT (md_batch 1; an ensemble of the QT tagging programs).  The pump models' QT substeps, the spin-up
// tagging and the tagged ions' moments and X distribution of all members, each in one launch (two for the
// distribution) on the ensemble's stream: the single-job kernels' bodies on each member's own block.  A QT
// chunk's blocks are what mdmc::qsteps_async builds (mdmc::substep_args) — each member's own qstep index and
// Philox key, so members need not be in lockstep; the by-lane table is member 0's, since all members share the
// model's parameters — and go through the pinned QT ring in stream order, as the tagging's do.  The moment and
// distribution blocks are resident with the stretch's.  The distribution's rows land in a slot of the
// ensemble's [kDistSlots][J][TKDE_BINS] device ring and one copy a slot brings all members' rows to the pinned
// ring; evDist[slot] behind the copy is all the host ever waits for.
// These are queued between ensemble_md_begin and ensemble_md_end (mdmc_run.cpp's stages), or by the entry points below between
// fence_in and a synchronisation of the ensemble's stream.
// ------------------------------------------------------------------------------------------------------------
int mdmc::ensemble_qt_steps(mdmc_ensemble* e, int n) {
    const size_t J = e->jobs.size();
    while (n > 0) {
        const int m = n < MAXSUB ? n : MAXSUB;
        char* h = nullptr;
        int slot = 0;
        if (e->qtRing.take(&h, &slot)) return -1;
        SubstepArgs* a = reinterpret_cast<SubstepArgs*>(h);
        int max_n = 0;
        for (size_t k = 0; k < J; ++k) {
            mdmc_ctx* c = e->jobs[k];
            mdmc::substep_args(c, m, a[k]);
            c->qidx += (uint64_t)m;
            max_n = std::max(max_n, c->N);
        }
        if (e->qtRing.send(slot, e->dQt, J * sizeof(SubstepArgs), e->stream)) return -1;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (e->timing && e->qtTimer.take(&e0, &e1)) return -1;
        // a[0] picks the instance (the slot is read by the copy only, and not rewritten before take() hands it out again)
        HIPCHK(launch_substeps_pump_ens(reinterpret_cast<const SubstepArgs*>(e->dQt.get()), a[0], (int)J, max_n, e->jobs[0]->dFTab,
                                        e->stream, e0, e1));
        ++e->qtLaunches;
        n -= m;
    }
    return 0;
}

int mdmc::ensemble_qt_tag(mdmc_ensemble* e) {                      // tagParticles, QTT:1022-1067
    const size_t J = e->jobs.size();
    char* h = nullptr;
    int slot = 0;
    if (e->qtRing.take(&h, &slot)) return -1;
    PumpTagArgs* a = reinterpret_cast<PumpTagArgs*>(h);
    int max_n = 0;
    for (size_t k = 0; k < J; ++k) {
        const mdmc_ctx* c = e->jobs[k];
        memset(&a[k], 0, sizeof a[k]);                               // mdmc_tag_qt's arguments
        a[k].psi = c->dPsi; a[k].n = c->N; a[k].S = c->S; a[k].gid0 = 0; a[k].q = c->qidx; a[k].tags = c->dTags;
        a[k].qc = c->qc;
        max_n = std::max(max_n, c->N);
    }
    if (e->qtRing.send(slot, e->dQt, J * sizeof(PumpTagArgs), e->stream)) return -1;
    HIPCHK(launch_tag_spin_up_ens(reinterpret_cast<const PumpTagArgs*>(e->dQt.get()), (int)J, max_n, e->stream));
    ++e->qtLaunches;
    return 0;
}

int mdmc::ensemble_qt_dist_x(mdmc_ensemble* e, int slot) {
    if (slot < 0 || slot >= mdmc_ensemble::kDistSlots) return set_error("ensemble_qt_dist_x: slot %d outside the ring", slot);
    const size_t J = e->jobs.size(), row = J * TKDE_BINS;
    int max_N = 0;
    for (const mdmc_ctx* c : e->jobs) max_N = std::max(max_N, c->N);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e->timing && e->distTimer.take(&e0, &e1)) return -1;
    HIPCHK(launch_tagged_kde_x_ens(e->dKdeX, (int)J, max_N, e->dDist + row * slot, e->stream, e0, e1));
    e->qtLaunches += 2;
    HIPCHK(hipMemcpyAsync(e->hDist + row * slot, e->dDist + row * slot, row * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipEventRecord(e->evDist[slot], e->stream));
    return 0;
}

const double* mdmc::ensemble_qt_dist_rows(mdmc_ensemble* e, int slot) {
    if (slot < 0 || slot >= mdmc_ensemble::kDistSlots) {
        set_error("ensemble_qt_dist_rows: slot %d outside the ring", slot);
        return nullptr;
    }
    const hipError_t r = hipEventSynchronize(e->evDist[slot]);
    if (r != hipSuccess) {
        set_error("ensemble_qt_dist_rows: %s", hipGetErrorString(r));
        return nullptr;
    }
    return e->hDist + e->jobs.size() * TKDE_BINS * (size_t)slot;
}

// mdmc_qsteps of every member
extern "C" int mdmc_ensemble_qsteps(mdmc_ensemble* e, int n) {
    if (need_qt(e, "mdmc_ensemble_qsteps")) return -1;
    HIPCHK(hipSetDevice(e->dev));
    const std::vector<mdmc::MdLane> lanes = mdmc::md_lanes(e->jobs.data(), (int)e->jobs.size(), e);
    // no stretch: an ensemble lane's launches go between the fence and a wait for the ensemble's stream
    if (lanes[0].e && fence_in(e)) return -1;
    for (const mdmc::MdLane& l : lanes)
        if (l.qt_steps(n)) return -1;
    if (!lanes[0].e) return sync_members(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// mdmc_tag_qt of every member: tags [J][N] or NULL, n_up [J] or NULL
extern "C" int mdmc_ensemble_tag_qt(mdmc_ensemble* e, int* tags, int* n_up) {
    if (need_qt(e, "mdmc_ensemble_tag_qt")) return -1;
    HIPCHK(hipSetDevice(e->dev));
    const size_t J = e->jobs.size();
    if (e->mdBatch != 1) {
        for (size_t k = 0; k < J; ++k)
            if (mdmc_tag_qt(e->jobs[k], tags ? tags + k * (size_t)e->jobs[k]->N : nullptr, n_up ? n_up + k : nullptr)) return -1;
        return 0;
    }
    if (fence_in(e) || mdmc::ensemble_qt_tag(e)) return -1;
    const size_t N = (size_t)e->jobs[0]->N;
    std::vector<int> h(tags || !n_up ? 0 : J * N);
    int* dst = tags ? tags : h.data();
    if (tags || n_up)
        for (size_t k = 0; k < J; ++k)
            HIPCHK(hipMemcpyAsync(dst + k * N, e->jobs[k]->dTags, N * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t k = 0; n_up && k < J; ++k) {
        int cnt = 0;
        for (size_t i = 0; i < N; ++i) cnt += dst[k * N + i];
        n_up[k] = cnt;
    }
    return 0;
}

// mdmc_tagged_moments_qt of every member: out4 [J][4]; distX [J][TKDE_BINS] or NULL — the X row only, the one
// the programs write (QTT:1128-1136)
extern "C" int mdmc_ensemble_tagged_moments_qt(mdmc_ensemble* e, double* out4, double* distX) {
    if (need_qt(e, "mdmc_ensemble_tagged_moments_qt")) return -1;
    if (!out4) return set_error("mdmc_ensemble_tagged_moments_qt: NULL argument");
    HIPCHK(hipSetDevice(e->dev));
    const size_t J = e->jobs.size();
    if (e->mdBatch != 1) {
        std::vector<double> d(distX ? (size_t)3 * TKDE_BINS : 0);
        for (size_t k = 0; k < J; ++k) {
            if (mdmc_tagged_moments_qt(e->jobs[k], out4 + 4 * k, distX ? d.data() : nullptr)) return -1;
            if (distX) std::copy_n(d.begin(), TKDE_BINS, distX + k * TKDE_BINS);
        }
        return 0;
    }
    if (fence_in(e)) return -1;
    // the members' blocks with the sums landing in their dOut, as their own call's do; through a slot of the
    // stretches' ring to where a stretch keeps them (the next stretch uploads its own)
    char* h = nullptr;
    int slot = 0;
    if (e->hdrRing.take(&h, &slot)) return -1;
    MDObsArgs* ob = reinterpret_cast<MDObsArgs*>(h);
    MDKdeXArgs* kx = reinterpret_cast<MDKdeXArgs*>(ob + J);
    for (size_t k = 0; k < J; ++k) obs_args(e->jobs[k], true, ob[k], kx[k]);
    if (e->hdrRing.send(slot, e->dObs, J * (sizeof(MDObsArgs) + sizeof(MDKdeXArgs)), e->stream)) return -1;
    HIPCHK(launch_tag_moments_ens(e->dObs, (int)J, 0, e->stream));
    ++e->qtLaunches;
    if (distX && mdmc::ensemble_qt_dist_x(e, 0)) return -1;
    for (size_t k = 0; k < J; ++k)
        HIPCHK(hipMemcpyAsync(e->hMom + kTagMomentSums * k, e->jobs[k]->dOut, kTagMomentSums * sizeof(double),
                              hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t k = 0; k < J; ++k) mdmc::moments_qt_from_sums(e->hMom + kTagMomentSums * k, out4 + 4 * k);
    if (distX) std::copy_n(e->hDist.get(), J * TKDE_BINS, distX);
    return 0;
}

extern "C" int mdmc_ensemble_qt_launches(mdmc_ensemble* e, unsigned long long* out) {
    if (!e || !out) return set_error("mdmc_ensemble_qt_launches: NULL argument");
    if (need_qt(e, "mdmc_ensemble_qt_launches")) return -1;
    *out = e->qtLaunches;
    return 0;
}

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
    for (hipEvent_t ev : e->evDist)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->evMember) (void)hipEventDestroy(ev);
    if (e->evEns) (void)hipEventDestroy(e->evEns);
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
        e->dArgs.alloc(J) != hipSuccess || e->hArgs.alloc(2 * J) != hipSuccess ||
        e->hMT.alloc(J * 625) != hipSuccess || e->hAcc.alloc(J) != hipSuccess)
        return set_error("mdmc_ensemble_create: allocating the argument blocks of %d jobs failed", njobs);
    if (md_blocks_create(e.get())) return -1;
    if (e->jobs[0]->qt && qt_blocks_create(e.get())) return -1;
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
        if (e->timing && e->annealTimer.take(&e0, &e1)) return -1;
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

// MDStep() x n of every member (:504-511) on the run's lanes: md_batch 0, each step queued member by member on
// the members' own streams; md_batch 1, one batched stretch on the ensemble's stream (none for nsteps <= 0)
extern "C" int mdmc_ensemble_md_steps(mdmc_ensemble* e, int nsteps) {
    if (!e) return set_error("NULL ensemble");
    HIPCHK(hipSetDevice(e->dev));
    if (nsteps > 0) {
        const std::vector<mdmc::MdLane> lanes = mdmc::md_lanes(e->jobs.data(), (int)e->jobs.size(), e);
        bool ok = true;
        for (const mdmc::MdLane& l : lanes) ok = ok && !l.begin();
        for (int k = 0; ok && k < nsteps; ++k)
            for (const mdmc::MdLane& l : lanes) ok = ok && !l.md_step();
        for (const mdmc::MdLane& l : lanes) ok = ok && !l.end();
        e->open = false;                       // a failed stretch is abandoned
        if (!ok) return -1;
    }
    if (sync_members(e)) return -1;
    for (mdmc_ctx* c : e->jobs) c->hitOff = 0;
    return 0;
}

// main() of every job in lockstep (:1030-1167; QTT:1140-1254): the stages of mdmc_run
extern "C" int mdmc_ensemble_run(mdmc_ensemble* e, int verbose) {
    if (!e) return set_error("NULL ensemble");
    HIPCHK(hipSetDevice(e->dev));
    std::fill(e->stage_ms, e->stage_ms + mdmc_ensemble::kStages, 0.);
    if (mdmc::run_members(e->jobs.data(), (int)e->jobs.size(), e, verbose)) {
        e->open = false;                       // a failed stretch is abandoned
        return -1;
    }
    return sync_members(e);
}

extern "C" int mdmc_ensemble_enable_timing(mdmc_ensemble* e, int on) {
    if (!e) return set_error("NULL ensemble");
    e->timing = on > 0;
    for (LaunchTimer* t : {&e->annealTimer, &e->forceTimer, &e->vvTimer, &e->qtTimer, &e->distTimer}) t->reset();
    return 0;
}

extern "C" int mdmc_ensemble_set_md_batch(mdmc_ensemble* e, int mode) {
    if (!e) return set_error("mdmc_ensemble_set_md_batch: NULL ensemble");
    if (mode != 0 && mode != 1) return set_error("mdmc_ensemble_set_md_batch: mode must be 0 (member by member) or 1 (batched), not %d", mode);
    e->mdBatch = mode;
    return 0;
}

extern "C" int mdmc_ensemble_md_batch(const mdmc_ensemble* e) {
    if (!e) return set_error("mdmc_ensemble_md_batch: NULL ensemble");
    return e->mdBatch;
}

extern "C" int mdmc_ensemble_md_launches(mdmc_ensemble* e, unsigned long long* out) {
    if (!e || !out) return set_error("mdmc_ensemble_md_launches: NULL argument");
    *out = e->mdLaunches;
    return 0;
}

// the batched launches' own durations (their dispatch timestamps) since the last call: out[0..5) = the anneal's
// sum (ms), launches, median, minimum, maximum (ms); out[5..11) = wall time (ms) of the last run's stages: anneal,
// pre-record MD, QT pump, recorded MD, autocorrelations, the rest; out[11..16) and out[16..21) = the five figures
// of the batched force and velocity-Verlet launches (md_batch 1); out[21..26) and out[26..31) = those of the
// batched QT launches and of the X distribution's chunk kernel.  Fills what n holds (n >= 3); resets the lists
extern "C" int mdmc_ensemble_kernel_times(mdmc_ensemble* e, double* out, int n) {
    if (!e || !out) return set_error("mdmc_ensemble_kernel_times: NULL argument");
    if (n < 3) return set_error("mdmc_ensemble_kernel_times: need at least 3 doubles");
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->stream));
    constexpr int kOut = 5 + mdmc_ensemble::kStages + 20;
    double v[kOut] = {};
    if (e->annealTimer.stats(v) || e->forceTimer.stats(v + 5 + mdmc_ensemble::kStages) ||
        e->vvTimer.stats(v + 10 + mdmc_ensemble::kStages) || e->qtTimer.stats(v + 15 + mdmc_ensemble::kStages) ||
        e->distTimer.stats(v + 20 + mdmc_ensemble::kStages))
        return -1;
    std::copy(e->stage_ms, e->stage_ms + mdmc_ensemble::kStages, v + 5);
    for (int i = 0; i < n && i < kOut; ++i) out[i] = v[i];
    return 0;
}
