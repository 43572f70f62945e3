// mdqt_ensemble's batched output() (include/mdqt.h, "ensembles": mdqt_ensemble_output, _observables,
// _epotential) — output()'s observables (SpeedUp:917-1032) and Epotential() (:244-281) of every member in
// six launches, two device-to-host copies and one synchronisation, where the members' own passes
// (observables_w1, mdqt_observables.cpp) are seven launches, two copies and a synchronisation each.
//
// A member is batched when its own pass would take potential_rows' Newton-3 tile branch and observables_w1:
// its blocks are then what that pass builds (potential_n3_block: the force call's block with the plain
// tile-pair table into the potential's own slots, so pending force slots stay pending and untouched), the
// batched kernels run the single-job kernels' bodies on them (mdqt_ensemble_obs.hip), and the host end is
// the same function (observables_from_rows) — every number is bit for bit the member's own.  The one
// difference in the launch sequence: k_sum_vx and k_energy_sums are one kernel (the same workgroup shape,
// the same sums in the same order, <vx> the same division).  Any other member (below 128 ions on the
// owner-computes rows, potential_n3 0, another force_kernel than the first batched member's) takes its own
// pass, as ens_forces gives a row member its own force launch.
//
// The blocks seldom change (pointers, sizes): they travel through the ensemble's argument ring when they
// differ from what the device holds.  The results land in ensemble-owned device buffers — a scratch row
// [kObsRow] per member in dScr's layout, the packed columns [sum 4 N_k] — and come back in one copy each
// into a pinned slot.

#include <algorithm>

#include "mdqt_ensemble.hpp"

using namespace mdqt;

namespace {

static_assert(sizeof(EnsObsArgs) <= sizeof(N3Args), "either kind of block fits the argument ring's slot of njobs N3Args");

enum ObsWhat : int { kObsEpot = 0, kObsKde = 1, kObsPack = 2 };   // the sums; + the KDE; + the per-ion columns

// what one batched pass left on the host (the pinned slot: valid until the next pass)
struct EnsObs {
    std::vector<int> member;       // the batched members' job indices, ascending
    std::vector<size_t> col0;      // their offsets into cols (doubles)
    const double* rows = nullptr;  // [members][stride]
    size_t stride = 0;             // kObsRow, or 64 (the sums only)
    const double* cols = nullptr;
};

bool batched(const mdqt_ctx* s, int variant) {
    return potential_on_tiles(s) && observables_w1_applies(s) && (variant < 0 || s->force_variant == variant);
}

int ens_observe(mdqt_ensemble* e, ObsWhat what, EnsObs& r, bool sync = true) {
    const int J = (int)e->jobs.size();
    int variant = -1;
    size_t total = 0;
    for (int k = 0; k < J; ++k) {
        const mdqt_ctx* s = e->jobs[k];
        if (!batched(s, variant)) continue;
        variant = s->force_variant;
        r.member.push_back(k);
        r.col0.push_back(total);
        total += (size_t)4 * s->N;
    }
    const int nb = (int)r.member.size();
    if (nb == 0) return 0;
    if (e->dPot.reserve((size_t)J) != hipSuccess || e->dObs.reserve((size_t)J) != hipSuccess ||
        e->dObsRows.reserve((size_t)J * kObsRow) != hipSuccess)
        return set_error("allocating the output blocks and rows of %d jobs failed", J);
    if (total > e->dObsCols.capacity()) {
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(e->dObsCols.reserve(total));
    }
    std::vector<N3Args> pot((size_t)nb);
    std::vector<EnsObsArgs> obs((size_t)nb);
    int maxp = 0, maxN = 0, maxch = 0;
    bool guard = false;
    for (int q = 0; q < nb; ++q) {
        mdqt_ctx* s = e->jobs[(size_t)r.member[(size_t)q]];
        N3Args& a = pot[(size_t)q];
        if (potential_n3_block(s, a)) return -1;
        guard = guard || a.guard;
        maxp = std::max(maxp, a.npairs);
        EnsObsArgs& b = obs[(size_t)q];
        memset(&b, 0, sizeof b);
        b.V = s->dV; b.psi = s->dPsi; b.Upart = s->dUpart; b.Urow = s->dUrow; b.kde = s->dKde;
        b.scr = e->dObsRows + (size_t)q * kObsRow;
        b.pack = e->dObsCols + r.col0[(size_t)q];
        b.N = s->N; b.S = s->S; b.nslots = s->nslots;
        b.nch = std::min(std::max(s->N / 32, 1), s->kdeChunks);      // observables_w1's
        b.chunk = (s->N + b.nch - 1) / b.nch;                        // launch_kde's
        b.model = s->p.qt_model;
        maxN = std::max(maxN, b.N);
        maxch = std::max(maxch, b.nch);
    }
    if (e->ring.send_if_changed(pot, e->pot_held, e->dPot, e->stream)) return -1;
    if (e->ring.send_if_changed(obs, e->obs_held, e->dObs, e->stream)) return -1;

    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e->timing && e->obs_timers[0].take(&e0, &e1)) return -1;
    HIPCHK(launch_potential_n3_ens(e->dPot, nb, maxp, variant, guard, e->stream, e0, e1));
    HIPCHK(launch_potential_sums_ens(e->dObs, nb, maxN, e->stream));
    e->output_launches += 3;
    if (what >= kObsKde) {
        e0 = e1 = nullptr;
        if (e->timing && e->obs_timers[1].take(&e0, &e1)) return -1;
        HIPCHK(launch_kde_ens(e->dObs, nb, maxch, e->stream, e0, e1));
        e->output_launches += 2;
    }
    if (what >= kObsPack) {
        HIPCHK(launch_output_pack_ens(e->dObs, nb, maxN, e->stream));
        e->output_launches += 1;
    }

    r.stride = what == kObsEpot ? 64 : (size_t)kObsRow;
    const size_t nrows = (size_t)nb * r.stride, ncols = what >= kObsPack ? total : 0;
    const size_t need = (nrows + ncols) * sizeof(double);
    if (e->obs_ring.slot_bytes < need) {
        e->obs_ring.destroy();
        if (e->obs_ring.create(need + need / 4, 1, hipEventDisableTiming)) return -1;
    }
    char* slot = nullptr;
    int idx = 0;
    if (e->obs_ring.take(&slot, &idx)) return -1;
    double* h = reinterpret_cast<double*>(slot);
    if (what == kObsEpot)
        HIPCHK(hipMemcpy2DAsync(h, 64 * sizeof(double), e->dObsRows, kObsRow * sizeof(double), 64 * sizeof(double), (size_t)nb,
                                hipMemcpyDeviceToHost, e->stream));
    else HIPCHK(hipMemcpyAsync(h, e->dObsRows, nrows * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (ncols) HIPCHK(hipMemcpyAsync(h + nrows, e->dObsCols, ncols * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    r.rows = h;
    r.cols = h + nrows;
    return 0;
}

}  // namespace

// output() of every member (the files are left to the writers: the caller flushes)
int mdqt::ens_output(mdqt_ensemble* e) {
    EnsObs r;
    if (e->output_batch && ens_observe(e, kObsPack, r)) return -1;
    size_t q = 0;
    for (int k = 0; k < (int)e->jobs.size(); ++k) {
        mdqt_ctx* s = e->jobs[(size_t)k];
        if (q == r.member.size() || r.member[q] != k) {          // its own pass and synchronisation
            if (output_async(s)) return -1;
            continue;
        }
        const size_t n1 = (size_t)(s->N > 0 ? s->N : 1);
        double o[7];
        auto P = std::make_shared<std::vector<double>>((size_t)3 * NBINS);
        auto pops = std::make_shared<std::vector<double>>(3 * n1);
        auto V = std::make_shared<std::vector<double>>(3 * n1, 0.);
        observables_from_rows(s, r.rows + q * r.stride, r.cols + r.col0[q], o, P->data(), pops->data(), V->data());
        if (output_files(s, o, P, pops, V)) return -1;
        ++q;
    }
    return 0;
}

double mdqt::ens_epot_of(const mdqt_ctx* s, const double* row) {
    return s->N > 0 ? (row[19] / 2.) / (double)s->N : 0.;        // mdqt_epotential's (:280)
}

int mdqt::ens_epotential_queue(mdqt_ensemble* e, std::vector<int>& member, const double** rows) {
    EnsObs r;
    if (ens_observe(e, kObsEpot, r, false)) return -1;
    member = r.member;
    *rows = r.rows;
    return 0;
}

// Epotential() of every member: the potential, slot-sum and sums launches only
int mdqt::ens_epotential(mdqt_ensemble* e, double* Epot) {
    EnsObs r;
    if (e->output_batch && ens_observe(e, kObsEpot, r)) return -1;
    size_t q = 0;
    for (int k = 0; k < (int)e->jobs.size(); ++k) {
        mdqt_ctx* s = e->jobs[(size_t)k];
        if (q == r.member.size() || r.member[q] != k) {
            if (mdqt_epotential(s, Epot ? Epot + k : nullptr)) return -1;
            continue;
        }
        s->Epot = ens_epot_of(s, r.rows + q * r.stride);
        if (Epot) Epot[k] = s->Epot;
        ++q;
    }
    return 0;
}

extern "C" int mdqt_ensemble_output(mdqt_ensemble* e) {           // output() of every job, SpeedUp:917-1032
    if (ens_check(e, "mdqt_ensemble_output")) return -1;
    HIPCHK(hipSetDevice(e->dev));
    if (ens_output(e)) return -1;
    return flush_files(e->jobs[0]);                      // the shared pool: every member's files
}

extern "C" int mdqt_ensemble_observables(mdqt_ensemble* e, double* out7, double* Pvel, double* pops) {
    if (ens_check(e, "mdqt_ensemble_observables")) return -1;
    if (!out7) return set_error("mdqt_ensemble_observables: NULL argument (out7: 7 doubles per job)");
    HIPCHK(hipSetDevice(e->dev));
    EnsObs r;
    if (e->output_batch && ens_observe(e, pops ? kObsPack : kObsKde, r)) return -1;
    size_t q = 0, ion0 = 0;
    for (int k = 0; k < (int)e->jobs.size(); ++k) {
        mdqt_ctx* s = e->jobs[(size_t)k];
        double* o = out7 + (size_t)7 * k;
        double* P = Pvel ? Pvel + (size_t)3 * NBINS * k : nullptr;
        double* pp = pops ? pops + 3 * ion0 : nullptr;
        ion0 += (size_t)s->N;
        if (q == r.member.size() || r.member[q] != k) {
            if (mdqt_observables(s, o, P, pp)) return -1;
            continue;
        }
        observables_from_rows(s, r.rows + q * r.stride, r.cols + r.col0[q], o, P, pp, nullptr);
        ++q;
    }
    return 0;
}

extern "C" int mdqt_ensemble_epotential(mdqt_ensemble* e, double* Epot) {    // Epotential() of every job, :244-281
    if (ens_check(e, "mdqt_ensemble_epotential")) return -1;
    if (!Epot) return set_error("mdqt_ensemble_epotential: NULL argument (Epot: one double per job)");
    HIPCHK(hipSetDevice(e->dev));
    return ens_epotential(e, Epot);
}

extern "C" unsigned long long mdqt_ensemble_output_launches(const mdqt_ensemble* e) { return e ? e->output_launches : 0; }
