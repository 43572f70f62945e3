// ---------------------------------------------------------------------------------------------
// observables (Epotential :244-281, output :917-1032)
// ---------------------------------------------------------------------------------------------

#include <math.h>

#include "mdqt_ctx.hpp"

using namespace mdqt;

// does potential_rows take the Newton-3 tile kernel's POT mode for this context?
bool mdqt::potential_on_tiles(const mdqt_ctx* s) {
    return s->use_n3 && !s->use_n3b && s->p.world_size == 1 && s->local.empty() && s->force_variant <= 1 &&
           s->n3_potential;
}

// the potential launch's block on the tiles: the force call's block with the plain table, into the
// potential's own slots (one plane per slot: component 0) — pending force slots stay pending and untouched
int mdqt::potential_n3_block(mdqt_ctx* s, N3Args& a) {
    const size_t need = (size_t)s->nslots * s->S;
    HIPCHK(s->dUpart.reserve(need));
    if (n3_force_args(s, a, true)) return -1;
    a.P = s->dUpart;
    a.arrive = nullptr;
    return 0;
}

// device: scratch[0] = sum over owned rows of the full-row pair potential.  World 1, partials up
// to 64 MB: the potential rows get a buffer of their own, so pending force slots stay pending
// (the next substep launch sums them in its prologue: no reduce launch, and that launch stays the
// production instance); otherwise they reuse the force partials after settling them.
static int potential_rows(mdqt_ctx* s, double* urow_dev) {
    if (s->nloc == 0) return 0;
    // world 1 with the Newton-3 tile scheme: each distinct pair's potential once (the tile kernel's
    // POT mode), the ntiles slots of component 0 summed per ion (half the pair evaluations of the
    // rows; the same per-ion row sums up to summation order)
    if (potential_on_tiles(s)) {
        N3Args a;
        if (potential_n3_block(s, a)) return -1;
        HIPCHK(launch_potential_n3(a, s->force_variant, s->stream));
        HIPCHK(launch_reduce_segments(s->dUpart, urow_dev, s->nslots, s->nloc, s->S, 1, s->stream, (size_t)s->S));
        return 0;
    }
    // world 1 with Newton-3 blocks (N > 65,536): the block kernel's POT mode, per-ion row sums by
    // k_n3b_reduce (the block slots are free between force calls: the force path reduces at once)
    // Round 6 (option potential_plan): on the force call's plan — the same skip radius,
    // sub-tile groups and error-bounded forms (pair_u_cut, the f32 ultra-far form), the same measured and
    // enforced tail (tiles whose sub-tile force sums exceed eps get their U_i recomputed exactly).  Since
    // u(r) < lDeb g(r) and each form's relative error on u is at most its error on the force, every U_i is
    // within lDeb x (the force call's per-ion bound: tail eps + the tiers') of its sum to L/2, and Epot =
    // sum U_i / 2N within half that (C4, N = 1M: ~1e-12 absolute on Epot ~ 5; north_star asks 1e-6
    // relative).  Tests: tests/test_gpu_large.py test_epotential_on_the_plan.
    if (s->use_n3b && s->p.world_size == 1 && s->local.empty() && s->force_variant <= 1 && s->n3_potential) {
        if (settle_forces(s)) return -1;
        N3BArgs a;
        if (n3b_args(s, a)) return -1;
        const bool planned = s->pot_plan && a.plan && s->force_variant == 1 && !a.guard;
        if (!planned) {
            a.plan = nullptr; a.tmask = nullptr; a.tmw = 0; a.tailb = nullptr;
            a.Rskip = a.Rcut;                       // (the no-plan kernel skips only beyond L/2 for potentials)
        } else if (a.tailb) {
            HIPCHK(hipMemsetAsync(a.tailb, 0, (size_t)4 * a.T * sizeof(double), s->stream));
            HIPCHK(hipMemsetAsync(s->dTailSt + 8 + 3, 0, sizeof(unsigned long long), s->stream));
        }
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (s->timing && (s->tkinds & 4u) && take_events(s, 3, &e0, &e1)) return -1;
        HIPCHK(launch_potential_n3b(a, s->force_variant, urow_dev, s->stream, e0, e1));
        if (a.tailb) {                              // the enforcement (its own counters: dTailSt[8, 16))
            HIPCHK(launch_tail_max(a.tailb, a.T, error_eps(s, a), s->dTailSt + 8, s->dTailList, s->stream));
            HIPCHK(launch_tail_fix(a, s->dTailSt + 8, s->dTailList, urow_dev, s->stream, true));
        }
        return 0;
    }
    double* buf = s->dFpart;
    const size_t need = (size_t)s->nseg * 3 * s->S;
    if (s->p.world_size == 1 && s->local.empty() && need * sizeof(double) <= ((size_t)64 << 20)) {
        HIPCHK(s->dUpart.reserve(need));
        buf = s->dUpart;
    } else if (settle_forces(s)) {
        return -1;
    }
    HIPCHK(launch_potential_rows(force_args(s, buf), s->stream));
    HIPCHK(launch_reduce_segments(buf, urow_dev, s->nseg, s->nloc, s->S, 1, s->stream));
    return 0;
}

extern "C" int mdqt_partial_observables(mdqt_ctx* s, double vxAvg, double out5[5], double* Pvel) {
    if (!s) return set_error("NULL context");
    HIPCHK(hipSetDevice(s->dev));
    double* scr = s->dScr;           // [0] sum vx, [8] vxAvg, [16..19] sums, [64..] KDE bins
    if (potential_rows(s, s->dUrow)) return -1;
    HIPCHK(launch_sum_vx(s->dV, s->nloc, scr, s->stream));
    HIPCHK(hipMemcpyAsync(scr + 8, &vxAvg, sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIPCHK(launch_energy_sums(s->dV, s->nloc, s->S, scr + 8, s->dUrow, scr + 16, s->stream));
    int nch = s->nloc / 32;                                 // cold ions sit in the first bins:
    if (nch < 1) nch = 1;                                    // short chunks spread that work
    if (nch > s->kdeChunks) nch = s->kdeChunks;
    double* Pout = scr + 64;
    if (s->nloc > 0) HIPCHK(launch_kde(s->dV, s->nloc, s->S, scr + 8, s->dKde, nch, Pout, s->stream));
    else HIPCHK(hipMemsetAsync(Pout, 0, 3 * NBINS * sizeof(double), s->stream));
    double h[64 + 3 * NBINS];
    HIPCHK(hipMemcpyAsync(h, scr, sizeof h, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    out5[0] = s->nloc ? h[0] : 0.;
    out5[1] = s->nloc ? h[16] : 0.; out5[2] = s->nloc ? h[17] : 0.; out5[3] = s->nloc ? h[18] : 0.;
    out5[4] = s->nloc ? h[19] : 0.;
    if (Pvel) memcpy(Pvel, h + 64, 3 * NBINS * sizeof(double));
    return 0;
}

// the per-ion pair-potential row sums U_i that Epotential() adds up (world 1; by ion index): the same path as
// Epotential() (Newton-3 tiles or blocks — on the force call's plan unless potential_plan 0 — or rows)
extern "C" int mdqt_potential_rows(mdqt_ctx* s, double* U, int n) {
    if (!s || !U) return set_error("mdqt_potential_rows: NULL argument");
    if (s->p.world_size != 1 || !s->local.empty()) return set_error("mdqt_potential_rows: world 1 only");
    if (n < s->N) return set_error("mdqt_potential_rows: need %d doubles", s->N);
    HIPCHK(hipSetDevice(s->dev));
    if (potential_rows(s, s->dUrow)) return -1;
    HIPCHK(hipMemcpyAsync(U, s->dUrow, (size_t)s->N * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int mdqt_epotential(mdqt_ctx* s, double* Epot) {   // Epotential(), :244-281
    if (!s) return set_error("NULL context");
    double o[5];
    if (mdqt_allgather_positions(s)) return -1;          // collective when sharded
    if (mdqt_partial_observables(s, 0., o, nullptr)) return -1;
    if (mdqt_allreduce_sum(s, o, 5)) return -1;
    // sum_{i<j} u = (sum_i sum_{j != i} u) / 2 ; Epot /= N (:280)
    s->Epot = s->N > 0 ? (o[4] / 2.) / (double)s->N : 0.;
    if (Epot) *Epot = s->Epot;
    return 0;
}

// output()'s energies and velocity distributions from the device sums: sums[4] = sum vx'^2 / 2, vy^2 / 2, vz^2 / 2
// and the row potentials, kde[3 NBINS] the unnormalised bins
static void finish_observables(mdqt_ctx* s, const double* sums, double velXAvg, const double* kde, double out7[7], double* Pvel) {
    const double N = (double)s->N;
    const double EkinX = sums[0] / N, EkinY = sums[1] / N, EkinZ = sums[2] / N;                 // :945-947
    s->Epot = (sums[3] / 2.) / N;                                                               // :948
    out7[0] = s->t; out7[1] = EkinX; out7[2] = EkinY; out7[3] = EkinZ; out7[4] = s->Epot;
    out7[5] = EkinX + EkinY + EkinZ + s->Epot - s->Epot0; out7[6] = velXAvg;                   // :954
    if (Pvel) {
        const double norm = (6.0 * sqrt(2 * M_PI * 0.002 * 0.002));                            // :975-978
        for (int j = 0; j < 3 * NBINS; ++j) Pvel[j] = kde[j] / norm;
    }
}

// output()'s observables at world 1 in one device pass and one synchronisation: <vx> stays on
// the device (k_sum_vx writes sum / N for the energy sums and the KDE), the per-ion columns
// (vx, S / P / D populations) come from k_output_pack instead of a full wavefunction download.
// Same operations as the general path below (the populations: the host loop's order).
int mdqt::observables_w1(mdqt_ctx* s, double out7[7], double* Pvel, double* pops, double* vx) {
    const int N = s->N;
    double* scr = s->dScr;           // [0] sum vx, [8] vxAvg, [16..19] sums, [64..] KDE bins
    HIPCHK(hipSetDevice(s->dev));
    if (potential_rows(s, s->dUrow)) return -1;
    HIPCHK(launch_sum_vx(s->dV, N, scr, s->stream, scr + 8, N));
    HIPCHK(launch_energy_sums(s->dV, N, s->S, scr + 8, s->dUrow, scr + 16, s->stream));
    int nch = N / 32;
    if (nch < 1) nch = 1;
    if (nch > s->kdeChunks) nch = s->kdeChunks;
    HIPCHK(launch_kde(s->dV, N, s->S, scr + 8, s->dKde, nch, scr + 64, s->stream));
    const bool pack = pops || vx;
    if (pack) HIPCHK(launch_output_pack(s->dV, s->dPsi, N, s->S, s->p.qt_model, s->dPack, s->stream));
    std::vector<double> h(64 + 3 * NBINS), col(pack ? (size_t)4 * N : 0);
    HIPCHK(hipMemcpyAsync(h.data(), scr, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (pack) HIPCHK(hipMemcpyAsync(col.data(), s->dPack, col.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    observables_from_rows(s, h.data(), col.data(), out7, Pvel, pops, vx);
    return 0;
}

// the host end of observables_w1 (and of the ensemble's batched pass, mdqt_ensemble_output.cpp): h = the
// scratch row [kObsRow] as the device left it, col = the packed columns [4][N] (read only with pops or vx)
void mdqt::observables_from_rows(mdqt_ctx* s, const double* h, const double* col, double out7[7], double* Pvel,
                                 double* pops, double* vx) {
    const int N = s->N;
    const double velXAvg = h[8];
    finish_observables(s, h + 16, velXAvg, h + 64, out7, Pvel);
    if (vx) memcpy(vx, col, (size_t)N * sizeof(double));
    if (pops)
        for (int i = 0; i < N; i++) {
            pops[3 * i + 0] = col[(size_t)N + i];
            pops[3 * i + 1] = col[2 * (size_t)N + i];
            pops[3 * i + 2] = col[3 * (size_t)N + i];
        }
}

bool mdqt::observables_w1_applies(const mdqt_ctx* s) {
    return s->p.world_size == 1 && s->local.empty() && s->N > 0 && s->nloc == s->N;
}

extern "C" int mdqt_observables(mdqt_ctx* s, double out7[7], double* Pvel, double* pops) {
    if (!s) return set_error("NULL context");
    if (observables_w1_applies(s)) return observables_w1(s, out7, Pvel, pops, nullptr);
    const int N = s->N;
    double o[5];
    if (mdqt_allgather_positions(s)) return -1;          // collective when sharded
    // pass 1: <vx> (:934-938)
    HIPCHK(hipSetDevice(s->dev));
    HIPCHK(launch_sum_vx(s->dV, s->nloc, s->dScr, s->stream));
    double sumvx = 0.;
    HIPCHK(hipMemcpyAsync(&sumvx, s->dScr, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->nloc == 0) sumvx = 0.;
    if (mdqt_allreduce_sum(s, &sumvx, 1)) return -1;
    const double velXAvg = N > 0 ? sumvx / (double)N : 0.;
    std::vector<double> P((size_t)3 * NBINS + 5);
    if (mdqt_partial_observables(s, velXAvg, o, P.data())) return -1;
    memcpy(P.data() + 3 * NBINS, o, sizeof o);
    if (mdqt_allreduce_sum(s, P.data(), P.size())) return -1;
    memcpy(o, P.data() + 3 * NBINS, sizeof o);
    finish_observables(s, o + 1, velXAvg, P.data(), out7, Pvel);
    if (pops) {                                                                                 // :1016-1023
        std::vector<double> psi((size_t)24 * N, 0.);
        if (mdqt_get_state(s, nullptr, nullptr, nullptr, N, psi.data(), nullptr, nullptr)) return -1;
        if (mdqt_allreduce_sum(s, psi.data(), psi.size())) return -1;   // zero-padded gather
        for (int i = 0; i < N; i++) {
            const double* w = psi.data() + (size_t)24 * i;
            auto nrm = [&](int k) { return w[2 * k] * w[2 * k] + w[2 * k + 1] * w[2 * k + 1]; };
            pops[3 * i + 0] = nrm(0) + nrm(1);
            if (s->p.qt_model == 3) {                       // 422 pumping: P = 2, 3; D = 4
                pops[3 * i + 1] = nrm(2) + nrm(3);
                pops[3 * i + 2] = nrm(4);
            } else {
                pops[3 * i + 1] = nrm(2) + nrm(3) + nrm(4) + nrm(5);
                pops[3 * i + 2] = nrm(6) + nrm(7) + nrm(8) + nrm(9) + nrm(10) + nrm(11);
            }
        }
    }
    return 0;
}
