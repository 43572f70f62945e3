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
//
// The pooled output() (options "pool" and "member_files", mdqt_ensemble_pool_observables): what the users of the
// reference's job array look at is the average over the jobs of a laser setting.  A pooled pass is the batched
// pass plus two launches (mdqt_ensemble_pool.hip: the S / P / D populations binned against vx over all ions of a
// point's replicas, from the packed columns where they lie) whose result [npoints][kPopPlanes][kPopSlots] follows
// the rows on the device and comes back in the rows' copy; the means, standard errors and summed velocity
// distributions of a point are host sums over the rows' published values (pool_points: R x 6,010 additions per
// point).  With member_files 0 the packed columns are not copied to the host at all.

#include <errno.h>
#include <math.h>
#include <sys/stat.h>

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
    const double* pool = nullptr;  // a pooled pass: [npoints][kPopPlanes][kPopSlots]
};

constexpr size_t kPopPoint = (size_t)kPopPlanes * kPopSlots;

bool batched(const mdqt_ctx* s, int variant) {
    return potential_on_tiles(s) && observables_w1_applies(s) && (variant < 0 || s->force_variant == variant);
}

// pool: also the points' slot sums (what = kObsPack, every member batched: ens_pool_check has passed); cols: copy
// the packed columns to the host
int ens_observe(mdqt_ensemble* e, ObsWhat what, EnsObs& r, bool sync = true, bool pool = false, bool cols = true) {
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
    const size_t npool = pool ? (size_t)e->npoints * kPopPoint : 0;
    if (pool && (size_t)J * kObsRow + npool > e->dObsRows.capacity()) {      // the rows, then the points' slot sums
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(e->dObsRows.reserve((size_t)J * kObsRow + npool));
    }
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
    if (pool) {
        hipEvent_t p[4] = {nullptr, nullptr, nullptr, nullptr};
        if (e->timing && (e->obs_timers[2].take(&p[0], &p[1]) || e->obs_timers[3].take(&p[2], &p[3]))) return -1;
        HIPCHK(launch_popv_ens(e->dObs, e->npoints, nb / e->npoints, maxch, e->dObsRows + (size_t)nb * kObsRow, e->stream, p[0],
                               p[1], p[2], p[3]));
        e->output_launches += 2;
    }

    r.stride = what == kObsEpot ? 64 : (size_t)kObsRow;
    const size_t nrows = (size_t)nb * r.stride, ncols = what >= kObsPack && cols ? total : 0;
    const size_t need = (nrows + npool + ncols) * sizeof(double);
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
    else HIPCHK(hipMemcpyAsync(h, e->dObsRows, (nrows + npool) * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (ncols) HIPCHK(hipMemcpyAsync(h + nrows + npool, e->dObsCols, ncols * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    r.rows = h;
    r.pool = h + nrows;
    r.cols = h + nrows + npool;
    return 0;
}

// the pooled observables of every point, as mdqt_ensemble_pool_observables publishes them
struct EnsPooled {
    std::vector<double> mean7, sem6, Pvel, spd;    // [P][7], [P][6], [P][3 NBINS], [P][3][kPopSlots]
    std::vector<long long> count;                  // [P][kPopSlots]
};

// from the members' published out7 [J][7] and Pvel [J][3 NBINS] and the pass's slot sums: the replicas of a point in
// ascending order
void pool_points(const mdqt_ensemble* e, const double* out7, const double* Pvel, const double* slots, EnsPooled& o) {
    const size_t P = (size_t)e->npoints, R = e->jobs.size() / P;
    o.mean7.assign(P * 7, 0.);
    o.sem6.assign(P * 6, 0.);
    o.Pvel.assign(P * 3 * NBINS, 0.);
    o.spd.resize(P * 3 * kPopSlots);
    o.count.resize(P * kPopSlots);
    for (size_t q = 0; q < P; ++q) {
        mdqt_pool_rows(out7 + q * R * 7, (int)R, o.mean7.data() + q * 7, o.sem6.data() + q * 6);
        double* pv = o.Pvel.data() + q * 3 * NBINS;
        for (size_t r = 0; r < R; ++r) {
            const double* m = Pvel + (q * R + r) * 3 * NBINS;
            for (int j = 0; j < 3 * NBINS; ++j) pv[j] += m[j];
        }
        memcpy(o.count.data() + q * kPopSlots, slots + q * kPopPoint, kPopSlots * sizeof(long long));   // plane 0: integers
        memcpy(o.spd.data() + q * 3 * kPopSlots, slots + q * kPopPoint + kPopSlots, (size_t)3 * kPopSlots * sizeof(double));
    }
}

int pool_directory(const mdqt_params* p, int njobs, char* buf, size_t cap) {
    char name[256];
    speedup_run_name(p, name, sizeof name);
    const int n = snprintf(buf, cap, "%.255s%s/pool_job%dto%d/", p->saveDirectory, name, (int)p->job, (int)p->job + njobs - 1);
    if (n < 0 || (size_t)n >= cap) return set_error("the pooled directory's name needs %d bytes", n + 1);
    return 0;
}

// The pooled files of every point (docs/PROGRAMS.md "Pooled output()"), %lg text as the members': the three
// appended files' lines here, in order; the velocity distributions and the velocity-resolved populations from a
// snapshot by the ensemble's writers.  counter: the first replica's, before this output() counted.
int pool_files(mdqt_ensemble* e, std::shared_ptr<EnsPooled> pl, const std::vector<int>& counter) {
    const int R = (int)e->jobs.size() / e->npoints;
    for (int q = 0; q < e->npoints; ++q) {
        const mdqt_ctx* s = e->jobs[(size_t)q * R];
        char dir[1400], run[1400];
        if (pool_directory(&s->p, R, dir, sizeof dir)) return -1;
        char name[256];
        speedup_run_name(&s->p, name, sizeof name);
        snprintf(run, sizeof run, "%.255s%s", s->p.saveDirectory, name);
        mkdir(s->p.saveDirectory, 0777);
        mkdir(run, 0777);
        mkdir(dir, 0777);
        const std::string d(dir);
        const double* m = pl->mean7.data() + (size_t)q * 7;
        const double* se = pl->sem6.data() + (size_t)q * 6;
        const long long* cnt = pl->count.data() + (size_t)q * kPopSlots;
        const double* spd = pl->spd.data() + (size_t)q * 3 * kPopSlots;
        FILE* fa = fopen((d + "energies.dat").c_str(), "a");
        if (!fa) return set_error("cannot open %senergies.dat: %s", dir, strerror(errno));
        fprintf(fa, "%lg\t%lg\t%lg\t%lg\t%lg\t%lg\t%lg\n", m[0], m[1], m[2], m[3], m[4], m[5], m[6]);
        fclose(fa);
        if (!(fa = fopen((d + "energies_sem.dat").c_str(), "a"))) return set_error("cannot open %senergies_sem.dat: %s", dir, strerror(errno));
        fprintf(fa, "%lg\t%lg\t%lg\t%lg\t%lg\t%lg\t%lg\n", m[0], se[0], se[1], se[2], se[3], se[4], se[5]);
        fclose(fa);
        long long total = 0;
        double tot[3] = {0., 0., 0.};
        for (int b = 0; b < kPopSlots; ++b) {
            total += cnt[b];
            for (int c = 0; c < 3; ++c) tot[c] += spd[(size_t)c * kPopSlots + b];
        }
        if (!(fa = fopen((d + "populations.dat").c_str(), "a"))) return set_error("cannot open %spopulations.dat: %s", dir, strerror(errno));
        fprintf(fa, "%lg\t%lg\t%lg\t%lg\t%lg\t%lg\n", m[0], tot[0] / (double)total, tot[1] / (double)total, tot[2] / (double)total,
                (double)total, (double)cnt[kPopSlots - 1]);
        fclose(fa);
        const double* vel = s->vel;                                  // constant bin centres (every member's)
        const char* axes[3] = {"X", "Y", "Z"};
        char b[64];
        for (int a = 0; a < 3; ++a) {
            snprintf(b, sizeof b, "vel_dist%s_time%06d.dat", axes[a], counter[(size_t)q]);
            const double shift = a == 0 ? m[6] : 0.;
            e->writer->submit(d + b, "w", [pl, vel, q, a, shift](LgText& t) {
                const double* p = pl->Pvel.data() + ((size_t)q * 3 + a) * NBINS;
                for (int i = 0; i < NBINS; i++) {
                    t.num(vel[i] + shift); t.ch('\t'); t.num(p[i]); t.ch('\n');
                }
            });
        }
        snprintf(b, sizeof b, "statePopulationsVsV_time%06d.dat", counter[(size_t)q]);
        e->writer->submit(d + b, "w", [pl, q](LgText& t) {
            const long long* cnt = pl->count.data() + (size_t)q * kPopSlots;
            const double* spd = pl->spd.data() + (size_t)q * 3 * kPopSlots;
            for (int b = 0; b < kPopSlots - 1; ++b) {                // the 1,001 slots with a centre
                const double n = (double)cnt[b];
                t.num((double)(b - 500) * 0.01); t.ch('\t'); t.num(n);
                for (int c = 0; c < 3; ++c) { t.ch('\t'); t.num(cnt[b] ? spd[(size_t)c * kPopSlots + b] / n : 0.); }
                t.ch('\n');
            }
        });
    }
    return 0;
}

}  // namespace

// mean7 / sem6 of R replicas' out7 rows: sequential sums in replica order onto 0, one division each
extern "C" int mdqt_pool_rows(const double* out7, int R, double* mean7, double* sem6) {
    if (!out7 || !mean7 || !sem6) return set_error("mdqt_pool_rows: NULL argument");
    if (R < 1) return set_error("mdqt_pool_rows: R = %d replicas (at least 1)", R);
    mean7[0] = out7[0];                                              // t: the first replica's (the members are in lockstep)
    for (int c = 1; c < 7; ++c) {
        double sum = 0.;
        for (int r = 0; r < R; ++r) sum += out7[(size_t)7 * r + c];
        mean7[c] = sum / (double)R;
        double ss = 0.;
        for (int r = 0; r < R; ++r) {
            const double d = out7[(size_t)7 * r + c] - mean7[c];
            ss += d * d;
        }
        sem6[c - 1] = R > 1 ? sqrt(ss / ((double)R * (double)(R - 1))) : 0.;
    }
    return 0;
}

extern "C" int mdqt_ensemble_pool_directory(const mdqt_params* points, int npoints, int njobs, int point, char* buf, size_t cap) {
    if (!points || !buf) return set_error("mdqt_ensemble_pool_directory: NULL argument");
    if (npoints < 1 || njobs < 1) return set_error("mdqt_ensemble_pool_directory: npoints and njobs must be >= 1");
    if (point < 0 || point >= npoints) return set_error("mdqt_ensemble_pool_directory: point index %d outside [0, %d)", point, npoints);
    return pool_directory(points + point, njobs, buf, cap);
}

int mdqt::ens_pool_check(const mdqt_ensemble* e, const char* what) {
    if (!e->output_batch)
        return set_error("%s: the pooled sums come from the batched pass: set output_batch 1 (it is 0)", what);
    const int J = (int)e->jobs.size();
    for (int k = 0; k < J; ++k) {
        const mdqt_ctx* s = e->jobs[(size_t)k];
        if (!s->use_n3 && !s->use_n3b)
            return set_error("%s: job index %d has %d ions on the owner-computes rows: set force_scheme 2 (a pooled pass takes "
                             "every member on the Newton-3 tiles)", what, k, s->N);
        if (!batched(s, -1))
            return set_error("%s: job index %d takes its own output pass (potential_n3 %d, force_kernel %d, N = %d): a pooled "
                             "pass takes every member in the batched one", what, k, (int)s->n3_potential, s->force_variant, s->N);
        if (s->force_variant != e->jobs[0]->force_variant)
            return set_error("%s: job index %d has force_kernel %d and job index 0 has %d: one batched potential launch is one "
                             "kernel", what, k, s->force_variant, e->jobs[0]->force_variant);
    }
    return 0;
}

// output() of every member (the files are left to the writers: the caller flushes)
int mdqt::ens_output(mdqt_ensemble* e) {
    const bool pool = e->pool != 0, files = e->member_files != 0;
    if (!pool && !files)
        return set_error("output() of the ensemble: member_files 0 with pool 0 would write nothing: set pool 1 (or member_files 1)");
    if (pool && ens_pool_check(e, "output() of the ensemble with pool 1")) return -1;
    const size_t J = e->jobs.size();
    EnsObs r;
    if (e->output_batch && ens_observe(e, kObsPack, r, true, pool, files)) return -1;
    std::vector<double> o7, Pall;                               // a pooled pass: every member's published out7 and Pvel
    std::vector<int> counter;                                   // and each point's first replica's counter
    if (pool) {
        o7.resize(J * 7);
        Pall.resize(J * 3 * NBINS);
        for (size_t k = 0; k < J; k += J / (size_t)e->npoints) counter.push_back(e->jobs[k]->counter);
    }
    size_t q = 0;
    for (int k = 0; k < (int)J; ++k) {
        mdqt_ctx* s = e->jobs[(size_t)k];
        if (q == r.member.size() || r.member[q] != k) {          // its own pass and synchronisation
            if (output_async(s)) return -1;
            continue;
        }
        const size_t n1 = (size_t)(s->N > 0 ? s->N : 1);
        double o[7];
        auto P = std::make_shared<std::vector<double>>((size_t)3 * NBINS);
        if (files) {
            auto pops = std::make_shared<std::vector<double>>(3 * n1);
            auto V = std::make_shared<std::vector<double>>(3 * n1, 0.);
            observables_from_rows(s, r.rows + q * r.stride, r.cols + r.col0[q], o, P->data(), pops->data(), V->data());
            if (output_files(s, o, P, pops, V)) return -1;
        } else {                                                 // Epot and the counter as output() leaves them, no file
            observables_from_rows(s, r.rows + q * r.stride, nullptr, o, P->data(), nullptr, nullptr);
            s->counter++;
        }
        if (pool) {
            memcpy(o7.data() + (size_t)7 * k, o, sizeof o);
            memcpy(Pall.data() + (size_t)3 * NBINS * k, P->data(), (size_t)3 * NBINS * sizeof(double));
        }
        ++q;
    }
    if (pool) {
        auto pl = std::make_shared<EnsPooled>();
        pool_points(e, o7.data(), Pall.data(), r.pool, *pl);
        if (pool_files(e, pl, counter)) return -1;
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

// the pooled observables of every point in one pooled pass, no files
extern "C" int mdqt_ensemble_pool_observables(mdqt_ensemble* e, double* mean7, double* sem6, double* Pvel, long long* count,
                                              double* spd) {
    if (ens_check(e, "mdqt_ensemble_pool_observables")) return -1;
    if (!mean7 || !sem6) return set_error("mdqt_ensemble_pool_observables: NULL argument (mean7: 7, sem6: 6 doubles per point)");
    if (e->pump) return set_error("mdqt_ensemble_pool_observables: the pump programs' output() has no pooled pass");
    if (ens_pool_check(e, "mdqt_ensemble_pool_observables")) return -1;
    HIPCHK(hipSetDevice(e->dev));
    EnsObs r;
    if (ens_observe(e, kObsPack, r, true, true, false)) return -1;
    const size_t J = e->jobs.size();
    std::vector<double> o7(J * 7), Pall(J * 3 * NBINS);
    for (size_t k = 0; k < J; ++k)
        observables_from_rows(e->jobs[k], r.rows + k * r.stride, nullptr, o7.data() + 7 * k, Pall.data() + (size_t)3 * NBINS * k,
                              nullptr, nullptr);
    EnsPooled pl;
    pool_points(e, o7.data(), Pall.data(), r.pool, pl);
    memcpy(mean7, pl.mean7.data(), pl.mean7.size() * sizeof(double));
    memcpy(sem6, pl.sem6.data(), pl.sem6.size() * sizeof(double));
    if (Pvel) memcpy(Pvel, pl.Pvel.data(), pl.Pvel.size() * sizeof(double));
    if (count) memcpy(count, pl.count.data(), pl.count.size() * sizeof(long long));
    if (spd) memcpy(spd, pl.spd.data(), pl.spd.size() * sizeof(double));
    return 0;
}

extern "C" int mdqt_ensemble_epotential(mdqt_ensemble* e, double* Epot) {    // Epotential() of every job, :244-281
    if (ens_check(e, "mdqt_ensemble_epotential")) return -1;
    if (!Epot) return set_error("mdqt_ensemble_epotential: NULL argument (Epot: one double per job)");
    HIPCHK(hipSetDevice(e->dev));
    return ens_epotential(e, Epot);
}

extern "C" unsigned long long mdqt_ensemble_output_launches(const mdqt_ensemble* e) { return e ? e->output_launches : 0; }
