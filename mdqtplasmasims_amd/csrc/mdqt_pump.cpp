// ---------------------------------------------------------------------------------------------
// The optical-pumping programs' main() — randomFrozenStartTag408Linear.cpp (":" lines below), 408Quad and
// 422Linear (same flow): its pieces for one context, and mdqt_run_pump — the preamble, this context's driver
// (its operations: a context's own calls) and the time loop both pump entry points share (mdqt_main_loops.hpp).
// ---------------------------------------------------------------------------------------------

#include <math.h>

#include <functional>

#include "mdqt_ctx.hpp"

using namespace mdqt;

// measureSpinUps / tagParticles of the optical-pumping programs (see include/mdqt.h)
extern "C" int mdqt_tag_spin_up(mdqt_ctx* s, int* tags, int* n_up) {
    if (!s) return set_error("NULL context");
    if (s->p.qt_model == 0) return set_error("mdqt_tag_spin_up: qt_model 0 (laser cooling) has no spin tagging");
    HIPCHK(hipSetDevice(s->dev));
    const int n = s->nloc;
    DevBuf<int> d;
    if (n > 0) {
        HIPCHK(d.alloc((size_t)n));
        HIPCHK(launch_tag_spin_up(s->dPsi, n, s->S, (uint64_t)s->lo, s->qidx, s->qc, d, s->stream));
    }
    std::vector<int> h((size_t)n, 0);
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(h.data(), d, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += h[i];
    if (tags)
        for (int i = 0; i < n; ++i) tags[s->lo + i] = h[i];
    if (n_up) *n_up = cnt;
    return 0;
}

int mdqt::pump_setup_directories(mdqt_ctx* s) {                // :985-999
    const mdqt_params* p = &s->p;
    char name[256];
    snprintf(name, sizeof name, "PumpTime%dPumpStart%dDet%dOm%dDensity%dGe%dNumIons%d",
             (int)(unsigned)(1000000000. * p->tpumpreal), (int)(unsigned)(p->tstartV0),
             (int)(unsigned)(100. * fabs(p->detuning)), (int)(unsigned)(100. * p->Om),
             (int)(unsigned)(10. * p->density), (int)(unsigned)(1000 * p->Ge), (int)(unsigned)p->N0);
    return finish_directories(s, name);
}

// step() :377-394: step_R(dt/2) (at t == 0 with forces() first and the DT^2 F term), step_V(dt)
// with forces() at the half-drifted positions, step_R(dt/2)
int mdqt::pump_md_step(mdqt_ctx* s) {
    const double dt = s->dtQ * s->ratio;                         // :389 dt=quantumTimestep*ratio
    const double DT = 0.5 * dt, DT2 = DT * DT;
    const int moving = s->t > 0 ? 1 : 0;
    HIPCHK(hipSetDevice(s->dev));
    double* R = s->dR;
    if (!moving) {                                               // :331 forces() before the first drift
        if (mdqt_forces(s)) return -1;
        if (settle_forces(s)) return -1;
    }
    HIPCHK(launch_leapfrog_half(R, s->dV, s->dF, s->nloc, s->S, s->L, DT, DT2, moving, 0., s->stream));
    if (mdqt_forces(s)) return -1;                               // step_V: forces() :361
    if (settle_forces(s)) return -1;
    HIPCHK(launch_leapfrog_half(R, s->dV, s->dF, s->nloc, s->S, s->L, DT, DT2, moving, dt, s->stream));
    return 0;
}

extern "C" int mdqt_pump_md_steps(mdqt_ctx* s, int n) {         // n x (step(); c0++) at the context's t
    if (!s) return set_error("NULL context");
    if (n < 0) return set_error("negative step count");
    if (s->p.world_size != 1) return set_error("mdqt_pump_md_steps: world_size 1 only");
    for (int k = 0; k < n; ++k) {
        if (pump_md_step(s)) return -1;
        s->c0++;
    }
    return 0;
}

// measureSpinUps() :600-665: the file of the count (:651-662)
int mdqt::pump_spin_ups_file(mdqt_ctx* s) {
    char b[96];
    snprintf(b, sizeof b, "spinUpIons_timestep%06d.dat", s->c0);
    FILE* fa = open_in(s, b, "w");
    if (!fa) return -1;
    fprintf(fa, "%i", s->nSpinUp);                               // :651-662
    fclose(fa);
    return 0;
}

// measureSpinUps() :600-665 (tags from the Philox stream, mdqt_tag_spin_up)
static int measure_spin_ups(mdqt_ctx* s) {
    const int N = s->N;
    s->spinUp.assign((size_t)(N > 0 ? N : 1), 0);
    int n_up = 0;
    if (mdqt_tag_spin_up(s, s->spinUp.data(), &n_up)) return -1;
    s->nSpinUp = n_up;
    HIPCHK(s->dSpinUp.reserve((size_t)s->capS));
    HIPCHK(hipMemcpyAsync(s->dSpinUp, s->spinUp.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, s->stream));
    return pump_spin_ups_file(s);
}

// output()'s device buffers: the tagged distribution's partials and result, the device copy of the tags
int mdqt::pump_output_buffers(mdqt_ctx* s) {
    const int nch = (s->N + 255) / 256;
    HIPCHK(s->dTkde.reserve(((size_t)(nch > 0 ? nch : 1) + 1) * 3 * TKDE_BINS));
    if (s->dSpinUp.capacity() < (size_t)s->capS) {
        HIPCHK(s->dSpinUp.reserve((size_t)s->capS));
        HIPCHK(hipMemsetAsync(s->dSpinUp, 0, (size_t)s->capS * sizeof(int), s->stream));
    }
    return 0;
}

// output() :799-935, the host part: energies (EkinX without subtracting <vx>; Epotential() is the
// context's own call), the spin-up ions' moments, the files, counter++; host sums in the reference's
// order.  V = the velocities [3][N], P = the tagged distribution [3][TKDE_BINS] (filled by `tagged`,
// which runs after the energies as in output_pump, or beforehand by the caller: tagged == nullptr).
// pool != nullptr: the 4001-line distribution file is formatted ("%lg", byte-identical) on that pool.
// epot != nullptr: Epotential()'s value, computed by the caller (the pump ensemble's batched pass).
int mdqt::pump_output_host(mdqt_ctx* s, const std::vector<double>& V, std::vector<double>& P,
                           const std::function<int()>& tagged, FileWriter* pool, const double* epot) {
    const int N = s->N;
    double EkinX = 0., EkinY = 0., EkinZ = 0.;
    for (int i = 0; i < N; i++) {                                // :812-817
        EkinX += 0.5 * (V[i] * V[i]);
        EkinY += 0.5 * (V[(size_t)N + i] * V[(size_t)N + i]);
        EkinZ += 0.5 * (V[(size_t)2 * N + i] * V[(size_t)2 * N + i]);
    }
    EkinX /= (double)N; EkinY /= (double)N; EkinZ /= (double)N;
    double e;
    if (epot) s->Epot = *epot;
    else if (mdqt_epotential(s, &e)) return -1;                  // :821
    FILE* fa = open_in(s, "energies.dat", "a");                  // :825-829
    if (!fa) return -1;
    fprintf(fa, "%lg\t%lg\t%lg\t%lg\t%lg\t%lg\n", s->t, EkinX, EkinY, EkinZ, s->Epot,
            EkinX + EkinY + EkinZ + s->Epot - s->Epot0);
    fclose(fa);
    if (tagged && tagged()) return -1;
    // moments of the tagged x velocities (:836-851, :866-876)
    double m1 = 0, m2 = 0, m3 = 0, m4 = 0;
    unsigned nt = 0;
    const bool have = !s->spinUp.empty() && (int)s->spinUp.size() >= N;
    for (int i = 0; i < N; i++) {
        const double v = V[i];
        if (have && s->spinUp[i]) {
            m1 += v; m2 += v * v; m3 += v * v * v; m4 += v * v * v * v;
            nt += 1;
        }
    }
    m1 /= nt; m2 /= nt; m3 /= nt; m4 /= nt;
    fa = open_in(s, "taggedMoments.dat", "a");
    if (!fa) return -1;
    fprintf(fa, "%lg\t%lg\t%lg\t%lg\t%lg\n", s->t, m1, m2, m3, m4);
    fclose(fa);
    char b[96];
    snprintf(b, sizeof b, "vel_distX_timestep%06d.dat", s->c0);   // :887-901 (X only)
    if (pool) {
        const int bin0 = s->pumpBin0;
        pool->submit(std::string(s->saveDirectory) + b, "w",
                     [bin0, Px = std::vector<double>(P.begin(), P.begin() + TKDE_BINS)](LgText& t) {
                         for (int j = 0; j < TKDE_BINS; j++) {
                             t.num((double)(j + bin0) * 0.0025); t.ch('\t'); t.num(Px[j]); t.ch('\n');
                         }
                     });
    } else {
        fa = open_in(s, b, "w");
        if (!fa) return -1;
        for (int j = 0; j < TKDE_BINS; j++) fprintf(fa, "%lg\t%lg\n", (double)(j + s->pumpBin0) * 0.0025, P[j]);
        fclose(fa);
    }
    s->counter++;                                                // :929
    return 0;
}

// output() :799-935: the velocities, then the host part with the tagged x distribution on the device
// (:831-864 exp(-V2 (vel_j - v)^2) summed over spin-up ions, 4001 bins)
static int output_pump(mdqt_ctx* s) {
    const int N = s->N;
    std::vector<double> V((size_t)3 * (N > 0 ? N : 1), 0.);
    if (mdqt_get_state(s, nullptr, V.data(), nullptr, N, nullptr, nullptr, nullptr)) return -1;
    std::vector<double> P((size_t)3 * TKDE_BINS, 0.);
    auto tagged = [&]() -> int {
        if (pump_output_buffers(s)) return -1;
        if (N > 0) {
            HIPCHK(launch_tagged_kde(s->dV, s->dSpinUp, N, s->S, s->dTkde + (size_t)3 * TKDE_BINS, s->dTkde, s->stream,
                                     s->pumpBin0));
            HIPCHK(hipMemcpyAsync(P.data(), s->dTkde, P.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
            HIPCHK(hipStreamSynchronize(s->stream));
        }
        return 0;
    };
    return pump_output_host(s, V, P, tagged, nullptr);
}

// Zfunc(c1V) + printVAF(t) :938-975 (host, the reference's order) on the velocities V [3][N]
int mdqt::pump_vaf_host(mdqt_ctx* s, const std::vector<double>& V, int c1V) {
    const int N = s->N;
    if (c1V == 0) s->vaHold.assign(V.begin(), V.begin() + N);
    if ((int)s->vaHold.size() < N) s->vaHold.resize((size_t)N, 0.);
    double VAF = 0.0;
    for (int j = 0; j < N; j++) VAF += 1 / ((double)(N)) * (s->vaHold[j] * V[j]);
    FILE* fa = open_in(s, "VAF.dat", "a");
    if (!fa) return -1;
    fprintf(fa, "%lg\t%lg\n", s->t, VAF);
    fclose(fa);
    return 0;
}

static int vaf_pump(mdqt_ctx* s, int c1V) {
    const int N = s->N;
    std::vector<double> V((size_t)3 * (N > 0 ? N : 1), 0.);
    if (mdqt_get_state(s, nullptr, V.data(), nullptr, N, nullptr, nullptr, nullptr)) return -1;
    return pump_vaf_host(s, V, c1V);
}

int mdqt::pump_write_conditions(mdqt_ctx* s, int c0) {        // :667-707
    const int N = s->N;
    std::vector<double> R((size_t)3 * (N > 0 ? N : 1), 0.), V(R.size(), 0.);
    if (mdqt_get_state(s, R.data(), V.data(), nullptr, N, nullptr, nullptr, nullptr)) return -1;
    char b[96];
    snprintf(b, sizeof b, "ions_timestep%06d.dat", c0);
    FILE* fa = open_in(s, b, "w");
    if (!fa) return -1;
    fprintf(fa, "%i\t%i", N, s->counter);
    fclose(fa);
    snprintf(b, sizeof b, "spinUpIonsList_timestep%06d.dat", c0);
    fa = open_in(s, b, "w");
    if (!fa) return -1;
    for (int i = 0; i < N; i++) fprintf(fa, "%i\n", (int)s->spinUp.size() > i ? s->spinUp[i] : 0);
    fclose(fa);
    snprintf(b, sizeof b, "conditions_timestep%06d.dat", c0);
    fa = open_in(s, b, "w");
    if (!fa) return -1;
    for (int i = 0; i < N; i++)
        fprintf(fa, "%lg\t%lg\t%lg\t%lg\t%lg\t%lg\t\n", R[i], R[(size_t)N + i], R[(size_t)2 * N + i], V[i],
                V[(size_t)N + i], V[(size_t)2 * N + i]);
    fclose(fa);
    return 0;
}

int mdqt::pump_read_conditions(mdqt_ctx* s, int c0) {         // :709-797
    s->pumpBin0 = 0;                                             // :721-724 vel[i] = i 0.0025
    std::vector<double> R, V;
    const int N = read_ions_conditions(s, c0, R, V);             // :713-770
    if (N < 0) return -1;
    std::vector<int> up((size_t)(N > 0 ? N : 1), 0);
    char b[96];
    snprintf(b, sizeof b, "spinUpIonsList_timestep%06d.dat", c0);
    FILE* fa = open_in(s, b, "r");
    if (!fa) return -1;
    int i = 0, sUp;
    while (i < N && fscanf(fa, "%i\n", &sUp) == 1) up[i++] = sUp;
    fclose(fa);
    const double t = s->t;
    if (resize(s, N)) return -1;
    // wvFns are not read (the reference's read loop is commented out, :772-795): they stay zero
    std::vector<double> psi((size_t)24 * (N > 0 ? N : 1), 0.), tp((size_t)(N > 0 ? N : 1), 0.);
    if (upload(s, R.data(), V.data(), N, psi.data(), tp.data())) return -1;
    s->spinUp = up;
    s->nSpinUp = 0;
    for (int k = 0; k < N; ++k) s->nSpinUp += up[k] ? 1 : 0;
    HIPCHK(s->dSpinUp.reserve((size_t)s->capS));
    HIPCHK(hipMemcpyAsync(s->dSpinUp, up.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, s->stream));
    s->t = t;
    s->c0 = c0;
    return 0;
}

extern "C" int mdqt_get_spin_up_list(mdqt_ctx* s, int* tags, int* n_up) {
    if (!s) return set_error("NULL context");
    for (int i = 0; i < s->N && tags; ++i) tags[i] = (int)s->spinUp.size() > i ? s->spinUp[i] : 0;
    if (n_up) *n_up = s->nSpinUp;
    return 0;
}

PumpSchedule mdqt::pump_schedule(const mdqt_ctx* s) {
    const double tpump = s->p.tpumpreal * 813490 * sqrt(s->p.density);      // :79
    const double tendV0 = s->p.tstartV0 + tpump;                             // :80
    return {s->dtQ, s->p.tmax + 0.0009, s->p.tstartV0, tendV0, s->p.sampleFreq, s->ratio, MAXSUB};
}

// main() :981-1076; the time loop itself is pump_loop (mdqt_main_loops.hpp)
extern "C" int mdqt_run_pump(mdqt_ctx* s) {
    if (!s) return set_error("NULL context");
    if (s->p.qt_model < 1 || s->p.qt_model > 3) return set_error("mdqt_run_pump: qt_model must be 1, 2 or 3");
    if (s->p.world_size != 1) return set_error("mdqt_run_pump: world_size 1 only");
    if (pump_setup_directories(s)) return -1;
    s->spinUp.clear();
    s->nSpinUp = 0;
    s->pumpBin0 = -2000;
    const int recorded = s->p.newRun == 1 ? 0 : 1;               // recordedSpinUps :81
    if (recorded ? pump_read_conditions(s, s->p.c0) : mdqt_init(s)) return -1;   // :1036-1046
    struct {                                                     // the loop's driver: this context's own calls
        mdqt_ctx* s;
        double t() const { return s->t; }
        int c0() const { return s->c0; }
        int qsteps(int n) { return run_substeps(s, n, 0, 1, 1); }    // qstep() x n :396-598
        int measure() { return measure_spin_ups(s); }
        int output(int vaf) { return output_pump(s) || vaf_pump(s, vaf); }
        int md_step(bool, bool) { return mdqt_pump_md_steps(s, 1); }   // pump_md_step does both of its own half drifts
        int idle() { s->t += s->dtQ; return 0; }
        int fail(const char* what) { return set_error("mdqt_run_pump: %s", what); }
    } d{s};
    if (pump_loop(pump_schedule(s), recorded, d)) return -1;
    if (flush_files(s)) return -1;
    return pump_write_conditions(s, s->c0);                      // :1084
}
