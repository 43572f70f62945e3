// ---------------------------------------------------------------------------------------------
// files (reference formats, SpeedUp:725-1032) and main() (:1139-1383): mdqt_run is the preamble, this context's
// driver and the time loop that mdqt_ensemble_run shares (mdqt_main_loops.hpp: speedup_loop)
// ---------------------------------------------------------------------------------------------

#include <errno.h>
#include <sys/stat.h>

#include "mdqt_ctx.hpp"

using namespace mdqt;

FILE* mdqt::open_in(const mdqt_ctx* s, const char* name, const char* mode) {
    char path[1400];
    snprintf(path, sizeof(path), "%s%s", s->saveDirectory, name);
    FILE* f = fopen(path, mode);
    if (!f) set_error("cannot open %s: %s", path, strerror(errno));
    return f;
}

extern "C" const char* mdqt_save_directory(const mdqt_ctx* s) { return s->saveDirectory; }

// the directory of a run, common to every program: <params' saveDirectory>/<name>/job<k>/, created
int mdqt::finish_directories(mdqt_ctx* s, const char* name) {
    const mdqt_params* p = &s->p;
    char base[512];
    strncpy(base, p->saveDirectory, sizeof(base) - 1);
    base[sizeof(base) - 1] = 0;
    mkdir(base, 0777);
    snprintf(s->saveDirectory, sizeof(s->saveDirectory), "%s%s", base, name);
    mkdir(s->saveDirectory, 0777);
    char jb[64];
    snprintf(jb, sizeof jb, "/job%d/", (int)p->job);
    strncat(s->saveDirectory, jb, sizeof(s->saveDirectory) - strlen(s->saveDirectory) - 1);
    mkdir(s->saveDirectory, 0777);
    struct stat st;
    if (stat(s->saveDirectory, &st) != 0 || !S_ISDIR(st.st_mode))
        return set_error("cannot create output directory %s", s->saveDirectory);
    return 0;
}

// the SpeedUp program's name of a run, SpeedUp:1145-1160 (the jobs' job<k>/ and an ensemble's pooled directory
// lie below it)
void mdqt::speedup_run_name(const mdqt_params* p, char* name, size_t cap) {
    snprintf(name, cap, "Ge%dDensity%dE+11Sig0%dTe%dSigFrac%dDetSP%dDetDP%dOmSP%dOmDP%dNumIons%d",
             ref_udcast(100 * p->Ge), ref_udcast(p->density * 1000), ref_udcast(10 * p->sig0), ref_udcast(p->Te),
             ref_udcast(p->fracOfSig * 100), ref_udcast(p->detuning * 100), ref_udcast(p->detuningDP * 100),
             ref_udcast(p->Om * 100), ref_udcast(p->OmDP * 100), ref_udcast((double)p->N0));
}

extern "C" int mdqt_setup_directories(mdqt_ctx* s) {       // SpeedUp:1145-1160
    char name[256];
    speedup_run_name(&s->p, name, sizeof name);
    return finish_directories(s, name);
}

static FileWriter& writer_of(mdqt_ctx* s) {
    if (s->shared_writer) return *s->shared_writer;    // a member of an ensemble: the ensemble's pool
    if (!s->writer) s->writer.reset(new FileWriter(4));
    return *s->writer;
}

static std::string path_in(const mdqt_ctx* s, const char* name) { return std::string(s->saveDirectory) + name; }

// wait for the background writers; reports the first file error
int mdqt::flush_files(mdqt_ctx* s) {
    FileWriter* w = s->shared_writer ? s->shared_writer : s->writer.get();
    if (!w) return 0;
    std::string e;
    if (w->flush(&e)) return set_error("%s", e.c_str());
    return 0;
}

// output(), SpeedUp:917-1032.  The observables are computed on the device and snapshotted here;
// the files are formatted by the background writers (the caller flushes: mdqt_output at once,
// mdqt_run at the end of the run).
int mdqt::output_async(mdqt_ctx* s) {
    const int N = s->N;
    double o[7];
    auto P = std::make_shared<std::vector<double>>((size_t)3 * NBINS);
    auto pops = std::make_shared<std::vector<double>>((size_t)3 * (N > 0 ? N : 1));
    auto V = std::make_shared<std::vector<double>>((size_t)3 * (N > 0 ? N : 1), 0.);
    if (observables_w1_applies(s)) {                                 // one pass, one synchronisation
        if (observables_w1(s, o, P->data(), pops->data(), V->data())) return -1;
    } else {
        if (mdqt_observables(s, o, P->data(), pops->data())) return -1;
        if (mdqt_get_state(s, nullptr, V->data(), nullptr, N, nullptr, nullptr, nullptr)) return -1;
        if (mdqt_allreduce_sum(s, V->data(), (size_t)N)) return -1;  // vx column, zero-padded gather
    }
    return output_files(s, o, P, pops, V);
}

// output() after its observables: energies.dat's line in place, the velocity distributions and the state
// populations from the snapshots by the background writers, counter++ (o[7], P [3][NBINS], pops [N][3], V:
// vx in [0, N))
int mdqt::output_files(mdqt_ctx* s, const double* o, std::shared_ptr<std::vector<double>> P,
                       std::shared_ptr<std::vector<double>> pops, std::shared_ptr<std::vector<double>> V) {
    const int N = s->N;
    if (s->p.rank != 0) { s->counter++; return 0; }                 // files are rank 0's
    FILE* fa = open_in(s, "energies.dat", "a");                      // appended in order: here
    if (!fa) return -1;
    fprintf(fa, "%lg\t%lg\t%lg\t%lg\t%lg\t%lg\t%lg\n", o[0], o[1], o[2], o[3], o[4], o[5], o[6]);   // :954
    fclose(fa);
    FileWriter& w = writer_of(s);
    const double* vel = s->vel;                                      // constant bin centres
    const char* axes[3] = {"X", "Y", "Z"};
    for (int a = 0; a < 3; ++a) {                                                        // :983-1006
        char b[64];
        snprintf(b, sizeof b, "vel_dist%s_time%06d.dat", axes[a], s->counter);
        const double shift = a == 0 ? o[6] : 0.;
        w.submit(path_in(s, b), "w", [P, vel, a, shift](LgText& t) {
            const double* p = P->data() + (size_t)a * NBINS;
            for (int i = 0; i < NBINS; i++) {
                t.num(vel[i] + shift); t.ch('\t'); t.num(p[i]); t.ch('\n');
            }
        });
    }
    char b[64];
    snprintf(b, sizeof b, "statePopulationsVsVTime%06d.dat", s->counter);
    w.submit(path_in(s, b), "w", [V, pops, N](LgText& t) {                              // :1010-1024
        const double *v = V->data(), *q = pops->data();
        for (int i = 0; i < N; i++) {
            t.num(v[i]); t.ch('\t'); t.num(q[3 * i]); t.ch('\t'); t.num(q[3 * i + 1]); t.ch('\t');
            t.num(q[3 * i + 2]); t.ch('\n');
        }
    });
    s->counter++;                                                                        // :1027
    return 0;
}

extern "C" int mdqt_output(mdqt_ctx* s) {                 // output(), SpeedUp:917-1032
    if (!s) return set_error("NULL context");
    if (output_async(s)) return -1;
    return flush_files(s);
}

// writeConditions, SpeedUp:725-784 (files formatted by the background writers)
int mdqt::write_conditions_async(mdqt_ctx* s, int c0) {
    const int N = s->N;
    const size_t n1 = (size_t)(N > 0 ? N : 1);
    auto R = std::make_shared<std::vector<double>>(3 * n1, 0.);
    auto V = std::make_shared<std::vector<double>>(3 * n1, 0.);
    auto psi = std::make_shared<std::vector<double>>(24 * n1, 0.);
    if (mdqt_allgather_positions(s)) return -1;           // collective when sharded
    if (mdqt_get_state(s, R->data(), V->data(), nullptr, N, psi->data(), nullptr, nullptr)) return -1;
    if (mdqt_allreduce_sum(s, V->data(), V->size())) return -1;
    if (mdqt_allreduce_sum(s, psi->data(), psi->size())) return -1;
    if (s->p.rank != 0) return 0;
    char b[96];
    snprintf(b, sizeof b, "ions_timestep%06d.dat", c0);
    FILE* fa = open_in(s, b, "w");
    if (!fa) return -1;
    fprintf(fa, "%i\t%i", N, s->counter);                                                // :737
    fclose(fa);
    FileWriter& w = writer_of(s);
    snprintf(b, sizeof b, "conditions_timestep%06d.dat", c0);
    w.submit(path_in(s, b), "w", [R, V, N](LgText& t) {                                 // :747
        const double *r = R->data(), *v = V->data();
        for (int i = 0; i < N; i++) {
            for (int k = 0; k < 3; ++k) { t.num(r[(size_t)k * N + i]); t.ch('\t'); }
            for (int k = 0; k < 3; ++k) { t.num(v[(size_t)k * N + i]); t.ch('\t'); }
            t.ch('\n');
        }
    });
    auto vholder = std::make_shared<std::vector<double>>(s->Vholder);
    for (int v = 0; v < NINTERVALV; v++) {                                              // :752-763
        snprintf(b, sizeof b, "VZERO_timestep%06d_interval%d.dat", c0, v);
        w.submit(path_in(s, b), "w", [vholder, v, N](LgText& t) {
            const double* vh = vholder->data() + (size_t)v * 3 * N;
            for (int i = 0; i < N; i++) {
                t.num(vh[i]); t.ch('\t'); t.num(vh[(size_t)N + i]); t.ch('\t'); t.num(vh[(size_t)2 * N + i]);
                t.ch('\n');
            }
        });
    }
    snprintf(b, sizeof b, "wvFns_timestep%06d.dat", c0);
    w.submit(path_in(s, b), "w", [psi, N](LgText& t) {                                  // :777-779
        for (int j = 0; j < N; j++) {
            const double* ps = psi->data() + (size_t)24 * j;
            for (int k = 0; k < NS; k++) { t.num(ps[2 * k]); t.ch('\t'); t.num(ps[2 * k + 1]); t.ch('\t'); }
            t.ch('\n');
        }
    });
    return 0;
}

extern "C" int mdqt_write_conditions(mdqt_ctx* s, int c0) {   // writeConditions, :725-784
    if (!s) return set_error("NULL context");
    if (write_conditions_async(s, c0)) return -1;
    return flush_files(s);
}

extern "C" int mdqt_flush_files(mdqt_ctx* s) {
    if (!s) return set_error("NULL context");
    return flush_files(s);
}

// The start of readConditions in every program (SpeedUp:785-832; the pumping programs' :709-770): t of
// step c0, the ion count and the output counter from ions_timestep, positions and velocities [3][N] from
// conditions_timestep.  Returns N, -1 on error.
int mdqt::read_ions_conditions(mdqt_ctx* s, int c0, std::vector<double>& R, std::vector<double>& V) {
    s->t = ((double)c0 - 9.) * TIMESTEP + 0.02;                                         // :789
    char b[96];
    snprintf(b, sizeof b, "ions_timestep%06d.dat", c0);
    FILE* fa = open_in(s, b, "r");
    if (!fa) return -1;
    int j, m, N = -1;
    while (fscanf(fa, "%i\t%i", &j, &m) == 2) { N = j; s->counter = (unsigned)m; }      // :805-814
    fclose(fa);
    if (N < 0) return set_error("%s: no ion count", b);
    R.assign((size_t)3 * (N > 0 ? N : 1), 0.);
    V.assign(R.size(), 0.);
    snprintf(b, sizeof b, "conditions_timestep%06d.dat", c0);
    fa = open_in(s, b, "r");
    if (!fa) return -1;
    double a, bb, z, d, e, f;
    int i = 0;
    while (i < N && fscanf(fa, "%lg\t%lg\t%lg\t%lg\t%lg\t%lg\n", &a, &bb, &z, &d, &e, &f) == 6) {   // :818-832
        R[i] = a; R[(size_t)N + i] = bb; R[(size_t)2 * N + i] = z;
        V[i] = d; V[(size_t)N + i] = e; V[(size_t)2 * N + i] = f;
        i++;
    }
    fclose(fa);
    if (i != N) return set_error("%s: %d of %d rows", b, i, N);
    return N;
}

extern "C" int mdqt_read_conditions(mdqt_ctx* s, int c0) {    // readConditions, :785-916
    if (!s) return set_error("NULL context");
    if (flush_files(s)) return -1;                       // the files may still be being written
    std::vector<double> R, V;
    const int N = read_ions_conditions(s, c0, R, V);
    if (N < 0) return -1;
    std::vector<double> psi((size_t)24 * (N > 0 ? N : 1), 0.);
    char b[96];
    snprintf(b, sizeof b, "wvFns_timestep%06d.dat", c0);
    FILE* fa = open_in(s, b, "r");
    if (!fa) return -1;
    int i = 0;
    double w[24];
    while (i < N &&
           fscanf(fa, "%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\t%lg%lg\n",
                  &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8], &w[9], &w[10], &w[11], &w[12],
                  &w[13], &w[14], &w[15], &w[16], &w[17], &w[18], &w[19], &w[20], &w[21], &w[22], &w[23]) == 24) {  // :859-894
        memcpy(psi.data() + (size_t)24 * i, w, sizeof(w));
        i++;
    }
    fclose(fa);
    if (i != N) return set_error("%s: %d of %d rows", b, i, N);
    const double t = s->t;
    if (resize(s, N)) return -1;
    for (int v = 0; v < NINTERVALV; v++) {                                              // :898-913
        snprintf(b, sizeof b, "VZERO_timestep%06d_interval%d.dat", c0, v);
        fa = open_in(s, b, "r");
        if (!fa) return -1;
        double* vh = s->Vholder.data() + (size_t)v * 3 * N;
        double a, bb, z;
        i = 0;
        while (i < N && fscanf(fa, "%lg\t%lg\t%lg", &a, &bb, &z) == 3) {
            vh[i] = a; vh[(size_t)N + i] = bb; vh[(size_t)2 * N + i] = z;
            i++;
        }
        fclose(fa);
    }
    std::vector<double> tp((size_t)(N > 0 ? N : 1), 0.);       // tPart not restored (App. C-8)
    if (upload(s, R.data(), V.data(), N, psi.data(), tp.data())) return -1;
    s->t = t;
    s->c0 = c0;
    s->qidx = (uint64_t)(c0 + 1) * (uint64_t)s->ratio;
    return 0;
}

// main(), SpeedUp:1139-1383; the time loop itself is speedup_loop (mdqt_main_loops.hpp)
extern "C" int mdqt_run(mdqt_ctx* s) {
    if (!s) return set_error("NULL context");
    if (s->p.world_size > 1 && !s->comm) return set_error("mdqt_run: sharded run needs mdqt_comm_init first");
    if (mdqt_setup_directories(s)) return -1;
    if (s->p.newRun == 1 ? mdqt_init(s) : mdqt_read_conditions(s, s->p.c0)) return -1;
    struct {                                            // the loop's driver: this context's own calls
        mdqt_ctx* s;
        double t() const { return s->t; }
        int c0() const { return s->c0; }
        int output() { return output_async(s); }        // files formatted while the loop goes on
        bool may_fuse_interval() { return fused_applies(s); }
        int start_interval(bool whole) {                // whole: the interval as one k_md_step launch; else §8e, forces()
            s->last_fused = whole;
            if (whole ? local_reduce(s) || md_step_fused(s) : mdqt_allgather_positions(s) || mdqt_forces(s)) return -1;
            s->c0++;
            return 0;
        }
        int substeps(int n) { return mdqt_substeps(s, n); }
    } d{s};
    if (speedup_loop(speedup_schedule(s), d)) return -1;
    return mdqt_write_conditions(s, s->c0);             // :1381; also joins the writers
}
