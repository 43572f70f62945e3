// main() of the Monte-Carlo + MD programs (MCMD:1030-1167; QTT:1140-1254) by stage, for J contexts in lockstep:
// mdmc_run is J = 1, an ensemble's run J members.  Every stage queues all members' launches and copies of a step
// first and then drains member by member (wait for the copies, format, write), so a step with a host round trip
// costs one wait, not J in a row, and the host formats one member's rows while the device runs the others' MD step.
// An MD stage has one body, `for k: for lane: <the step's operations>`, on the run's lanes (mdmc_ctx.hpp's MdLane):
// J member lanes, each on its member's own stream, or, for an ensemble with md_batch 1, one lane of batched launches
// on the ensemble's stream (mdmc_ensemble.cpp), every stage one stretch.  The mode is chosen where the lanes are
// built and at stage_record_qtt's entry, nowhere else.
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "mdmc_ctx.hpp"      // struct mdmc_ctx, MdLane; HIPCHK, mdqt::set_error
#include "mdqt_writer.hpp"   // FileWriter, LgText: the QT tagging programs' distribution files

using namespace mdqt;
using namespace mdmc;

namespace {

typedef std::chrono::steady_clock Clock;
enum Stage { ST_ANNEAL = 0, ST_PRE, ST_PUMP, ST_REC, ST_AUTO, ST_REST };

struct Run {
    mdmc_ctx* const* c;
    int J;
    mdmc_ensemble* ens;           // NULL: one context, annealed by its own launch
    int verbose;
    Clock::time_point t0;
    std::vector<MdLane> lanes;    // what the MD stages queue on
    std::unique_ptr<FileWriter> writer;   // stage_record_qtt's pool: one per run, joined before the stage ends
};

struct Files {                    // one open file per member, closed on every way out
    std::vector<FILE*> f;
    ~Files() {
        for (FILE* x : f)
            if (x) fclose(x);
    }
};

// with an ensemble's timing on: the wall time since the last stage ended, the queued work included
int stage_end(Run& r, int stage) {
    if (!r.ens || !r.ens->timing) return 0;
    for (int j = 0; j < r.J; ++j) HIPCHK(hipStreamSynchronize(r.c[j]->st));
    const Clock::time_point t = Clock::now();
    r.ens->stage_ms[stage] += std::chrono::duration<double, std::milli>(t - r.t0).count();
    r.t0 = t;
    return 0;
}

int write_pair_corr_file(mdmc_ctx* c, int stepNum) {             // :639-651, the histogram landed
    std::vector<double> g;
    pair_corr_finish(c, g);
    char name[256];
    snprintf(name, sizeof name, "pairPairCorrStepNum%d.dat", stepNum);
    FILE* fa = open_in(c, name, "w");
    if (!fa) return set_error("cannot open %s%s", c->saveDir.c_str(), name);
    for (int i = 0; i < (int)g.size(); i++) fprintf(fa, "%lg\t%lg\n", i * c->p.pairPairStep, g[i]);
    fclose(fa);
    return 0;
}

// the g(r) drain, per member in every mode: wait for the member's queued histogram, then its file
int drain_pair_corr(Run& r, int stepNum) {
    for (int j = 0; j < r.J; ++j) {
        HIPCHK(hipEventSynchronize(r.c[j]->evDrain));
        if (write_pair_corr_file(r.c[j], stepNum)) return -1;
    }
    return 0;
}

int write_pair_corr(Run& r, int stepNum) {
    for (int j = 0; j < r.J; ++j)
        if (pair_corr_queue(r.c[j])) return -1;
    return drain_pair_corr(r, stepNum);
}

// per-step observables buffered on the device, written when a stage ends
int ensure_step_buffers(mdmc_ctx* c, int steps) {
    if (steps <= c->temp_rows()) return 0;
    c->dTemp.reset();                                  // temp_rows() speaks for both: dTemp goes first and comes last
    HIPCHK(c->dMom.alloc((size_t)steps * 20));
    HIPCHK(c->dTemp.alloc((size_t)steps * 4));
    return 0;
}

int write_temp_axes(mdmc_ctx* c, const char* name, int nsteps) {   // recordTempForEachAxis :560-581
    std::vector<double> s((size_t)nsteps * 4);
    HIPCHK(hipMemcpyAsync(s.data(), c->dTemp, s.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    FILE* fa = open_in(c, name, "a");
    if (!fa) return set_error("cannot open %s%s", c->saveDir.c_str(), name);
    for (int k = 0; k < nsteps; ++k) {
        double t4[4];
        temps_from_sums(c, &s[(size_t)4 * k], t4);
        fprintf(fa, "%lg\t%lg\t%lg\t%lg\n", k * c->p.timeStep, t4[1], t4[2], t4[3]);
    }
    fclose(fa);
    return 0;
}

// main() :1037-1065 (QTT:1143-1196): the directories, init() and the potentials
int stage_start(Run& r) {
    for (int j = 0; j < r.J; ++j)
        if (mdmc_setup_directories(r.c[j]) || mdmc_init(r.c[j])) return -1;
    return 0;
}

// step 3 :1068-1078 (QTT:1198-1209): g(r) at every multiple of 10,000, then one chunk of the chains
int stage_anneal(Run& r) {
    const int mcs = r.c[0]->p.monteCarloSteps;
    for (int k = 0; k < mcs;) {
        if (k % 10000 == 0) {
            if (write_pair_corr(r, k)) return -1;
            if (r.verbose) printf("%d\n", k);
        }
        const int next = std::min(mcs, (k / 10000 + 1) * 10000);
        if (r.ens ? ensemble_anneal(r.ens, next - k, nullptr) : mdmc_monte_carlo(r.c[0], next - k, nullptr)) return -1;
        k = next;
    }
    return 0;
}

// one operation on every lane in order.  An MD stage opens and closes the lanes around its steps (begin, end): a
// stretch for the ensemble lane, nothing for a member's
int each_lane(Run& r, int (MdLane::*op)() const) {
    for (const MdLane& l : r.lanes)
        if ((l.*op)()) return -1;
    return 0;
}

// n MDStep()s of every member; `count` prints the step counter every 100 (:1081-1089, :1126-1135)
int stage_md(Run& r, int n, bool count) {
    if (each_lane(r, &MdLane::begin)) return -1;
    for (int k = 0; k < n; k++) {
        if (count && r.verbose && k % 100 == 0) printf("%d\n", k);
        if (each_lane(r, &MdLane::md_step)) return -1;
    }
    return each_lane(r, &MdLane::end);
}

// n MDStep()s with the axis temperatures of every step, written to `name` (:1115-1123, :1141-1165)
int stage_md_temp_axes(Run& r, int n, const char* name) {
    if (each_lane(r, &MdLane::begin)) return -1;
    for (int k = 0; k < n; k++)
        for (const MdLane& l : r.lanes)
            if (l.temperatures(k) || l.md_step()) return -1;
    if (each_lane(r, &MdLane::end)) return -1;
    for (int j = 0; j < r.J; ++j)
        if (write_temp_axes(r.c[j], name, n)) return -1;
    return 0;
}

// recordTemperature (:533-545) and recordTaggedParticleMoments (:1005-1027) of step 5, appended per step
int write_recorded_mcmd(mdmc_ctx* c) {
    const mdmc_params& p = c->p;
    const int T = c->T;
    std::vector<double> s((size_t)T * 4), m((size_t)T * 20);
    HIPCHK(hipMemcpyAsync(s.data(), c->dTemp, s.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(m.data(), c->dMom, m.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    static const char* names[5] = {"temperature.dat", "taggedVOneMoments.dat", "taggedVTwoMoments.dat",
                                   "taggedVThreeMoments.dat", "taggedVFourMoments.dat"};
    Files fs;
    for (int t = 0; t < 5; ++t) fs.f.push_back(open_in(c, names[t], "a"));
    for (FILE* x : fs.f)
        if (!x) return set_error("cannot open the stage-5 files");
    for (int k = 0; k < T; ++k) {
        double t4[4], m16[16];
        temps_from_sums(c, &s[(size_t)4 * k], t4);
        moments_from_sums(c, &m[(size_t)20 * k], m16);
        for (int t = 0; t < 4; ++t)
            fprintf(fs.f[t + 1], "%lg\t%lg\t%lg\t%lg\t%lg\n", k * p.timeStep, m16[4 * t], m16[4 * t + 1], m16[4 * t + 2],
                    m16[4 * t + 3]);
        fprintf(fs.f[0], "%lg\n", t4[0]);
    }
    return 0;
}

// step 5 :1093-1104: the tags, then collisionless MD recording moments, temperature and velocities; g(r)
// every 100 steps is each member's own, on its own stream, whatever the lane
int stage_record_mcmd(Run& r) {
    const mdmc_params& p = r.c[0]->p;
    const int T = r.c[0]->T;
    for (int j = 0; j < r.J; ++j) {
        mdmc_ctx* c = r.c[j];
        c->collisionFreq = 0;
        if (mdmc_tag_particles(c, nullptr)) return -1;
        if (ensure_step_buffers(c, std::max(T, std::max(p.numInstantaneousAnisotropySteps,
                                                        std::max(p.anisotropyFromForcesRelaxSteps, 1 << 16))))) return -1;
    }
    if (each_lane(r, &MdLane::begin)) return -1;
    for (int k = 0; k < T; k++) {
        const bool gr = k % 100 == 0;
        if (gr && r.verbose) printf("%d\n", k);
        for (const MdLane& l : r.lanes)
            if (l.tag_moments(k) || (gr && l.pair_corr_queue()) || l.temperatures(k) || l.md_step() ||
                l.store_velocities(k))
                return -1;
        if (gr && drain_pair_corr(r, k)) return -1;
    }
    if (each_lane(r, &MdLane::end)) return -1;
    for (int j = 0; j < r.J; ++j)
        if (write_recorded_mcmd(r.c[j])) return -1;
    return 0;
}

// step 6 :1107-1110 (QTT step 7 :1247-1251): :682-691 and the three siblings
int stage_autocorrelations(Run& r) {
    const int T = r.c[0]->T;
    std::vector<std::vector<double>> out((size_t)r.J, std::vector<double>((size_t)4 * T));
    for (int j = 0; j < r.J; ++j)
        if (autocorr_queue(r.c[j], out[j].data())) return -1;
    static const char* names[4] = {"VAF.dat", "longViscAutoCorr.dat", "vCubeAutoCorr.dat", "vFourthAutoCorr.dat"};
    for (int j = 0; j < r.J; ++j) {
        mdmc_ctx* c = r.c[j];
        HIPCHK(hipStreamSynchronize(c->st));
        for (int f = 0; f < 4; ++f) {
            FILE* fa = open_in(c, names[f], "w");
            if (!fa) return set_error("cannot open %s%s", c->saveDir.c_str(), names[f]);
            for (int td = 0; td < T; ++td) fprintf(fa, "%lg\t%lg\n", td * c->p.timeStep, out[j][(size_t)f * T + td]);
            fclose(fa);
        }
    }
    return 0;
}

// steps 7 and 8 :1115-1165: the anisotropy stages
int stage_anisotropy(Run& r) {
    const mdmc_params& p = r.c[0]->p;
    for (int j = 0; j < r.J; ++j)
        if (mdmc_anisotropize(r.c[j])) return -1;                // step 7 :1115-1123
    if (stage_md_temp_axes(r, p.numInstantaneousAnisotropySteps, "TemperaturesAlongAxesInstantaneous.dat")) return -1;
    for (int j = 0; j < r.J; ++j) r.c[j]->collisionFreq = 0.25;  // :1125-1135
    if (stage_md(r, p.numReestablishEquilSteps, true)) return -1;
    const int nest = (int)round(.8 * p.anisotropyEstablishmentTime * sqrt(p.n) / p.timeStep);   // :106
    for (int j = 0; j < r.J; ++j) {                              // step 8 :1138-1151
        mdmc_ctx* c = r.c[j];
        c->addLaserForce = 1;
        c->collisionFreq = 0;
        if (ensure_step_buffers(c, std::max(nest, c->temp_rows()))) return -1;
    }
    if (stage_md_temp_axes(r, nest, "TemperaturesAlongAxesDuringForcePeriod.dat")) return -1;
    for (int j = 0; j < r.J; ++j) r.c[j]->addLaserForce = 0;     // :1155-1165
    return stage_md_temp_axes(r, p.anisotropyFromForcesRelaxSteps, "TemperaturesAlongAxesAfterForcePeriod.dat");
}

// QTT step 5 :1222-1233: the pump period (QT steps between collisionless MD steps), then the tags, inside the
// ensemble lane's stretch one launch for all members; nobody reads the counts, so nothing comes back
int stage_pump(Run& r) {
    for (int j = 0; j < r.J; ++j) r.c[j]->collisionFreq = 0;
    if (r.verbose) printf("pumpMDTimeSteps=%d\nquantumStepsPerMD=%d\n", r.c[0]->pumpSteps, r.c[0]->qtRatio);
    if (each_lane(r, &MdLane::begin)) return -1;
    for (int k = 0; k < r.c[0]->pumpSteps; k++)
        for (const MdLane& l : r.lanes)
            if (l.qt_steps(r.c[0]->qtRatio) || l.md_step()) return -1;
    if (each_lane(r, &MdLane::qt_tag)) return -1;
    return each_lane(r, &MdLane::end);
}

// vel_distX_timestep%06d.dat of one member and step (QTT:1128-1136) from a snapshot of its 4,001 values, on
// the run's writer pool: LgText's rows are fprintf("%lg\t%lg\n")'s bytes
void submit_dist_file(Run& r, const mdmc_ctx* c, int k, const double* dist) {
    char name[64];
    snprintf(name, sizeof name, "vel_distX_timestep%06d.dat", k);
    auto snap = std::make_shared<const std::vector<double>>(dist, dist + TKDE_BINS);
    r.writer->submit(c->saveDir + name, "w", [snap](LgText& t) {
        for (int i = 0; i < TKDE_BINS; i++) {
            t.num((double)(i - 2000) * 0.0025); t.ch('\t'); t.num((*snap)[i]); t.ch('\n');
        }
    });
}

// the pool of a run: at most 16 threads whatever J is, and a cap on the files in flight, so the snapshots
// held stay (cap + 1) x 32 KB however far the stage runs ahead of the disk
void start_writer(Run& r) {
    const int hw = (int)std::thread::hardware_concurrency();
    const int threads = std::min(16, std::max(1, hw - 1));
    r.writer.reset(new FileWriter(threads, (size_t)4 * threads));
}

int join_writer(Run& r) {
    std::string err;
    if (r.writer && r.writer->flush(&err)) return set_error("%s", err.c_str());
    return 0;
}

// the stage's taggedMoments.dat and temperature.dat of one member from its buffered rows (md_batch 1): the
// lines stage_record_qtt writes step by step otherwise, through the same two functions
int write_recorded_qtt(mdmc_ctx* c, FILE* fm, FILE* ft) {
    const int T = c->T;
    std::vector<double> s((size_t)T * 4), m((size_t)T * kTagMomentSums);
    HIPCHK(hipMemcpyAsync(s.data(), c->dTemp, s.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(m.data(), c->dMom, m.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (int k = 0; k < T; ++k) {
        double mom[4], tt[4];
        moments_qt_from_sums(&m[(size_t)kTagMomentSums * k], mom);
        fprintf(fm, "%lg\t%lg\t%lg\t%lg\t%lg\n", k * c->p.timeStep, mom[0], mom[1], mom[2], mom[3]);   // :1114
        temps_from_sums(c, &s[(size_t)4 * k], tt);
        fprintf(ft, "%lg\n", tt[0]);
    }
    return 0;
}

// the recorded stage on the ensemble lane (md_batch 1), one stretch.  Per step seven launches whatever J is:
// the tag moments into row k of every member's dMom, the X distribution (two) into a slot of the ensemble's
// ring and one copy of all members' rows to the pinned ring, the temperatures into row k of dTemp, the force
// and velocity-Verlet launches, the velocity store.  The host formats nothing itself: it hands the rows of the
// step kLag back to the pool, so it queues that far ahead of the device.  g(r) every 100 steps stays each
// member's own.  The moments and temperatures come back once, at the end.
int stage_record_qtt_batched(Run& r, Files& fm, Files& ft) {
    const MdLane& l = r.lanes[0];
    const int T = r.c[0]->T;
    constexpr int kLag = mdmc_ensemble::kDistSlots - 1;
    for (int j = 0; j < r.J; ++j)
        if (ensure_step_buffers(r.c[j], T)) return -1;
    auto drain = [&](int k) {
        const double* rows = ensemble_qt_dist_rows(l.e, k % mdmc_ensemble::kDistSlots);
        if (!rows) return -1;
        for (int j = 0; j < r.J; ++j) submit_dist_file(r, r.c[j], k, rows + (size_t)j * TKDE_BINS);
        return 0;
    };
    if (l.begin()) return -1;
    for (int k = 0; k < T; k++) {
        const bool gr = k % 100 == 0;
        if (ensemble_tag_moments(l.e, k, true) || ensemble_qt_dist_x(l.e, k % mdmc_ensemble::kDistSlots) ||
            (gr && l.pair_corr_queue()) || l.temperatures(k) || l.md_step() || l.store_velocities(k))
            return -1;
        if (gr && r.verbose) printf("%d\n", k);
        if (gr && drain_pair_corr(r, k)) return -1;
        if (k >= kLag && drain(k - kLag)) return -1;
    }
    for (int k = std::max(0, T - kLag); k < T; ++k)
        if (drain(k)) return -1;
    if (l.end()) return -1;
    for (int j = 0; j < r.J; ++j)
        if (write_recorded_qtt(r.c[j], fm.f[j], ft.f[j])) return -1;
    return 0;
}

// QTT step 6 :1235-1245: per step the tagged moments and distribution, g(r) every 100, the temperature
// (all read back into the member's landing area, evDrain behind them), then the MD step.  The distribution
// files are formatted and written by the run's pool in every mode; taggedMoments.dat and temperature.dat are
// one appended line a step, in order, and stay here.  The ensemble lane has a body of its own (above).
int stage_record_qtt(Run& r) {
    const int T = r.c[0]->T;
    start_writer(r);
    Files fm, ft;
    for (int j = 0; j < r.J; ++j) {
        fm.f.push_back(open_in(r.c[j], "taggedMoments.dat", "a"));
        ft.f.push_back(open_in(r.c[j], "temperature.dat", "a"));
        if (!fm.f.back() || !ft.f.back())
            return set_error("cannot open taggedMoments.dat / temperature.dat in %s", r.c[j]->saveDir.c_str());
    }
    if (r.lanes[0].e) return stage_record_qtt_batched(r, fm, ft) || join_writer(r) ? -1 : 0;
    for (int k = 0; k < T; k++) {
        const bool gr = k % 100 == 0;
        for (const MdLane& l : r.lanes) {
            mdmc_ctx* c = l.c;
            if (tagged_moments_qt_queue(c, c->dOut, true)) return -1;
            HIPCHK(hipMemcpyAsync(c->hStage, c->dOut, 20 * sizeof(double), hipMemcpyDeviceToHost, c->st));
            HIPCHK(hipMemcpyAsync(c->hStage + 24, c->dKde, (size_t)3 * TKDE_BINS * sizeof(double), hipMemcpyDeviceToHost,
                                  c->st));
            if (gr && l.pair_corr_queue()) return -1;
            HIPCHK(launch_temperatures(c->dV, c->N, c->S, c->dOut, c->st));   // recordTemperature :771-792
            HIPCHK(hipMemcpyAsync(c->hStage + 20, c->dOut, 4 * sizeof(double), hipMemcpyDeviceToHost, c->st));
            HIPCHK(hipEventRecord(c->evDrain, c->st));
            if (l.md_step() || l.store_velocities(k)) return -1;
        }
        if (gr && r.verbose) printf("%d\n", k);
        for (int j = 0; j < r.J; ++j) {
            mdmc_ctx* c = r.c[j];
            HIPCHK(hipEventSynchronize(c->evDrain));
            double mom[4], tt[4];
            moments_qt_from_sums(c->hStage, mom);
            fprintf(fm.f[j], "%lg\t%lg\t%lg\t%lg\t%lg\n", k * c->p.timeStep, mom[0], mom[1], mom[2], mom[3]);   // :1114
            submit_dist_file(r, c, k, c->hStage + 24);            // the X row, snapshotted: the next step lands here
            if (gr && write_pair_corr_file(c, k)) return -1;
            temps_from_sums(c, c->hStage + 20, tt);
            fprintf(ft.f[j], "%lg\n", tt[0]);
        }
    }
    return join_writer(r);
}

}  // namespace

int mdmc::run_members(mdmc_ctx* const* cs, int J, mdmc_ensemble* ens, int verbose) {
    Run r{cs, J, ens, verbose, Clock::now(), md_lanes(cs, J, ens)};
    const mdmc_params& p = cs[0]->p;
    if (stage_start(r) || stage_end(r, ST_REST)) return -1;
    if (stage_anneal(r) || stage_end(r, ST_ANNEAL)) return -1;
    if (stage_md(r, p.numPreRecordMDSteps, true) || stage_end(r, ST_PRE)) return -1;     // step 4
    if (cs[0]->qt) {                                             // the QT tagging programs, QTT:1222-1251
        if (stage_pump(r) || stage_end(r, ST_PUMP)) return -1;
        if (stage_record_qtt(r) || stage_end(r, ST_REC)) return -1;
        if (stage_autocorrelations(r) || stage_end(r, ST_AUTO)) return -1;
    } else {
        if (stage_record_mcmd(r) || stage_end(r, ST_REC)) return -1;
        if (stage_autocorrelations(r) || stage_end(r, ST_AUTO)) return -1;
        if (stage_anisotropy(r) || stage_end(r, ST_REST)) return -1;
    }
    if (verbose) fflush(stdout);
    return 0;
}

// main() :1030-1167 (QTT:1140-1254)
extern "C" int mdmc_run(mdmc_ctx* c, int verbose) {
    if (!c) return set_error("NULL context");
    mdmc_ctx* one[1] = {c};
    return mdmc::run_members(one, 1, nullptr, verbose);
}
