// mdqt — drop-in command line for laserCoolingPlusExpansionMDQTSpeedUp.cpp.
//
//   reference:  ./a.out <job>                      (SpeedUp:1145, parameters are #defines :56-85)
//   this:       mdqt <job> [--Name=value ...]      (same parameter names and defaults)
//
// Writes the same directory tree (SpeedUp:1143-1160) and the same files
// (energies.dat, vel_dist{X,Y,Z}_time%06d.dat, statePopulationsVsVTime%06d.dat,
// ions_/conditions_/VZERO_/wvFns_timestep%06d.dat) through the C ABI of include/mdqt.h.
//
//   --pump_program=1|2|3 runs instead the main() of randomFrozenStartTag408Linear.cpp /
//   408Quad.cpp / 422Linear.cpp (their defaults, :52-80; mdqt_run_pump): the PumpTime...
//   directory, spinUpIons_*, taggedMoments.dat, tagged vel_distX_*, VAF.dat, the conditions.
//
//   --njobs=J runs the jobs <job> .. <job>+J-1 of the reference's Slurm array (exampleSlurmFile.slurm:3)
//   as one ensemble (mdqt_ensemble_run: one force and one QT launch per MD step for all of them), job k
//   seeded seed + k; each job's files are those of `mdqt <job>+k --seed=<seed>+k`; prints every N.
//   --output_batch=0|1 (with --njobs): output() of all jobs in one device pass (1) or job after job (0, the
//   default); the same files either way.
//   --pool=0|1 (with --njobs): 1 = every output() also writes the observables pooled over the jobs of each parameter
//   point — the energies averaged with their standard errors, the velocity distributions added up, the S / P / D
//   populations binned against vx — into pool_job<first>to<last>/ beside the jobs' directories; implies
//   --output_batch=1.  --member_files=0|1 (with --pool=1): 0 = the jobs' energies.dat, vel_dist* and
//   statePopulationsVsVTime* are not written (their conditions files still are: the run can be resumed).
//
//   --sweep=NAME:v1,v2,... (with --njobs=R; NAME one of detuning, detuningDP, Om, OmDP, fracOfSig; may be given
//   for several names) runs a parameter scan as one ensemble (mdqt_ensemble_create_sweep): the points are the
//   Cartesian product of the lists, the first-named axis slowest, every other parameter as given; each point
//   has the R jobs <job> .. <job>+R-1 (seeds seed .. seed+R-1), and each job's files are those of the single
//   run with the point's parameters; prints every N in member order (point-major).
//
//   --pump_program=m --pump_jobs=J does the same for the pumping programs (mdqt_pump_ensemble_run): the jobs
//   <job> .. <job>+J-1 stepped in batched launches, each job's tree byte for byte that of
//   `mdqt <job>+k --pump_program=m --seed=<seed>+k`; prints every N.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mdqt.h"
#include "mdqt_cli_args.hpp"

static void usage(void) {
    fprintf(stderr,
            "usage: mdqt <job> [--Ge=0.1] [--tmax=30] [--density=2] [--sig0=4] [--Te=19]\n"
            "                  [--fracOfSig=0] [--detuning=-1] [--detuningDP=1] [--Om=1] [--OmDP=1]\n"
            "                  [--N0=3500] [--newRun=1] [--c0=0] [--sampleFreq=40]\n"
            "                  [--reNormalizewvFns=0] [--saveDirectory=dataLaserCool/]\n"
            "                  [--seed=<srand48 seed; default time(NULL)+job as SpeedUp:1219>]\n"
            "                  [--qt=1] [--device=-1]\n"
            "       mdqt <job> --pump_program=1|2|3 [--tpumpreal=2e-7] [--tstartV0=15] [... as above]\n"
            "       mdqt <job> --njobs=J [... as above]   jobs <job> .. <job>+J-1 as one ensemble (J >= 1;\n"
            "                  seeds seed .. seed+J-1; not with --pump_program: --pump_jobs)\n"
            "                  [--output_batch=0|1]   output() of all jobs in one device pass (1) or job after job (0)\n"
            "                  [--pool=0|1]   1: every output() also writes each point's observables pooled over its jobs\n"
            "                  to pool_job<first>to<last>/ (implies --output_batch=1; not with --output_batch=0)\n"
            "                  [--member_files=0|1]   0 (with --pool=1): no energies.dat, vel_dist*, statePopulationsVsVTime*\n"
            "                  of the jobs themselves\n"
            "                  [--sweep=NAME:v1,v2,... ...]   with --njobs=R: a scan of detuning | detuningDP | Om | OmDP |\n"
            "                  fracOfSig, R jobs per point, as one ensemble (points: the product of the lists, the first\n"
            "                  NAME slowest; points x R <= 1024; each NAME once)\n"
            "       mdqt <job> --pump_program=1|2|3 --pump_jobs=J [...]   the pump jobs <job> .. <job>+J-1 as one\n"
            "                  ensemble (1 <= J <= 1024; seeds seed .. seed+J-1; not with --njobs)\n");
}

// --sweep: the NAMEs and their fields (mdqt_cli_args.hpp)
static const char* const sweep_names[] = {"detuning", "detuningDP", "Om", "OmDP", "fracOfSig"};
static double mdqt_params::*const sweep_fields[] = {&mdqt_params::detuning, &mdqt_params::detuningDP, &mdqt_params::Om,
                                                    &mdqt_params::OmDP, &mdqt_params::fracOfSig};

int main(int argc, char** argv) {
    if (argc < 2) { usage(); return 2; }
    mdqt_params p;
    mdqt_default_params(&p);
    int pump = 0;                                           // the pumping programs' defaults first
    for (int i = 2; i < argc; ++i)
        if (!strncmp(argv[i], "--pump_program=", 15)) pump = atoi(argv[i] + 15);
    if (pump < 0 || pump > 3) { usage(); return 2; }
    if (pump) mdqt_default_params_pump(&p, pump);
    const double job = atof(argv[1]);                       // SpeedUp:1145
    p.job = (uint32_t)job;
    int seed_given = 0;
    long njobs = -1;                                        // --njobs: the jobs of an ensemble (-1: not given)
    long pump_jobs = -1;                                    // --pump_jobs: the jobs of a pump ensemble
    long output_batch = -1;                                 // --output_batch: the ensemble's option (-1: its default)
    long pool = -1, member_files = -1;                      // --pool, --member_files: the ensemble's options
    SweepAxes axes;                                         // --sweep: the axes in the order given
    for (int i = 2; i < argc; ++i) {
        char key[64];
        const char* v;
        if (!cli_key_value(argv[i], key, sizeof key, &v)) { usage(); return 2; }
#define DPAR(name) if (!strcmp(key, #name)) { p.name = atof(v); continue; }
#define IPAR(name) if (!strcmp(key, #name)) { p.name = atoi(v); continue; }
        DPAR(Ge) DPAR(tmax) DPAR(density) DPAR(sig0) DPAR(Te) DPAR(fracOfSig) DPAR(detuning)
        DPAR(detuningDP) DPAR(Om) DPAR(OmDP) DPAR(tpumpreal) DPAR(tstartV0)
        IPAR(N0) IPAR(newRun) IPAR(c0) IPAR(sampleFreq) IPAR(reNormalizewvFns) IPAR(device) IPAR(qt_model)
#undef DPAR
#undef IPAR
        if (!strcmp(key, "qt")) { p.qt_enabled = atoi(v); continue; }
        if (!strcmp(key, "pump_program")) continue;         // applied above
        if (!strcmp(key, "njobs")) {
            char* end = NULL;
            njobs = strtol(v, &end, 10);
            if (end == v || *end || njobs < 1 || njobs > 1024) { usage(); return 2; }
            continue;
        }
        if (!strcmp(key, "output_batch")) {
            char* end = NULL;
            output_batch = strtol(v, &end, 10);
            if (end == v || *end || output_batch < 0 || output_batch > 1) { usage(); return 2; }
            continue;
        }
        if (!strcmp(key, "pool")) {
            if (!cli_switch(v, &pool)) { usage(); return 2; }
            continue;
        }
        if (!strcmp(key, "member_files")) {
            if (!cli_switch(v, &member_files)) { usage(); return 2; }
            continue;
        }
        if (!strcmp(key, "sweep")) {
            if (!axes.add(v, sweep_names)) { usage(); return 2; }
            continue;
        }
        if (!strcmp(key, "pump_jobs")) {
            char* end = NULL;
            pump_jobs = strtol(v, &end, 10);
            if (end == v || *end || pump_jobs < 1 || pump_jobs > 1024) { usage(); return 2; }
            continue;
        }
        if (!strcmp(key, "seed")) { p.seed = (uint32_t)strtoul(v, NULL, 10); seed_given = 1; continue; }
        if (!strcmp(key, "saveDirectory")) {
            strncpy(p.saveDirectory, v, sizeof(p.saveDirectory) - 1);
            continue;
        }
        fprintf(stderr, "mdqt: unknown parameter %s\n", key);
        return 2;
    }
    if (njobs > 0 && pump) { usage(); return 2; }
    if (pump_jobs > 0 && (!pump || njobs > 0)) { usage(); return 2; }
    if (output_batch >= 0 && njobs < 1) { usage(); return 2; }
    if (!axes.empty() && (njobs < 1 || pump)) { usage(); return 2; }
    if ((pool >= 0 || member_files >= 0) && (njobs < 1 || pump)) { usage(); return 2; }
    if (pool == 1 && output_batch == 0) { usage(); return 2; }
    if (member_files == 0 && pool != 1) { usage(); return 2; }
    if (pool == 1) output_batch = 1;
    if (!seed_given) p.seed = (uint32_t)(time(NULL) + job);   // SpeedUp:1219
    std::vector<mdqt_params> points;                        // of a scan: at most kSweepMax members in all
    if (!axes.empty() && !axes.points(p, sweep_fields, kSweepMax / njobs, &points)) { usage(); return 2; }
    if (njobs > 0) {
        mdqt_ensemble* e = NULL;
        int rc_create;
        if (!axes.empty()) {
            rc_create = mdqt_ensemble_create_sweep(points.data(), (int)points.size(), (int)njobs, &e);
            njobs *= (long)points.size();                   // the members
        } else {
            rc_create = mdqt_ensemble_create(&p, (int)njobs, &e);
        }
        if (rc_create) {
            fprintf(stderr, "mdqt: %s\n", mdqt_last_error());
            return 1;
        }
        if ((output_batch >= 0 && mdqt_ensemble_set_option(e, "output_batch", (int)output_batch)) ||
            (pool >= 0 && mdqt_ensemble_set_option(e, "pool", (int)pool)) ||
            (member_files >= 0 && mdqt_ensemble_set_option(e, "member_files", (int)member_files))) {
            fprintf(stderr, "mdqt: %s\n", mdqt_last_error());
            mdqt_ensemble_destroy(e);
            return 1;
        }
        const int rc = mdqt_ensemble_run(e);
        if (rc) fprintf(stderr, "mdqt: %s\n", mdqt_last_error());
        else
            for (int k = 0; k < (int)njobs; ++k) printf("%i\n", mdqt_get_N(mdqt_ensemble_job(e, k)));
        mdqt_ensemble_destroy(e);
        return rc ? 1 : 0;
    }
    if (pump_jobs > 0) {
        mdqt_pump_ensemble* e = NULL;
        if (mdqt_pump_ensemble_create(&p, (int)pump_jobs, &e)) {
            fprintf(stderr, "mdqt: %s\n", mdqt_last_error());
            return 1;
        }
        const int rc = mdqt_pump_ensemble_run(e);
        if (rc) fprintf(stderr, "mdqt: %s\n", mdqt_last_error());
        else
            for (int k = 0; k < (int)pump_jobs; ++k) printf("%i\n", mdqt_get_N(mdqt_pump_ensemble_job(e, k)));
        mdqt_pump_ensemble_destroy(e);
        return rc ? 1 : 0;
    }
    mdqt_ctx* c = NULL;
    if (mdqt_create(&p, &c)) {
        fprintf(stderr, "mdqt: %s\n", mdqt_last_error());
        return 1;
    }
    int rc = pump ? mdqt_run_pump(c) : mdqt_run(c);
    if (rc) fprintf(stderr, "mdqt: %s\n", mdqt_last_error());
    else printf("%i\n", mdqt_get_N(c));
    mdqt_destroy(c);
    return rc ? 1 : 0;
}
