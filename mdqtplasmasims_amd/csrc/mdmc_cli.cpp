// mdmc — drop-in command line for MonteCarloFollowedByMDAndTempAnisotropy.cpp and, with
// --qt_model=1|2|3, for MonteCarloFollowedByQTTagging408Linear.cpp / 408Quad.cpp / 422Linear.cpp.
//
//   reference:  ./a.out <job>                      (MCMD:1035; parameters are globals :62-107)
//   this:       mdmc <job> [--qt_model=m] [--Name=value ...]   (same parameter names and defaults;
//               --qt_model selects the tagging program and its defaults, QTT:75-121)
//
// Runs main()'s stages (MCMD:1030-1167) on the GPU through include/mdmc.h and writes the same
// directory tree and files (pairPairCorrStepNum%d.dat, temperature.dat, VAF.dat, ...).
//
//   --njobs=J runs the jobs <job> .. <job>+J-1 of the reference's Slurm array (exampleSlurmFile.slurm:3,16)
//   as one ensemble (mdmc_ensemble_run: the J Metropolis chains annealed by one launch), job k seeded
//   seed + k; each job's files are those of `mdmc <job>+k --seed=<seed>+k`.  --md_batch=1 steps the jobs' MD stages
//   in batched launches (mdmc_ensemble_set_md_batch), --md_batch=0 member by member: the same files either way.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mdmc.h"
#include "mdqt.h"
#include "mdqt_cli_args.hpp"

static void usage(void) {
    fprintf(stderr,
            "usage: mdmc <job> [--N=4096] [--kappa=0.5] [--Gamma=3] [--n=0.4] [--collisionFreq=0.25]\n"
            "                  [--monteCarloSteps=200000] [--maxRStep=0.3] [--pairPairStep=0.05]\n"
            "                  [--timeStep=0.005] [--numPreRecordMDSteps=200] [--numVelAutoCorrsSteps=2500]\n"
            "                  [--numInstantaneousAnisotropySteps=2500] [--numReestablishEquilSteps=500]\n"
            "                  [--tempPercentDiff=0.15] [--applyForceAlongOneAxisOnly=0] [--beta=26000]\n"
            "                  [--anisotropyEstablishmentTime=10] [--anisotropyFromForcesRelaxSteps=2000]\n"
            "                  [--saveDirectory=data/] [--seed=<mt19937 seed; default time(NULL)+job>]\n"
            "                  [--device=-1] [--force_kernel=1] [--quiet=0]\n"
            "                  [--qt_model=0|1|2|3] [--tpumpreal=2e-7] [--detuning=-2.5] [--Om=0.7]\n"
            "       mdmc <job> --njobs=J [... as above]   jobs <job> .. <job>+J-1 as one ensemble (J in 1 .. 1024;\n"
            "                  seeds seed .. seed+J-1; N <= 6144)\n"
            "                  [--md_batch=0|1]   with --njobs only: the MD stages member by member (0, default) or\n"
            "                  in batched launches, one force and one velocity-Verlet launch per step for all jobs (1)\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { usage(); return 2; }
    mdmc_params p;
    mdmc_default_params(&p);
    for (int i = 2; i < argc; ++i)                          // the tagging program's defaults first
        if (!strncmp(argv[i], "--qt_model=", 11) && atoi(argv[i] + 11) != 0) {
            if (mdmc_default_params_qt(&p, atoi(argv[i] + 11)) != 0) {
                fprintf(stderr, "mdmc: %s\n", mdqt_last_error());
                return 2;
            }
        }
    const double job = atof(argv[1]);                       // MCMD:1035
    p.job = (uint32_t)job;
    int seed_given = 0, quiet = 0;
    long njobs = -1;                                        // --njobs: the jobs of an ensemble (-1: not given)
    int md_batch = -1;                                      // --md_batch (-1: not given)
    for (int i = 2; i < argc; ++i) {
        char key[64];
        const char* v;
        if (!cli_key_value(argv[i], key, sizeof key, &v)) { usage(); return 2; }
#define DPAR(name) if (!strcmp(key, #name)) { p.name = atof(v); continue; }
#define IPAR(name) if (!strcmp(key, #name)) { p.name = atoi(v); continue; }
        DPAR(kappa) DPAR(Gamma) DPAR(n) DPAR(collisionFreq) DPAR(maxRStep) DPAR(pairPairStep) DPAR(timeStep)
        DPAR(tempPercentDiff) DPAR(beta) DPAR(tpumpreal) DPAR(detuning) DPAR(Om)
        IPAR(N) IPAR(monteCarloSteps) IPAR(numPreRecordMDSteps) IPAR(numVelAutoCorrsSteps)
        IPAR(numInstantaneousAnisotropySteps) IPAR(numReestablishEquilSteps) IPAR(applyForceAlongOneAxisOnly)
        IPAR(anisotropyEstablishmentTime) IPAR(anisotropyFromForcesRelaxSteps) IPAR(device) IPAR(force_kernel)
        IPAR(qt_model)
#undef DPAR
#undef IPAR
        if (!strcmp(key, "quiet")) { quiet = atoi(v); continue; }
        if (!strcmp(key, "njobs")) {
            char* end = NULL;
            njobs = strtol(v, &end, 10);
            if (end == v || *end || njobs < 1 || njobs > 1024) { usage(); return 2; }
            continue;
        }
        if (!strcmp(key, "md_batch")) {
            if (strcmp(v, "0") != 0 && strcmp(v, "1") != 0) { usage(); return 2; }
            md_batch = v[0] - '0';
            continue;
        }
        if (!strcmp(key, "seed")) { p.seed = (uint32_t)strtoul(v, NULL, 10); seed_given = 1; continue; }
        if (!strcmp(key, "saveDirectory")) {
            strncpy(p.saveDirectory, v, sizeof(p.saveDirectory) - 1);
            continue;
        }
        fprintf(stderr, "mdmc: unknown parameter %s\n", key);
        return 2;
    }
    if (md_batch >= 0 && njobs < 1) { usage(); return 2; }    // the mode of an ensemble's MD stages
    if (!seed_given) p.seed = (uint32_t)(time(NULL) + job);   // the reference: std::random_device (:52)
    if (njobs > 0) {
        mdmc_ensemble* e = NULL;
        if (mdmc_ensemble_create(&p, (int)njobs, &e) != 0) {
            fprintf(stderr, "mdmc: %s\n", mdqt_last_error());
            return 1;
        }
        if (md_batch >= 0 && mdmc_ensemble_set_md_batch(e, md_batch) != 0) {
            fprintf(stderr, "mdmc: %s\n", mdqt_last_error());
            mdmc_ensemble_destroy(e);
            return 1;
        }
        const int rc = mdmc_ensemble_run(e, !quiet);
        if (rc != 0) fprintf(stderr, "mdmc: %s\n", mdqt_last_error());
        mdmc_ensemble_destroy(e);
        return rc ? 1 : 0;
    }
    mdmc_ctx* c = NULL;
    if (mdmc_create(&p, &c) != 0) {
        fprintf(stderr, "mdmc: %s\n", mdqt_last_error());
        return 1;
    }
    const int rc = mdmc_run(c, !quiet);
    if (rc != 0) fprintf(stderr, "mdmc: %s\n", mdqt_last_error());
    mdmc_destroy(c);
    return rc ? 1 : 0;
}
