// mdlc — drop-in command line for laserCoolNoPlasmaThreeState.cpp.
//
//   reference:  ./a.out <job>                      (LC3:362; parameters are globals :54-88)
//   this:       mdlc <job> [--Name=value ...]      (same parameter names and defaults; --njobs=J runs
//               jobs <job> .. <job> + J - 1 as one ensemble, each into its own job%d directory)
//   --sweep=NAME:v1,v2,... (NAME one of detuning, Om, temperature; may be given once per name) runs a parameter
//   scan as one ensemble (mdlc_create_sweep): the points are the product of the lists, the first-given NAME
//   slowest, each with --njobs replicas; every member writes the tree the reference writes when it is compiled
//   and run at that point.
//
// Runs main() (LC3:356-408) on the GPU through include/mdlc.h and writes the same directory tree
// and energies.dat.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mdlc.h"
#include "mdqt.h"
#include "mdqt_cli_args.hpp"

static void usage(void) {
    fprintf(stderr,
            "usage: mdlc <job> [--N0=1000] [--detuning=-0.5] [--Om=0.5] [--tmax=45000] [--applyForce=1]\n"
            "                  [--sampleFreq=1000] [--temperature=0.01] [--vKick=0.0012076] [--dt=0.01]\n"
            "                  [--saveDirectory=dataLaserCoolTestDoppShift/] [--njobs=1]\n"
            "                  [--seed=<default time(NULL)+job>] [--device=-1] [--quiet=0]\n"
            "                  [--print-directory=0]\n"
            "                  [--sweep=NAME:v1,v2,... ...]   a scan of detuning | Om | temperature: the points are the\n"
            "                  product of the lists (the first NAME slowest; each NAME once), --njobs replicas of each\n");
}

// --sweep: the NAMEs and their fields (mdqt_cli_args.hpp)
static const char* const sweep_names[] = {"detuning", "Om", "temperature"};
static double mdlc_params::*const sweep_fields[] = {&mdlc_params::detuning, &mdlc_params::Om, &mdlc_params::temperature};

int main(int argc, char** argv) {
    if (argc < 2) { usage(); return 2; }
    mdlc_params p;
    mdlc_default_params(&p);
    const double job = atof(argv[1]);                       // LC3:362
    p.job = (uint32_t)job;
    int seed_given = 0, quiet = 0, print_dir = 0;
    SweepAxes axes;                                         // --sweep: the axes in the order given
    for (int i = 2; i < argc; ++i) {
        char key[64];
        const char* v;
        if (!cli_key_value(argv[i], key, sizeof key, &v)) { usage(); return 2; }
#define DPAR(name) if (!strcmp(key, #name)) { p.name = atof(v); continue; }
#define IPAR(name) if (!strcmp(key, #name)) { p.name = atoi(v); continue; }
        DPAR(detuning) DPAR(Om) DPAR(tmax) DPAR(temperature) DPAR(vKick) DPAR(dt)
        IPAR(N0) IPAR(applyForce) IPAR(sampleFreq) IPAR(device) IPAR(njobs)
#undef DPAR
#undef IPAR
        if (!strcmp(key, "quiet")) { quiet = atoi(v); continue; }
        if (!strcmp(key, "print-directory")) { print_dir = atoi(v); continue; }
        if (!strcmp(key, "sweep")) {
            if (!axes.add(v, sweep_names)) { usage(); return 2; }
            continue;
        }
        if (!strcmp(key, "seed")) { p.seed = (uint32_t)strtoul(v, NULL, 10); seed_given = 1; continue; }
        if (!strcmp(key, "saveDirectory")) {
            strncpy(p.saveDirectory, v, sizeof(p.saveDirectory) - 1);
            continue;
        }
        fprintf(stderr, "mdlc: unknown parameter %s\n", key);
        return 2;
    }
    const bool scan = !axes.empty();
    std::vector<mdlc_params> points;                        // of a scan (their number is the library's to refuse)
    if (scan) axes.points(p, sweep_fields, 0, &points);
    if (print_dir && scan) {                                // every member's directory, in member order: no GPU needed
        const long members = (long)points.size() * (p.njobs > 0 ? p.njobs : 1);
        for (long k = 0; k < members; ++k) {
            mdlc_params pk;
            char d[1024];
            if (mdlc_sweep_params(points.data(), (int)points.size(), (int)k, &pk) != 0 ||
                mdlc_format_directory(&pk, pk.job, d, sizeof d) != 0) {
                fprintf(stderr, "mdlc: %s\n", mdqt_last_error());
                return 1;
            }
            printf("%s\n", d);
        }
        return 0;
    }
    if (print_dir) {                                        // the directory names only: no GPU needed
        for (int k = 0; k < (p.njobs > 0 ? p.njobs : 1); ++k) {
            char d[1024];
            if (mdlc_format_directory(&p, p.job + (uint32_t)k, d, sizeof d) != 0) {
                fprintf(stderr, "mdlc: %s\n", mdqt_last_error());
                return 1;
            }
            printf("%s\n", d);
        }
        return 0;
    }
    if (!seed_given) p.seed = (uint32_t)(time(NULL) + job); // the reference: random_device (:45), srand48(time + job) (:389)
    mdlc_ctx* c = NULL;
    for (auto& q : points) q.seed = p.seed;
    if ((scan ? mdlc_create_sweep(points.data(), (int)points.size(), &c) : mdlc_create(&p, &c)) != 0) {
        fprintf(stderr, "mdlc: %s\n", mdqt_last_error());
        return 1;
    }
    const int rc = mdlc_run(c, !quiet);
    if (rc != 0) fprintf(stderr, "mdlc: %s\n", mdqt_last_error());
    mdlc_destroy(c);
    return rc ? 1 : 0;
}
