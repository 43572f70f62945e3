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

#include <vector>

#include "mdlc.h"
#include "mdqt.h"

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

// --sweep: one axis of the scan
enum { kSweepNames = 3, kSweepMax = 1024 };
static const char* const sweep_names[kSweepNames] = {"detuning", "Om", "temperature"};
struct SweepAxis {
    int field, n;
    double v[kSweepMax];
};
static double* sweep_field(mdlc_params* p, int field) {
    double* const f[kSweepNames] = {&p->detuning, &p->Om, &p->temperature};
    return f[field];
}
// "NAME:v1,v2,..." -> the axis; 0 if it is one (a sweepable NAME, a non-empty list of numbers)
static int parse_sweep(const char* v, SweepAxis* ax) {
    const char* colon = strchr(v, ':');
    if (!colon) return -1;
    ax->field = -1;
    for (int f = 0; f < kSweepNames; ++f)
        if (strlen(sweep_names[f]) == (size_t)(colon - v) && !strncmp(v, sweep_names[f], (size_t)(colon - v))) ax->field = f;
    if (ax->field < 0) return -1;
    ax->n = 0;
    for (const char* s = colon + 1;;) {
        char* end = NULL;
        const double x = strtod(s, &end);
        if (end == s || (*end != ',' && *end != 0) || ax->n >= kSweepMax) return -1;
        ax->v[ax->n++] = x;
        if (!*end) return 0;
        s = end + 1;
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { usage(); return 2; }
    mdlc_params p;
    mdlc_default_params(&p);
    const double job = atof(argv[1]);                       // LC3:362
    p.job = (uint32_t)job;
    int seed_given = 0, quiet = 0, print_dir = 0;
    static SweepAxis axes[kSweepNames];                     // --sweep: the axes in the order given
    int naxes = 0;
    for (int i = 2; i < argc; ++i) {
        const char* a = argv[i];
        if (strncmp(a, "--", 2) != 0 || !strchr(a, '=')) { usage(); return 2; }
        char key[64];
        const char* eq = strchr(a, '=');
        size_t kl = (size_t)(eq - a - 2);
        if (kl >= sizeof key) { usage(); return 2; }
        memcpy(key, a + 2, kl);
        key[kl] = 0;
        const char* v = eq + 1;
#define DPAR(name) if (!strcmp(key, #name)) { p.name = atof(v); continue; }
#define IPAR(name) if (!strcmp(key, #name)) { p.name = atoi(v); continue; }
        DPAR(detuning) DPAR(Om) DPAR(tmax) DPAR(temperature) DPAR(vKick) DPAR(dt)
        IPAR(N0) IPAR(applyForce) IPAR(sampleFreq) IPAR(device) IPAR(njobs)
#undef DPAR
#undef IPAR
        if (!strcmp(key, "quiet")) { quiet = atoi(v); continue; }
        if (!strcmp(key, "print-directory")) { print_dir = atoi(v); continue; }
        if (!strcmp(key, "sweep")) {
            SweepAxis* ax = &axes[naxes < kSweepNames ? naxes : 0];
            if (naxes >= kSweepNames || parse_sweep(v, ax)) { usage(); return 2; }
            for (int o = 0; o < naxes; ++o)
                if (axes[o].field == ax->field) { usage(); return 2; }     // a NAME given twice
            ++naxes;
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
    std::vector<mdlc_params> points;                        // the axes' product, the first axis slowest
    if (naxes > 0) {
        long npoints = 1;
        for (int o = 0; o < naxes; ++o) npoints *= axes[o].n;
        points.assign((size_t)npoints, p);
        for (long q = 0; q < npoints; ++q) {
            long rest = q;
            for (int o = naxes - 1; o >= 0; --o) {
                *sweep_field(&points[q], axes[o].field) = axes[o].v[rest % axes[o].n];
                rest /= axes[o].n;
            }
        }
    }
    if (print_dir && naxes > 0) {                           // every member's directory, in member order: no GPU needed
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
    if ((naxes > 0 ? mdlc_create_sweep(points.data(), (int)points.size(), &c) : mdlc_create(&p, &c)) != 0) {
        fprintf(stderr, "mdlc: %s\n", mdqt_last_error());
        return 1;
    }
    const int rc = mdlc_run(c, !quiet);
    if (rc != 0) fprintf(stderr, "mdlc: %s\n", mdqt_last_error());
    mdlc_destroy(c);
    return rc ? 1 : 0;
}
