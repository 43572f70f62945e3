/*
 * mdlc.h — C ABI of the MI355X engine for the reference's three-level laser-cooling program
 *   laserCoolNoPlasmaThreeState.cpp                    ("LC3" below, tlangin/MDQTPlasmaSims)
 * the group's Doppler-cooling benchmark: N0 non-interacting ions, a V system (ground state 0,
 * excited states 1 and 2), two counter-propagating beams along x, 4.5 million quantum-trajectory
 * steps per ion at the defaults.  No positions, forces or box.  The reference's seam is init(),
 * qstep() and output() over globals (LC3:105-107) driven by main() (LC3:356-408); every entry
 * point below names what it replaces.
 *
 * Ensemble: the reference is run as a SLURM array of jobs; a context holds `njobs` of them (jobs
 * job .. job + njobs - 1) and steps them in one launch.  Job k is exactly the single-job context
 * with job = k: same velocities, same draws, same files, bit for bit.
 *
 * Parameter scan: the reference is recompiled and rerun for every laser setting, into the tree
 * Om%d/Det%dNumIons%dInitialTemp%duK/job%d/ (LC3:371-380).  mdlc_create_sweep holds npoints parameter points x
 * R replicas (R = njobs) in one context, stepped in one set of launches.  Member k is point k / R, replica
 * r = k % R (point-major), and is exactly the single-job context of that point's parameters with job = job + r.
 * The points may differ in detuning, Om and temperature (the fields the directory name has a level for) and in
 * nothing else.  All points share seed and job, so replica r of every point draws the same u1 / randDir stream
 * (common random numbers), and where the temperature is equal it starts from the same velocities.  Every entry
 * point below works on such a context; where a buffer is job-major it is member-major.
 *
 * RNG.  Velocities: the reference's std::mt19937 (seeded from std::random_device, LC3:45-46; here
 * job number j's engine is mt19937(seed + j), as the reference's srand48(time + job), LC3:389)
 * with its std::normal_distribution (LC3:83), consumed in init()'s order after the one uniform
 * draw of LC3:48.  Quantum jumps: the Philox stream of include/mdqt.h — counter (ion, qstep index), key
 * (seed, job k); u1 is draw 0 and randDir draw 1.  The reference draws both from one drand48
 * stream shared by its OpenMP threads without synchronisation (LC3:163-181, :278): its order is a
 * race and is not reproduced; parity with the reference is statistical.
 *
 * Conventions as include/mdqt.h: opaque context, int status (0 ok, <0 error; message in
 * mdqt_last_error()), caller-owned host buffers, device state resident between calls.  Buffers of
 * an ensemble are job-major: V [njobs][3][N0] (each job's `double V[3][N0]`, LC3:84), psi
 * [njobs][N0][3][2] (re, im), tPart [njobs][N0].
 */
#ifndef MDLC_H
#define MDLC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's compile-time inputs, same names, same defaults. */
typedef struct mdlc_params {
    int N0;                       /* :59  ions                                                    */
    double detuning;              /* :60  detuning (units of gamma)                               */
    double Om;                    /* :61  Rabi frequency (units of gamma)                         */
    double tmax;                  /* :62  (units of 1/gamma)                                      */
    int applyForce;               /* :63  add the kicks to V[0] (:287)                            */
    int sampleFreq;               /* :67  output() every sampleFreq steps                         */
    double temperature;           /* :82  (K): velocity spread 1.0508 sqrt(temperature) (:83)     */
    double vKick;                 /* :88  recoil velocity                                         */
    double dt;                    /* :68, :393 time step (units of 1/gamma)                       */
    /* ---- extensions ---- */
    uint32_t seed;                /* Philox key word 0; mt19937 seed of job number j: seed + j   */
    uint32_t job;                 /* argv[1] (:362): the first job of the ensemble               */
    int device;                   /* HIP device ordinal (-1 = current)                           */
    int njobs;                    /* jobs job .. job + njobs - 1 in one context (default 1)      */
    char saveDirectory[256];      /* :54 */
} mdlc_params;

typedef struct mdlc_ctx mdlc_ctx;

void        mdlc_default_params(mdlc_params* p);               /* LC3:54-88, :393 defaults      */
int         mdlc_create(const mdlc_params* p, mdlc_ctx** out);
void        mdlc_destroy(mdlc_ctx* c);
/* A parameter scan: points[npoints], each with R = points[0].njobs replicas; members point-major.  Refused,
 * before any GPU call and naming the point and the field: npoints < 1; a point that mdlc_create refuses; a
 * field other than detuning, Om and temperature that differs from point 0; two identical points; two points
 * whose directory names collide (Om x 100, detuning x 100 and temperature x 1000000 as integers: detuning
 * -0.501 and -0.502); more than one launch grid of workgroups. */
int         mdlc_create_sweep(const mdlc_params* points, int npoints, mdlc_ctx** out);
/* member k's parameters as a single job (its point's fields, job + r, njobs = 1), after the same refusals;
 * without a context or a GPU */
int         mdlc_sweep_params(const mdlc_params* points, int npoints, int k, mdlc_params* out);
/* "N0", "njobs" (the replicas R of a scan), "npoints" (1 unless a scan), "members" (npoints x njobs), "dt",
 * "stride" (ions per job padded to whole workgroups), "iterations" and "outputs" (main()'s loop counts for
 * tmax, dt, sampleFreq), "qstep_index" */
double      mdlc_get_const(const mdlc_ctx* c, const char* name);

/* init()'s velocity draws (:119-124) for one job, without a context or a GPU: V [3][N0] from
 * mt19937(seed) after the uniform draw of :48, normal_distribution(0, 1.0508 sqrt(temperature)) */
int mdlc_sample_velocities(uint32_t seed, int N0, double temperature, double* V);
/* main()'s directory of job `job` (:371-380) without a context or a GPU:
 * <saveDirectory>Om%d/Det%dNumIons%dInitialTemp%duK/job%d/ into out[cap] */
int mdlc_format_directory(const mdlc_params* p, uint32_t job, char* out, size_t cap);

/* ---- the program's functions ---- */
int mdlc_init(mdlc_ctx* c);                 /* init() :115-131 for every job; qstep index = 0    */
int mdlc_qsteps(mdlc_ctx* c, long long n);  /* qstep() x n, :140-293                              */
/* NULL = skip; qstep: the number of qsteps taken so far (the Philox counter of the next step) */
int mdlc_get_state(mdlc_ctx* c, double* V, double* psi, double* tPart, uint64_t* qstep);
int mdlc_set_state(mdlc_ctx* c, const double* V, const double* psi, const double* tPart, const uint64_t* qstep);
int mdlc_ekin_x(mdlc_ctx* c, double* out);  /* output()'s EkinX (:309-316) of every job: out[njobs] */
int mdlc_setup_directories(mdlc_ctx* c);    /* main() :364-380 for every job                      */
const char* mdlc_save_directory(const mdlc_ctx* c, int k);   /* directory of job job + k          */
/* main() :356-408 for every job: directories, init(), the time loop, energies.dat ("%lg\t%lg\n"
 * of t and EkinX, appended, :319-323) */
int mdlc_run(mdlc_ctx* c, int verbose);

/* measurement (tools/mdlc_rate.py): `warmup` untimed launches of nsteps qsteps each, then `launches`
 * timed ones; ms[launches] = each kernel's own duration from its dispatch timestamps.  The state
 * and the qstep index advance as in mdlc_qsteps. */
int mdlc_time_qsteps(mdlc_ctx* c, int nsteps, int warmup, int launches, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* MDLC_H */
