/*
 * mdmc.h — C ABI of the MI355X engine for the reference's Monte-Carlo + MD analytics program
 *   MonteCarloFollowedByMDAndTempAnisotropy.cpp        ("MCMD" below, tlangin/MDQTPlasmaSims)
 * (SURVEY §8(f)4).  The reference's seam is a set of functions over globals (MCMD:130-147)
 * driven by main() (MCMD:1030-1167); every entry point below names the function it replaces.
 *
 * RNG: the reference's own std::mt19937 (seeded from std::random_device, MCMD:52-53; here from
 * `seed`) with std::uniform_real_distribution<double>(0,1) and std::normal_distribution
 * (MCMD:54, :87), consumed in the reference's order: the Metropolis draws inside the device
 * MC kernel (mt19937 + libstdc++ generate_canonical<double, 53> on the GPU, the state handed
 * over from and back to the host engine), the Maxwell-Boltzmann velocities, collision rolls and
 * tag rolls on the host.  With the same seed the trajectory follows the reference program's
 * stream: the Metropolis energy change is summed in a fixed tree order (and, with force_kernel 1,
 * from reciprocal-form pair energies with a polynomial exp) where the reference sums
 * sequentially with libm exp (MCMD:341-357), so an accept decision whose dice lies within a few
 * ulp of exp(-dE Gamma / 2) can go the other way — the stream then shifts and the runs part
 * statistically.  The parity tests pin 3,000 MC steps bit for bit against the reference build;
 * longer horizons are statistical parity, not a bitwise guarantee.
 *
 * Conventions as include/mdqt.h: opaque context, int status (0 ok, <0 error; message in
 * mdqt_last_error()), caller-owned host buffers, R/V/A as [3][N] row-major like the reference's
 * `double R[3][N]` (MCMD:110-112), device state resident between calls.
 *
 * The same engine runs the QT spin-tagging variants of the program ("QTT":
 * MonteCarloFollowedByQTTagging408Linear.cpp / 408Quad.cpp / 422Linear.cpp; qt_model 1 / 2 / 3):
 * the same MC anneal and collisional MD, then a pump period of QT steps (the optical-pumping
 * qstep of include/mdqt.h's qt_model, QTT:555, driven by this system's velocities) between MD
 * steps, QT tagging (QTT:1022) and collisionless MD recording the tagged ions' moments and
 * velocity distribution (QTT:1069-1138) and the autocorrelations.  Wavefunctions start as the
 * reference's random S superpositions from its drand48 stream (default seed, QTT:224-239); the
 * QT jump draws use the Philox stream of include/mdqt.h (keyed by seed, job, ion, qstep index)
 * instead of the reference's shared drand48.
 */
#ifndef MDMC_H
#define MDMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's compile-time inputs (MCMD:62-107), same names, same defaults. */
typedef struct mdmc_params {
    int N;                        /* :66  particles; a perfect cube (cubic-lattice init :182-201) */
    double kappa;                 /* :67  screening parameter                                    */
    double Gamma;                 /* :68  coupling (inverse normalised temperature)              */
    double n;                     /* :69  density (1e14 m^-3): laser-force units (:491-496)      */
    double collisionFreq;         /* :75  collision rate of the collisional MD stages           */
    int monteCarloSteps;          /* :80                                                         */
    double maxRStep;              /* :81  largest MC displacement                                */
    double pairPairStep;          /* :82  g(r) bin width (units of a)                            */
    double timeStep;              /* :88                                                         */
    int numPreRecordMDSteps;      /* :89                                                         */
    int numVelAutoCorrsSteps;     /* :90                                                         */
    int numInstantaneousAnisotropySteps; /* :96                                                  */
    int numReestablishEquilSteps; /* :97                                                         */
    double tempPercentDiff;       /* :98                                                         */
    int applyForceAlongOneAxisOnly; /* :103                                                      */
    double beta;                  /* :104 heating / cooling rate (s^-1)                          */
    int anisotropyEstablishmentTime; /* :105 (us)                                                */
    int anisotropyFromForcesRelaxSteps; /* :107                                                  */
    /* ---- extensions ---- */
    uint32_t seed;                /* mt19937 seed (reference: std::random_device, :52-53)       */
    uint32_t job;                 /* argv[1] (:1035)                                             */
    int device;                   /* HIP device ordinal (-1 = current)                           */
    int force_kernel;             /* 1 (default): reciprocal pair forms (MD forces, MC energies;
                                   * a few ulp per pair), 0: the reference's operations          */
    /* ---- QT tagging variants (QTT:84-121) ---- */
    int qt_model;                 /* 0: MCMD (no QT); 1: 408 linear, 2: 408 quad, 3: 422 linear    */
    double tpumpreal;             /* QTT:85 pump time (s)                                          */
    double detuning;              /* QTT:86 pump detuning (units of gamma)                         */
    double Om;                    /* QTT:87 Rabi frequency (units of gamma)                        */
    char saveDirectory[256];      /* :62 */
} mdmc_params;

typedef struct mdmc_ctx mdmc_ctx;

void        mdmc_default_params(mdmc_params* p);              /* MCMD:62-107 defaults         */
/* the QT tagging program's defaults (QTT:75-121: n = 2, 100000 MC steps, 1500 recorded steps,
 * the model's pump time, detuning, Rabi frequency and save directory); model 1..3 */
int         mdmc_default_params_qt(mdmc_params* p, int model);
int         mdmc_create(const mdmc_params* p, mdmc_ctx** out); /* + rng (:52-55), L, rCut (:73-74) */
void        mdmc_destroy(mdmc_ctx* c);
/* "N", "L", "rCut", "nbins", "collisionFreq"; QT: "plasmaToQuantumTimestepRatio",
 * "quantumTimestep", "gamToEinsteinFreq", "plasVelToQuantVel", "decayRatio", "pumpMDTimeSteps" */
double      mdmc_get_const(const mdmc_ctx* c, const char* name);

/* ---- the program's functions ---- */
int mdmc_init(mdmc_ctx* c);                 /* init() :173-203 + calculatePotentialEnergyForParticles() :207-245 */
int mdmc_monte_carlo(mdmc_ctx* c, int nsteps, long long* accepted); /* MonteCarloStep() x n, :315-382 */
int mdmc_md_steps(mdmc_ctx* c, int nsteps); /* MDStep() x n, :504-511 (stepPositions, calculateAccelerations,
                                             * stepVelocities with collisions and laser force :452-502) */
int mdmc_set_collision_freq(mdmc_ctx* c, double f); /* collisionFreq = f (main :1093, :1125, :1139) */
int mdmc_set_laser_force(mdmc_ctx* c, int on);      /* addLaserForce (main :1138, :1155)              */
/* recordPairPairCorr :584-652: g[nbins], nbins = (int)((L/2) / pairPairStep) (the file's rows) */
int mdmc_pair_corr(mdmc_ctx* c, double* g, int cap, int* nbins);
int mdmc_record_velocities(mdmc_ctx* c, int k);     /* recordVelsForAutocorrelations :513-523   */
/* recordVAF / recordLongViscAutoCorr / recordVCubeAutoCorr / recordVFourthAutoCorr :655-807 over
 * the stored velocities: out [4][numVelAutoCorrsSteps] */
int mdmc_autocorrelations(mdmc_ctx* c, double* out);
int mdmc_set_velocity_store(mdmc_ctx* c, const double* vs); /* [3][N][numVelAutoCorrsSteps] (tests) */
/* out4 = <v^2> over all components (recordTemperature :525-546), <vx^2>, <vy^2>, <vz^2> (:560-581) */
int mdmc_temperatures(mdmc_ctx* c, double out4[4]);
int mdmc_anisotropize(mdmc_ctx* c);                 /* anisotropizeVelocities :548-558          */
int mdmc_tag_particles(mdmc_ctx* c, int* tags4);    /* tagParticles :810-921; tags4 [4][N] or NULL */
/* recordTaggedParticleMoments :923-1028: out16 = (first, second - 1/Gamma, third,
 * fourth - 3/Gamma^2) for taggedOne .. taggedFour */
int mdmc_tagged_moments(mdmc_ctx* c, double out16[16]);
int mdmc_get_state(mdmc_ctx* c, double* R, double* V, double* A, double* U);    /* NULL = skip */
int mdmc_set_state(mdmc_ctx* c, const double* R, const double* V, const double* A, const double* U);
int mdmc_setup_directories(mdmc_ctx* c);            /* main() :1037-1058                        */
const char* mdmc_save_directory(const mdmc_ctx* c);
int mdmc_run(mdmc_ctx* c, int verbose);             /* main() :1030-1167 (QTT: :1140-1254): every stage and file */

/* ---- QT tagging variants (qt_model 1..3) ---- */
int mdmc_qsteps(mdmc_ctx* c, int n);                /* qstep() x n (QTT:555-756), velocities read from the MD state */
/* tagParticles (QTT:1022-1067): tags [N] 0/1 (or NULL), *n_up = number tagged (or NULL) */
int mdmc_tag_qt(mdmc_ctx* c, int* tags, int* n_up);
/* recordTaggedParticleMoments (QTT:1069-1138): out4 = first .. fourth moment of vx over the tagged
 * ions; dist (or NULL) = [3][4001] normalised velocity distributions of the tagged ions on the
 * bins (j - 2000) * 0.0025 (the reference writes the x row to vel_distX_timestep%06d.dat) */
int mdmc_tagged_moments_qt(mdmc_ctx* c, double out4[4], double* dist);
int mdmc_get_psi(mdmc_ctx* c, double* psi);         /* [N][12][2] (re, im; states past the model's zero) */
int mdmc_set_psi(mdmc_ctx* c, const double* psi);

/* ---- ensembles ----
 * The reference runs these programs as a Slurm array of independent jobs (exampleSlurmFile.slurm:3,16,
 * `srun tagQuad $SLURM_ARRAY_TASK_ID`).  An ensemble holds njobs such jobs in one process: member k has
 * job + k and seed + k, and its state and files are bit for bit those of its own run.  A single job's
 * Metropolis anneal is one workgroup on one CU (the chain is sequential); the ensemble anneals all members
 * with ONE launch of njobs workgroups, so N <= 6144 (the LDS-resident kernel).  The MD stages run one of two
 * ways (mdmc_ensemble_set_md_batch), with the same bits either way:
 *   md_batch 0 (default)  every member's own launches queued on its own stream, so they overlap on the chip;
 *   md_batch 1            one force launch and one velocity-Verlet launch per step for ALL members (plus one
 *                         collision scatter on a step where a member has a hit), and one launch per kind for
 *                         the per-step observables of the recorded stages, on the ensemble's stream: the
 *                         single-job kernels' bodies on each member's own argument block in device memory.
 *                         mdmc_ensemble_md_steps and, in mdmc_ensemble_run, every MD stage go this way; g(r) and
 *                         the autocorrelations stay per member.  For the QT tagging programs (qt_model 1..3) the
 *                         QT substeps, the tagging and the tagged ions' moments and X distribution are batched
 *                         too (the mdmc_ensemble_*qt* calls below; the pump and recorded stage of the run).
 * Members need no lockstep: any mdmc_* call on a member between ensemble calls is legal and the member simply
 * carries its state (its buffer parity, its stale pre-advanced positions, its own collision frequency and
 * laser force included). */
typedef struct mdmc_ensemble mdmc_ensemble;
int       mdmc_ensemble_job_params(const mdmc_params* base, int k, mdmc_params* out); /* job+k, seed+k only; k in [0,1024) */
int       mdmc_ensemble_create(const mdmc_params* p, int njobs, mdmc_ensemble** out); /* njobs x mdmc_create; 1..1024 */
void      mdmc_ensemble_destroy(mdmc_ensemble* e);
int       mdmc_ensemble_size(const mdmc_ensemble* e);
mdmc_ctx* mdmc_ensemble_job(mdmc_ensemble* e, int k);      /* owned by the ensemble */
int       mdmc_ensemble_init(mdmc_ensemble* e);            /* mdmc_init of every member */
/* mdmc_monte_carlo of every member in batched launches; accepted [njobs] or NULL */
int       mdmc_ensemble_monte_carlo(mdmc_ensemble* e, int nsteps, long long* accepted);
int       mdmc_ensemble_md_steps(mdmc_ensemble* e, int nsteps);  /* mdmc_md_steps of every member, step by step */
int       mdmc_ensemble_set_md_batch(mdmc_ensemble* e, int mode); /* 0: member by member, 1: batched; else an error */
int       mdmc_ensemble_md_batch(const mdmc_ensemble* e);         /* the mode (< 0: error) */
/* kernel launches the batched MD path has issued since creation (md_batch 0 leaves it unchanged): 2 per
 * collisionless step whatever njobs is, + 1 on a step with a hit, + 1 per observable kind and step, + 1 per
 * member whose pre-advanced positions were stale at the start of a call */
int       mdmc_ensemble_md_launches(mdmc_ensemble* e, unsigned long long* out);
int       mdmc_ensemble_run(mdmc_ensemble* e, int verbose);      /* mdmc_run of every member, stage by stage */
int       mdmc_ensemble_enable_timing(mdmc_ensemble* e, int on); /* timestamps on the batched launches, stage timers */
/* out[0..5): the anneal launches since the last call: sum (ms), count, median, min, max (ms);
 * out[5..11): wall ms of the last run's stages (timing on): anneal, pre-record MD, QT pump, recorded MD,
 * autocorrelations, the rest; out[11..16), out[16..21): the same five figures of the batched force and of the
 * batched velocity-Verlet launches (md_batch 1, timing on; the launches' own timestamps); out[21..26),
 * out[26..31): those of the batched QT launches and of the X distribution's chunk kernel.
 * Fills min(n, 31) entries, n >= 3 */
int       mdmc_ensemble_kernel_times(mdmc_ensemble* e, double* out, int n);

/* ---- ensembles of the QT tagging variants (qt_model 1..3; an error with the context-has-no-QT message
 * otherwise) ----
 * Under md_batch 0 each call is the members' own call, member by member.  Under md_batch 1 each is one launch
 * for all members (or the few stated) on the ensemble's stream, fenced behind the members' streams and
 * synchronised once; every member computes what its own call computes, bit for bit. */
/* mdmc_qsteps of every member: ceil(n / 32) launches whatever njobs is.  Every member keeps its own qstep index,
 * so members need not be in lockstep */
int       mdmc_ensemble_qsteps(mdmc_ensemble* e, int n);
/* mdmc_tag_qt of every member, one launch: tags [njobs][N] or NULL, n_up [njobs] or NULL */
int       mdmc_ensemble_tag_qt(mdmc_ensemble* e, int* tags, int* n_up);
/* mdmc_tagged_moments_qt of every member: out4 [njobs][4]; distX [njobs][4001] or NULL.  X ONLY: the row the
 * programs write (vel_distX_timestep%06d.dat, QTT:1128-1136) and the only one a recorded step needs, so the
 * batched kernel evaluates a third of the three-row kernel's terms; distX[k] holds the bits of row 0 of member
 * k's mdmc_tagged_moments_qt.  One launch for the moments, two more with distX */
int       mdmc_ensemble_tagged_moments_qt(mdmc_ensemble* e, double* out4, double* distX);
/* kernel launches the batched QT, tagging, moment and distribution paths have issued since creation (md_batch 0
 * leaves it unchanged); mdmc_ensemble_md_launches does not count them */
int       mdmc_ensemble_qt_launches(mdmc_ensemble* e, unsigned long long* out);

#ifdef __cplusplus
}
#endif
#endif /* MDMC_H */
