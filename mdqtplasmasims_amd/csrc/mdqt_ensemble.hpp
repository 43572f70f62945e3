// The MDQT ensembles' private host header: an ensemble over several contexts (struct mdqt_ensemble), the
// optical-pumping ensemble built on it (struct mdqt_pump_ensemble), and the ensemble functions that cross a file
// boundary.  Included by the ensembles' own sources and by the sources that name an ensemble; the sources of one
// context see mdqt_ctx.hpp alone.  Not installed: the C ABI of include/mdqt.h sees both structs as opaque.
#pragma once

#include "mdqt_ctx.hpp"
#include "mdqt_ens_args.hpp"

// J independent jobs stepped in batched launches (mdqt_ensemble.cpp)
struct mdqt_ensemble {
    std::vector<mdqt_ctx*> jobs;
    int dev = 0;
    hipStream_t stream = nullptr;                  // jobs[0]'s own stream, shared by every member
    std::unique_ptr<mdqt::FileWriter> writer;            // the members' output files (<= 16 threads in all)
    mdqt::DevBuf<mdqt::N3Args> dForce;                   // [J] the batched force launch's blocks (Newton-3 members, packed)
    mdqt::DevBuf<mdqt::SubstepArgs> dSub;                // [sub_blocks] the batched QT launches' blocks: [launch][J]
    int sub_blocks = 0;                            // max(J, 1024): mdqt_ensemble_md_steps builds launches ahead
    std::vector<mdqt::N3Args> force_held;                // what dForce holds
    mdqt::PinRing ring;                            // 8 slots: a launch's blocks of either kind, or md_steps' blocks ahead
    int qt_waves = 0;                              // option "qt_waves": register budget of the production QT instance
    bool timing = false;
    mdqt::LaunchTimer timers[2];                   // 0 = force launches, 1 = QT launches
    unsigned long long force_launches = 0;         // force launches issued by ens_forces (batched + the row members' own)
    // a sweep ensemble (mdqt_ensemble_create_sweep): npoints parameter points x replicas, member k = point
    // k / replicas; its QT launches are mdqt_ensemble_sweep_qt.hip's, which take the table per member
    int npoints = 1;
    bool sweep = false;                            // created through the sweep entry (one point included)
    mdqt::DevBuf<mdqt::FastTab> dTabs;             // [npoints] the points' by-lane tables (their first replica's ftabL)
    mdqt::DevBuf<int> dPoint;                      // [J] every member's point
    std::vector<mdqt::FastTab> tabs_held;          // what they hold
    std::vector<int> point_held;
    // the batched output() (mdqt_ensemble_output.cpp): the members' blocks, their results on the device (rows
    // [J][kObsRow] in dScr's layout, the packed columns [sum 4 N_k]) and the pinned slot they come back to
    int output_batch = 0;                          // option "output_batch": 1 = one pass for all members, 0 = member by member
                                                   // (the default: docs/PROGRAMS.md "Batched output()" has the measurement)
    mdqt::DevBuf<mdqt::N3Args> dPot;               // [J] the potential launch's blocks (batched members, packed)
    mdqt::DevBuf<mdqt::EnsObsArgs> dObs;           // [J] the observables' blocks (the same members)
    std::vector<mdqt::N3Args> pot_held;            // what they hold
    std::vector<mdqt::EnsObsArgs> obs_held;
    mdqt::DevBuf<double> dObsRows;                 // [J][kObsRow]
    mdqt::DevBuf<double> dObsCols;                 // [sum 4 N_k]
    mdqt::PinRing obs_ring;                        // one slot: the rows, then the columns
    unsigned long long output_launches = 0;        // kernel launches of the batched output path
    mdqt::LaunchTimer obs_timers[4];               // 0 = the batched potential launches, 1 = the batched KDE launches,
                                                   // 2 = the pooled pass's slot partials, 3 = its sum over replicas
    // the pooled output() (options "pool" and "member_files"; mdqt_ensemble_output.cpp, mdqt_ensemble_pool.hip): each
    // point's observables over its replicas, written to a directory beside the replicas'.  The points' slot sums
    // [npoints][kPopPlanes][kPopSlots] follow the rows in dObsRows and come back with them in one copy.
    bool pump = false;                             // the base of an mdqt_pump_ensemble: neither option applies
    int pool = 0;                                  // option "pool": 1 = every output() also pools each point
    int member_files = 1;                          // option "member_files": 0 = output() writes the pooled files only
};

// J independent jobs of an optical-pumping program stepped in batched launches (mdqt_pump_ensemble.cpp): an
// mdqt_ensemble's members, stream, argument ring, force launch and writer pool, and the pump kernels' blocks
struct mdqt_pump_ensemble {
    mdqt_ensemble* base = nullptr;
    mdqt::DevBuf<mdqt::PumpStepArgs> dStep[2];           // [J] the leading drift's blocks, the kick launch's blocks
    std::vector<mdqt::PumpStepArgs> step_held[2];        // what they hold
    mdqt::DevBuf<mdqt::PumpTagArgs> dTag;                // [J]
    mdqt::DevBuf<mdqt::PumpKdeArgs> dKde;                // [J]
    unsigned long long launches = 0;                     // the pump kernels' launches (the force launches: base)
    mdqt::LaunchTimer kick_timer;                        // the kick launches' timestamps
};

namespace mdqt {

// mdqt_ensemble.cpp: the ensemble's machinery the pump ensemble reuses
// members: npoints parameter points (mdqt_ensemble_create and the pump ensemble: one) x njobs replicas, point-major;
// sweep: the ensemble owns the points' tables and launches the sweep QT kernels
int ensemble_create(const mdqt_params* points, int npoints, int njobs, mdqt_ensemble** out, const char* what, bool pump,
                    bool sweep = false);
int ens_check(const mdqt_ensemble* e, const char* what, bool pump = false);
int ens_forces(mdqt_ensemble* e);
// the fused step();qstep() (do_step 1) or qstep() (0) launches of every member: `launch` issues one (blocks:
// the host copies of the launch's blocks, member by member; 0 or, after set_error, -1)
using EnsQtLaunch = std::function<int(const SubstepArgs* blocks, int maxn, hipEvent_t e0, hipEvent_t e1, int* inst)>;
int ens_qt_chunks(mdqt_ensemble* e, int n, int do_step, const EnsQtLaunch& launch);
int ens_range_flags(mdqt_ensemble* e, bool drain = true);

// mdqt_ensemble_output.cpp: output() of every member in one device pass
int ens_output(mdqt_ensemble* e);
int ens_epotential(mdqt_ensemble* e, double* Epot);
// the same queued without a synchronisation (the pump ensemble's output, which has one of its own): after it,
// batched member member[q]'s Epotential() is ens_epot_of(job, rows + 64 q)
int ens_epotential_queue(mdqt_ensemble* e, std::vector<int>& member, const double** rows);
double ens_epot_of(const mdqt_ctx* s, const double* row);
// what a pooled output() needs of the options and of every member, checked at the call (the options may be set in
// any order): 0, or -1 after set_error naming the first offending job index; nothing is launched or written
int ens_pool_check(const mdqt_ensemble* e, const char* what);

}  // namespace mdqt
