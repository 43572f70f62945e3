// The host engine's private header: the context of one simulation (struct mdqt_ctx) and the host functions of
// one context that cross a file boundary (namespace mdqt, as the kernel launchers of mdqt_internal.hpp and
// mdqt_n3b_args.hpp).  The ensembles over several contexts: mdqt_ensemble.hpp; the error plumbing every host
// source shares: mdqt_error.hpp.
// Not installed: the C ABI of include/mdqt.h sees the struct as opaque.  The host engine by file: DESIGN.md §1.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mdqt.h"
#include "mdqt_batch.hpp"
#include "mdqt_devbuf.hpp"
#include "mdqt_error.hpp"
#include "mdqt_internal.hpp"
#include "mdqt_main_loops.hpp"
#include "mdqt_n3b_args.hpp"
#include "mdqt_writer.hpp"

// rccl.h is included only where a collective is issued (mdqt_step.cpp, mdqt_comm.cpp); the context
// just holds the handle
struct ncclComm;
typedef struct ncclComm* ncclComm_t;

#define NCCLCHK(expr)                                                                   \
    do {                                                                                \
        ncclResult_t r_ = (expr);                                                       \
        if (r_ != ncclSuccess) return mdqt::set_error("%s failed: %s", #expr, ncclGetErrorString(r_)); \
    } while (0)

struct mdqt_ctx {
    mdqt_params p;
    // derived constants (SpeedUp:79-85, :146-149, :295-297)
    double gamToE, dtQ, pv2q, r, kRat, vKick, vKickDP, lDeb, L;
    int ratio;
    double gs[18];
    mdqt::QTConst qc;
    double vel[mdqt::NBINS];
    // sizes
    int N = 0, S = 0, lo = 0, hi = 0, nloc = 0;
    int capS = 0, nseg = 1, seglen = 1;
    // device
    int dev = 0;
    hipStream_t own = nullptr, stream = nullptr;
    mdqt::DevBuf<double> dR, dV, dF, dFpart, dPsi, dTp, dScr, dKde, dUrow;
    mdqt::DevBuf<double> dUpart;   // potential-row partials of its own (small systems, world 1)
    int n3_potential = 1;          // option "potential_n3": 1 = Newton-3 tiles where the forces use them
    int n3b_pairs = 1;             // option "force_n3b_pairs": the paired-wave block kernel (k_pairs_n3b_pw); A/B round 6
                                   // (r06e): N = 1M force call -4.3 %, C5 -2.3 %, C3 -2.3 %
    int pot_plan = 1;              // option "potential_plan": 1 = Epotential on the blocks takes the force call's
                                   // plan (skips, sub-tile groups, error-bounded forms); 0 = every pair to L/2 exactly
    mdqt::DevBuf<double> dPack;    // output()'s per-ion columns [4][S] (world 1)
    int kdeChunks = 0;
    mdqt::LaneTab tab;                   // lane-per-state QT kernel tables (host copy)
    mdqt::DevBuf<mdqt::LaneTab> dTab;    // device copy (uploaded once at create)
    mdqt::FastTab ftab;                  // qt_math 2 row tables by state (host copy)
    mdqt::FastTab ftabL;                 // the same by lane of the lane-per-state kernel (model 0: kStateOfLane0)
    mdqt::DevBuf<mdqt::FastTab> dFTab;   // device copies [2]: by state, by lane
    int substep_mode = 0;          // 0 auto, 1 thread-per-ion, 2 lane-per-state
    int force_variant = 1;         // 0 exact reference operations, 1 fast reciprocal form
    int qt_math = 2;               // 0 exact reference operations, 1 FMA-contracted, 2 reassociated (option "qt_math")
    bool f_pending = false;        // dFpart holds unreduced force partials (pend_nseg > 1)
    int pend_nseg = 1;             // partial count of the pending forces (segments or slots)
    int scheme_opt = 0;            // force scheme: 0 auto, 1 rows (owner computes), 2 Newton-3 tiles, 3 Newton-3 blocks
    bool use_n3 = false;
    bool use_n3b = false;          // Newton-3 block pairs (k_pairs_n3b): large N, one GPU or sharded
    mdqt::N3BArgs n3b;                   // its configuration (pointers and pair constants filled per call)
    mdqt::DevBuf<double> dSlots;   // its slots [nd + R][3][Npad]
    mdqt::DevBuf<double> dFr;      // sharded n3b: this rank's dense partial forces [world][3][S]
    // spatial order of the n3b scheme (mdqt_sort.hip; option "force_sort", default on)
    int sort_mode = 1;             // 0 off, 1 sorted + tile-pair skipping, 2 sorted, nothing skipped (tests)
    int ax1_mode = 1;              // option "force_ax1": the one-axis per-pair image instance (1, auto) or not (0)
    // error-bounded force tail (option "force_tail_exp" k: eps = 10^-k, 0 = off): tile pairs whose
    // boxes are >= r_t apart are skipped, r_t the smallest radius with (N - 1) g(r_t) <= eps,
    // g(r) = (1/r + 1/lDeb) e^(-r/lDeb) / r the pair force magnitude (SpeedUp:224) — so no ion's
    // force changes by more than eps; a no-op where r_t >= L/2 (every BASELINE size but N ~ 1e6)
    int tail_exp = 12;
    // how r_t is bounded (option "force_tail_mode"): 0 a priori, (N - 1) g(r_t) <= eps; 1 (default,
    // every world size) measured and enforced: r_t from the density model's sum over tile pairs
    // (tail_radius_sum), every force call sums, per tile, n_J g(box distance) over its skipped tile
    // pairs on the device (k_pairs_n3b; all-reduced over the ranks), and every tile whose sum
    // exceeds eps gets the exact sum over those tile pairs added to its rows (k_tail_fix) — so every
    // ion meets eps whatever the configuration; the host widens r_t when that happened (tail_check)
    int tail_mode = 1;
    mdqt::DevBuf<double> dTail;    // [4T]: the per-sub-tile sums of the current call
    mdqt::DevBuf<unsigned long long> dTailSt;   // [8]: k_tail_max's running maxima and counters
    mdqt::DevBuf<int> dTailList;   // [T]: this call's tiles over eps (this rank's)
    double tail_scale = 1.;        // r_t from 2 tail_scale B(r) <= eps: raised when a call exceeded eps
    unsigned long long tail_seen = 0;   // tiles over eps the host has reacted to
    int tail_warned = 0;                // stderr lines printed by tail_check
    bool tail_pending = false;     // in-process group: the sums wait for the group's (local_reduce)
    mdqt::N3BArgs tail_args;             // ... with the call's arguments
    mutable double tail_key[5] = {0, 0, 0, 0, 0}, tail_val[2] = {0, 0};   // tail_radius_sum memo (N, L, lDeb, k, scale)
    // the far pair form (option "force_far_exp" k: eps = 10^-k, 0 = off): tile pairs whose boxes are
    // >= r_far apart evaluate their pairs within kFarRelErr (rsq1, degree-6 2^f), r_far the smallest
    // radius with (N - 1) g(r_far) kFarRelErr <= eps — so no ion's force moves by more than eps
    int far_exp = 13;
    // the mid pair form (round 4; option "force_mid_exp" k, 0 = off): sub-tile groups >= r_mid apart
    // take rsq1 and the table's 2^t with a degree-4 series, r_mid the smallest radius with (N - 1)
    // g(r_mid) ((r_mid/lDeb + 3)(kRsq1RelErr + 2^-52) + kTab4RelErr) <= 10^-k
    int mid_exp = 13;
    // the very-far pair form (option "force_vfar_exp" k, 0 = off): tile pairs >= r_vfar apart use
    // the raw rsq and a degree-5 2^f; r_vfar the smallest radius with
    // (N - 1) g(r) ((r/lDeb + 3) kRsqRawErr + kExp5RelErr) <= 10^-k
    int vfar_exp = 13;
    // the ultra-far pair form (option "force_ufar_exp" k, 0 = off): raw rsq and v_exp_f32, r_ufar the
    // smallest radius with (N - 1) g(r) ((r/lDeb) (kRsqRawErr + 2^-24) + 3 kRsqRawErr + kExp2fRelErr) <= 10^-k
    int ufar_exp = 13;
    // how the tiers' radii are bounded (option "force_form_mode", round 6): 0 a priori, (N - 1) g(r)
    // err(r) <= 10^-k per tier (far_radius_l); 1 (where the tail is measured: force_tail_mode 1,
    // spatial order, the fast variant) measured and enforced — every sub-block the plan evaluates in an
    // error-bounded form adds n_b g(gap) err_form(gap) to its sub-tiles' sums (k_n3b_plan), a tile whose
    // sum exceeds the call's eps (the tail's where r_t < L/2, + 10^-k per active tier: error_eps) is
    // recomputed exactly (k_tail_fix), and the radii come from the density model of those sums
    // (tier_radius) — so every ion meets that eps whatever the configuration; 2 as 1, and where the tail
    // is exact (r_t = L/2) the tiers share its unused 10^-tail_exp (tier_eps): the same total per ion.  2 is the
    // default: where the tail is exact (C3 / C5) the per-ion bound is then 1.5e-12, not 1's 5e-13
    int form_mode = 2;
    mutable double form_key[6][6] = {}, form_val[6][2] = {};   // tier_radius memo by level (N, L, lDeb, k, tail_exp, scale)
    mdqt::DevBuf<uint32_t> dKeys;  // [2][N] Hilbert keys, sorted keys
    mdqt::DevBuf<int> dIon;        // [2][N] identity, sorted index -> ion
    mdqt::DevBuf<char> dSortTmp;   // the radix sort's scratch (its capacity: the bytes)
    mdqt::DevBuf<double> dRs;      // [3][Npad] positions in sorted order
    mdqt::DevBuf<double> dBoxes;   // [12][T] tile boxes, raw coordinate bounds
    mdqt::DevBuf<double> dSubBoxes;   // [6][4T] the 16-ion sub-tiles' boxes (the block kernel's sub-tile groups)
    mdqt::DevBuf<uint2> dPlan;     // [(Phi - Plo) nd][kN3BBlock^2] the block kernel's tile-pair words (k_n3b_plan)
    int tmask_mode = 1;            // option force_reduce_mask: k_n3b_reduce reads only the j-slots written
    int balance_opt = 1;           // option force_balance: sharded block ranges by census weight (1) or count (0)
    bool balanced = false;         // the block ranges of this N have been weighted (n3b_balance)
    double balance_ratio = NAN;    // max / mean of the ranks' evaluated lane-steps (the weighted ranges)
    double balance_ratio_eq = NAN; // the same for the equal-count ranges
    int capSortN = 0;
    // overlapped MD step (option "overlap", OFF by default — measured slower): the
    // QT launch of step k runs on its own stream beside step k's force launch and waits on the
    // device for the force workgroups' arrivals (see md_steps_overlapped)
    int overlap_opt = 0;
    hipStream_t qs = nullptr;              // the QT stream
    hipEvent_t evQ = nullptr, evS = nullptr;
    mdqt::DevBuf<unsigned long long> dArrive;   // [ntiles] finished tile pairs per tile, monotonic
    unsigned long long arriveEpoch = 0;    // each counter's value after the last launch (T per launch)
    // one MD step in one launch (option "fused_step", OFF by default — measured slower, DESIGN.md
    // §8): k_md_step, see md_step_fused
    int fused_opt = 0;
    int last_fused = 0;                    // the last MD step ran as one k_md_step launch
    int last_qt_kernel = 0;                // QT kernel instance of the last substep launch (QTKernel codes)
    int last_qt_nseg = 0;                  // force partials that launch summed in its prologue
    int* dSpinErr = nullptr;               // = dFlags + 1 (a view: host-mapped, see hFlags)
    unsigned long long* force_arrive = nullptr;   // a view of dArrive, set around a force launch of an overlapped step
    hipStream_t sub_stream = nullptr;             // set around the QT launch of an overlapped step
    unsigned long long sub_target = 0;
    // the optical-pumping programs' main() (mdqt_run_pump)
    std::vector<int> spinUp;       // SpinUpList (randomFrozenStartTag408Linear.cpp:105)
    int nSpinUp = 0;
    mdqt::DevBuf<int> dSpinUp;     // device copy for the tagged distribution
    mdqt::DevBuf<double> dTkde;    // tagged KDE partials + result
    int pumpBin0 = -2000;          // velocity bins (j + pumpBin0) 0.0025: init() :306 / readConditions :723
    std::vector<double> vaHold;    // Vholder of Zfunc (:938-961)
    bool rs_pending = false;       // in-process group: F = sum of the ranks' dFr chunks, not formed yet
    mdqt::DevBuf<const double*> dPeerParts;   // device array of the group's dFr pointers
    int nslots = 0, npairs = 0;
    mdqt::DevBuf<int2> dPairs;     // (I, J) tile pair of every wave of the Newton-3 kernel; after the
                                   // npairs entries, the split table (nsplit > 0: ensure_aux)
    int nsplit = 0;                // tile pairs the split table runs in parts (halves / quarters)
    int nsplit_wg = 0;             // workgroups of the split table
    int split_opt = 1;             // option force_tile_split: 0 off, 1 halves, 2 quarters (+ diagonal halves)
    int split_cus = 0;             // option force_split_cus: the CU count the split table is cut for (0: the device's)
    // rng_mode 0: the reference's drand48 stream, consumed in ion order on the device
    mdqt::DevBuf<unsigned long long> dX48;   // [1] stream state + [48] jA + [48] jC
    // the words the substep kernels raise, in host-pinned, device-mapped memory of this context: the
    // kernels store to them in the failure case only, the host reads them without a stream operation
    // ([0]: a position left [-L/8, 9L/8]; [1]: an overlapped / fused QT launch gave up its arrival wait)
    mdqt::PinBuf<volatile int> hFlags;
    int* dFlags = nullptr;         // the device address of hFlags (a view)
    bool guard = false;            // host view: range-check every pair (see ForceArgs::guard)
    mdqt::DevBuf<double> dU;              // [5][S] uniforms of the current substep
    ncclComm_t comm = nullptr;     // RCCL communicator over the world_size ranks (sharded runs)
    mdqt::DevBuf<double> dComm;    // device staging for small all-reduces
    std::vector<mdqt_ctx*> local;  // in-process group (tests on one GPU): all-gather by D2D copies
    // host-side state
    double t = 0.;
    uint64_t qidx = 0;
    int c0 = 0;
    unsigned counter = 0;
    double Epot = 0., Epot0 = 0.;
    uint64_t x48 = 0;
    std::vector<double> Vholder;   // [13][3][N] VZERO_* files (SpeedUp:752-763, :898-913)
    char saveDirectory[1024];
    std::unique_ptr<mdqt::FileWriter> writer;   // background formatting/writing of the output files
    mdqt::FileWriter* shared_writer = nullptr;  // a member of an ensemble writes through the ensemble's pool (16
                                          // threads in all, not 4 per job); owned by the ensemble
    int init_threads = 0;          // init() sampling threads (option "init_threads"; 0 auto, 1 sequential)
    // timing
    // per-launch HIP events of the hot kernels (kind 0 = force, 1 = substeps), recorded on
    // the launch stream while timing is on; summed by mdqt_kernel_time_totals
    bool timing = false;
    unsigned tkinds = 3;                        // bit 0: force launches, bit 1: fused-substep launches
    unsigned tperiod = 1, tcount[2] = {0, 0};   // bracket launches k = toffset mod tperiod of each kind
    unsigned toffset = 0;                        // tperiod / 2 unless mdqt_enable_timing_at
                                                // (mid-period: not the first launch after a sync)
    mdqt::LaunchTimer timers[4];                // 2: the Newton-3 block kernel's own timestamps (a timed force call)
                                                // 3: the block kernel of the potential calls (Epotential on the blocks)
    // force-call breakdown (timing kind bit 3): per timed block-scheme force call the
    // events between its stages on the context stream — the preceding position all-gather (ag), then
    // m[0] start | sort + boxes | m[1] | plan | m[2] | block kernel | m[3] | slot reduction | m[4] |
    // tail pass (all-reduce, list, exact fix) | m[5] | reduce-scatter | m[6]
    struct BdCall { hipEvent_t ag0 = nullptr, ag1 = nullptr; hipEvent_t m[7] = {}; };
    std::vector<BdCall> bdcalls;
    std::vector<hipEvent_t> bdfree;
    hipEvent_t bd_ag[2] = {nullptr, nullptr};   // the all-gather just before the next timed force call
};

namespace mdqt {

constexpr double TIMESTEP = 0.002;   // SpeedUp:80
constexpr int NINTERVALV = 13;       // numberOfIntervalV, SpeedUp:105
inline double u64_as_double(unsigned long long u) { double d; memcpy(&d, &u, sizeof d); return d; }

// is this launch of timing kind k (0 = force, 1 = substeps) one of the timed ones?  Advances the kind's count.
inline bool launch_timed(mdqt_ctx* s, int k) {
    return s->timing && (s->tkinds & (1u << k)) && (s->tcount[k]++ % s->tperiod == s->toffset);
}

// mdqt_engine.cpp
void n3b_set_range(N3BArgs& b, int lo, int hi);
void choose_segments(mdqt_ctx* s);
int split_slots(const mdqt_ctx* s);
int ensure_aux(mdqt_ctx* s);
int resize(mdqt_ctx* s, int N);
int upload(mdqt_ctx* s, const double* R, const double* V, size_t ld, const double* psi, const double* tPart);

// mdqt_force_plan.cpp
int tail_reset(mdqt_ctx* s, bool keep_scale = false);
double tail_radius_sum(const mdqt_ctx* s, double* bound);
bool tail_measured(const mdqt_ctx* s);
double skip_radius(const mdqt_ctx* s, double* bound);
bool form_measured(const mdqt_ctx* s);
double tier_radius(const mdqt_ctx* s, int k, int level, double* bound);
void tier_radii(const mdqt_ctx* s, N3BArgs& a);
double error_eps(const mdqt_ctx* s, const N3BArgs& a);
int tail_check(mdqt_ctx* s);
int tail_enforce(mdqt_ctx* s, const N3BArgs& a, double* out);
void fill_pair_consts(ForceArgs& a, double L, double lDeb, int variant);
ForceArgs force_args(mdqt_ctx* s, double* out);
int n3b_args(mdqt_ctx* s, N3BArgs& a);
int n3b_balance(mdqt_ctx* s);
int settle_forces(mdqt_ctx* s);

// mdqt_step.cpp
int range_flag_error(int job);
int check_range_flag(mdqt_ctx* s);
int n3_force_args(mdqt_ctx* s, N3Args& a, bool plain_table = false);
void n3_forces_pending(mdqt_ctx* s, const N3Args& a);
double substep_args(const mdqt_ctx* s, SubstepArgs& a, int m, int do_step, int do_qt, int advance_t);
int run_substeps(mdqt_ctx* s, int n, int do_step, int do_qt_flag, int advance_t);
int arrive_setup(mdqt_ctx* s);
bool fused_applies(mdqt_ctx* s);
int md_step_fused(mdqt_ctx* s);

// mdqt_observables.cpp
bool observables_w1_applies(const mdqt_ctx* s);
int observables_w1(mdqt_ctx* s, double out7[7], double* Pvel, double* pops, double* vx);
bool potential_on_tiles(const mdqt_ctx* s);
int potential_n3_block(mdqt_ctx* s, N3Args& a);
void observables_from_rows(mdqt_ctx* s, const double* h, const double* col, double out7[7], double* Pvel, double* pops,
                           double* vx);

// mdqt_io.cpp
FILE* open_in(const mdqt_ctx* s, const char* name, const char* mode);
void speedup_run_name(const mdqt_params* p, char* name, size_t cap);
int finish_directories(mdqt_ctx* s, const char* name);
int flush_files(mdqt_ctx* s);
int output_async(mdqt_ctx* s);
int output_files(mdqt_ctx* s, const double* o, std::shared_ptr<std::vector<double>> P,
                 std::shared_ptr<std::vector<double>> pops, std::shared_ptr<std::vector<double>> V);
int write_conditions_async(mdqt_ctx* s, int c0);
int read_ions_conditions(mdqt_ctx* s, int c0, std::vector<double>& R, std::vector<double>& V);
// the SpeedUp time loop's schedule (mdqt_main_loops.hpp) of a context, or of an ensemble's member 0
inline SpeedUpSchedule speedup_schedule(const mdqt_ctx* s) {
    return {s->dtQ, s->p.tmax + 0.0009, s->p.sampleFreq, s->ratio, MAXSUB};
}

// mdqt_pump.cpp: the pieces of the optical-pumping programs' main() the pump ensemble shares
int pump_setup_directories(mdqt_ctx* s);
int pump_md_step(mdqt_ctx* s);
int pump_spin_ups_file(mdqt_ctx* s);
int pump_output_buffers(mdqt_ctx* s);
int pump_output_host(mdqt_ctx* s, const std::vector<double>& V, std::vector<double>& P,
                     const std::function<int()>& tagged, FileWriter* pool, const double* epot = nullptr);
int pump_vaf_host(mdqt_ctx* s, const std::vector<double>& V, int c1V);
int pump_write_conditions(mdqt_ctx* s, int c0);
int pump_read_conditions(mdqt_ctx* s, int c0);
PumpSchedule pump_schedule(const mdqt_ctx* s);   // the pump time loop's, of a context or of an ensemble's member 0
inline bool tagged(const mdqt_ctx* s) { return !s->spinUp.empty(); }   // measureSpinUps() has run (pump programs)

// mdqt_options.cpp (timing events)
int mark(mdqt_ctx* s, int k);
inline int take_events(mdqt_ctx* s, int k, hipEvent_t* e0, hipEvent_t* e1) { return s->timers[k].take(e0, e1); }
hipEvent_t bd_event(mdqt_ctx* s);
bool force_timed_next(const mdqt_ctx* s);

// mdqt_comm.cpp
int local_reduce(mdqt_ctx* s);
void comm_destroy(mdqt_ctx* s);

}  // namespace mdqt
