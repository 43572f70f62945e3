// Internal interface between the host engine (mdqt_ctx.hpp and its sources) and the gfx950 kernels
// (mdqt_kernels.hip).  Plain structs passed BY VALUE as kernel arguments (no __constant__
// globals: several contexts with different parameters may live in one process).
// Beside it, each with its own users: mdqt_math.hpp (device math of the pair forms, canonical sums),
// mdqt_n3b_args.hpp (the Newton-3 block scheme), mdqt_ens_args.hpp (the ensembles' batched launches),
// mdmc_kernels.hpp and mdlc_kernels.hpp (the other two programs), mdqt_error.hpp (set_error, HIPCHK).
#pragma once
#include <hip/hip_runtime.h>
#if defined(__HIP__)
#include <hip/hip_ext.h>
#include <type_traits>
#endif
#include <stdint.h>

namespace mdqt {

constexpr int NS = 12;          // numStates, SpeedUp:153
constexpr int NBINS = 2001;     // SpeedUp:120-123
constexpr int MAXSUB = 32;      // substeps fused into one launch (ratio = 25 at density 2)
constexpr int NSTATIC = 20;     // static off-diagonal entries of M = I - i h H (App. A)
// Gaussian KDE of the velocity distributions (SpeedUp:958-979; the tagging programs' QTT:1072):
// exp(-V2 d^2), V2 = 1 / (2 0.002^2).  exp(x) is exactly +0 for x < -745.14 (below half the
// smallest subnormal), so a term with |d| >= kKdeSkip (V2 d^2 >= 746.9) adds an exact zero and the
// KDE kernels skip it; the assert ties the threshold to the bandwidth.
constexpr double kKdeV2 = 1. / (2. * 0.002 * 0.002);
constexpr double kKdeSkip = 0.0773;
static_assert(kKdeV2 * kKdeSkip * kKdeSkip * (1. - 1e-12) >= 746.0, "KDE skip threshold must lie beyond exp's underflow");

// Static couplings of the non-Hermitian Hamiltonian, as (row, col) of M; order of this
// table is the index used by the kernels (SpeedUp:1206-1215, cs[] at :1163-1180).
constexpr int kStaticRC[NSTATIC][2] = {
    {0, 3}, {0, 5}, {1, 2}, {1, 4}, {2, 1}, {2, 9}, {2, 11}, {3, 0}, {3, 8}, {3, 10},
    {4, 1}, {4, 7}, {5, 0}, {5, 6}, {6, 5}, {7, 4}, {8, 3}, {9, 2}, {10, 3}, {11, 2}};

// Constants of qstep() (SpeedUp:438-717), all precomputed on the host with the reference's
// own operation order so that device and oracle agree bit for bit where the math allows.
struct QTConst {
    double dtQ, gamToE;         // quantumTimestep, gamToEinsteinFreq (:79, :84)
    double h, dtHalf, invh;     // dtQ*gamToE, dtQ*gamToE/2, 1/(dtQ*gamToE)  (:525-567)
    double pv2q;                // plasVelToQuantVel (:85)
    double kRat, r;             // :146-147
    double det, detDP;          // detuning, detuningDP (:70-71)
    double kickS, kickD;        // 1*vKick*Om, vKickDP*(OmDP/r) (:503)
    double vKick, vKickDP;      // jump kicks (:589-610)
    double pD;                  // r/(r+1): D-decay branch probability (:589)
    double dP[4];               // decayMatrix diagonal on P levels 2..5 (:1203)
    double hdP[4];              // imag of hamDecayTerm diagonal on P levels (:1202)
    double hdPh[4];             // h dP[k]: qt_math 2 form of dp (= FastTab::hdp of the P levels)
    double a8, a11;             // OmDP/2*gs[8]/sqrt(r), OmDP/2*gs[11]/sqrt(r) (:508)
    double Mre[NSTATIC], Mim[NSTATIC];   // static off-diagonal M entries
    double thS3, thS4;          // gs[2]^2, gs[4]^2 (S-decay target thresholds)
    double thD[4][2];           // cumulative D-decay thresholds per P level (:612-697)
    double gs[18];
    double kickmax;             // bound on one substep's velocity kick (recoil or optical, model 0;
                                // |w|, |w_c| <= 4): the lane kernel's coupling-phase bound
    int renorm;                 // reNormalizewvFns (:706-712)
    int im01;                   // host: every static M entry of the lane table's slots 0 and 1 is
                                // purely imaginary (Re == +-0: -i h H with real couplings), so the
                                // FAST lane kernel drops their real-part FMAs (k_substeps_lanes_im)
    int model;                  // QT model (QTModel): level scheme, couplings and jump rule
    uint32_t seed, job;         // Philox key
};

// Per-lane tables of the lane-per-state QT kernel (16 lanes per ion, lane k <-> state k).
// Row k of M has its diagonal and up to three off-diagonal entries, in slots A < B < C by
// column; `order` says where the diagonal falls in the ascending-column sum:
//   0: D,A,B   1: A,D,B,C   2: A,D   3: A,B,D
struct LaneTab {
    int colA[16], colB[16], colC[16];
    int order[16], hasB[16], hasC[16];
    int dynB[16], dynC[16];      // slot holds a time-dependent entry: 1 = (8,5)/(9,4) form, 2 = (5,8)/(4,9)
    double cAre[16], cAim[16], cBre[16], cBim[16], cCre[16], cCim[16];   // static M entries
    double dynScale[16];         // a8 or a11 for the dynamic slot of rows 4, 5, 8, 9
    double gA[16], gB[16];       // optical-kick weights of rho_im(w_k, w_colA/colB) (:503)
    double dP[16];               // decayMatrix diagonal (0 off the P levels)
    double hd[16];               // imag of hamDecayTerm diagonal (0 off the P levels)
};

// qt_math 2 (reassociated QT arithmetic, mdqt_qtfast.hip): row k of M = I - i h H as its
// diagonal plus three off-diagonal slots with source states kFastCol[k][t] (unused slots point
// at k itself, or for model 0 at the zero state NS, with a zero coefficient; the time-dependent
// entry of rows 4, 5, 8, 9 sits in slot 2).  Both QT kernels evaluate every row as the same fixed
// FMA chain over these slots, so the thread-per-ion and lane-per-state forms stay bit-identical.
//
// Model 0's lane layout (lane-per-state kernel): the coupling graph (S-P and P-D edges, every P
// level of degree 3) is bipartite and splits into three matchings; states are placed on the 16
// lanes of an ion's row so that the matchings are lane ^ 2, lane + 8 (mod 16) and lane ^ 1 —
// three DPP moves (quad_perm, row_ror:8, quad_perm) instead of an LDS gather:
//   lane : 0  1  2  3  4  5  6  7  8  9  10 11 12 13 14 15
//   state: 2  1  9  4  3  0  8  5  11 -  -  7  10 -  -  6     (- : zero lanes; 9 = y, 10 = z)
// Slot 0 = lane ^ 2, slot 1 = lane + 8, slot 2 = lane ^ 1 (it carries the time-dependent
// couplings 4-9 and 5-8).  The sums over lanes (dp, kick, norm) follow lane order.
//
// QT models (mdqt_params.qt_model): 0 = the SpeedUp Sr+ 12-level laser cooling (default);
// the optical-pumping ("spin tagging") variants, one per reference program family:
//   1 = 408 nm linear, 7 levels   randomFrozenStartTag408Linear.cpp:396, MonteCarloFollowedByQTTagging408Linear.cpp:555
//   2 = 408 nm quad,   7 levels   randomFrozenStartTag408Quad.cpp (qstep :399: 2 couplings)
//   3 = 422 nm linear, 5 levels   randomFrozenStartTag422Linear.cpp:390, MonteCarloFollowedByQTTagging422Linear.cpp:552
// Levels of the pumping models: 0 S-1/2, 1 S+1/2, P levels from 2, then one D level (6 or 4).
// They have no optical-force kick, no time-dependent coupling and no jump kick; the kernels
// are the same template with another sparse H (FastTab) and jump table (jump_target_pump).
constexpr int NMODELS = 4;
constexpr int kModelStates[NMODELS] = {12, 7, 7, 5};
constexpr int kFastColM[NMODELS][NS][3] = {
    {{5, 12, 3}, {4, 12, 2}, {9, 11, 1}, {8, 10, 0}, {1, 7, 9}, {0, 6, 8},
     {12, 5, 12}, {12, 4, 12}, {3, 12, 5}, {2, 12, 4}, {12, 3, 12}, {12, 2, 12}},
    {{2, 4, 0}, {3, 5, 1}, {0, 2, 2}, {1, 3, 3}, {0, 4, 4}, {1, 5, 5},
     {6, 6, 6}, {7, 7, 7}, {8, 8, 8}, {9, 9, 9}, {10, 10, 10}, {11, 11, 11}},
    {{4, 0, 0}, {5, 1, 1}, {2, 2, 2}, {3, 3, 3}, {0, 4, 4}, {1, 5, 5},
     {6, 6, 6}, {7, 7, 7}, {8, 8, 8}, {9, 9, 9}, {10, 10, 10}, {11, 11, 11}},
    {{3, 0, 0}, {2, 1, 1}, {1, 2, 2}, {0, 3, 3}, {4, 4, 4}, {5, 5, 5},
     {6, 6, 6}, {7, 7, 7}, {8, 8, 8}, {9, 9, 9}, {10, 10, 10}, {11, 11, 11}}};
inline constexpr const int (&kFastCol)[NS][3] = kFastColM[0];
// model 0 lane layout (see above): state of lane l / lane of state k, as 4-bit fields (0xF: none)
constexpr uint64_t kStateOfLane0 = 0x6FFA7FFB58034912ull;   // lanes 15..0: 6 F F A 7 F F B 5 8 0 3 4 9 1 2
constexpr uint64_t kLaneOfState0 = 0x8C26BF734015ull;      // states 11..0: 8 C 2 6 B F 7 3 4 0 1 5
__host__ __device__ constexpr int state_of_lane0(int l) { return (int)((kStateOfLane0 >> (4 * l)) & 0xF); }
__host__ __device__ constexpr int lane_of_state0(int k) { return (int)((kLaneOfState0 >> (4 * k)) & 0xF); }
constexpr bool layout0_consistent() {      // slot j of state k's lane reads the lane of kFastColM[0][k][j]
    for (int k = 0; k < NS; ++k) {
        const int l = lane_of_state0(k);
        if (state_of_lane0(l) != k) return false;
        const int part[3] = {l ^ 2, (l + 8) & 15, l ^ 1};
        for (int j = 0; j < 3; ++j) {
            const int ps = state_of_lane0(part[j]);
            if ((ps >= NS ? NS : ps) != kFastColM[0][k][j]) return false;
        }
    }
    return true;
}
static_assert(layout0_consistent(), "model 0 lane layout and kFastColM[0] disagree");
struct FastTab {
    int col[3][16];              // kFastCol, lanes 12..15 point at themselves
    double cre[3][16], cim[3][16];   // static M entries of the slots (0 for unused / dynamic)
    double dms[16], dmc[16];     // slot 2 += {dms sin(phi), dmc cos(phi)} (rows 4, 5, 8, 9)
    double mre[16];              // Re M_kk = 1 + h Im(hamDecayTerm_kk)
    double mi0[16], mi1[16];     // Im M_kk = mi0 + mi1 u, u = velQuant + expDetuning (:506-510)
    double hdp[16];              // h decayMatrix_kk (P levels), 0 elsewhere: dp = sum hdp |y|^2
    double kw[3][16];            // optical-kick weight of Im(y_k conj(y_slot)), sign and scale folded (:503)
    double cphi;                 // 2 (1 + kRat) gamToE: phi = u cphi tPart (:508)
    double dt2;                  // (dtQ/2)^2 of step_R's first substep (:372-378)
};

struct SubstepArgs {
    double* R;          // this rank's slab of the gathered positions, [3][S]
    double* V;          // [3][S]
    double* F;          // [3][S]
    const double* Fpart;// if nseg > 1: force partials [nseg][3][S] summed here (in segment
    int nseg;           //   order) into F before the first substep, and F is written back
    double* psi;        // [24][S]: component-major (re0, im0, re1, ... im11)
    double* tPart;      // [S]
    int n;              // ions in this slab
    int S;              // slab stride (doubles)
    uint64_t gid0;      // global id of local ion 0
    uint64_t q0;        // qstep index of the first substep
    int nsub, do_step, do_qt;
    const double* U;    // rng_mode 0 (drand48 reference order): uniforms [5][S] of this substep
                        // (nsub == 1), from k_d48_resolve; nullptr = Philox stream
    int* oor;           // set to 1 if a final position leaves [-L/8, 9L/8] (see ForceArgs::oor)
    double L;
    double t[MAXSUB];       // global time at each substep (t before qstep advances it)
    double expDet[MAXSUB];  // expDetuning(t) (:447)
    uint32_t movmask;       // bit s: t[s] > 0 (step_R's moving branch, :360); set by the host
    int expdet_zero;        // every expDet[s] == 0 (fracOfSig = 0, the default)
    // overlapped / fused MD step (lane kernel, world 1): the force work runs concurrently (another
    // stream, or the first workgroups of k_md_step) and counts its finished tile pairs per tile in
    // arrive[ntiles]; this launch does its prologue, then waits until arrive[tile of its ions] >=
    // arrive_target before it reads the force partials (write-through stores there, L1-bypassing
    // loads here: mdqt_pairs.hpp n3_tile)
    const unsigned long long* arrive;
    unsigned long long arrive_target;
    int* spin_err;          // set if the wait gave up (bounded spin)
    int arrive_sleep;       // s_sleep 1 (64 cycles) units between polls (2)
    QTConst qc;
};

struct ForceArgs {
    const double* Rall; // gathered positions [world][3][S]
    double* Fpart;      // [nseg][3][S]: partial sums of the owned rows per j-segment
    int N, S;           // ions, slab stride
    int row_lo, nrows;  // owned global rows [row_lo, row_lo + nrows)
    int nseg, seglen;   // j segmentation (a function of N only)
    double L, lDeb, Rcut;
    double invlDeb;     // 1./lDeb (the reference recomputes it per pair; same IEEE value)
    double micT;        // smallest d with fl(d/L) >= 0.5: round(dx/L) = [dx >= micT] - [dx <= -micT]
    double micGuard;    // |dx| below this is inside the threshold rule's validity (|dx/L| < 1.5)
    int variant;        // 0 = exact (the reference's operations), 1 = fast (rsqrt/reciprocal form)
    int guard;          // positions may have left [-L/8, 9L/8] (set_state input or a device
                        // report): range-check every pair, far separations take the division form
};

// Newton-3 tile-pair scheme (world_size 1): one workgroup of 4 waves per 64x64 tile pair
// (I <= J); partials go to slot J (rows of I) and slot I (rows of J), the diagonal tile's two
// sides to slot I.  F = canonical sum of the ntiles slots (seg_sum), like the row segments.
struct N3Args {
    const double* R;    // [3][S] (world_size 1)
    double* P;          // [ntiles][3][S]
    const int2* pairs;  // (I, J) of every workgroup; I's bits 28-31: a part of the tile pair's rotation
                        // steps (mdqt_pairs.hpp n3_tile; later parts write the extra slots from ntiles on)
    int N, S, ntiles, npairs;
    double L, lDeb, Rcut, invlDeb, micT, micGuard;
    int guard;          // as ForceArgs::guard (exact variant only; the fast one needs no guard)
    double rc2;         // variant 2: smallest double x with sqrt(x) >= Rcut (pair kept iff r2 < rc2)
    unsigned long long* arrive;   // [ntiles] arrival counts (overlapped / fused MD step): a finished
                                  // tile pair (I, J) adds 1 to arrive[I] and arrive[J] after its
                                  // write-through slot stores — T per tile per launch; nullptr = off
};

// pumping-model QT tables for another engine (mdqt_engine.cpp; used by the MC + MD tagging programs)
void build_pump_program(int model, double detuning, double Om, double dtQ, double gamToE, double pv2q,
                        double decayRatio, uint32_t seed, uint32_t job, QTConst& q, FastTab& f);
// recordTaggedParticleMoments' velocity distribution of the tagged ions (QT tagging programs):
// out[c][j] = sum over tagged i (ascending) of exp(-V2 (vel_j - V[c][i])^2), vel_j = (j - 2000) 0.0025
// (defined in mdmc_kernels.hip; declared here because the MDQT pump programs call it too, mdqt_pump.cpp)
constexpr int TKDE_BINS = 4001;
// bins vel_j = (j + bin0) 0.0025: bin0 = -2000 (the programs' init(), e.g. randomFrozenStartTag408Linear.cpp:306),
// 0 after their readConditions (:723 sets vel[i] = i 0.0025)
hipError_t launch_tagged_kde(const double* V, const int* tags, int N, int S, double* part, double* out, hipStream_t s,
                             int bin0 = -2000);
// one half of the pumping programs' leapfrog MD step (randomFrozenStartTag408Linear.cpp step(), :317-394):
// if kick != 0, V += kick F first (step_V); then step_R: R += DT V (moving) or R += DT V + DT2 F
// (t == 0), and the reinsertion into [0, L]
hipError_t launch_leapfrog_half(double* R, double* V, const double* F, int n, int S, double L, double DT, double DT2,
                                int moving, double kick, hipStream_t s);

// drand48 in the reference's order (SpeedUp:486, :575-687: ions in index order, 1 draw per
// ion, 4-5 for a quantum jump): one workgroup assigns every ion its uniforms from the single
// stream, by LCG jump-ahead from the stream state, restarting after each (rare) jump.
struct D48Args {
    const double* psi;         // [24][S]
    int n, S;
    unsigned long long* state; // device: drand48 X before this substep's first draw; advanced
    const unsigned long long* jA;   // [48] multiplier of 2^b steps
    const unsigned long long* jC;   // [48] increment of 2^b steps
    double* U;                 // out: [5][S]
    int fast;                  // qt_math of the substep kernel (0, 1, 2: dp must be bit-identical)
    QTConst qc;
};
hipError_t launch_d48_resolve(const D48Args& a, hipStream_t s);

// ---- launchers (mdqt_kernels.hip; the force kernels': mdqt_forces.hip; the block scheme's: mdqt_n3b_args.hpp) ----
hipError_t launch_forces(const ForceArgs& a, hipStream_t s);
hipError_t launch_forces_n3(const N3Args& a, int variant, hipStream_t s, hipEvent_t ev0 = nullptr,
                            hipEvent_t ev1 = nullptr);
// Epotential on the Newton-3 tiles (world 1): pair potentials into slot p of a.P, plane stride S
// ([ntiles][S]: one component, a third of the force slots' memory)
hipError_t launch_potential_n3(const N3Args& a, int variant, hipStream_t s);
// partial p of component c at Fpart + p * plane + c * S (plane 0: 3 S, the force layout)
hipError_t launch_reduce_segments(const double* Fpart, double* F, int nseg, int nrows, int S, int ncomp,
                                  hipStream_t s, size_t plane = 0);
hipError_t launch_potential_rows(const ForceArgs& a, hipStream_t s);   // Fpart[seg][0][i]
// mode: 0 = auto (lane-per-state below kLaneKernelMaxIons ions, thread-per-ion above),
//       1 = thread-per-ion, 2 = lane-per-state.  Both are bit-identical.
constexpr int kLaneKernelMaxIons = 98304;
// fast: qt_math 1 (FMA contraction, refined rsq) instead of the reference's exact operations
#if defined(__HIP__)
// Launch with the kernel's own dispatch timestamps written to (ev0, ev1) when timing is on
// (hipExtLaunchKernelGGL): the measured interval is the kernel itself, without the event
// packets' queue time that a pair of hipEventRecord calls around the launch adds.
template <typename... Args, typename F = void (*)(Args...)>
inline void launch_timed(F kernel, dim3 grid, dim3 block, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1,
                         Args... args) {
    if (ev0) hipExtLaunchKernelGGL(kernel, grid, block, 0, s, ev0, ev1, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}
// The (variant, guard) ladder of the force kernels' launchers: calls f(V, G) with the force variant
// (0 .. NVAR - 1; one out of range goes to 0, as the ladders did) and the guard flag as
// std::integral_constant values, so that f names its kernel as k<decltype(V)::value, decltype(G)::value>
template <int NVAR, typename F>
inline void by_variant_guard(int variant, bool guard, F&& f) {
    auto g = [&](auto v) {
        if (guard) f(v, std::true_type{});
        else f(v, std::false_type{});
    };
    if constexpr (NVAR > 2) {
        if (variant == 2) return g(std::integral_constant<int, 2>{});
    }
    if (variant == 1) g(std::integral_constant<int, 1>{});
    else g(std::integral_constant<int, 0>{});
}
#endif

// The substep kernel instance a launch ran (mdqt_get_const "qt_kernel"; the launchers report it
// through `instance`): tests check which instance a configuration's production launch takes.
enum QTKernel : int {
    QTK_NONE = 0,
    QTK_LANES_IM_EDZ = 1,      // k_substeps_lanes_im<true, true, true>: model 0 FAST + IM01 + EDZ, no
                               // renormalisation (the C2 production launch)
    QTK_LANES_IM = 2,          // k_substeps_lanes_im<true, false>
    QTK_LANES_R_FAST = 3,      // k_substeps_lanes_r<true, true>
    QTK_LANES_R = 4,           // k_substeps_lanes_r<true, false>
    QTK_LANES_R_PUMP_FAST = 5, // k_substeps_lanes_r<false, true>
    QTK_LANES_R_PUMP = 6,      // k_substeps_lanes_r<false, false>
    QTK_LANES_IM_EDZ_RN = 7,   // k_substeps_lanes_im<true, true, false>: the same with reNormalizewvFns on
    QTK_THREAD_R = 10,         // k_substeps_r<model>: 10 + model
    QTK_MD_STEP = 20,          // k_md_step (one launch per MD step)
    QTK_EXACT_LANES = 30,      // k_substeps_lanes<fast>: 30 + qt_math
    QTK_EXACT_THREAD = 40,     // k_substeps<fast>: 40 + qt_math
};
// ev0/ev1 (optional): the kernel's own start/stop timestamps (hipExtLaunchKernelGGL)
hipError_t launch_substeps(const SubstepArgs& a, const LaneTab* tab, int mode, int fast, hipStream_t s,
                           hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int* instance = nullptr);
// qt_math 2: the reassociated kernels of mdqt_qtfast.hip (same modes as launch_substeps)
hipError_t launch_substeps_r(const SubstepArgs& a, const FastTab* tab, int mode, hipStream_t s,
                             hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                             int* instance = nullptr);   // tab[0] by state, tab[1] by lane
// one MD step in one launch: Newton-3 tile pairs + the FAST lane QT kernel (mdqt_qtfast.hip
// k_md_step); f.arrive / a.arrive = the per-tile arrival counters, a.arrive_target their value
// after this launch's tile pairs
hipError_t launch_md_step(const N3Args& f, const SubstepArgs& a, const FastTab* tab, int variant, hipStream_t s,
                          hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// measureSpinUps (randomFrozenStartTag408Linear.cpp:600, :422Linear) / tagParticles
// (MonteCarloFollowedByQTTagging408Linear.cpp:1022): tag[i] = 1 with probability of spin up
hipError_t launch_tag_spin_up(const double* psi, int n, int S, uint64_t gid0, uint64_t q, const QTConst& qc,
                              int* tags, hipStream_t s);
// deterministic sums: out[0] = sum vx; needs scratch >= 1024 doubles
// avg (optional, world 1): also avg[0] = sum / N on the device
hipError_t launch_sum_vx(const double* V, int n, double* out, hipStream_t s, double* avg = nullptr, int N = 0);
hipError_t launch_output_pack(const double* V, const double* psi, int n, int S, int model, double* out,
                              hipStream_t s);
// out[0..2] = sum 0.5 (vx-avg)^2, 0.5 vy^2, 0.5 vz^2 ; out[3] = sum of rows[0..nrows) of
// the potential partials reduced over segments (caller passes the reduced row buffer)
hipError_t launch_energy_sums(const double* V, int n, int S, const double* vxAvg,
                              const double* urow, double* out, hipStream_t s);
// KDE partials: P[ichunk][3][2001]; then reduce into Pout[3][2001] (unnormalised)
hipError_t launch_kde(const double* V, int n, int S, const double* vxAvg, double* Ppart,
                      int nchunk, double* Pout, hipStream_t s);

}  // namespace mdqt
