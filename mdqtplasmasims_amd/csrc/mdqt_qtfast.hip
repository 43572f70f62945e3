// qt_math 2: the fused step()+qstep() substeps (SpeedUp:356-430, :438-717) with reassociated
// arithmetic, for throughput.  Same algorithm as mdqt_kernels.hip's k_substeps/_lanes, but
// every quantity is evaluated in the form that needs the fewest dependent instructions:
//
//   * row k of M = I - i h H is ONE fixed FMA chain: diagonal, then three off-diagonal slots
//     (FastTab; zero coefficients where a row has fewer entries), instead of the dense
//     product's ascending-column order;
//   * the RK stages work on d = s - y with s = M y / sqrt(1 - dp(y)) (k = d / h): y1 = w + d1/2,
//     y2 = w + d2/2, y3 = w + d3, w' = w + (d1 + 3 d2 + 3 d3 + d4)/8 — the reference's
//     k1 + 3k2 + 3k3 + k4 propagator (:525-567) without the 1/h and h factors;
//   * dp, the optical kick and the renormalisation norm are fixed-shape trees (the lane
//     kernel's DPP tree order), constants folded on the host (kick scale, h dP, 2(1+kRat)gamToE);
//   * step(): one coordinate per lane (lanes 0..11 and 14..15 x, 12 y, 13 z), exact operations.
//
// Results differ from the exact mode (qt_math 0) by rounding only: tests/test_gpu_qt_accuracy.py holds
// every instance, per ion, to the rounding count of tests/qt_truth.py (K ~ 14 roundings of |psi| per
// substep, plus the coupling phase's own conditioning) against an extended-precision truth; measured
// err / bound <= 0.11 (docs/QT_KERNEL.md, "The QT kernels' per-ion gate").  The thread-per-ion and
// lane-per-state kernels below perform the same operations in the same order: bit-identical.
#include "mdqt_qtfast.hpp"
#include "mdqt_pump_device.hpp"   // the body k_tag_spin_up shares with the pump ensemble's batched kernel

namespace mdqt {

// ------------------------------------------------------------------------------------------
// thread per ion
// ------------------------------------------------------------------------------------------
// the P-level sum dp and the 16-lane trees in the lane kernel's order: model 0 places its states
// on lanes by kStateOfLane0 (see mdqt_internal.hpp), the other models on lane = state
template <int MODEL>
__device__ __forceinline__ double sum_p(const double* Tp) {     // Tp[q] of P state 2 + q
    if constexpr (MODEL == 0) return ((Tp[0] + Tp[2]) + Tp[1]) + Tp[3];   // lanes 0, 3, 4, 7
    return (Tp[0] + Tp[1]) + (Tp[2] + Tp[3]);
}
template <int MODEL>
__device__ __forceinline__ double tree_lanes(const double* vs) {   // vs by state
    double v[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) {
        const int st = MODEL == 0 ? state_of_lane0(l) : l;
        v[l] = st < NS ? vs[st] : 0.;
    }
    return tree16n(v);
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_substeps_r(SubstepArgs a, const FastTab* __restrict__ tab) {
    constexpr const int(&COL)[NS][3] = kFastColM[MODEL];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const QTConst& qc = a.qc;
    const FastTab& T = *tab;
    const int S = a.S;
    double P[3], Vv[3], Fv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        P[c] = a.R[(size_t)c * S + i];
        Vv[c] = a.V[(size_t)c * S + i];
        if (a.nseg > 1) {
            Fv[c] = slot_sum16(a.Fpart + (size_t)c * S + i, (size_t)3 * S, a.nseg);
            a.F[(size_t)c * S + i] = Fv[c];
        } else {
            Fv[c] = a.F[(size_t)c * S + i];
        }
    }
    double tPart = a.tPart[i];
    cxd w[NS + 1];                          // w[NS]: the zero state of model 0's unused slots
    w[NS] = {0., 0.};
    if (a.do_qt) {
#pragma unroll
        for (int k = 0; k < NS; ++k) w[k] = {a.psi[(size_t)(2 * k) * S + i], a.psi[(size_t)(2 * k + 1) * S + i]};
    }
    const double L = a.L, dt = qc.dtQ, DT = 0.5 * dt, DT2 = T.dt2;
    const uint64_t gid = a.gid0 + (uint64_t)i;
    for (int s = 0; s < a.nsub; ++s) {
        if (a.do_step) {
            const bool moving = a.t[s] > 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                P[c] = half_drift(P[c], Vv[c], Fv[c], moving, DT, DT2, L);
                Vv[c] = Vv[c] + dt * Fv[c];
                P[c] = half_drift(P[c], Vv[c], Fv[c], moving, DT, DT2, L);
            }
        }
        if (!a.do_qt) continue;
        const double u = Vv[0] * qc.pv2q + a.expDet[s];
        tPart += qc.dtQ;
        double Tp[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) Tp[q] = nrm2(w[2 + q]) * T.hdp[2 + q];
        const double dp = sum_p<MODEL>(Tp);
        double u1, u2;
        draw_pair(qc, a.U, S, i, gid, a.q0 + (uint64_t)s, 0, u1, u2);
        double kick;
        if (u1 > dp) {
            double kv[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k)
                kv[k] = kick_term(w[k], w[COL[k][0]], w[COL[k][1]], w[COL[k][2]], T.kw[0][k],
                                  T.kw[1][k], T.kw[2][k]);
            kick = sum_p<MODEL>(kv + 2);                 // the kick terms sit on the P lanes
            const double phi = (u * T.cphi) * tPart;
            double sn, cs;
            sincos_q2(phi, kSinCos64, sn, cs);
            cxd md[NS], c2[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                md[k] = {T.mre[k], fma(T.mi1[k], u, T.mi0[k])};
                c2[k] = {fma(T.dms[k], sn, T.cre[2][k]), fma(T.dmc[k], cs, T.cim[2][k])};
            }
            cxd y[NS + 1], acc[NS];
#pragma unroll
            for (int k = 0; k <= NS; ++k) y[k] = w[k];
#pragma unroll
            for (int stg = 0; stg < 4; ++stg) {
                double dpy = dp;
                if (stg > 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) Tp[q] = nrm2(y[2 + q]) * T.hdp[2 + q];
                    dpy = sum_p<MODEL>(Tp);
                }
                const double pref = rsq_nr(1. - dpy);
                cxd ws[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    ws[k] = row_r(md[k], y[k], cxd{T.cre[0][k], T.cim[0][k]}, y[COL[k][0]],
                                  cxd{T.cre[1][k], T.cim[1][k]}, y[COL[k][1]], c2[k], y[COL[k][2]]);
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const cxd d = {fma(pref, ws[k].re, -y[k].re), fma(pref, ws[k].im, -y[k].im)};
                    if (stg == 0) acc[k] = d;
                    else if (stg < 3) acc[k] = {fma(3., d.re, acc[k].re), fma(3., d.im, acc[k].im)};
                    else acc[k] = {acc[k].re + d.re, acc[k].im + d.im};
                    if (stg < 2) y[k] = {fma(0.5, d.re, w[k].re), fma(0.5, d.im, w[k].im)};
                    else if (stg == 2) y[k] = {w[k].re + d.re, w[k].im + d.im};
                }
            }
#pragma unroll
            for (int k = 0; k < NS; ++k) w[k] = {fma(0.125, acc[k].re, w[k].re), fma(0.125, acc[k].im, w[k].im)};
        } else {
            tPart = 0;
            double randDOrS, randDir, rand3, dummy;
            draw_pair(qc, a.U, S, i, gid, a.q0 + (uint64_t)s, 1, randDOrS, randDir);
            draw_pair(qc, a.U, S, i, gid, a.q0 + (uint64_t)s, 2, rand3, dummy);
            (void)dummy;
            const int target = MODEL == 0 ? jump_target(qc, sq(w[2]), sq(w[3]), sq(w[4]), sq(w[5]), u2, randDOrS,
                                                        randDir, rand3, kick)
                                          : jump_target_pump(qc, sq(w[2]), sq(w[3]), sq(w[4]), sq(w[5]), u2,
                                                             randDOrS, randDir, rand3, kick);
#pragma unroll
            for (int k = 0; k < NS; ++k) w[k] = {k == target ? 1. : 0., 0.};
        }
        if (qc.renorm) {                                                    // :706-712
            double nv[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) nv[k] = nrm2(w[k]);
            const double r = rsq_nr(tree_lanes<MODEL>(nv));
#pragma unroll
            for (int k = 0; k < NS; ++k) w[k] = {w[k].re * r, w[k].im * r};
        }
        Vv[0] = fma(1., kick, Vv[0]);                                       // :705
    }
    const double lo = -0.125 * L, hi = 1.125 * L;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.R[(size_t)c * S + i] = P[c];
        a.V[(size_t)c * S + i] = Vv[c];
        if (!(P[c] >= lo && P[c] <= hi)) *a.oor = 1;
    }
    if (a.do_qt) {
        a.tPart[i] = tPart;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            a.psi[(size_t)(2 * k) * S + i] = w[k].re;
            a.psi[(size_t)(2 * k + 1) * S + i] = w[k].im;
        }
    }
}

template <bool DPPX, bool FAST>
__global__ __launch_bounds__(256) void k_substeps_lanes_r(SubstepArgs a, const FastTab* __restrict__ tab) {
    lane_substeps<DPPX, FAST, false>(a, tab, blockIdx.x);
}
// the FAST launch when QTConst::im01 (the production model-0 case); EDZ: expdet_zero
template <bool DPPX, bool EDZ, bool NORN = false>
__global__ __launch_bounds__(256) void k_substeps_lanes_im(SubstepArgs a, const FastTab* __restrict__ tab) {
    lane_substeps<DPPX, true, false, true, EDZ, NORN>(a, tab, blockIdx.x);
}

// ------------------------------------------------------------------------------------------
// k_md_step: one MD step of one system (world 1, Newton-3 tiles, the lane QT kernel's FAST
// instance) in ONE launch — forces() (SpeedUp:192-236) then the interval's fused step(); qstep();
// substeps (:1376-1377).  Workgroups [0, npairs) are the tile pairs of k_pairs_n3 (same body,
// write-through slot stores, one arrival per tile whose rows they wrote); workgroups npairs.. are
// the lane kernel's 16-ion groups, which do their prologue (loads, Philox draws) while the force
// workgroups run and wait for the arrival count of their ions' tile before reading the slots.
// Workgroups are dispatched in index order, so every force workgroup is placed before any QT
// workgroup: the waits cannot starve a force workgroup of a slot.  Same operations on the same
// values as the two launches: bit-identical (tests/test_gpu_parity.py).  Saves the QT launch's
// dispatch and hides its prologue behind the force kernel's tail.
// ------------------------------------------------------------------------------------------
static_assert(kLaneWG == 64 * N3W, "k_md_step: one workgroup size for both parts");
#if defined(MDQT_EXPT_MDSTAMPS)
extern "C" int mdqt_expt_md_stamps(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_md_stamps), sizeof(unsigned long long) * 4 * n) == hipSuccess ? 0 : -1;
}
#define MD_STAMP(slot) \
    do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_md_stamps[4 * blockIdx.x + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define MD_STAMP(slot) ((void)0)
#endif
template <bool DPPX, int VARIANT>
__global__ __launch_bounds__(256) void k_md_step(N3Args f, SubstepArgs a, const FastTab* __restrict__ tab) {
    MD_STAMP(0);
    if ((int)blockIdx.x < f.npairs) {
        __shared__ double pj[3][128];
        __shared__ double accj[N3W][3][128];
        __shared__ double ia[N3W][3][64];
        __shared__ double mj[128];
        __shared__ double etab[64];
        stage_exp_tab(etab);
        const int2 IJ = f.pairs[blockIdx.x];
        const PairC c = {f.L, f.micT, f.micGuard, f.Rcut, f.lDeb, f.invlDeb, 1. / f.L, f.rc2, etab};
        const bool rag = (f.N & 63) && IJ.y == f.ntiles - 1;
        if (rag) n3_tile<VARIANT, false, true, true>(f, c, IJ.x, IJ.y, pj, accj, mj, ia);
        else n3_tile<VARIANT, false, false, true>(f, c, IJ.x, IJ.y, pj, accj, mj, ia);
        MD_STAMP(1);
        return;
    }
    lane_substeps<DPPX, true, true>(a, tab, (int)blockIdx.x - f.npairs);
    MD_STAMP(1);
}

hipError_t launch_md_step(const N3Args& f, const SubstepArgs& a, const FastTab* tab, int variant, hipStream_t s,
                          hipEvent_t ev0, hipEvent_t ev1) {
    if (a.n <= 0 || f.npairs <= 0 || a.nsub <= 0 || a.nsub > MAXSUB || !a.arrive || !f.arrive || f.guard)
        return hipErrorInvalidValue;
    if (a.qc.model < 0 || a.qc.model >= NMODELS || variant < 0 || variant > 1) return hipErrorInvalidValue;
    const dim3 gl(f.npairs + (a.n + kLaneWG / 16 - 1) / (kLaneWG / 16)), bl(kLaneWG);
    const FastTab* lt = tab + 1;                      // by lane
    if (a.qc.model == 0) {
        if (variant == 1) launch_timed(k_md_step<true, 1>, gl, bl, s, ev0, ev1, f, a, lt);
        else launch_timed(k_md_step<true, 0>, gl, bl, s, ev0, ev1, f, a, lt);
    } else {
        if (variant == 1) launch_timed(k_md_step<false, 1>, gl, bl, s, ev0, ev1, f, a, lt);
        else launch_timed(k_md_step<false, 0>, gl, bl, s, ev0, ev1, f, a, lt);
    }
    return hipGetLastError();
}

#if defined(MDQT_EXPT_QTSTAMPS)
extern "C" int mdqt_expt_qt_stamps(unsigned long long* out, int nwaves) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qt_stamps), sizeof(unsigned long long) * 16 * nwaves) == hipSuccess ? 0 : -1;
}
#endif

hipError_t launch_substeps_r(const SubstepArgs& a, const FastTab* tab, int mode, hipStream_t s, hipEvent_t ev0,
                             hipEvent_t ev1, int* instance) {
    if (a.n <= 0 || a.nsub <= 0) return hipSuccess;
    if (a.nsub > MAXSUB) return hipErrorInvalidValue;
    if (mode == 0) mode = (a.n < kLaneKernelMaxIons) ? 2 : 1;
    if (a.qc.model < 0 || a.qc.model >= NMODELS) return hipErrorInvalidValue;
    const dim3 gl((a.n + kLaneIons - 1) / kLaneIons), bl(kLaneWG), gt((a.n + 255) / 256), b(256);
    int inst = QTK_THREAD_R + a.qc.model;
    if (mode == 2) {
        const FastTab* lt = tab + 1;                  // by lane
        switch (inst = lane_qt_instance(a)) {
        case QTK_LANES_IM_EDZ: launch_timed(k_substeps_lanes_im<true, true, true>, gl, bl, s, ev0, ev1, a, lt); break;
        case QTK_LANES_IM_EDZ_RN: launch_timed(k_substeps_lanes_im<true, true>, gl, bl, s, ev0, ev1, a, lt); break;
        case QTK_LANES_IM: launch_timed(k_substeps_lanes_im<true, false>, gl, bl, s, ev0, ev1, a, lt); break;
        case QTK_LANES_R_FAST: launch_timed(k_substeps_lanes_r<true, true>, gl, bl, s, ev0, ev1, a, lt); break;
        case QTK_LANES_R: launch_timed(k_substeps_lanes_r<true, false>, gl, bl, s, ev0, ev1, a, lt); break;
        case QTK_LANES_R_PUMP_FAST: launch_timed(k_substeps_lanes_r<false, true>, gl, bl, s, ev0, ev1, a, lt); break;
        case QTK_LANES_R_PUMP: launch_timed(k_substeps_lanes_r<false, false>, gl, bl, s, ev0, ev1, a, lt); break;
        default: return hipErrorInvalidValue;         // (an instance lane_qt_instance has and this switch has not)
        }
    }
    else if (a.qc.model == 0) launch_timed(k_substeps_r<0>, gt, b, s, ev0, ev1, a, tab);
    else if (a.qc.model == 1) launch_timed(k_substeps_r<1>, gt, b, s, ev0, ev1, a, tab);
    else if (a.qc.model == 2) launch_timed(k_substeps_r<2>, gt, b, s, ev0, ev1, a, tab);
    else launch_timed(k_substeps_r<3>, gt, b, s, ev0, ev1, a, tab);
    if (instance) *instance = inst;
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// spin-up tagging after the pump window: measureSpinUps (randomFrozenStartTag408Linear.cpp:600,
// randomFrozenStartTag422Linear.cpp:568) = tagParticles (MonteCarloFollowedByQTTagging408Linear.cpp
// :1022).  Draws: Philox (ion, qstep index, draws 6 and 7) for rand and rand2/rand3.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tag_spin_up(const double* __restrict__ psi, int n, int S, uint64_t gid0,
                                                     uint64_t q, QTConst qc, int* __restrict__ tags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    tag_spin_up_ion(psi, i, S, gid0, q, qc, tags);                   // mdqt_pump_device.hpp
}

hipError_t launch_tag_spin_up(const double* psi, int n, int S, uint64_t gid0, uint64_t q, const QTConst& qc,
                              int* tags, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tag_spin_up, dim3((n + 255) / 256), dim3(256), 0, s, psi, n, S, gid0, q, qc, tags);
    return hipGetLastError();
}

}  // namespace mdqt
