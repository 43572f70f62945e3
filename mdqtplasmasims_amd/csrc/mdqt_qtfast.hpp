// lane_substeps — the lane-per-state body of the qt_math 2 substeps — and the device helpers and constants
// it needs, shared by the single-job kernels (mdqt_qtfast.hip) and the ensemble's batched kernels
// (mdqt_ensemble_qt.hip).  The arithmetic forms are described at the top of mdqt_qtfast.hip.  At the end, for
// the host: which instance of it a launch runs (lane_qt_instance) — the one part a .cpp file may include.
#pragma once
#include "mdqt_internal.hpp"
#if defined(__HIP__)
#include "mdqt_device.hpp"
#include "mdqt_pairs.hpp"

#include <math.h>

#include <type_traits>

namespace mdqt {

// threads per workgroup of the lane-per-state kernels (16 lanes per ion); measured at 64 / 128 / 256
// threads: 29.6 / 40.1 / 29.2 us per fused launch (docs/PERF_HISTORY.md)
constexpr int kLaneWG = 256;
static_assert(kLaneWG % 64 == 0 && kLaneWG >= 128, "whole waves; the first 128 threads stage the sincos table");
constexpr int kRows = 4;                             // ions per wave of the lane kernels: one per row of 16 lanes
constexpr int kLaneIons = kLaneWG / 64 * kRows;      // ions per workgroup

__device__ __forceinline__ double rsq_nr(double x) { return rsq3(x); }   // 1/sqrt(x), mdqt_math.hpp
__device__ __forceinline__ double nrm2(cxd y) { return fma(y.re, y.re, y.im * y.im); }
__device__ __forceinline__ double rho_im_r(cxd a, cxd b) { return fma(a.im, b.re, -(a.re * b.im)); }

// M_kk y + c0 y0 + c1 y1 + c2 y2, one chain per component
__device__ __forceinline__ cxd row_r(cxd md, cxd y, cxd c0, cxd y0, cxd c1, cxd y1, cxd c2, cxd y2) {
    double re = md.re * y.re, im = md.re * y.im;
    re = fma(-md.im, y.im, re);  im = fma(md.im, y.re, im);
    re = fma(c0.re, y0.re, re);  im = fma(c0.re, y0.im, im);
    re = fma(-c0.im, y0.im, re); im = fma(c0.im, y0.re, im);
    re = fma(c1.re, y1.re, re);  im = fma(c1.re, y1.im, im);
    re = fma(-c1.im, y1.im, re); im = fma(c1.im, y1.re, im);
    re = fma(c2.re, y2.re, re);  im = fma(c2.re, y2.im, im);
    re = fma(-c2.im, y2.im, re); im = fma(c2.im, y2.re, im);
    return {re, im};
}

// row_r when the static slots 0 and 1 are purely imaginary (c.re = +-0): their real-part FMAs
// add +-0 * y and are dropped — the same values up to the sign of an exact-zero result
__device__ __forceinline__ cxd row_r_im01(cxd md, cxd y, double c0im, cxd y0, double c1im, cxd y1, cxd c2, cxd y2) {
    double re = md.re * y.re, im = md.re * y.im;
    re = fma(-md.im, y.im, re);  im = fma(md.im, y.re, im);
    re = fma(-c0im, y0.im, re);  im = fma(c0im, y0.re, im);
    re = fma(-c1im, y1.im, re);  im = fma(c1im, y1.re, im);
    re = fma(c2.re, y2.re, re);  im = fma(c2.re, y2.im, im);
    re = fma(-c2.im, y2.im, re); im = fma(c2.im, y2.re, im);
    return {re, im};
}

__device__ __forceinline__ double kick_term(cxd w, cxd w0, cxd w1, cxd w2, double k0, double k1, double k2) {
    return fma(rho_im_r(w, w0), k0, fma(rho_im_r(w, w1), k1, rho_im_r(w, w2) * k2));
}

// sum of 16 values in the lane kernel's DPP tree order (row_shl 1, 2, 4, 8)
__device__ __forceinline__ double tree16(const double* v) {
    return (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) +
           (((v[8] + v[9]) + (v[10] + v[11])) + ((v[12] + v[13]) + (v[14] + v[15])));
}
__device__ __forceinline__ double lane_tree16(double v) {
    double a = v + dpp<SHL(1)>(v);
    a = a + dpp<SHL(2)>(a);
    a = a + dpp<SHL(4)>(a);
    a = a + dpp<SHL(8)>(a);
    return dpp<BCAST(0)>(a);
}
// renormalisation sum of the ion's 16 lanes: quads Q_m = (v_4m + v_4m+1) + (v_4m+2 + v_4m+3),
// then ((Q0 + Q1) + Q2) + Q3
__device__ __forceinline__ double tree16n(const double* v) {
    double q[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) q[m] = (v[4 * m] + v[4 * m + 1]) + (v[4 * m + 2] + v[4 * m + 3]);
    return ((q[0] + q[1]) + q[2]) + q[3];
}
// (T2 + T3) + (T4 + T5) of the ion's lanes 2..5, in every lane of the row
__device__ __forceinline__ double lane_sum_p(double T) {
    double a = T + dpp<SHL(1)>(T);
    a = a + dpp<SHL(2)>(a);
    return dpp<BCAST(2)>(a);
}

// step_R(dt/2) of one coordinate (:356-389), the reference's operations (step() stays bit-exact
// in every qt_math mode); `moving` = t > 0 (:360)
__device__ __forceinline__ double half_drift(double p, double v, double f, bool moving, double DT,
                                             double DT2, double L) {
    p = moving ? p + DT * v : p + (DT * v + DT2 * f);
    // (measured: one fma p + m L with m = +1 / -1 / 0 instead of the two conditional adds issues 6
    // instructions fewer per substep but lengthens the dependent chain — QT launch 21.3 -> 21.8 us,
    // A/B round 3; the reference's two adds are kept)
    if (p < 0) p += L;
    if (p > L) p -= L;
    return p;
}

// the quantum jump (:573-703), the exact-mode operations of mdqt_kernels.hip
__device__ __forceinline__ int jump_target(const QTConst& qc, double n3, double n4, double n5, double n6,
                                           double rand2, double randDOrS, double randDir, double rand3,
                                           double& kick) {
    const double tot = n3 + n4 + n5 + n6;
    const double prob3 = n3 / tot, prob4 = n4 / tot, prob5 = n5 / tot;
    const bool sDecay = !(randDOrS < qc.pD);
    if (!sDecay) kick = (randDir < 0.5) ? qc.vKickDP : -qc.vKickDP;
    else kick = (randDir < 0.5) ? qc.vKick : -qc.vKick;
    if (rand2 < prob3) {
        if (sDecay) return 1;
        return (rand3 < qc.thD[0][0]) ? 11 : (rand3 < qc.thD[0][1]) ? 10 : 9;
    } else if (rand2 < prob3 + prob4) {
        if (sDecay) return (rand3 < qc.thS3) ? 0 : 1;
        return (rand3 < qc.thD[1][0]) ? 10 : (rand3 < qc.thD[1][1]) ? 9 : 8;
    } else if (rand2 < prob3 + prob4 + prob5) {
        if (sDecay) return (rand3 < qc.thS4) ? 1 : 0;
        return (rand3 < qc.thD[2][0]) ? 9 : (rand3 < qc.thD[2][1]) ? 8 : 7;
    }
    if (sDecay) return 0;
    return (rand3 < qc.thD[3][0]) ? 8 : (rand3 < qc.thD[3][1]) ? 7 : 6;
}

// quantum jump of the optical-pumping models (no kick).  Draws in the reference's order: u1,
// rand2, randDOrS, then 408: randDir (unused), [rand3]; 422: [rand3] — i.e. rand3 is draw 4 for
// 408 (randomFrozenStartTag408Linear.cpp:521-590) and draw 3 for 422 (...422Linear.cpp:174-231)
__device__ __forceinline__ int jump_target_pump(const QTConst& qc, double n3, double n4, double n5, double n6,
                                                double rand2, double randDOrS, double d3, double d4,
                                                double& kick) {
    kick = 0.;
    const bool sDecay = !(randDOrS < qc.pD);
    if (qc.model == 3) {                            // 422: P levels 2, 3; D level 4
        const double tot = n3 + n4;
        const double prob3 = n3 / tot;
        if (rand2 < prob3) return sDecay ? ((d3 < 2. / 3) ? 1 : 0) : 4;
        return sDecay ? ((d3 < 2. / 3) ? 0 : 1) : 4;
    }
    const double tot = n3 + n4 + n5 + n6;           // 408: P levels 2..5; D level 6
    const double prob3 = n3 / tot, prob4 = n4 / tot, prob5 = n5 / tot;
    if (rand2 < prob3) return sDecay ? 0 : 6;
    if (rand2 < prob3 + prob4) return sDecay ? ((d4 < 2. / 3) ? 0 : 1) : 6;
    if (rand2 < prob3 + prob4 + prob5) return sDecay ? ((d4 < 1. / 3) ? 0 : 1) : 6;
    return sDecay ? 1 : 6;
}

__device__ __forceinline__ double sq(cxd y) { return y.re * y.re + y.im * y.im; }

// ------------------------------------------------------------------------------------------
// lane per state: one ion per 16-lane group (4 per wave64).  DPPX (model 0): states on lanes by
// kStateOfLane0 and the three coupling slots gathered with DPP moves (lane ^ 2, lane + 8,
// lane ^ 1); lanes 9 / 10 hold the y / z coordinate, every other lane x.  Otherwise (the pumping
// models): lane k = state k, slots gathered through LDS, lanes 12 / 13 hold y / z.  Lanes
// without a state carry zero amplitudes and zero coefficients.  `tab` is indexed by lane.
// ------------------------------------------------------------------------------------------
// dp of model 0's layout: ((T_lane0 + T_lane3) + T_lane4) + T_lane7 = ((T2 + T4) + T3) + T5, in
// every lane — one 64-bit broadcast, then three v_fmac_f64_dpp row_newbcast (the DP ALU takes a
// row_newbcast operand: broadcast and add in one instruction; x * 1 + a is exactly x + a).  `one`
// is 1.0 in a VGPR the compiler cannot see through, so the FMA is kept and the DPP move folds in.
__device__ __forceinline__ double opaque_one() {
    double o = 1.0;
    asm volatile("" : "+v"(o));
    return o;
}
// a + T[lane L of the row] * one as one v_fmac_f64_dpp (the compiler does not fold the 64-bit
// DPP move into the FMA).  DPP read-after-VALU-write hazard: T is also the operand of the
// compiler-emitted broadcast before the first of these, so the write is >= 2 states back.
template <int L>
__device__ __forceinline__ double fmac_bcast(double a, double T, double one) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "+v"(a) : "v"(T), "v"(one), "n"(L));
    return a;
#else
    return fma(T, one, a);
#endif
}
__device__ __forceinline__ double lane_norm16(double v, double one) {
    double a = v + dpp<SHL(1)>(v);                  // lane 2m: v_2m + v_2m+1
    a = a + dpp<SHL(2)>(a);                         // lane 4m: Q_m
    double b = dpp<BCAST(0)>(a);
    b = fmac_bcast<4>(b, a, one);
    b = fmac_bcast<8>(b, a, one);
    return fmac_bcast<12>(b, a, one);
}
__device__ __forceinline__ double lane_sum_p8(double T, double one) {
    double a = dpp<BCAST(0)>(T);
    a = fmac_bcast<3>(a, T, one);
    a = fmac_bcast<4>(a, T, one);
    return fmac_bcast<7>(a, T, one);
}

// the lane kernel's state stores (R, V, F, tPart, psi) write-through, like the force slots
// (mdqt_pairs.hpp slot_store): waves that finish early stream their ions out before the last
// wave ends, and the kernel-end L2 write-back has nothing left to do.  A/B at C2 against plain stores,
// on top of the slot stores: QT launch -0.4 us, MD step -0.6 us.
__device__ __forceinline__ void qt_store(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#if defined(MDQT_EXPT_QTSTAMPS)
// diagnostic build only: per-wave s_memtime at entry, loop start, loop end, exit + s_memrealtime
// at entry and exit, s_memtime after the force-slot loads (6), after the prologue's loads are
// issued (9) and after the Philox draws (8), and the number of substeps in which an ion of the
// wave jumped (7) (tools/qt_stamps.py)
__device__ unsigned long long g_qt_stamps[16 * 4096];
#define QT_STAMP(slot, v) (st_[slot] = (v))
#define QT_JCOUNT(c) (st_[7] += (__builtin_amdgcn_ballot_w64(c) != 0))
#else
#define QT_STAMP(slot, v) ((void)0)
#define QT_JCOUNT(c) ((void)0)
#endif

#if defined(MDQT_EXPT_MDSTAMPS)
// diagnostic build only (k_md_step): per-workgroup s_memrealtime at entry and exit (+ after the
// wait, QT workgroups)
__device__ unsigned long long g_md_stamps[4 * 4096];
#endif

// FAST: the production launch — step + qstep (do_step, do_qt), every substep with t > 0 (all but
// the simulation's first launch), F from the force slots (or F itself when nseg == 1), no arrival
// wait: step_R's
// non-moving branch (:360), the last substep's no-drift select and the other paths' loads and
// branches are compiled out (straight-line prologue: one memory round trip)
// FUSED (with FAST; the QT workgroups of k_md_step): the force partials of this launch's own
// tile pairs are read after the arrival count of the ions' tile is complete, with L1-bypassing
// loads (the tile pairs' slot stores are write-through: MI355X_MICROARCH.md, hand-off forms)
// IM01 (with FAST): the static coupling slots 0 and 1 are purely imaginary (QTConst::im01), their
// real-part FMAs are dropped.  EDZ: every expDetuning of the launch is 0 (u = vx pv2q).  The
// production model-0 launch is k_substeps_lanes_im<true, true> (FAST + IM01 + EDZ).
// NORN: reNormalizewvFns is off (the reference's default, SpeedUp:74) — the renormalisation and
// its uniform branch compiled out, so one substep's tail and the next one's head share a basic block
// JUNI: a substep in which an ion of the wave jumps runs as one straight-line block chosen wave-uniformly
// (see the substep body).  Off where the extra registers of that block cost more than
// the jump tail: the QT workgroups of k_md_step (one VGPR count for both parts: 214 instead of 168 would
// take the tile pairs from three waves per SIMD to two) and the ensemble's three-waves-per-SIMD set (168
// VGPRs: 196 bytes of scratch instead of 20) keep the per-lane branch.
template <bool DPPX, bool FAST, bool FUSED, bool IM01 = false, bool EDZ = false, bool NORN = false, bool JUNI = !FUSED>
__device__ __forceinline__ void lane_substeps(const SubstepArgs& a, const FastTab* __restrict__ tab, int blk) {
#if defined(MDQT_EXPT_QTSTAMPS)
    unsigned long long st_[16] = {};
#endif
    QT_STAMP(0, __builtin_amdgcn_s_memtime());
    QT_STAMP(4, __builtin_amdgcn_s_memrealtime());
    const int k = threadIdx.x & 15;
    const int grp = threadIdx.x >> 4;
    const int iraw = blk * (kLaneWG / 16) + grp;
    const bool store = iraw < a.n;
    const int i = store ? iraw : a.n - 1;             // idle groups shadow the last ion
    const QTConst& qc = a.qc;
    const int S = a.S;
    const int st = DPPX ? state_of_lane0(k) : k;      // >= NS: no state on this lane
    const int cy = DPPX ? 9 : 12, cz = DPPX ? 10 : 13;
    const int c = (k == cy) ? 1 : (k == cz) ? 2 : 0;
    const bool owner = (k == 0) || (k == cy) || (k == cz);   // stores coordinate c
    const int base = threadIdx.x & ~15;
    const int l0 = base + tab->col[0][k], l1 = base + tab->col[1][k], l2 = base + tab->col[2][k];
    const cxd c0 = {tab->cre[0][k], tab->cim[0][k]}, c1 = {tab->cre[1][k], tab->cim[1][k]};
    const double c2re = tab->cre[2][k], c2im = tab->cim[2][k], dms = tab->dms[k], dmc = tab->dmc[k];
    const double mre = tab->mre[k], mi0 = tab->mi0[k], mi1 = tab->mi1[k], hdp = tab->hdp[k];
    const double kw0 = tab->kw[0][k], kw1 = tab->kw[1][k], kw2 = tab->kw[2][k];
    const double cphi = tab->cphi, DT2 = tab->dt2;
    const double kmask = (c == 0) ? 1. : 0.;
    const double one = opaque_one();
    // Prologue: every load is issued before any is consumed (one memory round trip), and the
    // lane-parallel Philox draws below run while they are in flight.
    double p = a.R[(size_t)c * S + i], v = a.V[(size_t)c * S + i], f;
    double tPart = a.tPart[i];
    cxd w = {0., 0.};
    if ((FAST || a.do_qt) && st < NS) w = {a.psi[(size_t)(2 * st) * S + i], a.psi[(size_t)(2 * st + 1) * S + i]};
    const int nseg = a.nseg;
    // F: the canonical slot_sum16 distributed over the ion's 16 lanes — lane k forms the strided
    // partial q_k of all three components (its loads issued together, 4 slots per round), the
    // DPP tree combines them in slot_sum16's order
    double qf[3] = {0., 0., 0.};
    // overlapped MD step (a.arrive): the partials are read after the arrival wait below, with
    // L1-bypassing loads; otherwise right here, with the other prologue loads
    auto slot_round = [&](int s0, double (*t)[3], bool sc1) {   // slots s0, s0 + 16, + 32, + 48
        // FAST with nseg == 1 (F already summed): slot 0 is F itself, the other lanes add zeros
        const double* base_p = (FAST && nseg == 1 ? (const double*)a.F : a.Fpart) + i;
        const size_t plane = (size_t)3 * S;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int sl = s0 + 16 * u;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                if (FAST) {   // unconditional loads (clamped slot, in range), the select at the sum:
                              // no branch around the load, so nothing forces an early wait on it
                    const double* q = base_p + (size_t)min(sl, nseg - 1) * plane + (size_t)cc * S;
                    const double x = sc1 ? __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *q;
                    t[u][cc] = sl < nseg ? x : 0.;
                } else {
                    const double* q = base_p + (size_t)sl * plane + (size_t)cc * S;
                    t[u][cc] = sl < nseg ? (sc1 ? __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *q)
                                         : 0.;
                }
            }
        }
    };
    auto slot_add = [&](double (*t)[3]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) qf[cc] = qf[cc] + t[u][cc];
    };
    auto slot_partials = [&](bool sc1) {
        for (int s0 = k; s0 < nseg; s0 += 64) {
            double t[4][3];
            slot_round(s0, t, sc1);
            slot_add(t);
        }
    };
    // FAST: the first round's loads stay in flight across the Philox draws below; summed after
    double t0[4][3];
    if (FAST) {
        if (!FUSED) slot_round(k, t0, false);
    } else if (nseg > 1) {
        if (!a.arrive) slot_partials(false);
    } else {
        f = a.F[(size_t)c * S + i];
    }
    QT_STAMP(9, __builtin_amdgcn_s_memtime());
    const double L = a.L, dt = qc.dtQ, DT = 0.5 * dt;
    // the substep loop's tPart step and Doppler factor held in VGPRs: with every SGPR taken the
    // compiler otherwise re-loads them from the kernel arguments inside the loop, and the
    // s_waitcnt on that scalar load stalls every substep
    double dtq_v = qc.dtQ, pv2q_v = qc.pv2q;
    asm volatile("" : "+v"(dtq_v), "+v"(pv2q_v));
    const uint64_t gid = a.gid0 + (uint64_t)i;
    // per-substep constants out of kernel-argument loads inside the substep loop (a scalar load
    // indexed by the substep waits ~100+ cycles in every iteration): the moving flags as a bit
    // mask, expDetuning(t) of every substep in an LDS row (one broadcast read per substep, issued
    // with the uniforms; it replaces a readlane and its scalar branches in every iteration)
    const uint32_t movmask = a.movmask;
    __shared__ double edt[MAXSUB];
    // (loaded here, written to LDS after the force sum below: an LDS write of a loaded value waits
    // for every load issued before it, which would stall the Philox draws behind the slot loads)
    const double edv = (threadIdx.x < MAXSUB && a.expdet_zero == 0 && (int)threadIdx.x < a.nsub)
                           ? a.expDet[threadIdx.x] : 0.;
    // the coupling phase's e^(2 pi i j / 64) table (sincos_tab) in LDS, written with edt below
    __shared__ double sct[128];
    const double sctv = threadIdx.x < 128 ? kSinCos64[threadIdx.x] : 0.;
    // u1, u2 of every substep of the launch staged in LDS: Philox draws computed lane-parallel
    // (lane k: substeps k, k + 16), or the rng_mode 0 uniforms of the single substep
    __shared__ double su[kLaneWG / 16][MAXSUB][2];
    if (FAST || a.do_qt) {
        if (a.U) {
            if (k == 0) { su[grp][0][0] = a.U[i]; su[grp][0][1] = a.U[(size_t)S + i]; }
        } else {
            for (int s = k; s < a.nsub; s += 16) {
                double x0, x1;
                philox_pair(qc, gid, a.q0 + (uint64_t)s, 0, x0, x1);
                su[grp][s][0] = x0;
                su[grp][s][1] = x1;
            }
        }
    }
    QT_STAMP(8, __builtin_amdgcn_s_memtime());
    if (!FAST && a.arrive) {                          // wait for the concurrent force launch
        if (threadIdx.x == 0) {
            int it = 0;
            const unsigned long long* cnt = a.arrive + (blk * (kLaneWG / 16)) / 64;   // the ions' tile
            while (__hip_atomic_load(cnt, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < a.arrive_target) {
                for (int z = 0; z < a.arrive_sleep; ++z) __builtin_amdgcn_s_sleep(1);
                if (++it > (1 << 21)) { *a.spin_err = 1; break; }   // bounded: never hang the GPU
            }
        }
        __syncthreads();                              // thread 0's acquire, then the workgroup's loads
        __atomic_thread_fence(__ATOMIC_ACQUIRE);       // (workgroup fence: no early slot load)
        if (nseg > 1) slot_partials(true);
    }
    if (FUSED) {                                      // this launch's tile pairs of the ions' tile
        if (threadIdx.x == 0) {
            const unsigned long long* cnt = a.arrive + (blk * (kLaneWG / 16)) / 64;
            int it = 0;
            while (__hip_atomic_load(cnt, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < a.arrive_target) {
                __builtin_amdgcn_s_sleep(2);
                if (++it > (1 << 22)) { *a.spin_err = 1; break; }   // bounded: never hang the GPU
            }
        }
        __syncthreads();
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
#if defined(MDQT_EXPT_MDSTAMPS)
        if (threadIdx.x == 0 && blockIdx.x < 4096) g_md_stamps[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memrealtime();
#endif
        slot_round(k, t0, true);
    }
    if (FAST) {
        slot_add(t0);
        for (int s0 = k + 64; s0 < nseg; s0 += 64) {
            double t[4][3];
            slot_round(s0, t, FUSED);
            slot_add(t);
        }
    }
    QT_STAMP(6, __builtin_amdgcn_s_memtime());
    if (FAST || nseg > 1) {
        const double fx = lane_tree16(qf[0]), fy = lane_tree16(qf[1]), fz = lane_tree16(qf[2]);
        f = c == 0 ? fx : c == 1 ? fy : fz;
        if (store && owner) qt_store(&a.F[(size_t)c * S + i], f);
    }
    if (threadIdx.x < MAXSUB) edt[threadIdx.x] = edv;
    if (threadIdx.x < 128) sct[threadIdx.x] = sctv;
    __syncthreads();
    __shared__ double2 xg[DPPX ? 1 : kLaneWG];
    auto exchange = [&](cxd y, cxd& y0, cxd& y1, cxd& y2) {
        if constexpr (DPPX) {
            y0 = {dpp<QP_XOR2>(y.re), dpp<QP_XOR2>(y.im)};
            y1 = {dpp<ROR(8)>(y.re), dpp<ROR(8)>(y.im)};
            y2 = {dpp<QP_XOR1>(y.re), dpp<QP_XOR1>(y.im)};
            return;
        }
        wave_sync();
        xg[threadIdx.x] = make_double2(y.re, y.im);
        wave_sync();
        const double2 t0 = xg[l0], t1 = xg[l1], t2 = xg[l2];
        y0 = {t0.x, t0.y}; y1 = {t1.x, t1.y}; y2 = {t2.x, t2.y};
    };
    auto drift = [&](double& pp, double& vv, int sub) {   // step(): step_R, step_V, step_R (:418-430)
        const bool moving = FAST || ((movmask >> sub) & 1u);
        pp = half_drift(pp, vv, f, moving, DT, DT2, L);
        vv = vv + dt * f;                             // step_V(dt) :398-409
        pp = half_drift(pp, vv, f, moving, DT, DT2, L);
    };
    QT_STAMP(1, __builtin_amdgcn_s_memtime());
    if (!FAST && !a.do_qt) {
        if (a.do_step)
            for (int s = 0; s < a.nsub; ++s) drift(p, v, s);
    } else {
        // Software-pipelined substeps: once substep s has its kick, the drift of substep s + 1
        // and the sin / cos of its coupling phase (:508) depend on nothing else of substep s, so
        // they are evaluated before s's Runge-Kutta stages and overlap them.  Same operations on
        // the same values as the plain order: bit-identical.
        if (FAST || a.do_step) drift(p, v, 0);
        double pre_p = p, pre_v = v;                  // FAST: the state after the last substep
        double sn, cs;
        // (EDZ: every expDet of the launch is 0 — fracOfSig = 0, the default — so u = vx pv2q: the
        // + 0 and its LDS read dropped; the same values up to the sign of an exact zero)
        double u = EDZ ? v * pv2q_v : v * pv2q_v + edt[0];     // vx on every state lane (carried: the
        double tn = tPart + dtq_v;                    // next substep's is formed with its phase); tn:
        sincos_q2((u * cphi) * tn, sct, sn, cs);      // the next substep's tPart, formed once
        // Wave-uniform bound on every coupling phase of the launch (production instance): |v| grows
        // by at most |dt f| + kickmax per substep and tPart by dtQ, so when the bound on |phi| is
        // below 2^19 the per-substep |phi| >= 2^20 library fallback cannot trigger and is left out
        // of the loop (it would split every substep's tail from the next one's head into separate
        // basic blocks); otherwise the loop keeps it.  The same values either way.
        bool phase_small = false;
        if constexpr (FAST && EDZ && DPPX) {
            const double vb = fabs(v) + (double)(a.nsub + 1) * (fabs(dt * f) + qc.kickmax);
            const double tb = fabs(tPart) + (double)(a.nsub + 1) * dtq_v;
            const double pb = ((vb * fabs(pv2q_v)) * fabs(cphi)) * tb;
            phase_small = __builtin_amdgcn_ballot_w64(!(pb < 524288.)) == 0;
        }
        auto substep = [&](int s, auto chk) {
            tPart = tn;                               // tPart += dtQ (formed in the last next_phase)
            const double dp = DPPX ? lane_sum_p8(nrm2(w) * hdp, one) : lane_sum_p(nrm2(w) * hdp);
            const double u1 = su[grp][s][0], u2 = su[grp][s][1];
            cxd w0, w1, w2;
            exchange(w, w0, w1, w2);
            double kick;
            const bool nojump = u1 > dp;
            QT_JCOUNT(!nojump);
            // substep s + 1's drift and phase, placed in the same basic block as the work they
            // overlap (straight-line: the last substep computes a harmless extra value, the
            // |phi| >= 2^20 library fallback is applied afterwards)
            double vn, pn, un, phin, snn, csn;
            auto next_phase = [&]() {
                vn = fma(kmask, kick, v);             // :705 (x lanes)
                pn = p;
                const int s1 = s + 1 < a.nsub ? s + 1 : s;
                double pd = pn, vd = vn;
                drift(pd, vd, s1);
                if constexpr (FAST) {                 // always advance; the launch keeps the state
                    pre_p = pn;                       // before the last substep's extra drift
                    pre_v = vn;
                    pn = pd;
                    vn = vd;
                } else {
                    const bool adv = a.do_step && s + 1 < a.nsub;   // no drift after the last substep
                    pn = adv ? pd : pn;
                    vn = adv ? vd : vn;
                }
                un = EDZ ? vn * pv2q_v : vn * pv2q_v + edt[s1];
                tn = tPart + dtq_v;
                phin = (un * cphi) * tn;
                sincos_tab(phin, sct, snn, csn);
            };
            // the no-jump substep's kick (the kick terms on the P lanes, host table) and its four
            // Runge-Kutta stages: w after the substep
            auto rk_kick = [&]() {
                const double kt = kick_term(w, w0, w1, w2, kw0, kw1, kw2);
                return DPPX ? lane_sum_p8(kt, one) : lane_sum_p(kt);
            };
            auto rk_stages = [&]() {
                const cxd md = {mre, fma(mi1, u, mi0)};
                const cxd c2 = {fma(dms, sn, c2re), fma(dmc, cs, c2im)};
                cxd y = w, acc = {0., 0.};
                cxd y0 = w0, y1 = w1, y2 = w2;
#pragma unroll
                for (int stg = 0; stg < 4; ++stg) {
                    double dpy = dp;
                    if (stg > 0) {
                        dpy = DPPX ? lane_sum_p8(nrm2(y) * hdp, one) : lane_sum_p(nrm2(y) * hdp);
                        exchange(y, y0, y1, y2);
                    }
                    const double pref = rsq_nr(1. - dpy);
                    const cxd ws = IM01 ? row_r_im01(md, y, c0.im, y0, c1.im, y1, c2, y2)
                                        : row_r(md, y, c0, y0, c1, y1, c2, y2);
                    const cxd d = {fma(pref, ws.re, -y.re), fma(pref, ws.im, -y.im)};
                    if (stg == 0) acc = d;
                    else if (stg < 3) acc = {fma(3., d.re, acc.re), fma(3., d.im, acc.im)};
                    else acc = {acc.re + d.re, acc.im + d.im};
                    if (stg < 2) y = {fma(0.5, d.re, w.re), fma(0.5, d.im, w.im)};
                    else if (stg == 2) y = {w.re + d.re, w.im + d.im};
                }
                return cxd{fma(0.125, acc.re, w.re), fma(0.125, acc.im, w.im)};
            };
            // the quantum jump (:573-703) of w: the state it lands on and its kick.  TAPE: the
            // uniforms of the drand48 tape (a.U), else Philox
            auto jump = [&](auto tape, double& jkick) {
                const double nk = sq(w);
                double n3, n4, n5, n6;                    // |w|^2 of the P states 2..5
                if constexpr (DPPX) {
                    n3 = dpp<BCAST(0)>(nk); n4 = dpp<BCAST(4)>(nk); n5 = dpp<BCAST(3)>(nk); n6 = dpp<BCAST(7)>(nk);
                } else {
                    n3 = dpp<BCAST(2)>(nk); n4 = dpp<BCAST(3)>(nk); n5 = dpp<BCAST(4)>(nk); n6 = dpp<BCAST(5)>(nk);
                }
                double randDOrS, randDir, rand3, dummy;
                if constexpr (decltype(tape)::value) {
                    draw_pair(qc, a.U, S, i, gid, a.q0 + (uint64_t)s, 1, randDOrS, randDir);
                    draw_pair(qc, a.U, S, i, gid, a.q0 + (uint64_t)s, 2, rand3, dummy);
                    (void)dummy;
                } else {                              // both pairs in one Philox evaluation: lanes 0-7
                    double x0, x1;                    // draw pair 1, lanes 8-15 pair 2 (the whole
                    philox_pair(qc, gid, a.q0 + (uint64_t)s, k < 8 ? 1 : 2, x0, x1);   // group is active)
                    randDOrS = dpp<BCAST(0)>(x0);
                    randDir = dpp<BCAST(0)>(x1);
                    rand3 = dpp<BCAST(8)>(x0);
                }
                return (DPPX || qc.model == 0)            // DPPX: model 0
                           ? jump_target(qc, n3, n4, n5, n6, u2, randDOrS, randDir, rand3, jkick)
                           : jump_target_pump(qc, n3, n4, n5, n6, u2, randDOrS, randDir, rand3, jkick);
            };
            if constexpr (JUNI) {
            // A wave-uniform choice.  No ion of the wave jumps (the common case): the no-jump substep,
            // one basic block with the pipelined next_phase().  Some ion jumps: every lane runs ONE
            // straight-line block — the Runge-Kutta stages (kept by the ions that do not jump), the
            // jump's draws and target (kept by those that do), per-lane selects, and one next_phase()
            // on the selected kick — instead of both sides of a per-lane branch, each with its own
            // next_phase().  A lane's values come from the same operations on the same operands
            // either way (an ion's 16 lanes jump together, and every cross-lane move stays inside
            // them): bit-identical to the per-lane branch.
            auto jump_substep = [&](auto tape) {
                const double kick_rk = rk_kick();
                const cxd w_rk = rk_stages();
                double kick_j;
                const int target = jump(tape, kick_j);
                w = {nojump ? w_rk.re : (st == target ? 1. : 0.), nojump ? w_rk.im : 0.};
                kick = nojump ? kick_rk : kick_j;
                tPart = nojump ? tPart : 0.;
                next_phase();
            };
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!nojump) == 0, 1)) {
                kick = rk_kick();
                next_phase();
                w = rk_stages();
            } else if (a.U) {
                jump_substep(std::true_type{});
            } else {
                jump_substep(std::false_type{});
            }
            } else if (nojump) {                      // the per-lane branch, whose two sides a wave with a jumping
                kick = rk_kick();                     // ion executes one after the other
                next_phase();
                w = rk_stages();
            } else {                                  // quantum jump (:573-703)
                tPart = 0;
                int target;
                if (a.U) target = jump(std::true_type{}, kick);
                else target = jump(std::false_type{}, kick);
                w = {st == target ? 1. : 0., 0.};
                next_phase();
            }
            if constexpr (decltype(chk)::value)
                if (!(fabs(phin) < 1048576.)) sincos(phin, &snn, &csn);
            if (!NORN && qc.renorm) w = [&] {             // :706-712
                const double r = rsq_nr(lane_norm16(nrm2(w), one));
                return cxd{w.re * r, w.im * r};
            }();
            v = vn;
            p = pn;
            u = un;
            sn = snn;
            cs = csn;
        };
        auto loop = [&](auto chk) {
            int s = 0;                                // two substeps per iteration (register copies)
            for (; s + 1 < a.nsub; s += 2) {
                substep(s, chk);
                substep(s + 1, chk);
            }
            if (s < a.nsub) substep(s, chk);
        };
        if (phase_small) loop(std::false_type{});
        else loop(std::true_type{});
        if constexpr (FAST) {
            p = pre_p;
            v = pre_v;
        }
    }
    QT_STAMP(2, __builtin_amdgcn_s_memtime());
    if (store) {
        if (owner) {
            qt_store(&a.R[(size_t)c * S + i], p);
            qt_store(&a.V[(size_t)c * S + i], v);
            if (!(p >= -0.125 * L && p <= 1.125 * L)) *a.oor = 1;
        }
        if (FAST || a.do_qt) {
            if (k == 0) qt_store(&a.tPart[i], tPart);
            if (st < NS) {
                qt_store(&a.psi[(size_t)(2 * st) * S + i], w.re);
                qt_store(&a.psi[(size_t)(2 * st + 1) * S + i], w.im);
            }
        }
    }
#if defined(MDQT_EXPT_QTSTAMPS)
    __builtin_amdgcn_s_waitcnt(0);
    st_[3] = __builtin_amdgcn_s_memtime();
    st_[5] = __builtin_amdgcn_s_memrealtime();
    const int wv = (int)(blk * (kLaneWG / 64) + (threadIdx.x >> 6));
    if ((threadIdx.x & 63) < 16 && wv < 4096) {             // vector stores, one slot per lane
        const int q = threadIdx.x & 63;
        unsigned long long v = st_[0];
#pragma unroll
        for (int m = 1; m < 16; ++m) v = (q == m) ? st_[m] : v;
        g_qt_stamps[16 * wv + q] = v;
    }
#endif
}

}  // namespace mdqt
#endif  // __HIP__

namespace mdqt {

// ------------------------------------------------------------------------------------------
// Host: the lane_substeps instance of a launch with the block `a` (every launcher of the lane kernels:
// launch_substeps_r's mode 2, launch_substeps_r_ens, launch_substeps_r_sweep, launch_substeps_pump_ens), and
// beside it what that choice reads.  A sweep launch runs ONE instance for members with different parameters, so
// it is issued only where sweep_choice_differs finds no difference between the members' blocks.  CHANGE THE TWO
// TOGETHER: lane_qt_instance may read nothing of `a` that sweep_choice_differs does not compare.
// ------------------------------------------------------------------------------------------
inline QTKernel lane_qt_instance(const SubstepArgs& a) {
    const uint64_t all = (1ull << a.nsub) - 1;
    const bool allmove = a.do_step && a.do_qt && a.nseg >= 1 && !a.arrive && (a.movmask & all) == all;
    if (a.qc.model != 0) return allmove ? QTK_LANES_R_PUMP_FAST : QTK_LANES_R_PUMP;
    if (!allmove) return QTK_LANES_R;
    if (!a.qc.im01) return QTK_LANES_R_FAST;
    if (!a.expdet_zero) return QTK_LANES_IM;
    return a.qc.renorm ? QTK_LANES_IM_EDZ_RN : QTK_LANES_IM_EDZ;   // (without renormalisation: the production launch)
}
// the first of what the choice reads in which b differs from a (nullptr: none)
inline const char* sweep_choice_differs(const SubstepArgs& a, const SubstepArgs& b) {
    if (a.nsub != b.nsub) return "nsub";
    if (a.do_step != b.do_step) return "do_step";
    if (a.do_qt != b.do_qt) return "do_qt";
    if (a.movmask != b.movmask) return "movmask (t > 0 per substep)";
    if (a.expdet_zero != b.expdet_zero) return "expdet_zero (fracOfSig == 0 against != 0)";
    if (a.qc.im01 != b.qc.im01) return "qt_im01";
    if (a.qc.renorm != b.qc.renorm) return "reNormalizewvFns";
    if (a.qc.model != b.qc.model) return "qt_model";
    if ((a.nseg >= 1) != (b.nseg >= 1)) return "nseg";
    if (!a.arrive != !b.arrive || !a.U != !b.U) return "arrive / U (another launch scheme)";
    return nullptr;
}

}  // namespace mdqt
