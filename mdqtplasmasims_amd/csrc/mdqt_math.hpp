// Device math of the pair forms (1/sqrt and the Yukawa factor at each precision tier, with the error constants
// the force plan builds its bounds from) and the canonical sums of force partials.  Included by the device
// headers that evaluate them and by mdqt_force_plan.cpp for the constants.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mdqt {

// 1/sqrt(x): v_rsq_f64 (2^-24 relative on gfx950, tools/rsq_precision.hip) refined by one
// third-order step r (1 + e/2 + 3e^2/8), e = 1 - x r^2: 1.7e-16 max relative error measured
// (two Newton steps: 2.4e-16) in 5 dependent operations instead of 7.  tests/test_gpu_device_math.py
// holds it to 2 x 2^-53 relative on [2^-20, 2^20] and on (0.9, 1] (the budget of tests/force_truth.py and
// tests/qt_truth.py); measured there 1.49 x 2^-53 = 1.66e-16
__device__ __forceinline__ double rsq3(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double q = __builtin_amdgcn_rsq(x);
#else
    const double q = 1. / sqrt(x);                 // host parse of device code only
#endif
    const double e = fma(-x, q * q, 1.0);
    return fma(q * e, fma(e, 0.375, 0.5), q);
}

// e^x for x = -r/lDeb in [-L/(2 lDeb), 0] (no overflow, no subnormal results for any box the
// reference runs): Cody-Waite x = n ln2 + r, |r| <= ln2/2, then the degree-11 minimax polynomial
// of e^r on [-ln2/2, ln2/2] (relative approximation error 3.1e-18; Remez exchange in 60-digit
// arithmetic, coefficients rounded to double) in FMA Horner form, exponent shift: <= 1.1 ulp vs
// the exact value over the range (two FMAs fewer per pair than a degree-13 Taylor polynomial); 0.95 ulp
// measured on [-40, 0] (tests/test_gpu_device_math.py).
__device__ __forceinline__ double exp_neg(double x) {
    const double n = __builtin_rint(x * 1.4426950408889634);
    double r = fma(-n, 0x1.62e42fefa39efp-1, x);
    r = fma(-n, 0x1.abc9e3b39803fp-56, r);
    double p = 2.4994304884817207e-08;
    p = fma(p, r, 2.7632293279459877e-07);
    p = fma(p, r, 2.7557622530872255e-06);
    p = fma(p, r, 2.4801486521427463e-05);
    p = fma(p, r, 0.00019841269432679237);
    p = fma(p, r, 0.0013888888951223987);
    p = fma(p, r, 0.00833333333355927);
    p = fma(p, r, 0.04166666666649277);
    p = fma(p, r, 0.1666666666666617);
    p = fma(p, r, 0.5000000000000018);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

// 2^t for t = -(r/lDeb) log2(e) <= 0 (the pair kernels' Yukawa factor e^(-r/lDeb) = 2^t, t formed
// as r * (-log2(e)/lDeb)): n = rint(t), f = t - n exactly (|f| <= 1/2, no reduction constant to
// round), then the degree-11 minimax-type polynomial of 2^f on [-1/2, 1/2] (Chebyshev fit in
// 50-digit arithmetic, coefficients rounded to double; <= 1.14 ulp with double FMA Horner),
// exponent shift.  Two operations fewer than exp_neg's Cody-Waite form; the only rounding before
// the polynomial is t's own, the same size as x = -r/lDeb's in exp_neg.
__device__ __forceinline__ double exp2_neg(double t) {
    const double n = __builtin_rint(t);
    const double f = t - n;
    double p = 0x1.e9ec1fcb69a7fp-32;
    p = fma(p, f, 0x1.e6228acd1c6e5p-28);
    p = fma(p, f, 0x1.b524ebd13a55fp-24);
    p = fma(p, f, 0x1.62bfc2c86d700p-20);
    p = fma(p, f, 0x1.ffcbfc6da6ed1p-17);
    p = fma(p, f, 0x1.430913112c61bp-13);
    p = fma(p, f, 0x1.5d87fe78a3f9cp-10);
    p = fma(p, f, 0x1.3b2ab6fb9f1a5p-7);
    p = fma(p, f, 0x1.c6b08d704a0c6p-5);
    p = fma(p, f, 0x1.ebfbdff82c5aep-3);
    p = fma(p, f, 0x1.62e42fefa39efp-1);
    p = fma(p, f, 1.0);
    return ldexp(p, (int)n);
}
constexpr double kNegLog2e = -1.4426950408889634;   // -log2(e)

// Far tile pairs of the Newton-3 blocks (box gap >= the far radius, mdqt_force_plan.cpp far_radius_l):
// every pair term there is below g(r_far), so a term error of relative size kFarRelErr is below
// g(r_far) kFarRelErr and an ion's force moves by at most (N - 1) g(r_far) kFarRelErr (<= 1e-13 by
// the choice of r_far).  Their pair form: rsq1 (v_rsq_f64 + ONE Newton step: 1e-14 relative) and
// 2^f by a degree-6 Chebyshev fit on [-1/2, 1/2] (2.6e-9 relative in double Horner, mpmath fit,
// measured on 4,001 points) — 6 operations fewer per pair than the exact form.
constexpr double kFarRelErr = 3e-9;
// The mid tier (round 4, sub-tile groups >= r_mid apart): rsq1 — relative error 1.5 e^2 + 2u for the
// raw rsq's e <= kRsqRawErr: <= kRsq1RelErr — and 2^t by the 64-entry table with a degree-4 series
// (2.53e-15 measured, + the table entry's and the product's rounding: kTab4RelErr).  t carries ri's
// error times r/lDeb, the force factor 3 ri's: a term is within (r/lDeb + 3)(kRsq1RelErr + 2^-52) +
// kTab4RelErr of itself (mdqt_force_plan.cpp far_err, level 5).
constexpr double kRsq1RelErr = 2.2e-14;
// 2^t of the exact (and mid) pair forms by the 64-entry LDS table (mdqt_pairs.hpp exp2_neg_cut_tab)
// (A/B round 4 against the polynomial 2^t, plan-based block kernel: C3 -3.5 %, C5 -0.8 %, N = 1M +0.3 %; round 3:
// C2 MD step -0.2 us)
constexpr double kTab4RelErr = 4e-15;
__device__ __forceinline__ double rsq1(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double q = __builtin_amdgcn_rsq(x);
#else
    const double q = 1. / sqrt(x);
#endif
    const double e = fma(-x, q * q, 1.0);
    return fma(0.5 * q, e, q);
}
// The very-far tier (box gap >= r_vfar): the raw v_rsq_f64 (relative error <= kRsqRawErr: measured
// 2^-24 by tools/rsq_precision.hip over r^2 in [1e-4, 1e6], checked by a GPU test; twice that here)
// and a degree-5 fit of 2^f (1.02e-7 relative).  A term at distance r is then within
// ((r/lDeb + 3) kRsqRawErr + kExp5RelErr) of itself relatively — r/lDeb from t = r log2(e)/lDeb
// carrying ri's error into 2^t, 3 from ri^3 — and g(r) times that factor decreases in r, so
// (N - 1) g(r_vfar) ((r_vfar/lDeb + 3) kRsqRawErr + kExp5RelErr) bounds every ion (far_radius).
constexpr double kRsqRawErr = 0x1p-23;
constexpr double kExp5RelErr = 1.1e-7;
// The ultra-far tier (box gap >= r_ufar): the raw v_rsq_f64 and 2^t by v_exp_f32 on t rounded to
// float (relative 2^-24): a term is within (r/lDeb) (kRsqRawErr + 2^-24) + 3 kRsqRawErr +
// kExp2fRelErr of itself (kExp2fRelErr: twice what tools/exp2f_precision measures, re-checked by a
// GPU test).  f32's range holds 2^t down to t = -126: r <= 87 lDeb, beyond every L/2 it serves.
constexpr double kExp2fRelErr = 0x1p-22;
// The ultra-far tier in f32 (round 3; round 5: relative to J's first ion, packed): a
// uniform-image tile pair's sub-tile group whose sub-boxes are >= r_ufar32 apart — and whose gap g is
// at least the J tile's raw box diagonal D (k_n3b_plan) — evaluates its pair terms in f32: the J tile
// staged as fl32(xj - c_J), c_J its first ion, the lane's ion as fl32(xi - n L - c_J), dx their f32
// difference; r^2 by f32 FMAs, v_rsq_f32 (<= kRsqF32RelErr = 1 ulp, measured by tools/rsq_precision
// and a GPU test), t = (r^2 ri) cf with cf = fl32(-log2(e)/lDeb), v_exp_f32, then the force factor and
// the three products in f32; the i side summed in two f32 partials of 8 steps, then in f64; the j side
// rotated along the wave over the 16 steps (one ds_add_f64 per component).  With u = 2^-24, per axis
// |ddx| <= u (|xi - n L - c_J| + |xj - c_J| + |dx|), and |xi - n L - c_J| <= r + D, |xj - c_J| <= D, so
// |ddx| <= u (2 r + 2 D) <= 4 u r as a vector (D <= g <= r).  To first order: r^2 8u + 3u = 11u,
// ri 5.5u + 2u = 7.5u, r 19.5u, t 21.5u — so 2^t is within (r/lDeb) 21.5u + kExp2fRelErr — the force
// factor ((ri + invl) 9.5u, times 2^t 1u, ri^2 16u, product 1u) 27.5u more, the product with dx 5u;
// each 16-term f32 sum adds 15u: a term is within (r/lDeb) 22u + 52u of itself (kUfar32A, kUfar32B,
// rounded up).  The cutoff is decided on the f32 r^2 (<= 11u off): pairs within 6u Rcut of L/2 may
// land on either side, each at most g(Rcut (1 - 2^-20)) — so far_radius_l's level 4 bounds every ion
// by (N - 1) g(r) err(r) + (N - 1) g(Rcut (1 - 2^-20)), and the tier is off where that cannot meet
// 10^-k (C5: N g(L/2) is ~1e-8; N = 1e6 at C2's parameters: ~5e-16).  force_form_mode 1 (round 6) has
// no such term: the plan gives a group the f32 form only if its far distance is below Rcut (1 - 2^-20)
// (N3BArgs::u32lim2), so its f32 r^2 never decides a cutoff.
constexpr double kRsqF32RelErr = 0x1p-23;
constexpr double kUfar32A = 22. * 0x1p-24;
constexpr double kUfar32B = 52. * 0x1p-24;
// a term's relative error in the pair form of plan level e (0 exact, 1 mid, 2 far, 3 very far, 4 ultra
// far, 5 ultra far in f32) as kFormErrA[e] r/lDeb + kFormErrB[e] (mdqt_force_plan.cpp far_err; the measured
// form bound of k_n3b_plan, force_form_mode 1)
constexpr double kFormErrA[6] = {0., kRsq1RelErr + 0x1p-52, 0., kRsqRawErr, kRsqRawErr + 0x1p-24, kUfar32A};
constexpr double kFormErrB[6] = {0., 3. * (kRsq1RelErr + 0x1p-52) + kTab4RelErr, kFarRelErr,
                                 3. * kRsqRawErr + kExp5RelErr, 3. * kRsqRawErr + kExp2fRelErr, kUfar32B};
__device__ __forceinline__ double exp2_neg_cut5(double t, bool keep) {
    const double n = __builtin_rint(t);
    const double f = t - n;
    double p = 0x1.5f0890162a90ap-10;
    p = fma(p, f, 0x1.3d10705276a1dp-7);
    p = fma(p, f, 0x1.c6af6cdbbdcc7p-5);
    p = fma(p, f, 0x1.ebf906e26e833p-3);
    p = fma(p, f, 0x1.62e4302fc626ep-1);
    p = fma(p, f, 0x1.0000014413897p+0);
    return ldexp(p, keep ? (int)n : -1100);
}
__device__ __forceinline__ double exp2_neg_cut6(double t, bool keep) {
    const double n = __builtin_rint(t);
    const double f = t - n;
    double p = 0x1.443fffc90db59p-13;
    p = fma(p, f, 0x1.5f48c04f62e50p-10);
    p = fma(p, f, 0x1.3b2a1b7152befp-7);
    p = fma(p, f, 0x1.c6aecc669b6ddp-5);
    p = fma(p, f, 0x1.ebfbe045f4d3cp-3);
    p = fma(p, f, 0x1.62e430d034702p-1);
    p = fma(p, f, 1.0);
    return ldexp(p, keep ? (int)n : -1100);
}

// Canonical sum of nseg partials p[0], p[stride], ... : eight interleaved accumulators
// (partial s goes to s % 8, ascending) combined as ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)).  One
// fixed order wherever it is evaluated (deterministic); independent loads, short chains.
__device__ __forceinline__ double seg_sum(const double* __restrict__ p, size_t stride, int nseg) {
    double a[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    int s = 0;
    for (; s + 8 <= nseg; s += 8) {
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] += p[(size_t)(s + q) * stride];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (s + q < nseg) a[q] += p[(size_t)(s + q) * stride];
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// THE canonical sum of the nseg force partials of one ion component (MDQT engine): sixteen
// strided partial sums, q_k = (((0 + p[k]) + p[k + 16]) + p[k + 32]) + ... (k = 0..15, the
// slots < nseg), combined by the lane kernel's DPP tree
//   (((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7))) + (((q8 + q9) + ...) + ((q12 + q13) + (q14 + q15))).
// The lane-per-state QT kernel evaluates it distributed over an ion's 16 lanes (lane k: q_k, all
// of its loads in flight at once), the thread-per-ion kernels and k_reduce_segments serially:
// the same operations, so every consumer of the partials sees the same F bit for bit.
__device__ __forceinline__ double slot_sum16_partial(const double* __restrict__ p, size_t stride, int nseg, int k) {
    double q = 0.;
    for (int s = k; s < nseg; s += 16) q = q + p[(size_t)s * stride];
    return q;
}
__device__ __forceinline__ double tree16_sum(const double* q) {
    return (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) +
           (((q[8] + q[9]) + (q[10] + q[11])) + ((q[12] + q[13]) + (q[14] + q[15])));
}
__device__ __forceinline__ double slot_sum16(const double* __restrict__ p, size_t stride, int nseg) {
    double q[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) q[k] = slot_sum16_partial(p, stride, nseg, k);
    return tree16_sum(q);
}

}  // namespace mdqt
