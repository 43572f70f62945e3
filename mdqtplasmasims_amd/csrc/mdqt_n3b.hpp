// What the files of the Newton-3 block scheme share: the block kernels (mdqt_n3b.hip) and the scheme's
// plan, census and tail kernels (mdqt_n3b_plan.hip) classify a tile pair with the same device
// functions, in the same operations, so that the plan, the census and the on-the-fly classification
// of an unplanned call agree bit for bit.
#pragma once
#include "mdqt_internal.hpp"
#include "mdqt_math.hpp"
#include "mdqt_n3b_args.hpp"

#include <math.h>

namespace mdqt {

constexpr int BW = kN3BBlock;                       // tiles per block = waves per workgroup
// the far levels that take the one-axis per-pair image (n3b_pack_class): bit x = far level x (1 mid, 2 far,
// 3 very far, 4 ultra far and its f32 level: the f64 ultra-far form, round 6)
constexpr unsigned kAx1Levels = 0x1E;
__device__ __forceinline__ double uniform_f64(double v) {   // a wave-uniform value into SGPRs
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__device__ __forceinline__ const double* tile_base(const double* Rall, int tile, int S) {
    const int g = tile * 64;                        // S is a multiple of 64: tiles never straddle slabs
    const int w = g / S;
    return Rall + (size_t)w * 3 * S + (g - w * S);
}

// Sub-tile groups (round 4).  The J tile sits in LDS by 16-ion sub-tiles, each twice over: J ion
// 16 b + m at LDS index 32 b + m and 32 b + 16 + m (n3b_lds).  Lane l = 16 a + m (I sub-tile a) runs a
// tile pair as four groups of 16 steps: group d pairs I sub-tile a with J sub-tile (a + d) & 3 — a
// cyclic diagonal of the 4 x 4 sub-block matrix — and at step t lane l meets J ion
// 16 ((a + d) & 3) + ((m + t) & 15) at LDS index 32 ((a + d) & 3) + m + t (immediate offsets t).  A
// group covers its four sub-blocks once, and at every step the 64 lanes meet 64 distinct J ions (the
// j-side ds_add_f64 stays conflict-free).  Group d runs iff bit d of `groups` (wave-uniform): a group
// whose four sub-blocks all have sub-tile boxes farther apart than the skip radius is skipped — the
// pairs of a tile pair that straddles the cutoff sphere (or the tail radius) by less than a whole
// tile pair (tools/subtile_cull_model.py).  The diagonal tile (I = J): group 0 with
// t = 1..8 (t = 8 for m < 8 only: each pair inside a sub-tile once), group 1, and group 2 for a < 2
// (the sub-tile pairs (0, 2), (1, 3) once); group 3 would repeat group 1's pairs.
__device__ __forceinline__ int n3b_lds(int l) { return 32 * (l >> 4) + (l & 15); }   // J ion l's first copy

// The lane index recomputed where it is used: two VALU (v_mbcnt) in volatile asm, which
// the compiler neither hoists nor merges — so no VGPR holds the lane index, or a value derived from it,
// across the block kernel's J-step loop (at its 80-VGPR budget such values were spilled and reloaded
// with a vmcnt(0) wait at every pair-form dispatch)
__device__ __forceinline__ int lane_opaque(int) {   // (the argument: the lane index it stands for)
    int r;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(r));
    return r;
}
// The class of tile pair (Iw, J) in spatial order (SpeedUp:222 keeps a pair only below r = L/2):
// returns the minimum-image multiples n_x, n_y, n_z of a uniform image and the class — skip when the
// boxes are farther apart than sqrt(r.rc2) (use_sort 1): -1 beyond L/2 (no pair inside the cutoff),
// -2 inside L/2 (the error-bounded tail: its pairs count in the tail sums) — else bit 0 = uniform
// image (FAST: the fast variant) + 2 x the far level (1 far, 2 very far, 3 ultra far, 4 ultra far in
// f32); g2 = the squared box gap.  Shared by k_pairs_n3b (the staging wave's lanes) and k_n3b_census.
struct N3BRadii { double rc2, rf2, rv2, ru2, ru32, rm2; };
// the squared radii of the classes: skip below the cutoff only for the forces (error-bounded tail,
// mdqt_engine.cpp tail_radius); the far forms are the fast force variant's
template <int VARIANT, bool POT>
__device__ __forceinline__ N3BRadii n3b_radii(const N3BArgs& a) {
    N3BRadii r;
    r.rc2 = POT ? a.Rcut * a.Rcut : a.Rskip * a.Rskip;
    r.rm2 = (POT || VARIANT != 1 || !(a.Rmid < a.Rcut)) ? INFINITY : a.Rmid * a.Rmid;
    r.rf2 = (POT || VARIANT != 1 || !(a.Rfar < a.Rcut)) ? INFINITY : a.Rfar * a.Rfar;
    r.rv2 = (POT || VARIANT != 1 || !(a.Rvfar < a.Rcut)) ? INFINITY : a.Rvfar * a.Rvfar;
    r.ru2 = (POT || VARIANT != 1 || !(a.Rufar < a.Rcut)) ? INFINITY : a.Rufar * a.Rufar;
    r.ru32 = (POT || VARIANT != 1 || !(a.Rufar32 < a.Rcut)) ? INFINITY : a.Rufar32 * a.Rufar32;
    return r;
}
// the far level of a squared gap: 0 exact, 1 mid, 2 far, 3 very far, 4 ultra far, 5 ultra far in f32
__device__ __forceinline__ int n3b_level(double g2, const N3BRadii& r) {
    return g2 > r.ru32 ? 5 : g2 > r.ru2 ? 4 : g2 > r.rv2 ? 3 : g2 > r.rf2 ? 2 : g2 > r.rm2 ? 1 : 0;
}
// strad (when asked): bit c = axis c's minimum-image multiple varies over the tile pair's pairs
// (the core on two box columns: Bi = box column of Iw, Bj = of J, row stride ld — global [12][T], or the
// plan's LDS copy of its workgroup's tiles; the same operations in the same order either way)
template <bool FAST>
__device__ __forceinline__ double4 n3b_classify_p(const double* Bi, const double* Bj, int ld, double L, double invL,
                                                  double Rcut, int use_sort, const N3BRadii& r, double& g2,
                                                  int* strad = nullptr) {
    g2 = 0.;
    bool uni = true;
    int sm = 0;
    double n[3];
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) {
        double d = Bi[c3 * ld] - Bj[c3 * ld];
        d = fma(-__builtin_rint(d * invL), L, d);
        const double gap = fabs(d) - (Bi[(3 + c3) * ld] + Bj[(3 + c3) * ld]);
        g2 = gap > 0. ? fma(gap, gap, g2) : g2;
        const double lo = Bi[(6 + c3) * ld] - Bj[(9 + c3) * ld];
        const double hi = Bi[(9 + c3) * ld] - Bj[(6 + c3) * ld];
        const double nlo = __builtin_rint(lo * invL), nhi = __builtin_rint(hi * invL);
        uni = uni && (nlo == nhi);
        sm |= (nlo == nhi ? 0 : 1) << c3;
        n[c3] = nlo;
    }
    if (strad) *strad = sm;
    const double cls = (use_sort == 1 && g2 > r.rc2) ? (g2 < Rcut * Rcut ? -2. : -1.)
                                                      : ((FAST && uni) ? 1. : 0.) + 2. * n3b_level(g2, r);
    return make_double4(n[0], n[1], n[2], cls);
}
template <bool FAST>
__device__ __forceinline__ double4 n3b_classify(const N3BArgs& a, double invL, const N3BRadii& r, int Iw, int J,
                                                double& g2, int* strad = nullptr) {
    return n3b_classify_p<FAST>(a.boxes + Iw, a.boxes + J, a.T, a.L, invL, a.Rcut, a.use_sort, r, g2, strad);
}

// the squared minimum-image gap between the boxes of 16-ion sub-tiles s and u ([6][T4] layout)
// (the core on two box columns Bs, Bu of row stride ld, as n3b_classify_p)
__device__ __forceinline__ double sub_gap2_p(const double* Bs, const double* Bu, int ld, double L, double invL) {
    double g2 = 0.;
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) {
        double d = Bs[c3 * ld] - Bu[c3 * ld];
        d = fma(-__builtin_rint(d * invL), L, d);
        const double gap = fabs(d) - (Bs[(3 + c3) * ld] + Bu[(3 + c3) * ld]);
        g2 = gap > 0. ? fma(gap, gap, g2) : g2;
    }
    return g2;
}
__device__ __forceinline__ double sub_gap2(const double* __restrict__ SB, int T4, int s, int u, double L,
                                           double invL) {
    return sub_gap2_p(SB + s, SB + u, T4, L, invL);
}
// the sub-blocks (a, (a + d) & 3) of sub-tile group d as bits 4 a + b
constexpr unsigned kGroupBits[4] = {0x8421u, 0x1842u, 0x2184u, 0x4218u};
// each group's far level from the sub-blocks beyond r_mid / r_far / r_vfar / r_ufar / r_ufar32 (bit
// 4 a + b): the highest level all four of its sub-blocks reach, 4 bits per group (k_n3b_census: the
// same levels as k_n3b_plan's least group gap, counted another way)
__host__ __device__ __forceinline__ unsigned sub_group_levels(unsigned mm, unsigned mf, unsigned mv, unsigned mu,
                                                              unsigned m32) {
    unsigned lv = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned g = kGroupBits[d];
        const unsigned x = (m32 & g) == g ? 5u : (mu & g) == g ? 4u : (mv & g) == g ? 3u : (mf & g) == g ? 2u
                         : (mm & g) == g ? 1u : 0u;
        lv |= x << (4 * d);
    }
    return lv;
}
// the groups of a staging word (n3b_stage_groups) that run in the pair form of far level x
__device__ __forceinline__ unsigned level_groups(unsigned word, int x) { return (word >> (4 + 4 * x)) & 15u; }
// the group mask of an off-diagonal tile pair from its 16 sub-block activities (bit 4 a + b: sub-tiles
// (a, b) closer than the skip radius): bit d = any sub-block (a, (a + d) & 3) active
__host__ __device__ __forceinline__ unsigned sub_groups_of(unsigned act16) {
    unsigned g = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int a = 0; a < 4; ++a) g |= ((act16 >> (4 * a + ((a + d) & 3))) & 1u) << d;
    return g;
}
// one pair's |F| bound at distance >= the gap d (g2 = d^2 > 0): g(d) = (1/d + 1/lDeb) e^(-d/lDeb) / d
// (SpeedUp:224 times r), the tail sums' term, as an upper bound in a few f32 operations: v_rsq_f32
// and v_exp_f32 (each within 2^-22 relative, tests/test_gpu_large.py), d^2 and the exponent's
// constant rounded to f32 (e^(-d/lDeb) within (d/lDeb) 2^-23 relative), the result x (1 + 2^-12):
// an upper bound while d/lDeb < 1000; beyond f32's range e^(-d/lDeb) flushes to 0 (< 1e-44)
__device__ __forceinline__ double tail_g(double g2, float invl, float cf) {
    const float s = (float)g2;
    const float ri = __builtin_amdgcn_rsqf(s);
    const float e = __builtin_amdgcn_exp2f((s * ri) * cf);
    return (double)(((ri + invl) * e) * ri) * (1. + 0x1p-12);
}
// force_form_mode 1: the bound on the error of one pair term at distance >= the gap d (g2 = d^2) in the
// pair form of level e >= 1: g(d) err_e(d) = g(d) (kFormErrA[e] d/lDeb + kFormErrB[e]) — both factors as
// upper bounds in f32 (tail_g's; d/lDeb within 3 2^-23), the product x (1 + 2^-10).  g err_e decreases
// in d for every form (its log-derivative is below 1/(1 + x) - 1/x - 1 < 0, x = d/lDeb), so each of the
// sub-block's pairs (distance >= its gap) is bounded by it.
// (the constants rounded up to f32; the whole term in f32 — f32 VALU issues at twice the f64 rate — and
// x (1 + 2^-10) covers every rounding: tail_g's 2^-12 bound, d/lDeb's 3 2^-23, the err factor's and the
// product's 2^-23 each)
__constant__ const float kFormA[6] = {(float)kFormErrA[0], (float)(kFormErrA[1] * (1. + 0x1p-20)),
                                      (float)kFormErrA[2], (float)(kFormErrA[3] * (1. + 0x1p-20)),
                                      (float)(kFormErrA[4] * (1. + 0x1p-20)), (float)(kFormErrA[5] * (1. + 0x1p-20))};
__constant__ const float kFormB[6] = {(float)kFormErrB[0], (float)(kFormErrB[1] * (1. + 0x1p-20)),
                                      (float)(kFormErrB[2] * (1. + 0x1p-20)), (float)(kFormErrB[3] * (1. + 0x1p-20)),
                                      (float)(kFormErrB[4] * (1. + 0x1p-20)), (float)(kFormErrB[5] * (1. + 0x1p-20))};
__device__ __forceinline__ double form_term(double g2, float invl, float cf, int e) {
    const float s = (float)g2;
    const float ri = __builtin_amdgcn_rsqf(s);
    const float r = s * ri;
    const float ex = __builtin_amdgcn_exp2f(r * cf);
    const float g = ((ri + invl) * ex) * ri;
    return (double)(g * fmaf(r * invl, kFormA[e], kFormB[e])) * (1. + 0x1p-10);
}
// force_form_mode 1: an upper bound on the squared distance of any pair of boxes s and u in the minimum
// image — a uniform-image tile pair's pairs are each at their minimum image in the block kernel (its shift
// is every pair's rint(dx / L)), and per axis min_k |x_i - x_j - k L| <= |mi(c_s - c_u)| + h_s + h_u, whatever
// frame the boxes' centres were taken in (a box is the min / max about its first ion, k_tile_boxes)
__device__ __forceinline__ double sub_far2_p(const double* Bs, const double* Bu, int ld, double L, double invL) {
    double f2 = 0.;
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) {
        double d = Bs[c3 * ld] - Bu[c3 * ld];
        d = fma(-__builtin_rint(d * invL), L, d);
        const double f = fabs(d) + (Bs[(3 + c3) * ld] + Bu[(3 + c3) * ld]);
        f2 = fma(f, f, f2);
    }
    return f2;
}
__device__ __forceinline__ double sub_far2(const double* __restrict__ SB, int T4, int s, int u, double L, double invL) {
    return sub_far2_p(SB + s, SB + u, T4, L, invL);
}
// a tile pair's class and uniform-image multiples in one LDS word: bits 0-3 class + 2, 4-11 / 12-19 /
// 20-27 n_x, n_y, n_z (signed); a uniform image with a multiple beyond +-127 (positions that far
// outside the box) is taken per pair instead.  A per-pair image that varies on ONE axis only (strad:
// n3b_classify's mask; FAST) carries that axis + 1 in bits 28-29 and the other two axes' multiples
// (the varying axis's field 0): the block kernel then takes the minimum image per pair on that axis
// alone (the tile pairs that straddle the image boundary, ~97 % of the per-pair-image ones, C3/C5)
__device__ __forceinline__ int n3b_pack_class(double4 t4, int strad = 0) {
    int cls = (int)t4.w;
    const bool uni = cls >= 0 && (cls & 1);
    if (uni && !(fabs(t4.x) <= 127. && fabs(t4.y) <= 127. && fabs(t4.z) <= 127.)) cls -= 1;
    const bool u2 = cls >= 0 && (cls & 1);
    const int ax1 = strad == 1 ? 1 : strad == 2 ? 2 : strad == 4 ? 3 : 0;
    const bool one = cls >= 0 && !(cls & 1) && ax1 &&
                     fabs(t4.x) <= 127. && fabs(t4.y) <= 127. && fabs(t4.z) <= 127.;
    const int nx = (u2 || (one && ax1 != 1)) ? (int)t4.x : 0, ny = (u2 || (one && ax1 != 2)) ? (int)t4.y : 0,
              nz = (u2 || (one && ax1 != 3)) ? (int)t4.z : 0;
    return (cls + 2) | ((nx & 255) << 4) | ((ny & 255) << 12) | ((nz & 255) << 20) | ((one ? ax1 : 0) << 28);
}
// real ions of 16-ion sub-tile s (0 for the padding of the ragged last tile)
__device__ __forceinline__ double sub_count(int N, int s) { return (double)max(0, min(16, N - 16 * s)); }
// tile J's raw box (the exact min / max of its coordinates, boxes [6, 12)): its squared half-diagonal —
// the f32 ultra-far form (n3b_group_uf32) stages J relative to J's first ion and takes a sub-tile group
// only where the box diagonal (twice this) is within the group's gap (kUfar32A/B's premise)
__device__ __forceinline__ double raw_half2_p(const double* Bj, int ld) {
    double h2 = 0.;
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) {
        const double h = 0.5 * (Bj[(9 + c3) * ld] - Bj[(6 + c3) * ld]);
        h2 = fma(h, h, h2);
    }
    return h2;
}
__device__ __forceinline__ double raw_half2(const double* B, int T, int J) { return raw_half2_p(B + J, T); }
// a sub-tile group's estimated VALU instructions per lane (16 steps; the pairing's weights per wave-step of
// each pair form — exact, mid, far, very far, ultra far, f32 ultra far — uniform image / per-pair image; the
// ragged tile's exact form)
__device__ __forceinline__ unsigned n3b_pair_cost(int level, bool uni, bool rag) {
    constexpr unsigned wu[6] = {39u, 36u, 31u, 27u, 25u, 9u}, wi[6] = {48u, 44u, 38u, 32u, 32u, 32u};
    return 16u * (rag ? 52u : uni ? wu[level] : wi[level]);
}
// the AXP instance where tile pairs whose image varies on one axis can be evaluated: their pairs are >=
// L/2 - (the two tiles' extents) apart on that axis, so only when the skip radius reaches within two tile
// widths (L (64/N)^(1/3)) of L/2 (C3, C5: r_s = L/2; not N = 1M, r_s = 61 < 80.6 - 12.9).  A function of
// the call's parameters alone: every rank of a sharded run, and every call of one configuration, takes
// the same kernel.
__host__ __device__ static bool n3b_axp(const N3BArgs& a) {
    return a.ax1 && a.use_sort != 0 && a.Rskip > 0.5 * a.L - 2. * a.L * cbrt(64. / a.N);
}
// the half-covered block distance: with an even number of blocks NB, block distance NB / 2 joins every
// block pair {P, P + NB / 2} from both sides; the blocks P < NB / 2 take it, for the others it is skipped
__host__ __device__ __forceinline__ bool n3b_half_covered(int NB, int P, int db) {
    return !(NB & 1) && db == NB / 2 && P >= NB / 2;
}

// the plan (k_n3b_plan, mdqt_n3b_plan.hip) of a force or potential call in spatial order, its per-J-tile
// masks zeroed first: launch_forces_n3b and launch_potential_n3b run it ahead of the block kernel
hipError_t launch_n3b_plan(const N3BArgs& a, int variant, hipStream_t s);

}  // namespace mdqt
