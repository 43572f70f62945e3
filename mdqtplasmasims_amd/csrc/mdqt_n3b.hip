// gfx950 force kernels, Newton-3 over BLOCK pairs (large N, one GPU or sharded): forces() (SpeedUp:192-236)
// and the pair potential of Epotential() (SpeedUp:244-281).
//
//   k_pairs_n3b<VARIANT, GUARD, POT, AXP>      a workgroup of BW waves, one I tile of block P each
//   k_pairs_n3b_pw<VARIANT, GUARD, POT, AXP>   BW / 2 waves, two I tiles each (option force_n3b_pairs)
//   k_n3b_reduce                               canonical per-ion sum of the slots
//
// The variants are mdqt_forces.hip's; the call's plan, the census and the tail kernels are in
// mdqt_n3b_plan.hip, what they share with the kernels here in mdqt_n3b.hpp.
#include "mdqt_n3b.hpp"
#include "mdqt_pairs.hpp"

#include <type_traits>

namespace mdqt {

// ------------------------------------------------------------------------------------------
// Newton-3 over BLOCK pairs (large N, one GPU or sharded): blocks of BW tiles (kN3BBlock: 8, 512
// ions; 16 until round 4); a workgroup of BW waves holds block P (wave q: tile I = BW P + q in registers;
// k_pairs_n3b_pw: NWP = BW / 2 waves with two I tiles each) and walks the block distances db of its run,
// db in [0, NB/2] of the cyclic half shell (block Q = P + db mod NB; db = NB/2 only from P < NB/2 when NB
// is even, n3b_half_covered; db = 0: tile pairs I <= J).  For every J
// tile of Q all BW waves run their (I, J) rotation (64 steps; 32 on the diagonal tile) against
// the J tile in LDS with per-wave j accumulators, which are then combined in wave order and
// written to j-slot db (rows of J); each wave's i accumulator spans the whole run and goes to
// i-slot nd + run.  Slots: [nd + R][3][Npad], nd = NB/2 + 1 — O(N^2/1024) doubles, not O(N^2/64).
// The canonical per-ion sum (k_n3b_reduce) takes the j-slots in db order, then the i-slots in
// run order, skipping slots this rank does not write.
// ------------------------------------------------------------------------------------------
#if defined(MDQT_EXPT_CLS)
// diagnostic build only: tile-pair classes of k_pairs_n3b (skip, per pair, uniform image)
__device__ unsigned long long g_cls_count[3];
extern "C" int mdqt_expt_cls_count(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cls_count), sizeof(unsigned long long) * 3) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[3] = {0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_cls_count), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
// every 16 steps the LDS arrays are re-based at the lane's index (an opaque register), so the 16
// unrolled steps address them with immediate offsets t, 128 + t, 256 + t: without it the compiler's
// strength reduction moved the base past the arrays and spent a v_add_u32 per ds_add_f64 (3.5 VALU
// per pair, ~8 % of the block kernel's instructions)
#define N3B_REBASE(b0)                                                                     \
    int b_ = (b0);                                                                         \
    asm volatile("" : "+v"(b_));                                                           \
    const double (*pjb)[128] = (const double (*)[128])(&pj[0][0] + b_);                    \
    const double* mjb = mj + b_;                                                           \
    double *axb = ax + b_, *ayb = ay + b_, *azb = az + b_

// one sub-tile group: 16 rotation steps from LDS index b0 (the lane's first J ion) with weight w
template <int VARIANT, bool GUARD, bool RAGGED, bool SHIFT = false, bool CUT = VARIANT == 1,
          bool POT = false, int FAR = 0, int NSTEP = 16, int MAX = -1>
__device__ __forceinline__ void n3b_group(int b0, double w, double xi, double yi, double zi, double mi,
                                          const double (*pj)[128], const double* mj, double* ax, double* ay,
                                          double* az, double& fx, double& fy, double& fz, const PairC& c,
                                          double w_last = 1.) {
    N3B_REBASE(b0);
#pragma unroll
    for (int t = 0; t < NSTEP; ++t)
        n3_step<VARIANT, GUARD, RAGGED, SHIFT, CUT, POT, FAR, MAX>(t, t == NSTEP - 1 ? w * w_last : w, xi, yi, zi, mi, pjb,
                                                                   mjb, axb, ayb, azb, fx, fy, fz, c);
}

// a whole tile pair in one pair form: the groups of `groups` (off the diagonal) or the diagonal
// tile's three groups
template <int VARIANT, bool GUARD, bool RAGGED, bool SHIFT = false, bool CUT = VARIANT == 1,
          bool POT = false, int FAR = 0, int MAX = -1>
__device__ __forceinline__ void n3b_pair(bool diag, unsigned groups, int l, double xi, double yi, double zi,
                                         double mi, const double (*pj)[128], const double* mj, double* ax,
                                         double* ay, double* az, double& fx, double& fy, double& fz,
                                         const PairC& c) {
    l = lane_opaque(l);
    const int a = l >> 4, m = l & 15;
    if (!diag) {
        for (int d = 0; d < 4; ++d) {
            if (!((groups >> d) & 1u)) continue;    // wave-uniform
            n3b_group<VARIANT, GUARD, RAGGED, SHIFT, CUT, POT, FAR, 16, MAX>(32 * ((a + d) & 3) + m, 1., xi, yi, zi, mi, pj,
                                                                             mj, ax, ay, az, fx, fy, fz, c);
        }
    } else if constexpr (MAX < 0) {                 // (a tile with itself has one image)
        // sub-tile distance 1..8 inside each sub-tile, the 8th once (m < 8)
        n3b_group<VARIANT, GUARD, RAGGED, SHIFT, CUT, POT, FAR, 8>(32 * a + m + 1, 1., xi, yi, zi, mi, pj, mj, ax, ay, az,
                                                                   fx, fy, fz, c, m >= 8 ? 0. : 1.);
        for (int d = 1; d < 3; ++d)
            n3b_group<VARIANT, GUARD, RAGGED, SHIFT, CUT, POT, FAR>(32 * ((a + d) & 3) + m, (d == 2 && a >= 2) ? 0. : 1.,
                                                                    xi, yi, zi, mi, pj, mj, ax, ay, az, fx, fy, fz, c);
    }
}

__device__ __forceinline__ float row_rol1f(float v) {   // lane 16 a + m <- lane 16 a + ((m + 1) & 15)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x12F, 0xF, 0xF, false));   // row_ror:15
}

// An ultra-far tile pair (boxes >= r_ufar32 apart) with a uniform image, pair terms in f32
// (error analysis and bound in mdqt_math.hpp kUfar32A/B).  Round 5: the staging wave
// also holds the J tile in f32 relative to its first ion c_J (pj32 = fl32(xj - c_J)), the wave takes
// xi32 = fl32(xi - n L - c_J) once per tile pair and dx = fl32(xi32 - pj32) — no f64 subtraction and
// f32 conversion per pair — and runs two rotation steps t, t + 1 through each packed
// instruction (v_pk_add_f32, v_pk_mul_f32, v_pk_fma_f32; v_rsq_f32, v_exp_f32 and the cutoff select
// per step): 16.75 VALU instructions per pair instead of 29.  The cutoff on the f32 r^2 (t = -inf).  The
// i side is summed in two f32 partials (even and odd steps), added, then added to the f64 partial; the j
// side is a running sum rotated one lane down inside the lane's row of 16 each step (row_ror:15 folded
// into the f32 add: lane m + 1's sum of the previous step is for lane m's current J ion; two steps at
// once: row_ror:14 of the sum plus row_ror:15 of step t's term plus step t + 1's) and ends in one
// ds_add_f64 per component at the group's last index.  Off the diagonal only (a tile's pair with
// itself is never ultra far).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float row_rol2f(float v) {   // lane 16 a + m <- lane 16 a + ((m + 2) & 15)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x12E, 0xF, 0xF, false));   // row_ror:14
}
// two rotation steps per v_pk_* instruction: gfx950 runs a packed f32 operation at half
// the rate of a scalar one (tools/ubench_f64: the same VALU cycles per pair) but issues half the
// instructions — A/B round 5 (profiles/r05h_uf32_force_ab.txt): C4 force call 244.8 ms packed, 248.3 scalar,
// 254.1 with the round-4 form (f64 separations); N = 1M 198.0 / 200.3 / 205.3

// POT (Epotential on the plan, round 6): u = 2^t ri in the same f32 operations, one component (i side in
// fx, j side in ax); its relative error is within the force form's (one factor ri instead of three)
template <bool POT = false>
__device__ __forceinline__ void n3b_group_uf32(int b0, float xi, float yi, float zi, const float (*pj32)[128],
                                               double* ax, double* ay, double* az, double& fx, double& fy, double& fz,
                                               float cf, float invlf, float rc2f) {
    // one opaque LDS address per component, so the 16 steps read them at immediate offsets (N3B_REBASE;
    // the array's own LDS offset and a shared base for the three components would not fit the
    // ds_read2_b32 offset field)
    typedef __attribute__((address_space(3))) const float* lds_f32p;
    lds_f32p px0 = (lds_f32p)&pj32[0][b0], py0 = (lds_f32p)&pj32[1][b0], pz0 = (lds_f32p)&pj32[2][b0];
    asm volatile("" : "+v"(px0), "+v"(py0), "+v"(pz0));
    if constexpr (POT) {
        f32x2 iu = {0.f, 0.f};
        float ju = 0.f;
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
            const f32x2 dx = f32x2{xi, xi} - f32x2{px0[t], px0[t + 1]};
            const f32x2 dy = f32x2{yi, yi} - f32x2{py0[t], py0[t + 1]};
            const f32x2 dz = f32x2{zi, zi} - f32x2{pz0[t], pz0[t + 1]};
            const f32x2 r2 = __builtin_elementwise_fma(dx, dx, __builtin_elementwise_fma(dy, dy, dz * dz));
            const f32x2 ri = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
            const f32x2 tt = (r2 * ri) * cf;
            const f32x2 e = {__builtin_amdgcn_exp2f(r2.x < rc2f ? tt.x : -INFINITY),
                             __builtin_amdgcn_exp2f(r2.y < rc2f ? tt.y : -INFINITY)};
            const f32x2 u = e * ri;
            const float uu = row_rol1f(u.x) + u.y;   // (the j side's rotation, as the forces')
            if (t == 0) { iu = u; ju = uu; }
            else { iu += u; ju = row_rol2f(ju) + uu; }
            asm volatile("" : "+v"(iu));
        }
        __hip_atomic_fetch_add(ax + b0 + 15, (double)ju, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        fx += (double)(iu.x + iu.y);
        (void)ay; (void)az; (void)fy; (void)fz; (void)invlf;
    } else {
        f32x2 ix = {0.f, 0.f}, iy = {0.f, 0.f}, iz = {0.f, 0.f};
        float jx = 0.f, jy = 0.f, jz = 0.f;
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
            const f32x2 dx = f32x2{xi, xi} - f32x2{px0[t], px0[t + 1]};
            const f32x2 dy = f32x2{yi, yi} - f32x2{py0[t], py0[t + 1]};
            const f32x2 dz = f32x2{zi, zi} - f32x2{pz0[t], pz0[t + 1]};
            const f32x2 r2 = __builtin_elementwise_fma(dx, dx, __builtin_elementwise_fma(dy, dy, dz * dz));
            const f32x2 ri = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
            const f32x2 tt = (r2 * ri) * cf;
            const f32x2 e = {__builtin_amdgcn_exp2f(r2.x < rc2f ? tt.x : -INFINITY),
                             __builtin_amdgcn_exp2f(r2.y < rc2f ? tt.y : -INFINITY)};
            const f32x2 ft = ((ri + invlf) * e) * (ri * ri);
            const f32x2 px = dx * ft, py = dy * ft, pz = dz * ft;
            // j side: S_t(m) = S_(t-1)(m + 1) + p_t(m); two steps: S_(t+1) = rol2(S_(t-1)) + (rol1(p_t) + p_(t+1))
            const float ux = row_rol1f(px.x) + px.y, uy = row_rol1f(py.x) + py.y, uz = row_rol1f(pz.x) + pz.y;
            if (t == 0) {
                ix = px; iy = py; iz = pz;
                jx = ux; jy = uy; jz = uz;
            } else {
                ix += px; iy += py; iz += pz;
                jx = row_rol2f(jx) + ux; jy = row_rol2f(jy) + uy; jz = row_rol2f(jz) + uz;
            }
            // each step pair's sums formed in their step pair (without it: 79 VGPRs spilled instead of 50)
            asm volatile("" : "+v"(ix), "+v"(iy), "+v"(iz));
        }
        const int b_ = b0;
        __hip_atomic_fetch_add(ax + b_ + 15, (double)jx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __hip_atomic_fetch_add(ay + b_ + 15, (double)jy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __hip_atomic_fetch_add(az + b_ + 15, (double)jz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        fx += (double)(ix.x + ix.y); fy += (double)(iy.x + iy.y); fz += (double)(iz.x + iz.y);
    }
}

// the f32 ultra-far form over the groups of `groups` (off the diagonal); xi, yi, zi: the lane's ion
// relative to the J tile's raw box centre, in f32
template <bool POT = false>
__device__ __forceinline__ void n3b_pair_uf32(unsigned groups, int l, float xi, float yi, float zi,
                                              const float (*pj32)[128], double* ax, double* ay, double* az,
                                              double& fx, double& fy, double& fz, float cf, float invlf, float rc2f) {
    l = lane_opaque(l);
    const int a = l >> 4, m = l & 15;
    for (int d = 0; d < 4; ++d) {
        if (!((groups >> d) & 1u)) continue;        // wave-uniform
        n3b_group_uf32<POT>(32 * ((a + d) & 3) + m, xi, yi, zi, pj32, ax, ay, az, fx, fy, fz, cf, invlf, rc2f);
    }
}

// One tile pair (I, J) of the block kernels (k_pairs_n3b, k_pairs_n3b_pw): its sub-tile groups of `word`
// (k_n3b_plan) in the pair forms of their levels, the image of the class word `tw` (n3b_pack_class); the i
// side into tx, ty, tz (a fresh sum per tile pair), the j side into the wave's accumulators ax, ay, az.
// rag: the ragged last tile is one of the two (exact form, validity weights)
template <int VARIANT, bool GUARD, bool POT, bool AXP>
__device__ __forceinline__ void n3b_tile_pair(const N3BArgs& a, const PairC& c, int l, bool diag, bool rag, int tw,
                                              unsigned word, double xi, double yi, double zi, double mi,
                                              const double (*pj)[128], const double* mj, const float (*pj32)[128],
                                              double* ax, double* ay, double* az, double& tx, double& ty, double& tz,
                                              float cf32, float invl32, float rc2f) {
    constexpr bool CUT = VARIANT == 1;
    constexpr bool FARF = VARIANT == 1 && !GUARD && CUT;   // the error-bounded pair forms
    const unsigned groups = word & 15u;
    const int ci = (tw & 15) - 2;       // bit 0 uniform image (the tile pair's)
    if (rag)
        n3b_pair<VARIANT, GUARD, true, false, CUT, POT>(diag, groups, l, xi, yi, zi, mi, pj, mj, ax, ay,
                                                        az, tx, ty, tz, c);
    else if (VARIANT == 1 && (ci & 1)) {       // uniform image
        const double nsh[3] = {(double)((tw << 20) >> 24), (double)((tw << 12) >> 24), (double)((tw << 4) >> 24)};
        // xi - n L once per tile pair (n3_step SHIFT)
        const double sx = fma(-nsh[0], a.L, xi);
        const double sy = fma(-nsh[1], a.L, yi);
        const double sz = fma(-nsh[2], a.L, zi);
        if constexpr (FARF) {
            if (diag) {                 // (a tile with itself: the exact form)
                n3b_pair<VARIANT, GUARD, false, true, CUT, POT>(true, groups, l, sx, sy, sz, mi, pj, mj, ax, ay,
                                                                az, tx, ty, tz, c);
            } else {                    // each form over the groups at its level
                const unsigned g5 = level_groups(word, 5), g4 = level_groups(word, 4),
                               g3 = level_groups(word, 3), g2 = level_groups(word, 2),
                               g1 = level_groups(word, 1), g0 = level_groups(word, 0);
                if (g4) n3b_pair<VARIANT, GUARD, false, true, CUT, POT, 4>(false, g4, l, sx, sy, sz, mi, pj, mj,
                                                                           ax, ay, az, tx, ty, tz, c);
                if (g3) n3b_pair<VARIANT, GUARD, false, true, CUT, POT, 3>(false, g3, l, sx, sy, sz, mi, pj, mj,
                                                                           ax, ay, az, tx, ty, tz, c);
                if (g2) n3b_pair<VARIANT, GUARD, false, true, CUT, POT, 2>(false, g2, l, sx, sy, sz, mi, pj, mj,
                                                                           ax, ay, az, tx, ty, tz, c);
                if (g1) n3b_pair<VARIANT, GUARD, false, true, CUT, POT, 1>(false, g1, l, sx, sy, sz, mi, pj, mj,
                                                                           ax, ay, az, tx, ty, tz, c);
                if (g0) n3b_pair<VARIANT, GUARD, false, true, CUT, POT>(false, g0, l, sx, sy, sz, mi, pj, mj, ax,
                                                                        ay, az, tx, ty, tz, c);
                // last: nothing after it keeps sx live
                if (g5) n3b_pair_uf32<POT>(g5, l, (float)(sx - pj[0][0]), (float)(sy - pj[1][0]),
                                           (float)(sz - pj[2][0]), pj32, ax, ay, az, tx, ty, tz, cf32,
                                           invl32, rc2f);
            }
        } else {
            n3b_pair<VARIANT, GUARD, false, VARIANT == 1, CUT, POT>(diag, groups, l, sx, sy, sz, mi, pj, mj,
                                                                    ax, ay, az, tx, ty, tz, c);
        }
    } else if constexpr (FARF) {       // per-pair image
        const int ax1 = (tw >> 28) & 3;  // 1 + the one axis whose image varies (n3b_pack_class)
        if (diag) {
            n3b_pair<VARIANT, GUARD, false, false, CUT, POT>(true, groups, l, xi, yi, zi, mi, pj, mj, ax, ay,
                                                             az, tx, ty, tz, c);
        } else if (AXP && ax1) {        // one axis: the other two shifted once (xi - n L)
          if constexpr (AXP) {
            const double sx = fma(-(double)((tw << 20) >> 24), a.L, xi);   // (0 on the varying axis:
            const double sy = fma(-(double)((tw << 12) >> 24), a.L, yi);   //  fma(-0, L, x) = x)
            const double sz = fma(-(double)((tw << 4) >> 24), a.L, zi);
            constexpr unsigned LV = kAx1Levels;             // the levels that take it (bit x: level x)
            // (levels 4 and 5 in the f64 ultra-far form with the one-axis image — the f32 form needs a
            // uniform image; without LV bit 4 they ride in the very-far form)
            const unsigned g45 = level_groups(word, 4) | level_groups(word, 5);
            const unsigned g3 = level_groups(word, 3) | ((LV & 16u) ? 0u : g45), g4 = (LV & 16u) ? g45 : 0u,
                           g2 = level_groups(word, 2), g1 = level_groups(word, 1), g0 = level_groups(word, 0);
            auto one_axis = [&](auto axc) {
                constexpr int AX = decltype(axc)::value;
                if ((LV & 16u) && g4)
                    n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 4, AX>(false, g4, l, sx, sy, sz, mi, pj, mj,
                                                                            ax, ay, az, tx, ty, tz, c);
                if ((LV & 8u) && g3)
                    n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 3, AX>(false, g3, l, sx, sy, sz, mi, pj, mj,
                                                                            ax, ay, az, tx, ty, tz, c);
                if ((LV & 4u) && g2)
                    n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 2, AX>(false, g2, l, sx, sy, sz, mi, pj, mj,
                                                                            ax, ay, az, tx, ty, tz, c);
                if ((LV & 2u) && g1)
                    n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 1, AX>(false, g1, l, sx, sy, sz, mi, pj, mj,
                                                                            ax, ay, az, tx, ty, tz, c);
            };
            if (ax1 == 1) one_axis(std::integral_constant<int, 0>{});
            else if (ax1 == 2) one_axis(std::integral_constant<int, 1>{});
            else one_axis(std::integral_constant<int, 2>{});
            // the other levels per pair (the exact level with a varying image: ~never, C3 1.6e-5
            // of the pairs)
            if (!(LV & 8u) && g3)
                n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 3>(false, g3, l, xi, yi, zi, mi, pj, mj, ax, ay,
                                                                    az, tx, ty, tz, c);
            if (!(LV & 4u) && g2)
                n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 2>(false, g2, l, xi, yi, zi, mi, pj, mj, ax, ay,
                                                                    az, tx, ty, tz, c);
            if (!(LV & 2u) && g1)
                n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 1>(false, g1, l, xi, yi, zi, mi, pj, mj, ax, ay,
                                                                    az, tx, ty, tz, c);
            if (g0) n3b_pair<VARIANT, GUARD, false, false, CUT, POT>(false, g0, l, xi, yi, zi, mi, pj, mj, ax,
                                                                     ay, az, tx, ty, tz, c);
          }
        } else {                        // (ultra far with a per-pair image: rare, very-far form)
            const unsigned g3 = level_groups(word, 3) | level_groups(word, 4) | level_groups(word, 5),
                           g2 = level_groups(word, 2), g1 = level_groups(word, 1), g0 = level_groups(word, 0);
            if (g3) n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 3>(false, g3, l, xi, yi, zi, mi, pj, mj, ax,
                                                                        ay, az, tx, ty, tz, c);
            if (g2) n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 2>(false, g2, l, xi, yi, zi, mi, pj, mj, ax,
                                                                        ay, az, tx, ty, tz, c);
            if (g1) n3b_pair<VARIANT, GUARD, false, false, CUT, POT, 1>(false, g1, l, xi, yi, zi, mi, pj, mj, ax,
                                                                        ay, az, tx, ty, tz, c);
            if (g0) n3b_pair<VARIANT, GUARD, false, false, CUT, POT>(false, g0, l, xi, yi, zi, mi, pj, mj, ax, ay,
                                                                     az, tx, ty, tz, c);
        }
    } else
        n3b_pair<VARIANT, GUARD, false, false, CUT, POT>(diag, groups, l, xi, yi, zi, mi, pj, mj, ax, ay, az,
                                                         tx, ty, tz, c);
}

// ------------------------------------------------------------------------------------------
// What the two block kernels share — the 8-wave k_pairs_n3b and the paired-wave k_pairs_n3b_pw (NWP = BW / 2
// waves, two I tiles each): the workgroup's frame and the scaffolding of a J step, one copy of each (a fix to
// the staging or to the combine is made here, and in tests/test_n3b_protocol.py, which mirrors the loops).
// The pair-form dispatch (n3b_tile_pair) is shared too; each kernel's i-side bookkeeping is its own.
//
// Every J step: the staging wave (the last; not one of the combining waves 0..2) loads J, one barrier, the
// pair work, one barrier, then waves 0..2 combine the workgroup's j accumulators of one component each into
// the j-slot and zero them for the next step — while the staging wave already loads the next J (no third
// barrier: nothing reads pj or the plan words after the second, and the accumulators are zero again before
// the combining waves reach the next one).
// ------------------------------------------------------------------------------------------
constexpr int NWP = BW / 2;                         // k_pairs_n3b_pw's waves per workgroup
// the block kernels' LDS, one object; W: the workgroup's waves (BW or NWP)
template <int W>
struct N3BShared {
    double pj[3][128];                              // J positions by sub-tiles twice over (n3b_lds)
    float pj32[3][128];                             // the same, fl32(xj - c_J), c_J = J's first ion (the f32 ultra-far form)
    double accj[W][3][128];                         // per-wave j accumulators
    double mjs[2][128];                             // J validity weights: all ones / the ragged last tile's
    double etab[64];                                // 2^(k/64)
    double irun[BW][3][64];                         // the run's i sums, per I tile of the block
    uint2 pw[BW];                                   // the J step's plan words (class, sub-tile groups), per I tile
};

// A workgroup's frame: its block and run, and the call's constants as the J steps take them.
// Workgroup order: run-major dispatches every block's first run — the near block distances, the heaviest
// work — first and the far, mostly skipped runs last, so the kernel's last round is short (round 3 was
// block-major).
struct N3BFrame {
    int P, run, d0, d1;                             // block P and its run's block distances [d0, d1)
    PairC c;
    int T, N, PS;                                   // tiles, ions, the positions' component stride
    bool ragN, srt;                                 // a ragged last tile; spatial order
    double pad;                                     // pad ions: distinct points (pair_ft_cut: r > 0)
    N3BRadii rad;
    float cf32, invl32, rc2f;                       // the f32 form's constants
    const uint2* plan;                              // (potentials: the plan of launch_potential_n3b, or none)
    const unsigned* jsteps;                         // the plan's J-step words, after its tile-pair words: .x bit b =
                                                    // some tile pair of J step b has work, .y the paired waves' tiles
    size_t plane;                                   // a slot's stride
};
template <int VARIANT, bool POT>
__device__ __forceinline__ N3BFrame n3b_frame(const N3BArgs& a, const double* etab, int l) {
    N3BFrame f;
    const int nP = a.Phi - a.Plo;
    f.P = a.Plo + (int)blockIdx.x % nP;
    f.run = (int)blockIdx.x / nP;
    f.d0 = f.run * a.runlen;
    f.d1 = min(a.nd, f.d0 + a.runlen);
    f.c = {a.L, a.micT, a.micGuard, a.Rcut, a.lDeb, a.invlDeb, 1. / a.L, a.rc2, etab};
    f.T = a.T;
    f.N = a.N;
    f.ragN = (a.N & 63) != 0;
    // positions: the sorted copy [3][Npad] (spatial order) or the gathered slabs
    f.srt = a.use_sort != 0;
    f.PS = f.srt ? a.Npad : a.S;
    f.pad = (double)(l + 1) * 0x1p-10;
    f.rad = n3b_radii<VARIANT, POT>(a);
    // the f32 form's constants as wave-uniform SGPR values (in VGPRs they were spilled and reloaded
    // inside the pair loop at the kernel's VGPR budget)
    auto sgpr_f = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    f.cf32 = sgpr_f((float)(a.invlDeb * kNegLog2e));
    f.invl32 = sgpr_f((float)a.invlDeb);
    f.rc2f = sgpr_f((float)a.rc2);
    f.plan = a.plan;
    return f;
}
// the frame's slot stride and J-step words, set after the kernel has written its accumulators and weights (the
// order the kernels were tuned in: set in n3b_frame, the 8-wave force instance spilled 50 VGPRs instead of 43
// and its C4 and N = 1M force calls ran 0.2-0.5 % slower, docs/PERF_HISTORY.md)
__device__ __forceinline__ void n3b_frame_slots(const N3BArgs& a, N3BFrame& f) {
    f.plane = (size_t)3 * a.Npad;
    f.jsteps = f.plan ? (const unsigned*)(f.plan + (size_t)(a.Phi - a.Plo) * a.nd * (BW * BW)) : nullptr;
}
__device__ __forceinline__ const double* n3b_tile_ptr(const N3BArgs& a, const N3BFrame& f, int tile) {
    return f.srt ? a.Rs + tile * 64 : tile_base(a.Rall, tile, a.S);
}
// the J-step words' index of (P, db)
__device__ __forceinline__ size_t n3b_jword(const N3BArgs& a, const N3BFrame& f, int db) {
    return 2 * ((size_t)(f.P - a.Plo) * a.nd + db);
}

// the J tile's validity weights (RAGGED pair steps): all ones, or the ragged last tile's pattern — constant
// over the launch, written once by the staging wave (a J tile takes mjs[J == T - 1])
template <int W>
__device__ __forceinline__ void n3b_init_mjs(N3BShared<W>& sh, const N3BFrame& f, int l) {
    const int li = n3b_lds(l);
    const double m1 = (f.T - 1) * 64 + l < f.N ? 1. : 0.;
    sh.mjs[0][li] = 1.; sh.mjs[0][li + 16] = 1.;
    sh.mjs[1][li] = m1; sh.mjs[1][li + 16] = m1;
}

// a J step whose every tile pair the plan skips (wave-uniform): J's rows get the combine's value, -0, and no
// barrier (with the reduction's masks: nothing, the slot is not read)
template <bool POT>
__device__ __forceinline__ void n3b_skip_j(const N3BArgs& a, const N3BFrame& f, int db, int q, int J, int l0) {
    if (q < (POT ? 1 : 3) && !a.tmask)
        a.slots[(size_t)db * f.plane + (size_t)q * a.Npad + J * 64 + lane_opaque(l0)] = POT ? 0. : -0.;
}

// The staging wave's part of J step b of (P, db): J by sub-tiles, twice over (n3b_lds); where the error-bounded
// forms run, its f32 copy relative to c_J = J's first ion (pj[.][0]); and the step's BW words, one per I tile.
// Tile-pair classes in spatial order (SpeedUp:222 keeps a pair only below r = L/2):
//  * skip (force_sort 1): boxes beyond the skip radius in the minimum image — at L/2 no pair
//    inside the cutoff (exact zeros), inside L/2 the error-bounded tail (tail sums);
//  * uniform image: every pair's raw separation fl(xi - xj) lies in [fl(lo_I - hi_J),
//    fl(hi_I - lo_J)] (rounding is monotone), and so does rint(fl(dx / L)) between the rints
//    of the two ends; equal ends = one minimum-image multiple per axis for every pair, bit for
//    bit what mic_r computes per pair (the fast variant then skips that rint per pair);
//  * otherwise the per-pair minimum image.
// class: -1 / -2 skip; otherwise bit 0 = uniform image, + 2 x the far level (n3b_level: 1 mid, 2
// far, 3 very far, 4 ultra far, 5 ultra far in f32; forces only): 0 .. 11 (n3b_pack_class: pw[.].x).
// The forces take them, with the sub-tile groups (pw[.].y), from the call's plan (k_n3b_plan: one
// 8-byte word per tile pair, loaded by lanes 0..BW-1); without a plan (potentials, unsorted order)
// the staging lanes classify the tile pairs themselves and every group runs in the exact form.
template <int VARIANT, bool GUARD, bool AXP, int W>
__device__ __forceinline__ void n3b_stage_j(const N3BArgs& a, const N3BFrame& f, N3BShared<W>& sh, int db, int b,
                                            int J, int l) {
    constexpr bool FARF = VARIANT == 1 && !GUARD;   // the error-bounded pair forms (potentials: on a plan)
    const int j = J * 64 + l;
    const bool vj = j < f.N;
    const double* p = n3b_tile_ptr(a, f, J) + l;
    const double xj = vj ? p[0] : f.pad, yj = vj ? p[f.PS] : f.pad, zj = vj ? p[2 * f.PS] : f.pad;
    const int li = n3b_lds(l);
    sh.pj[0][li] = xj; sh.pj[0][li + 16] = xj;
    sh.pj[1][li] = yj; sh.pj[1][li + 16] = yj;
    sh.pj[2][li] = zj; sh.pj[2][li + 16] = zj;
    if constexpr (FARF) {
        const float x32 = (float)(xj - uniform_f64(xj)), y32 = (float)(yj - uniform_f64(yj)),
                    z32 = (float)(zj - uniform_f64(zj));
        sh.pj32[0][li] = x32; sh.pj32[0][li + 16] = x32;
        sh.pj32[1][li] = y32; sh.pj32[1][li + 16] = y32;
        sh.pj32[2][li] = z32; sh.pj32[2][li + 16] = z32;
    }
    if (l < BW) {
        if (f.plan) {                               // (P, db, b): one word per I tile
            sh.pw[l] = f.plan[((size_t)(f.P - a.Plo) * a.nd + db) * (BW * BW) + b * BW + l];
        } else {
            int w = 2;                              // class 0 (unsorted: every tile pair, per-pair image)
            if (f.srt && f.P * BW + l < f.T) {
                double g2;
                int sm = 0;
                w = n3b_pack_class(n3b_classify<VARIANT == 1>(a, f.c.invL, f.rad, f.P * BW + l, J, g2,
                                                              AXP ? &sm : nullptr), sm);
            }
            sh.pw[l] = make_uint2((unsigned)w, 0xFFu);
        }
    }
}

// the j side of J's rows -> j-slot db, by waves 0..2 (POT: wave 0), one component each: the W waves' two
// copies, summed as a fixed pairwise tree (dependency depth log2(W) + 1, not W), then zeroed for the next J step
template <bool POT, int W>
__device__ __forceinline__ void n3b_combine_j(const N3BArgs& a, const N3BFrame& f, N3BShared<W>& sh, int db, int q,
                                              int J, int l0) {
    const int l = lane_opaque(l0);
    const int li = n3b_lds(l);
    double sw[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        sw[w] = sh.accj[w][q][li] + sh.accj[w][q][li + 16];
        sh.accj[w][q][li] = 0.;
        sh.accj[w][q][li + 16] = 0.;
    }
#pragma unroll
    for (int h = W / 2; h >= 1; h /= 2)
#pragma unroll
        for (int w = 0; w < h; ++w) sw[w] = sw[2 * w] + sw[2 * w + 1];
    a.slots[(size_t)db * f.plane + (size_t)q * a.Npad + J * 64 + l] = POT ? sw[0] : -sw[0];
}

// POT: Epotential's pair potential (component 0 of the slots, both rows +u) instead of the force
// waves per SIMD of the fast variant: 6 (VGPR budget 512 / 6 = 80), three workgroups of BW = 8 waves per CU
// (41.5 KB LDS each); the exact one (libm exp, divisions) gets 128 VGPRs at 4
constexpr int kN3BWpe = 6;
static_assert(BW == 8, "kN3BWpe: three workgroups of BW waves per CU");
// AXP: the one-axis per-pair image (n3b_pack_class bits 28-29) in an instance of its own, launched
// only where such tile pairs can lie inside the skip radius (n3b_kernel): compiled into the
// one instance it cost the calls without any (N = 1M) 0.5 %.
template <int VARIANT, bool GUARD, bool POT = false, bool AXP = false>
__global__ __launch_bounds__(BW * 64) __attribute__((amdgpu_waves_per_eu(VARIANT == 1 ? kN3BWpe : 4, VARIANT == 1 ? kN3BWpe : 4)))
void k_pairs_n3b(N3BArgs a) {
    __shared__ N3BShared<BW> sh;                    // all LDS in one object
    stage_exp_tab(sh.etab);
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // q: wave-uniform
    const int l0 = l;
    N3BFrame f = n3b_frame<VARIANT, POT>(a, sh.etab, l);
    const int P = f.P, T = f.T;
    const int I = P * BW + q;                       // the wave's I tile, in registers over the run
    const bool vI = I < T;
    double xi = f.pad, yi = f.pad, zi = f.pad, mi = 0.;
    if (vI && I * 64 + l < f.N) {
        const double* p = n3b_tile_ptr(a, f, I) + l;
        xi = p[0]; yi = p[f.PS]; zi = p[2 * f.PS]; mi = 1.;
    }
    // waited for here, once: as load results the compiler waited vmcnt(0) for them at every pair-form
    // dispatch
    asm volatile("" : "+v"(xi), "+v"(yi), "+v"(zi));
    // the run's i accumulator: in LDS (read and written once per block distance, so that the
    // three-level blocking fits the VGPR budget)
    auto fiptr = [&]() { return sh.irun[q][0] + lane_opaque(l0); };
    constexpr size_t FS = 64;
    bool fi_first = true;
    constexpr int kStage = BW - 1;                  // stages J; waves 0..2 combine the j sums
#pragma unroll
    for (int k = 0; k < 3; ++k) { sh.accj[q][k][l] = 0.; sh.accj[q][k][l + 64] = 0.; }
    double* ax = sh.accj[q][0];
    double* ay = sh.accj[q][1];
    double* az = sh.accj[q][2];
    if (q == kStage) n3b_init_mjs(sh, f, l);
    n3b_frame_slots(a, f);
    for (int db = f.d0; db < f.d1; ++db) {
        if (n3b_half_covered(a.NB, P, db)) continue;
        const int Q = (P + db) % a.NB;
        double bx = 0., by = 0., bz = 0.;          // this block distance's i partial (3-level blocking)
        // the block distance's J-step mask, read once and held in an SGPR (wave-uniform; read per J step
        // it was a vector load and a vmcnt(0) wait at the top of every step)
        const unsigned jmask = f.jsteps ? __builtin_amdgcn_readfirstlane(f.jsteps[n3b_jword(a, f, db)]) : ~0u;
        for (int b = 0; b < BW; ++b) {
            const int J = Q * BW + b;
            if (J >= T) break;
            if (f.jsteps && !((jmask >> b) & 1u)) {
                n3b_skip_j<POT>(a, f, db, q, J, l0);
                continue;
            }
            if (q == kStage) n3b_stage_j<VARIANT, GUARD, AXP>(a, f, sh, db, b, J, l);
            __syncthreads();
            const double (*pj)[128] = sh.pj;
            const double* mj = sh.mjs[J == T - 1];
            const int tw = __builtin_amdgcn_readfirstlane((int)sh.pw[q].x);
            const int cls = (tw & 15) - 2;
            const bool mine = vI && (db > 0 || J >= I);
            const bool diag = (db == 0 && J == I);
            // this wave's sub-tile groups, by pair form (k_n3b_plan)
            const unsigned word = __builtin_amdgcn_readfirstlane(sh.pw[q].y);
            const unsigned groups = word & 15u;
            if (mine && cls >= 0 && groups) {
                // blocked i accumulation: the tile pair's steps into a fresh sum, those into the
                // block distance's sum, those into the run's (a run is ~1e5 pair terms at N = 1e6;
                // in spatial order they arrive in coherent groups, and one serial chain would
                // carry their rounding: momentum |sum F| / mean |F| 1.8e-8 -> 1e-10 at C4)
                double tx = 0., ty = 0., tz = 0.;
                n3b_tile_pair<VARIANT, GUARD, POT, AXP>(a, f.c, l, diag, f.ragN && (I == T - 1 || J == T - 1), tw, word, xi,
                                                        yi, zi, mi, pj, mj, sh.pj32, ax, ay, az, tx, ty, tz, f.cf32,
                                                        f.invl32, f.rc2f);
                bx += tx; by += ty; bz += tz;
            }
            __syncthreads();
            if (q < (POT ? 1 : 3)) n3b_combine_j<POT>(a, f, sh, db, q, J, l0);
        }
        if (vI) {                                   // (0 + bx: the first block distance's partial as is)
            double* fi = fiptr();
            fi[0] = fi_first ? 0. + bx : fi[0] + bx;
            fi[FS] = fi_first ? 0. + by : fi[FS] + by;
            fi[2 * FS] = fi_first ? 0. + bz : fi[2 * FS] + bz;
        }
        fi_first = false;
    }
    if (vI) {                                       // i side -> i-slot nd + run
        double* fi = fiptr();
        double* o = a.slots + (size_t)(a.nd + f.run) * f.plane + I * 64 + lane_opaque(l0);
        const double r0 = fi_first ? 0. : fi[0], r1 = fi_first ? 0. : fi[FS], r2 = fi_first ? 0. : fi[2 * FS];
        o[0] = r0; o[a.Npad] = r1; o[2 * (size_t)a.Npad] = r2;
    }
}

// k_pairs_n3b_pw's tile pairing of a block distance: wave k runs I tiles (bits 6k..6k+2, 6k+3..6k+5);
// without a plan the fixed pairing (k, 7 - k)
constexpr unsigned kN3BPairsDefault = (0u | 7u << 3) | (1u | 6u << 3) << 6 | (2u | 5u << 3) << 12 | (3u | 4u << 3) << 18;
static_assert(BW == 8, "the paired-wave pairing word holds 8 tiles");

// ------------------------------------------------------------------------------------------
// Paired waves (round 6, option force_n3b_pairs): the blocks, plan, slots and reduction of k_pairs_n3b
// with a workgroup of NWP = BW / 2 = 4 waves, each running TWO of block P's 8 I tiles against every J tile of
// the block distance — tiles paired per block distance by k_n3b_plan, the one with the most estimated
// work with the one with the least (n3b_pairing).  k_pairs_n3b's J-step barriers wait for the busiest of
// its 8 waves, and within a block distance the same tiles are the busy ones (the I tiles nearest block Q):
// the busiest wave of a J step carried 1.19-1.28 x the mean (k_n3b_census bal, tools/jstep_balance.py),
// a no-barrier timing build ran 4-12 % faster.  A wave's two tile pairs of a J step add to one j
// accumulator (the J tile is the same), and the combine sums 4 of them; the I positions of the wave's two
// tiles are loaded once per block distance, the run's i sums are per tile in LDS.  LDS 31 KB: five
// workgroups per CU.  Deterministic (the pairing is a function of the positions), not bit-identical to
// k_pairs_n3b (another summation tree on the j side).
// ------------------------------------------------------------------------------------------
constexpr int kN3BPwWpe = 5;                        // waves per SIMD: five 4-wave workgroups per CU (LDS 31 KB)
template <int VARIANT, bool GUARD, bool POT = false, bool AXP = false>
__global__ __launch_bounds__(NWP * 64) __attribute__((amdgpu_waves_per_eu(VARIANT == 1 ? kN3BPwWpe : 4, VARIANT == 1 ? kN3BPwWpe : 4)))
void k_pairs_n3b_pw(N3BArgs a) {
    __shared__ N3BShared<NWP> sh;
    stage_exp_tab(sh.etab);
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // q: wave-uniform
    const int l0 = l;
    N3BFrame f = n3b_frame<VARIANT, POT>(a, sh.etab, l);
    const int P = f.P, T = f.T, N = f.N, PS = f.PS;
    const double pad = f.pad;
    constexpr int kStage = NWP - 1;                 // stages J; waves 0..2 combine the j sums
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sh.accj[q][k][l] = 0.; sh.accj[q][k][l + 64] = 0.;
        sh.irun[q][k][l] = 0.; sh.irun[q + NWP][k][l] = 0.;
    }
    double* ax = sh.accj[q][0];
    double* ay = sh.accj[q][1];
    double* az = sh.accj[q][2];
    if (q == kStage) n3b_init_mjs(sh, f, l);
    n3b_frame_slots(a, f);
    for (int db = f.d0; db < f.d1; ++db) {
        if (n3b_half_covered(a.NB, P, db)) continue;
        const int Q = (P + db) % a.NB;
        const size_t jw = n3b_jword(a, f, db);
        const unsigned jmask = f.jsteps ? __builtin_amdgcn_readfirstlane(f.jsteps[jw]) : ~0u;
        // the wave's two I tiles of this block distance (k_n3b_plan; without a plan: q and 7 - q)
        const unsigned pr = f.jsteps ? __builtin_amdgcn_readfirstlane(f.jsteps[jw + 1]) : kN3BPairsDefault;
        const int tA = (pr >> (6 * q)) & 7, tB = (pr >> (6 * q + 3)) & 7;
        const int IA = P * BW + tA, IB = P * BW + tB;
        const bool vA = IA < T, vB = IB < T;
        double xA = pad, yA = pad, zA = pad, mA = 0., xB = pad, yB = pad, zB = pad, mB = 0.;
        if (vA && IA * 64 + l < N) {
            const double* p = n3b_tile_ptr(a, f, IA) + l;
            xA = p[0]; yA = p[PS]; zA = p[2 * PS]; mA = 1.;
        }
        if (vB && IB * 64 + l < N) {
            const double* p = n3b_tile_ptr(a, f, IB) + l;
            xB = p[0]; yB = p[PS]; zB = p[2 * PS]; mB = 1.;
        }
        double bxA = 0., byA = 0., bzA = 0., bxB = 0., byB = 0., bzB = 0.;
        bool work = false;
        for (int b = 0; b < BW; ++b) {
            const int J = Q * BW + b;
            if (J >= T) break;
            if (f.jsteps && !((jmask >> b) & 1u)) {
                n3b_skip_j<POT>(a, f, db, q, J, l0);
                continue;
            }
            work = true;
            if (q == kStage) n3b_stage_j<VARIANT, GUARD, AXP>(a, f, sh, db, b, J, l);
            __syncthreads();
            const double (*pj)[128] = sh.pj;
            const double* mj = sh.mjs[J == T - 1];
#pragma unroll 1
            for (int u = 0; u < 2; ++u) {            // the wave's two tile pairs (I_A, J), (I_B, J)
                const int tI = u ? tB : tA;
                const int I = P * BW + tI;
                const int tw = __builtin_amdgcn_readfirstlane((int)sh.pw[tI].x);
                const unsigned word = __builtin_amdgcn_readfirstlane(sh.pw[tI].y);
                const bool mine = (u ? vB : vA) && (db > 0 || J >= I);
                if (mine && (tw & 15) >= 2 && (word & 15u)) {
                    double tx = 0., ty = 0., tz = 0.;
                    n3b_tile_pair<VARIANT, GUARD, POT, AXP>(a, f.c, l, db == 0 && J == I, f.ragN && (I == T - 1 || J == T - 1),
                                                            tw, word, u ? xB : xA, u ? yB : yA, u ? zB : zA,
                                                            u ? mB : mA, pj, mj, sh.pj32, ax, ay, az, tx, ty, tz, f.cf32,
                                                            f.invl32, f.rc2f);
                    if (u) { bxB += tx; byB += ty; bzB += tz; }
                    else { bxA += tx; byA += ty; bzA += tz; }
                }
            }
            __syncthreads();
            if (q < (POT ? 1 : 3)) n3b_combine_j<POT>(a, f, sh, db, q, J, l0);
        }
        if (work) {                                 // this block distance's i sums into the run's, per tile
            const int lo = lane_opaque(l0);
            double* fa = sh.irun[tA][0] + lo;
            fa[0] += bxA; fa[64] += byA; fa[128] += bzA;
            double* fb = sh.irun[tB][0] + lo;
            fb[0] += bxB; fb[64] += byB; fb[128] += bzB;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {                   // i side -> i-slot nd + run: tiles q and q + 4
        const int tI = q + u * NWP, I = P * BW + tI;
        if (I < T) {
            const int lo = lane_opaque(l0);
            const double* fi = sh.irun[tI][0] + lo;
            double* o = a.slots + (size_t)(a.nd + f.run) * f.plane + I * 64 + lo;
            o[0] = fi[0]; o[a.Npad] = fi[64]; o[2 * (size_t)a.Npad] = fi[128];
        }
    }
}

// canonical per-ion sum of the slots this rank wrote: j-slots db = 0 .. nd-1, then i-slots.
// out: world 1 -> F [3][S]; sharded -> the rank's dense partial [world][3][S] (reduce-scattered)
// With the plan's per-J-tile masks (a.tmask) only the j-slots the block kernel wrote are read — the
// others held the -0 of empty J steps, and acc + -0 = acc: the same sum, bit for bit, without ~2/3 of
// the reads at N = 1M.  The masks are wave-uniform (a wave is one J tile): 8 slot loads in flight per
// round, added in ascending db order.
__global__ __launch_bounds__(256) void k_n3b_reduce(N3BArgs a, double* __restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (g >= a.N) return;
    const int B = (g >> 6) / BW;
    const size_t plane = (size_t)3 * a.Npad;
    const double* p = a.slots + (size_t)k * a.Npad + g;
    double acc = 0.;
    if (a.tmask) {
        const unsigned long long* tm = a.tmask + (size_t)(g >> 6) * a.tmw;
        for (int w = 0; w < a.tmw; ++w) {
            // (readfirstlane returns int: each half zero-extended, not sign-extended)
            unsigned long long m = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)tm[w]) |
                                   ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(tm[w] >> 32)) << 32);
            while (m) {
                int idx[8];
                int n = 0;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (m) { idx[u] = 64 * w + __builtin_ctzll(m); m &= m - 1; n = u + 1; }
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = u < n ? p[(size_t)idx[u] * plane] : 0.;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (u < n) acc = acc + v[u];
            }
        }
    } else {
        for (int db = 0; db < a.nd; ++db) {
            const int P = (B - db + a.NB) % a.NB;
            if (!n3b_half_covered(a.NB, P, db) && P >= a.Plo && P < a.Phi) acc = acc + p[(size_t)db * plane];
        }
    }
    if (B >= a.Plo && B < a.Phi)
        for (int r = 0; r < a.R; ++r) acc = acc + p[(size_t)(a.nd + r) * plane];
    const int ion = a.use_sort ? a.perm[g] : g;     // spatial order: scatter back to the ion's place
    const int w = ion / a.S;
    out[(size_t)w * 3 * a.S + (size_t)k * a.S + (ion - w * a.S)] = acc;
}

// in-process rank group (tests): F of rank `rank` = sum over ranks r = 0.. of part[r]'s chunk
__global__ __launch_bounds__(256) void k_sum_rank_chunks(const double* const* parts, int world, int rank, int S,
                                                         double* __restrict__ F) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * S) return;
    double acc = 0.;
    for (int r = 0; r < world; ++r) acc = acc + parts[r][(size_t)rank * 3 * S + i];
    F[i] = acc;
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
// The block kernel of a call and its workgroup size.  The paired-wave kernel (option force_n3b_pairs) is
// the fast variant's without guard; the AXP instances (n3b_axp) are the fast variant's without guard too,
// and the potential takes one only on a plan (unplanned, its staging lanes classify every group exact)
struct N3BKernel {
    void (*fn)(N3BArgs);
    int threads;
};
template <bool POT>
static N3BKernel n3b_kernel_of(int variant, bool guard, bool pairs, bool axp) {
    if (variant == 1 && !guard) {
        if (pairs) return {axp ? k_pairs_n3b_pw<1, false, POT, true> : k_pairs_n3b_pw<1, false, POT, false>, NWP * 64};
        return {axp ? k_pairs_n3b<1, false, POT, true> : k_pairs_n3b<1, false, POT, false>, BW * 64};
    }
    if (variant == 1) return {k_pairs_n3b<1, true, POT, false>, BW * 64};
    return {guard ? k_pairs_n3b<0, true, POT, false> : k_pairs_n3b<0, false, POT, false>, BW * 64};
}
static N3BKernel n3b_kernel(int variant, bool pot, bool planned, const N3BArgs& a) {
    const bool axp = n3b_axp(a) && (planned || !pot);
    return pot ? n3b_kernel_of<true>(variant, a.guard, a.pairs, axp) : n3b_kernel_of<false>(variant, a.guard, a.pairs, axp);
}

hipError_t launch_forces_n3b(const N3BArgs& a, int variant, double* out, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1,
                             hipEvent_t* marks) {
    const int nblk = (a.Phi - a.Plo) * a.R;
    const int nplan = (a.Phi - a.Plo) * a.nd;
    if (hipError_t e = launch_n3b_plan(a, variant, s); e != hipSuccess) return e;
    if (marks && hipEventRecord(marks[0], s) != hipSuccess) return hipGetLastError();
    if (nblk > 0) {
        const N3BKernel k = n3b_kernel(variant, false, a.plan && nplan > 0, a);
        launch_timed(k.fn, dim3(nblk), dim3(k.threads), s, ev0, ev1, a);
    } else if (ev0) {                                   // (no block of this rank: an empty interval)
        if (hipEventRecord(ev0, s) != hipSuccess || hipEventRecord(ev1, s) != hipSuccess) return hipGetLastError();
    }
    // a rank without blocks (Phi == Plo, sharded with NB < W) has no plan and so no masks to follow:
    // the unmasked reduction reads none of its (unwritten) slots and leaves its dense partial 0
    N3BArgs r = a;
    if (!(a.plan && nplan > 0)) r.tmask = nullptr;
    if (marks && hipEventRecord(marks[1], s) != hipSuccess) return hipGetLastError();
    hipLaunchKernelGGL(k_n3b_reduce, dim3((a.N + 255) / 256, 3), dim3(256), 0, s, r, out);
    if (marks && hipEventRecord(marks[2], s) != hipSuccess) return hipGetLastError();
    return hipGetLastError();
}

// Epotential()'s pair sums on the blocks.  With a plan (a.plan, the fast variant in spatial order; round
// 6): the force call's skip radius, sub-tile groups and error-bounded forms (pair_u_cut, the f32
// ultra-far form), the tail sums in a.tailb for the caller's enforcement; without: every pair to L/2 in
// the exact form (the staging lanes classify)
hipError_t launch_potential_n3b(const N3BArgs& a, int variant, double* out, hipStream_t s, hipEvent_t ev0,
                                hipEvent_t ev1) {
    if (variant < 0 || variant > 1) return hipErrorInvalidValue;
    const int nblk = (a.Phi - a.Plo) * a.R;
    const int nplan = (a.Phi - a.Plo) * a.nd;
    const bool planned = a.plan && nplan > 0;
    if (planned && (variant != 1 || a.guard)) return hipErrorInvalidValue;   // (the far forms are the fast variant's)
    if (hipError_t e = launch_n3b_plan(a, variant, s); e != hipSuccess) return e;
    N3BArgs r = a;
    if (!planned) { r.plan = nullptr; r.tmask = nullptr; }   // (no plan: every j-slot written, every one read)
    if (nblk > 0) {
        const N3BKernel k = n3b_kernel(variant, true, planned, a);
        launch_timed(k.fn, dim3(nblk), dim3(k.threads), s, ev0, ev1, r);
    } else if (ev0) {
        if (hipEventRecord(ev0, s) != hipSuccess || hipEventRecord(ev1, s) != hipSuccess) return hipGetLastError();
    }
    hipLaunchKernelGGL(k_n3b_reduce, dim3((a.N + 255) / 256, 1), dim3(256), 0, s, r, out);   // component 0
    return hipGetLastError();
}

hipError_t launch_sum_rank_chunks(const double* const* parts, int world, int rank, int S, double* F, hipStream_t s) {
    hipLaunchKernelGGL(k_sum_rank_chunks, dim3((3 * S + 255) / 256), dim3(256), 0, s, parts, world, rank, S, F);
    return hipGetLastError();
}

}  // namespace mdqt
