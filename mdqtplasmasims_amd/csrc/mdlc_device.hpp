// The body of the three-level laser-cooling step kernels (qstep() of laserCoolNoPlasmaThreeState.cpp, "LC3",
// :140-293) as a device function that two translation units call: mdlc_kernels.hip (k_lc_steps: one laser
// setting for the whole launch, its constants kernel arguments) and mdlc_sweep_kernels.hip (k_lc_steps_sweep: a
// parameter scan, the member's constants from its point's LCPoint).  One body, so a member of a scan steps
// bit for bit as the single job with its parameters.  The arithmetic and its limits: mdlc_kernels.hip.
#pragma once

#include "mdlc_kernels.hpp"
#include "mdqt_device.hpp"

namespace mdqt {

__device__ __forceinline__ double lc_nrm2(cxd y) { return fma(y.re, y.re, y.im * y.im); }
// Im(a conj(b))
__device__ __forceinline__ double lc_rho_im(cxd a, cxd b) { return fma(a.im, b.re, -(a.re * b.im)); }

// sum over the wave's 64 lanes, the same value in every lane (each level adds the two halves of
// a pair; IEEE addition is commutative, so both lanes of a pair get the same bits)
__device__ __forceinline__ double lc_wave_sum(double e) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) e = e + __shfl_xor(e, off, 64);
    return e;
}

// a.nsteps steps of the workgroup's ions of member `job` (the member's index in the launch: its slot in the
// arrays), Philox key word 1 `key1`, and the workgroup's partial sum of 0.5 vx^2.  mi0, cim, ks: the laser's
// constants (LCArgs' fields of these names), workgroup-uniform
__device__ __forceinline__ void lc_steps_body(const LCArgs& a, const int job, const uint32_t key1, const double mi0,
                                              const double cim, const double ks) {
    __shared__ double wsum[kLCBlock / 64];
    const int ion = (blockIdx.x - job * a.B) * kLCBlock + threadIdx.x;
    const bool active = ion < a.N0;
    const size_t g = (size_t)job * a.S + ion;          // < J S: the grid is J B workgroups, B kLCBlock = S
    const size_t cs = (size_t)gridDim.x * kLCBlock;    // component stride of psi: J S
    double e = 0.;
    if (active) {
        double v = a.vx[g], tPart = a.tPart[g];
        cxd w0 = {a.psi[g], a.psi[cs + g]}, w1 = {a.psi[2 * cs + g], a.psi[3 * cs + g]},
            w2 = {a.psi[4 * cs + g], a.psi[5 * cs + g]};
        const double dt = a.dt, mre = a.mre;
        for (int s = 0; s < a.nsteps; ++s) {
            tPart += dt;                                                      // :171
            const double dp = (lc_nrm2(w1) + lc_nrm2(w2)) * dt;               // :172-180 (cs = |0><1|, |0><2|, gs = 1)
            double u1, randDir;
            philox_pair(a.seed, key1, (uint64_t)ion, a.q0 + (uint64_t)s, 0, u1, randDir);
            double kick;
            if (u1 > dp) {                                                    // :182
                kick = (lc_rho_im(w0, w2) - lc_rho_im(w0, w1)) * ks;          // :185-189
                const double m1 = fma(-dt, v, mi0), m2 = fma(dt, v, mi0);     // Im M11, Im M22 (:192-193)
                cxd y0 = w0, y1 = w1, y2 = w2, acc0, acc1, acc2;
#pragma unroll
                for (int stg = 0; stg < 4; ++stg) {                           // :212-271
                    const double dpy = stg == 0 ? dp : (lc_nrm2(y1) + lc_nrm2(y2)) * dt;
                    const double pref = rsq3(1. - dpy);                       // :222
                    const cxd s0 = {fma(-cim, y2.im, fma(-cim, y1.im, y0.re)), fma(cim, y2.re, fma(cim, y1.re, y0.im))};
                    const cxd s1 = {fma(-cim, y0.im, fma(-m1, y1.im, mre * y1.re)),
                                    fma(cim, y0.re, fma(m1, y1.re, mre * y1.im))};
                    const cxd s2 = {fma(-cim, y0.im, fma(-m2, y2.im, mre * y2.re)),
                                    fma(cim, y0.re, fma(m2, y2.re, mre * y2.im))};
                    const cxd d0 = {fma(pref, s0.re, -y0.re), fma(pref, s0.im, -y0.im)};
                    const cxd d1 = {fma(pref, s1.re, -y1.re), fma(pref, s1.im, -y1.im)};
                    const cxd d2 = {fma(pref, s2.re, -y2.re), fma(pref, s2.im, -y2.im)};
                    if (stg == 0) {
                        acc0 = d0; acc1 = d1; acc2 = d2;
                    } else if (stg < 3) {
                        acc0 = {fma(3., d0.re, acc0.re), fma(3., d0.im, acc0.im)};
                        acc1 = {fma(3., d1.re, acc1.re), fma(3., d1.im, acc1.im)};
                        acc2 = {fma(3., d2.re, acc2.re), fma(3., d2.im, acc2.im)};
                    } else {
                        acc0 = {acc0.re + d0.re, acc0.im + d0.im};
                        acc1 = {acc1.re + d1.re, acc1.im + d1.im};
                        acc2 = {acc2.re + d2.re, acc2.im + d2.im};
                    }
                    if (stg < 2) {                                            // y = w + d / 2
                        y0 = {fma(0.5, d0.re, w0.re), fma(0.5, d0.im, w0.im)};
                        y1 = {fma(0.5, d1.re, w1.re), fma(0.5, d1.im, w1.im)};
                        y2 = {fma(0.5, d2.re, w2.re), fma(0.5, d2.im, w2.im)};
                    } else if (stg == 2) {                                    // y = w + d
                        y0 = {w0.re + d0.re, w0.im + d0.im};
                        y1 = {w1.re + d1.re, w1.im + d1.im};
                        y2 = {w2.re + d2.re, w2.im + d2.im};
                    }
                }
                w0 = {fma(0.125, acc0.re, w0.re), fma(0.125, acc0.im, w0.im)};   // :271
                w1 = {fma(0.125, acc1.re, w1.re), fma(0.125, acc1.im, w1.im)};
                w2 = {fma(0.125, acc2.re, w2.re), fma(0.125, acc2.im, w2.im)};
            } else {                                                          // :273-285
                tPart = 0.;
                w0 = {1., 0.}; w1 = {0., 0.}; w2 = {0., 0.};
                kick = randDir < 0.5 ? a.vKick : -a.vKick;
            }
            if (a.applyForce) v = v + kick;                                   // :287-289
        }
        if (a.nsteps > 0) {
            a.vx[g] = v;
            a.tPart[g] = tPart;
            a.psi[g] = w0.re;          a.psi[cs + g] = w0.im;
            a.psi[2 * cs + g] = w1.re; a.psi[3 * cs + g] = w1.im;
            a.psi[4 * cs + g] = w2.re; a.psi[5 * cs + g] = w2.im;
        }
        e = 0.5 * (v * v);                                                    // :313
    }
    e = lc_wave_sum(e);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double p = wsum[0];
#pragma unroll
        for (int k = 1; k < kLCBlock / 64; ++k) p = p + wsum[k];
        a.part[blockIdx.x] = p;
    }
}

}  // namespace mdqt
