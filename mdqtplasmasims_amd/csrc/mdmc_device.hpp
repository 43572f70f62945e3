// Device bodies of the MC + MD program's velocity-Verlet and per-step observable kernels, shared by the
// single-job kernels (mdmc_kernels.hip) and the batched ones of an ensemble (mdmc_ensemble_kernels.hip):
// each __global__ kernel of either file is a one-line caller, so a member of an ensemble runs the arithmetic
// of its own launch — one body, inlined into both (as mc_lds_chain and lane_substeps are).
#pragma once

#include "mdmc_kernels.hpp"
#include "mdqt_math.hpp"

namespace mdqt {

__device__ __forceinline__ double wave_sum(double v) {      // butterfly: every lane holds the same sum
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------
// velocity Verlet (MDStep :504-511).  vv_positions_body is stepPositions :452-467 (R -> Rn).  After
// the Newton-3 force kernel, vv_step_body sums the force slots (canonical order) into a(t + dt),
// runs stepVelocities :469-502 (Verlet update + laser force) and pre-advances the positions of
// the next MDStep, r + dt v + dt^2/2 a with the box wrap, into Rn: the same expression on the same
// values stepPositions would read, so a step is two launches.  collide_body then overwrites the
// collided particles of the step from the host-drawn list (and redoes their Rn).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double step_pos(double r, double v, double a, double dt, double L) {   // :455-464
    r = r + dt * v + dt * dt / 2 * a;
    if (r < 0) r += L;
    if (r > L) r -= L;
    return r;
}

// thread = particle blk * 256 + threadIdx.x
__device__ __forceinline__ void vv_positions_body(const double* __restrict__ R, const double* __restrict__ V,
                                                  const double* __restrict__ A, double* __restrict__ Rn, int N, int S,
                                                  double dt, double L, unsigned blk) {
    const int i = blk * 256 + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t k = (size_t)c * S + i;
        Rn[k] = step_pos(R[k], V[k], A[k], dt, L);
    }
}

__device__ __forceinline__ void laser_kick(const VVArgs& a, double* v) {      // :488-498
    if (a.oneAxis) {
        v[0] += v[0] * a.dt * 1.234 * a.p6 * a.beta / a.sqrtn;
    } else {
        v[0] += v[0] * a.dt * 1.234 * a.p6 * a.beta / a.sqrtn / 2;
        v[1] += v[1] * a.dt * 1.234 * a.p6 * a.beta / a.sqrtn / 4 * (-1);
        v[2] += v[2] * a.dt * 1.234 * a.p6 * a.beta / a.sqrtn / 4 * (-1);
    }
}

__device__ __forceinline__ double laser_term(const VVArgs& a, int c, double v) {   // :488-498, component c
    if (a.oneAxis) return c == 0 ? v + v * a.dt * 1.234 * a.p6 * a.beta / a.sqrtn : v;
    if (c == 0) return v + v * a.dt * 1.234 * a.p6 * a.beta / a.sqrtn / 2;
    return v + v * a.dt * 1.234 * a.p6 * a.beta / a.sqrtn / 4 * (-1);
}

// workgroup (512 threads) = 64 particles (tile blk) x one component c; wave q sums the slots q, q + 8,
// q + 16, ... of its 64 particles (coalesced rows) = seg_sum's accumulator a[q], and wave 0 combines the
// eight in seg_sum's tree: bit-identical to seg_sum, with 8x the loads in flight.  acc: the workgroup's LDS
__device__ __forceinline__ void vv_step_body(const VVArgs& a, unsigned blk, int c, double (*acc)[64]) {
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = blk * 64 + lane;
    const size_t k = (size_t)c * a.S + i;
    const size_t stride = (size_t)3 * a.S;
    double sq = 0.;
    if (i < a.N)
        for (int sl = q; sl < a.nslots; sl += 8) sq += a.slots[(size_t)sl * stride + k];
    acc[q][lane] = sq;
    __syncthreads();
    if (q != 0 || i >= a.N) return;
    const double an = ((acc[0][lane] + acc[1][lane]) + (acc[2][lane] + acc[3][lane])) +
                      ((acc[4][lane] + acc[5][lane]) + (acc[6][lane] + acc[7][lane]));
    double v = a.V[k] + a.dt / 2 * (a.A[k] + an);                    // :484-486 (oldA + A)
    if (a.laser) v = laser_term(a, c, v);
    a.V[k] = v;
    a.A[k] = an;
    a.Rn[k] = step_pos(a.R[k], v, an, a.dt, a.L);
}

// the collided particles of the step (:477-482): V = the host-drawn Maxwellian, then the laser term;
// thread = hit blk * 64 + threadIdx.x
__device__ __forceinline__ void collide_body(const VVArgs& a, unsigned blk) {
    const int h = blk * 64 + threadIdx.x;
    if (h >= a.nhits) return;
    const double* e = a.hits + 4 * (size_t)h;
    const int i = (int)e[0];
    double v[3] = {e[1], e[2], e[3]};
    if (a.laser) laser_kick(a, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t k = (size_t)c * a.S + i;
        a.V[k] = v[c];
        a.Rn[k] = step_pos(a.R[k], v[c], a.A[k], a.dt, a.L);
    }
}

// ------------------------------------------------------------------------------------------
// block reductions of the per-step observables: temperatures (:525-546, :560-581) and the
// tagged-particle moments (:937-971); one workgroup of RBT threads, fixed order
// ------------------------------------------------------------------------------------------
constexpr int RBT = 1024;

__device__ __forceinline__ void temperatures_body(const double* __restrict__ V, int N, int S, double* __restrict__ out,
                                                  double (*sp)[RBT / 64]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double a = 0., x = 0., y = 0., z = 0.;
    for (int i = tid; i < N; i += RBT) {
        const double vx = V[i], vy = V[S + i], vz = V[2 * S + i];
        a = a + vx * vx; a = a + vy * vy; a = a + vz * vz;
        x = x + vx * vx; y = y + vy * vy; z = z + vz * vz;
    }
    a = wave_sum(a); x = wave_sum(x); y = wave_sum(y); z = wave_sum(z);
    if (lane == 0) { sp[0][w] = a; sp[1][w] = x; sp[2][w] = y; sp[3][w] = z; }
    __syncthreads();
    if (tid < 4) {
        double s = 0.;
        for (int q = 0; q < RBT / 64; ++q) s = s + sp[tid][q];
        out[tid] = s;
    }
}

__device__ __forceinline__ void tag_moments_body(const double* __restrict__ V, const int* __restrict__ tags, int N,
                                                 double* __restrict__ out, double (*sp)[RBT / 64]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double m[kTagMomentSums];
#pragma unroll
    for (int q = 0; q < kTagMomentSums; ++q) m[q] = 0.;
    for (int i = tid; i < N; i += RBT) {
        const double v = V[i];
        const double v2 = v * v, v3 = v * v * v, v4 = v * v * v * v;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (tags[(size_t)t * N + i]) {
                m[5 * t] += v; m[5 * t + 1] += v2; m[5 * t + 2] += v3; m[5 * t + 3] += v4; m[5 * t + 4] += 1.;
            }
    }
#pragma unroll
    for (int q = 0; q < kTagMomentSums; ++q) {
        const double s = wave_sum(m[q]);
        if (lane == 0) sp[q][w] = s;
    }
    __syncthreads();
    if (tid < kTagMomentSums) {
        double s = 0.;
        for (int q = 0; q < RBT / 64; ++q) s = s + sp[tid][q];
        out[tid] = s;
    }
}

// recordVelsForAutocorrelations (:513-523): vStore[c][i][t] = V[c][i]; thread = particle blk * 256 + threadIdx.x
__device__ __forceinline__ void store_velocities_body(const double* __restrict__ V, int N, int S, int T, int t,
                                                      double* __restrict__ vs, unsigned blk) {
    const int i = blk * 256 + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) vs[((size_t)c * N + i) * T + t] = V[(size_t)c * S + i];
}

}  // namespace mdqt
