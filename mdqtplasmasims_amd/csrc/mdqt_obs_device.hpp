// The observables kernels' bodies (output(), SpeedUp:917-1032; Epotential(), :244-281) as device functions
// that two translation units call: mdqt_kernels.hip (the single-job kernels k_sum_vx, k_energy_sums, k_kde,
// k_kde_reduce, k_output_pack) and mdqt_ensemble_obs.hip (the ensemble's batched kernels over members).  One
// body per kernel, so a member's sums, bins and columns are bit for bit its own launch's.  Deterministic
// fixed-shape reductions.
#pragma once

#include "mdqt_internal.hpp"

namespace mdqt {

constexpr int RT = 1024;   // the sums' workgroup

__device__ __forceinline__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int w = RT / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] = sh[t] + sh[t + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// sum of V[0 .. n): each thread's strided partial, then block_sum (the value in every thread)
__device__ __forceinline__ double sum_vx_body(const double* __restrict__ V, int n, double* sh) {
    double acc = 0.;
    for (int i = threadIdx.x; i < n; i += RT) acc += V[i];
    return block_sum(acc, sh);
}

// out[0..2] = sum 0.5 (vx - avg)^2, 0.5 vy^2, 0.5 vz^2; out[3] = sum urow (thread 0 writes)
__device__ __forceinline__ void energy_sums_body(const double* __restrict__ V, int n, int S, double avg,
                                                 const double* __restrict__ urow, double* out, double* sh) {
    double ex = 0., ey = 0., ez = 0., u = 0.;
    for (int i = threadIdx.x; i < n; i += RT) {
        const double vx = V[i], vy = V[S + i], vz = V[2 * S + i];
        ex += 0.5 * ((vx - avg) * (vx - avg));                  // :939-944
        ey += 0.5 * (vy * vy);
        ez += 0.5 * (vz * vz);
        if (urow) u += urow[i];
    }
    const double rx = block_sum(ex, sh);
    const double ry = block_sum(ey, sh);
    const double rz = block_sum(ez, sh);
    const double ru = block_sum(u, sh);
    if (threadIdx.x == 0) { out[0] = rx; out[1] = ry; out[2] = rz; out[3] = ru; }
}

// output()'s per-ion columns in one array [4][n]: vx and the S / P / D populations of
// statePopulationsVsVTime (:1010-1024), the host loop's operations and order (pumping model 3:
// P = 2, 3; D = 4)
__device__ __forceinline__ void output_pack_ion(const double* V, const double* psi, int i,
                                                int n, int S, int model, double* out) {
    auto nrm = [&](int k) {
        const double re = psi[(size_t)(2 * k) * S + i], im = psi[(size_t)(2 * k + 1) * S + i];
        return re * re + im * im;
    };
    out[i] = V[i];
    out[(size_t)n + i] = nrm(0) + nrm(1);
    if (model == 3) {
        out[2 * (size_t)n + i] = nrm(2) + nrm(3);
        out[3 * (size_t)n + i] = nrm(4);
    } else {
        out[2 * (size_t)n + i] = nrm(2) + nrm(3) + nrm(4) + nrm(5);
        out[3 * (size_t)n + i] = nrm(6) + nrm(7) + nrm(8) + nrm(9) + nrm(10) + nrm(11);
    }
}

// Gaussian KDE of the velocity distributions (:957-979): bin j of axis c sums, over the
// ions of chunk z in ascending order, exp(-V2 (b_j - v)^2) + exp(-V2 (b_j + v)^2).
constexpr int KT = 256;
// jb: the workgroup's block of KT bins; sv: KT doubles of LDS.  Every thread of the workgroup calls it
// (barriers, a wave ballot).
__device__ __forceinline__ void kde_chunk(const double* V, int n, int S, double vxAvg, double* Ppart,
                                          int chunk, unsigned jb, int c, int z, double* sv) {
    const int j = jb * KT + threadIdx.x;
    const double V2 = kKdeV2;                                    // 1 / (2 * 0.002^2), :967
    const double b = (double)j * 0.0025;                         // vel[j], :340-344
    const double avg = (c == 0) ? vxAvg : 0.;
    const int i0 = z * chunk, i1 = min(n, i0 + chunk);
    double acc = 0.;
    for (int it = i0; it < i1; it += KT) {
        __syncthreads();
        if (it + (int)threadIdx.x < i1) {
            const double v = V[(size_t)c * S + it + threadIdx.x];
            sv[threadIdx.x] = (c == 0) ? (v - avg) : v;
        }
        __syncthreads();
        const int m = min(KT, i1 - it);
        for (int k = 0; k < m; ++k) {
            const double v = sv[k];
            // exp(x) is exactly +0 for x < -745.14, i.e. for |b -+ v| >= 0.0773 (V2 d^2 >= 746.9):
            // an ion whose two terms are 0 on every bin of the wave adds exact zeros there and is
            // skipped (a wave spans 0.16 of the 5.0 bin range, an ion's terms 2 x 0.155): the same
            // sums, ~15x fewer exp.  NaN velocities still take the exp path.
            const bool near = !(fabs(b - v) >= kKdeSkip) || !(fabs(b + v) >= kKdeSkip);
            if (!__builtin_amdgcn_ballot_w64(near)) continue;
            acc += exp(-V2 * (b - v) * (b - v)) + exp(-V2 * (b + v) * (b + v));
        }
    }
    if (j < NBINS) Ppart[((size_t)z * 3 + c) * NBINS + j] = acc;
}

// Pout[j] = the chunks' partials of bin j (of [3][NBINS]) in chunk order
__device__ __forceinline__ void kde_reduce_bin(const double* Ppart, int nchunk, double* Pout,
                                               int j) {
    double acc = Ppart[j];
    for (int z = 1; z < nchunk; ++z) acc += Ppart[(size_t)z * 3 * NBINS + j];
    Pout[j] = acc;
}

}  // namespace mdqt
