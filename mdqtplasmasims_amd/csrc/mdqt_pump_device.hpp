// Device bodies of the optical-pumping programs' small kernels — the leapfrog halves of step(), the
// spin-up tagging and the tagged velocity distribution — shared by the single-job kernels
// (k_leapfrog_half in mdqt_kernels.hip, k_tag_spin_up in mdqt_qtfast.hip, k_tagged_kde and
// k_tagged_kde_reduce in mdmc_kernels.hip) and the batched kernels of an ensemble of pump jobs
// (mdqt_pump_ensemble_kernels.hip): one body each, so a member of the ensemble computes what it
// computes alone, bit for bit.
#pragma once

#include "mdqt_device.hpp"

#include <math.h>

namespace mdqt {

// One component of one ion through one half of step() (randomFrozenStartTag408Linear.cpp:317-375), in two
// pieces: step_V's kick v += kick f (callers skip it where kick == 0), and step_R: r += DT v (moving) or
// r += DT v + DT2 f (t == 0) with the reinsertion into [0, L].  Built with -ffp-contract=off: v += kick * f
// stays two operations.
__device__ __forceinline__ double leapfrog_kick(double v, double f, double kick) {
    v += kick * f;                                               // V[c][i] += DT*F[c][i]   :366-370
    return v;
}
__device__ __forceinline__ double leapfrog_drift(double r, double v, double f, double L, double DT, double DT2,
                                                 int moving) {
    r = moving ? r + DT * v : r + (DT * v + DT2 * f);            // :320-338
    if (r < 0) r += L;                                           // :346-354
    if (r > L) r -= L;
    return r;
}

// k_leapfrog_half's ion i
__device__ __forceinline__ void leapfrog_half_ion(double* __restrict__ R, double* __restrict__ V,
                                                  const double* __restrict__ F, int i, int S, double L, double DT,
                                                  double DT2, int moving, double kick) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t k = (size_t)c * S + i;
        double v = V[k];
        const double f = F[k];
        if (kick != 0.) { v = leapfrog_kick(v, f, kick); V[k] = v; }
        double r = R[k];
        R[k] = leapfrog_drift(r, v, f, L, DT, DT2, moving);
    }
}

// k_tag_spin_up's ion i: Philox (ion, qstep index, draws 6 and 7) for rand and rand2 / rand3
__device__ __forceinline__ void tag_spin_up_ion(const double* __restrict__ psi, int i, int S, uint64_t gid0, uint64_t q,
                                                const QTConst& qc, int* __restrict__ tags) {
    double nr[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double re = psi[(size_t)(2 * k) * S + i], im = psi[(size_t)(2 * k + 1) * S + i];
        nr[k] = re * re + im * im;                                   // std::norm
    }
    double rnd, r2;
    philox_pair(qc, gid0 + (uint64_t)i, q, 3, rnd, r2);
    int up;
    if (qc.model == 3) {                                             // 422 (:592-631)
        if (rnd < nr[0]) up = 1;
        else if (rnd < nr[0] + nr[2]) up = r2 < 1. / 3;
        else if (rnd < nr[0] + nr[2] + nr[3]) up = r2 < 2. / 3;
        else up = 0;
    } else {                                                         // 408 (:600-640)
        if (rnd < nr[0] + nr[2]) up = 1;
        else if (rnd < nr[0] + nr[2] + nr[3]) up = r2 < 2. / 3;
        else if (rnd < nr[0] + nr[2] + nr[3] + nr[4]) up = r2 < 1. / 3;
        else up = 0;
    }
    tags[i] = up;
}

// k_tagged_kde's workgroup: 256 bins (bx) x chunk `ch` of TKDE_CHUNK ions, LDS staged, ascending.
// NC = the components evaluated, the first NC of (x, y, z): 3 in the programs' own kernels, 1 where only the
// X row is written (mdmc_ensemble_qt_kernels.hip).  A component's terms, their order and its skips do not
// depend on the others, so component c of any NC holds the same bits; the partials are [chunks][NC][TKDE_BINS].
constexpr int TKDE_CHUNK = 256;

template <int NC = 3>
__device__ __forceinline__ void tagged_kde_chunk(const double* __restrict__ V, const int* __restrict__ tags, int N,
                                                 int S, int bin0, double* __restrict__ part, int bx, int ch,
                                                 double (*sv)[TKDE_CHUNK], int* st) {
    const int j = bx * 256 + threadIdx.x;
    const int i0 = ch * TKDE_CHUNK;
    const int i = i0 + threadIdx.x;
    if (i < N) {
#pragma unroll
        for (int c = 0; c < NC; ++c) sv[c][threadIdx.x] = V[c * S + i];
        st[threadIdx.x] = tags[i];
    } else {
        st[threadIdx.x] = 0;
    }
    __syncthreads();
    const double vel = (double)(j + bin0) * 0.0025;                 // QTT:250 (bin0 = -2000)
    const double V2 = kKdeV2;                                      // 1 / (2 * 0.002^2), QTT:1072
    double p[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = 0.;
    const int m = min(TKDE_CHUNK, N - i0);
    for (int k = 0; k < m; ++k) {
        if (!st[k]) continue;                                      // uniform over the workgroup
        // a component whose term is exactly +0 on every bin of the wave (|vel - v| >= 0.0773:
        // V2 d^2 >= 746.9, below exp's underflow) adds exact zeros there and is skipped
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (__builtin_amdgcn_ballot_w64(!(fabs(vel - sv[c][k]) >= kKdeSkip)))
                p[c] += exp(-V2 * (vel - sv[c][k]) * (vel - sv[c][k]));   // :1100-1102
    }
    if (j < TKDE_BINS)
#pragma unroll
        for (int c = 0; c < NC; ++c) part[((size_t)ch * NC + c) * TKDE_BINS + j] = p[c];
}

// k_tagged_kde_reduce's element k = c * TKDE_BINS + j (c < NC): the chunk partials in chunk order
template <int NC = 3>
__device__ __forceinline__ void tagged_kde_reduce_1(const double* __restrict__ part, int nch, double* __restrict__ out,
                                                    int k) {
    double s = 0.;
    for (int q = 0; q < nch; ++q) s = s + part[(size_t)q * NC * TKDE_BINS + k];
    out[k] = s / (6.0 * sqrt(2 * M_PI * 0.002 * 0.002));            // :1121-1123
}

}  // namespace mdqt
