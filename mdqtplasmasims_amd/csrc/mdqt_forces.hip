// gfx950 force kernels: forces() (SpeedUp:192-236) and the pair potential of Epotential()
// (SpeedUp:244-281).
//
//   k_pairs<MODE, VARIANT>   owner-computes rows, LDS-staged j tiles, j split in segments
//   k_pairs_n3<VARIANT>      Newton-3 over 64x64 tile pairs, 4 waves per pair (one GPU)
//   k_reduce_segments        canonical sum of the partials when a caller asks for F
// (Newton-3 over block pairs, large N and sharded: mdqt_n3b.hip, mdqt_n3b_plan.hip)
//
// VARIANT 0 keeps the reference's operations (sqrt, the three divisions, libm exp) without
// contraction; VARIANT 1 (default) is the reciprocal form (rsq3) with a range-specialised exp and
// FMA contraction — a few ulp per pair, inside the 1e-13 force gate.  VARIANT 2 (Newton-3
// tiles; the MC + MD program, whose lattice start puts pairs exactly on the cutoff and on the
// image boundary) has variant 1's values with variant 0's pair set: the exact minimum image and
// the cutoff as r2 < rc2, rc2 the smallest double with sqrt(rc2) >= Rcut.
#include "mdqt_internal.hpp"
#include "mdqt_pairs.hpp"

#include <math.h>

namespace mdqt {

// ------------------------------------------------------------------------------------------
// rows: owner computes row i over the j of its segment in ASCENDING j (the single-thread
// reference's F_i is exactly that sum; the self pair has r = 0 and is dropped
// by the 0 < r test like the reference's coincident pairs)
// ------------------------------------------------------------------------------------------
constexpr int FT = 256;

template <int MODE, int VARIANT, bool GUARD>
__device__ __forceinline__ void rows_body(const ForceArgs& a, const PairC& c, double* sx, double* sy,
                                          double* sz) {
    const int tid = threadIdx.x;
    const int li = blockIdx.x * FT + tid;
    const int seg = blockIdx.y;
    const bool active = li < a.nrows;
    const int gi = a.row_lo + li;
    double rx = 0., ry = 0., rz = 0.;
    if (active) {
        const double* p = pos_base(a.Rall, gi, a.S);
        rx = p[0]; ry = p[a.S]; rz = p[2 * a.S];
    }
    double fx = 0., fy = 0., fz = 0.;
    const int j0 = seg * a.seglen;
    const int j1 = min(a.N, j0 + a.seglen);
    for (int jt = j0; jt < j1; jt += FT) {
        const int jl = jt + tid;
        __syncthreads();
        if (jl < j1) {
            const double* p = pos_base(a.Rall, jl, a.S);
            sx[tid] = p[0]; sy[tid] = p[a.S]; sz[tid] = p[2 * a.S];
        }
        __syncthreads();
        const int nj = min(FT, j1 - jt);
        if (active) {
#pragma unroll 2
            for (int k = 0; k < nj; ++k) {
                double dx = rx - sx[k], dy = ry - sy[k], dz = rz - sz[k];   // :213-215
                mic_v<VARIANT, GUARD>(dx, dy, dz, c);
                if (MODE == 0) {
                    const double ft = pair_ft<VARIANT>(dx, dy, dz, c);
                    accum<VARIANT>(fx, dx, ft);
                    accum<VARIANT>(fy, dy, ft);
                    accum<VARIANT>(fz, dz, ft);
                } else {
                    const double u = pair_u<VARIANT>(dx, dy, dz, c);
                    if (VARIANT == 0) fx += u;
                    else fx += u;
                }
            }
        }
    }
    if (active) {
        double* o = a.Fpart + (size_t)seg * 3 * a.S;
        o[li] = fx;
        if (MODE == 0) { o[a.S + li] = fy; o[2 * a.S + li] = fz; }
    }
}

template <int MODE, int VARIANT, bool GUARD>
__global__ __launch_bounds__(FT) void k_pairs(ForceArgs a) {
    __shared__ double sx[FT], sy[FT], sz[FT];
    const PairC c = {a.L, a.micT, a.micGuard, a.Rcut, a.lDeb, a.invlDeb, 1. / a.L};
    rows_body<MODE, VARIANT, GUARD>(a, c, sx, sy, sz);
}

__global__ __launch_bounds__(256) void k_reduce_segments(const double* __restrict__ Fpart,
                                                         double* __restrict__ F, int nseg,
                                                         int nrows, int S, int ncomp, size_t plane) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= nrows || c >= ncomp) return;
    reduce_segments_row(Fpart, F, nseg, S, plane, i, c);
}

#if defined(MDQT_EXPT_STAMPS)
// diagnostic build only: per-workgroup start/end (s_memrealtime, 100 MHz) and placement
__device__ unsigned long long g_n3_stamps[6 * 8192];
#endif

template <int VARIANT, bool GUARD>
__global__ __launch_bounds__(64 * N3W) void k_pairs_n3(N3Args a) {
    __shared__ double pj[3][128];
    __shared__ double accj[N3W][3][128];
    __shared__ double ia[N3W][3][64];
    __shared__ double mj[128];
    __shared__ double etab[64];
#if defined(MDQT_EXPT_STAMPS)
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    const unsigned long long c_start = __builtin_amdgcn_s_memtime();
#endif
    stage_exp_tab(etab);
    const int2 IJ = a.pairs[blockIdx.x];
    const PairC c = {a.L, a.micT, a.micGuard, a.Rcut, a.lDeb, a.invlDeb, 1. / a.L, a.rc2, etab};
    const bool rag = (a.N & 63) && IJ.y == a.ntiles - 1;
    if (a.arrive) {
        if (rag) n3_tile<VARIANT, GUARD, true, true>(a, c, IJ.x, IJ.y, pj, accj, mj, ia);
        else n3_tile<VARIANT, GUARD, false, true>(a, c, IJ.x, IJ.y, pj, accj, mj, ia);
    } else {
        if (rag) n3_tile<VARIANT, GUARD, true, false>(a, c, IJ.x, IJ.y, pj, accj, mj, ia);
        else n3_tile<VARIANT, GUARD, false, false>(a, c, IJ.x, IJ.y, pj, accj, mj, ia);
    }
#if defined(MDQT_EXPT_STAMPS)
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < 8192) {
        const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
        const unsigned long long c_end = __builtin_amdgcn_s_memtime();
        g_n3_stamps[6 * blockIdx.x] = t_start;
        g_n3_stamps[6 * blockIdx.x + 1] = t_end;
        g_n3_stamps[6 * blockIdx.x + 2] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID
        g_n3_stamps[6 * blockIdx.x + 3] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // XCC_ID
        g_n3_stamps[6 * blockIdx.x + 4] = c_start;                                       // core clock
        g_n3_stamps[6 * blockIdx.x + 5] = c_end;
    }
#endif
}

// Epotential() (:244-281) on the Newton-3 tiles: each distinct pair's u once, to both ions' rows
// (slot component 0; the caller sums the ntiles slots per ion)
template <int VARIANT, bool GUARD>
__global__ __launch_bounds__(64 * N3W) void k_pairs_n3_pot(N3Args a) {
    __shared__ double pj[3][128];
    __shared__ double accj[N3W][3][128];
    __shared__ double ia[N3W][3][64];
    __shared__ double mj[128];
    n3_pot_pair<VARIANT, GUARD>(a, blockIdx.x, pj, accj, mj, ia);   // mdqt_pairs.hpp
}

#if defined(MDQT_EXPT_STAMPS)
extern "C" int mdqt_expt_n3_stamps(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_n3_stamps), sizeof(unsigned long long) * 6 * n) == hipSuccess ? 0 : -1;
}
#endif

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
static int seg_blocks(int nrows) { return (nrows + FT - 1) / FT; }

template <int MODE>
static hipError_t launch_rows(const ForceArgs& a, hipStream_t s) {
    if (a.nrows <= 0) return hipSuccess;
    dim3 grid(seg_blocks(a.nrows), a.nseg);
    by_variant_guard<2>(a.variant, a.guard, [&](auto V, auto G) {
        hipLaunchKernelGGL((k_pairs<MODE, decltype(V)::value, decltype(G)::value>), grid, dim3(FT), 0, s, a);
    });
    return hipGetLastError();
}

hipError_t launch_forces(const ForceArgs& a, hipStream_t s) { return launch_rows<0>(a, s); }
hipError_t launch_potential_rows(const ForceArgs& a, hipStream_t s) { return launch_rows<1>(a, s); }

hipError_t launch_reduce_segments(const double* Fpart, double* F, int nseg, int nrows, int S, int ncomp,
                                  hipStream_t s, size_t plane) {
    if (nrows <= 0) return hipSuccess;
    if (ncomp < 1 || ncomp > 3) return hipErrorInvalidValue;
    if (plane == 0) plane = (size_t)3 * S;
    if (plane < (size_t)ncomp * S) return hipErrorInvalidValue;
    dim3 grid((nrows + 255) / 256, ncomp);
    hipLaunchKernelGGL(k_reduce_segments, grid, dim3(256), 0, s, Fpart, F, nseg, nrows, S, ncomp, plane);
    return hipGetLastError();
}

hipError_t launch_forces_n3(const N3Args& a, int variant, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (a.npairs <= 0) return hipSuccess;
    dim3 grid(a.npairs);
    by_variant_guard<3>(variant, a.guard, [&](auto V, auto G) {
        launch_timed(k_pairs_n3<decltype(V)::value, decltype(G)::value>, grid, dim3(64 * N3W), s, ev0, ev1, a);
    });
    return hipGetLastError();
}

hipError_t launch_potential_n3(const N3Args& a, int variant, hipStream_t s) {
    if (a.npairs <= 0) return hipSuccess;
    if (variant < 0 || variant > 1) return hipErrorInvalidValue;
    const dim3 grid(a.npairs), blk(64 * N3W);
    by_variant_guard<2>(variant, a.guard, [&](auto V, auto G) {
        hipLaunchKernelGGL((k_pairs_n3_pot<decltype(V)::value, decltype(G)::value>), grid, blk, 0, s, a);
    });
    return hipGetLastError();
}

}  // namespace mdqt
