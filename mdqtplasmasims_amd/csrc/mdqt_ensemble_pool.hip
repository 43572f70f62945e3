// The pooled output() kernels of an ensemble of SpeedUp jobs (ensemble option "pool", mdqt_ensemble_pool_observables;
// host: mdqt_ensemble_output.cpp): the S / P / D populations binned against vx over all ions of a parameter
// point's replicas — the reference README's dark-state plot ("bin column 3 vs column 1" of
// statePopulationsVsVTime) of the whole job array.  A translation unit — hence a code object — of their own:
// the batched output kernels' code object (mdqt_ensemble_obs.hip) stays what it is, and so does EnsObsArgs.
//
// Both kernels read what k_output_pack_ens wrote (a.pack: vx, S, P, D as [4][N]) and run after k_kde_reduce_ens
// in the same stream, so the member's KDE partials (a.kde, [nch][3][NBINS]) are spent: k_popv_ens writes the
// member's slot partials over them, [nch][kPopPlanes][kPopSlots] (4,008 doubles per chunk where the KDE had
// 6,003), plane 0 holding the counts as 64-bit integers.
//
// Slots: ion i goes to slot 500 + (int)rint(vx * 100.0) when fabs(rint(vx * 100.0)) <= 500, otherwise (NaN
// included) to slot 1001, "outside"; the centres of slots 0 .. 1000 are (slot - 500) * 0.01.
// The order of every sum is fixed, with no atomics: a chunk's matching ions in ascending order onto 0, a member's
// chunks in ascending order onto 0, a point's replicas in ascending order onto 0.
#include "mdqt_ens_args.hpp"

namespace mdqt {

constexpr int PT = 256;                                       // slots per workgroup, ions per staging round
constexpr int kPopBlocks = (kPopSlots + PT - 1) / PT;         // 4

// grid (kPopBlocks, largest nch, members): one thread per slot, the chunk's ions staged in LDS PT at a time
__global__ __launch_bounds__(PT) void k_popv_ens(const EnsObsArgs* __restrict__ jobs) {
    __shared__ int ss[PT];
    __shared__ double sS[PT], sP[PT], sD[PT];
    const EnsObsArgs a = jobs[blockIdx.z];
    const int z = blockIdx.y;
    if (z >= a.nch) return;                                   // uniform over the workgroup: before any barrier
    const int slot = blockIdx.x * PT + threadIdx.x;
    const size_t n = (size_t)a.N;
    const int i0 = z * a.chunk, i1 = min(a.N, i0 + a.chunk);
    long long cnt = 0;
    double S = 0., P = 0., D = 0.;
    for (int it = i0; it < i1; it += PT) {
        __syncthreads();
        const int i = it + (int)threadIdx.x;
        if (i < i1) {
            const double r = rint(a.pack[i] * 100.0);
            ss[threadIdx.x] = (fabs(r) <= 500.) ? 500 + (int)r : kPopSlots - 1;   // NaN: the comparison is false
            sS[threadIdx.x] = a.pack[n + i];
            sP[threadIdx.x] = a.pack[2 * n + i];
            sD[threadIdx.x] = a.pack[3 * n + i];
        }
        __syncthreads();
        const int m = min(PT, i1 - it);
        for (int k = 0; k < m; ++k) {
            const bool hit = ss[k] == slot;
            if (!__builtin_amdgcn_ballot_w64(hit)) continue;  // none of the wave's 64 slots: as the KDE skips an ion
            if (hit) {
                cnt += 1;
                S += sS[k];
                P += sP[k];
                D += sD[k];
            }
        }
    }
    if (slot >= kPopSlots) return;
    double* out = a.kde + (size_t)z * kPopPlanes * kPopSlots + slot;
    reinterpret_cast<long long*>(out)[0] = cnt;
    out[kPopSlots] = S;
    out[2 * kPopSlots] = P;
    out[3 * kPopSlots] = D;
}

// grid (kPoolBlocks, points), PS slots x PL replica lanes: slot by slot, the members' chunk partials summed per member,
// the members' sums per point, into out [points][kPopPlanes][kPopSlots] (plane 0: 64-bit integers).  Point q's
// replicas are the blocks q R .. q R + R - 1.  The sums are chains of dependent additions over partials that the
// launch before left in memory, so what a thread waits for is the loads: PL replicas' member sums are formed side
// by side (one wave per lane, PS consecutive slots: the lane's block is wave-uniform), each with the loads of four
// chunks in flight ahead of their additions, and lane 0 then adds the round's sums in replica order.  Neither
// changes the order of any sum.
constexpr int PS = 64, PL = 16;
constexpr int kPoolBlocks = (kPopSlots + PS - 1) / PS;
constexpr size_t kPopChunk = (size_t)kPopPlanes * kPopSlots;  // a chunk's partials

__global__ __launch_bounds__(PS * PL) void k_popv_pool(const EnsObsArgs* __restrict__ jobs, int R, double* __restrict__ out) {
    __shared__ long long lc[PL][PS];
    __shared__ double ls[PL][3][PS];
    const int t = threadIdx.x, y = threadIdx.y;
    const int slot = blockIdx.x * PS + t;
    const bool live = slot < kPopSlots;                       // (no early return: the barriers below)
    const int q = blockIdx.y;
    long long cnt = 0;
    double S = 0., P = 0., D = 0.;
    for (int r0 = 0; r0 < R; r0 += PL) {                      // R is uniform: every thread takes every barrier
        long long c = 0;
        double s = 0., p = 0., d = 0.;
        if (live && r0 + y < R) {
            const EnsObsArgs& a = jobs[(size_t)q * R + r0 + y];
            const double* part = a.kde + slot;
            const int nch = a.nch;
            int z = 0;
            for (; z + 4 <= nch; z += 4, part += 4 * kPopChunk) {
                long long cc[4];
                double ss[4], pp[4], dd[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double* w = part + u * kPopChunk;
                    cc[u] = reinterpret_cast<const long long*>(w)[0];
                    ss[u] = w[kPopSlots];
                    pp[u] = w[2 * kPopSlots];
                    dd[u] = w[3 * kPopSlots];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { c += cc[u]; s += ss[u]; p += pp[u]; d += dd[u]; }
            }
            for (; z < nch; ++z, part += kPopChunk) {
                c += reinterpret_cast<const long long*>(part)[0];
                s += part[kPopSlots];
                p += part[2 * kPopSlots];
                d += part[3 * kPopSlots];
            }
        }
        lc[y][t] = c;
        ls[y][0][t] = s;
        ls[y][1][t] = p;
        ls[y][2][t] = d;
        __syncthreads();
        if (y == 0) {
            const int m = min(PL, R - r0);
            for (int k = 0; k < m; ++k) {
                cnt += lc[k][t];
                S += ls[k][0][t];
                P += ls[k][1][t];
                D += ls[k][2][t];
            }
        }
        __syncthreads();
    }
    if (y != 0 || !live) return;
    double* o = out + (size_t)q * kPopChunk + slot;
    reinterpret_cast<long long*>(o)[0] = cnt;
    o[kPopSlots] = S;
    o[2 * kPopSlots] = P;
    o[3 * kPopSlots] = D;
}

hipError_t launch_popv_ens(const EnsObsArgs* jobs, int npoints, int R, int max_nch, double* out, hipStream_t s, hipEvent_t ev0,
                           hipEvent_t ev1, hipEvent_t ev2, hipEvent_t ev3) {
    if (npoints <= 0 || R <= 0 || max_nch <= 0) return hipSuccess;
    if (!jobs || !out || (long long)npoints * R > 65535 || max_nch > 65535) return hipErrorInvalidValue;
    launch_timed(k_popv_ens, dim3(kPopBlocks, max_nch, npoints * R), dim3(PT), s, ev0, ev1, jobs);
    launch_timed(k_popv_pool, dim3(kPoolBlocks, npoints), dim3(PS, PL), s, ev2, ev3, jobs, R, out);
    return hipGetLastError();
}

}  // namespace mdqt
