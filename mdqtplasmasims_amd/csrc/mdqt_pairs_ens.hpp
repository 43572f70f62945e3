// k_pairs_n3_ens — the batched Newton-3 force kernel of an ensemble of jobs — as a template that two
// translation units instantiate: mdqt_ensemble_forces.hip (the SpeedUp ensemble's variants 0 and 1, with and
// without the guard) and mdmc_ensemble_kernels.hip (the MC + MD ensemble's variants 2 and 0 without it).  Each
// unit is a code object of its own, so adding an instance for one program leaves the other's as it was.
#pragma once

#include "mdqt_internal.hpp"
#include "mdqt_pairs.hpp"

namespace mdqt {

// forces() of an ensemble of independent jobs in one launch: grid (max npairs, jobs), x fastest, so
// consecutive workgroups are one job's tile pairs (its positions and slots stay close in time for L2).
// Each job's argument block — its own pairs table (split or plain), slots and one-slot case — lives in
// device memory; the body is k_pairs_n3's without arrival counts, so a job's F is bit for bit what its
// own launch gives.  Workgroups past a job's last tile pair leave before any LDS use or barrier.
template <int VARIANT, bool GUARD>
__global__ __launch_bounds__(64 * N3W) void k_pairs_n3_ens(const N3Args* __restrict__ jobs) {
    __shared__ double pj[3][128];
    __shared__ double accj[N3W][3][128];
    __shared__ double ia[N3W][3][64];
    __shared__ double mj[128];
    __shared__ double etab[64];
    const N3Args& a = jobs[blockIdx.y];
    if ((int)blockIdx.x >= a.npairs) return;
    stage_exp_tab(etab);
    const int2 IJ = a.pairs[blockIdx.x];
    const PairC c = {a.L, a.micT, a.micGuard, a.Rcut, a.lDeb, a.invlDeb, 1. / a.L, a.rc2, etab};
    const bool rag = (a.N & 63) && IJ.y == a.ntiles - 1;
    if (rag) n3_tile<VARIANT, GUARD, true, false>(a, c, IJ.x, IJ.y, pj, accj, mj, ia);
    else n3_tile<VARIANT, GUARD, false, false>(a, c, IJ.x, IJ.y, pj, accj, mj, ia);
}

}  // namespace mdqt
