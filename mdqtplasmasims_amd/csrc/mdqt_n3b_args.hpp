// The Newton-3 block scheme's interface between the host engine and its kernels (mdqt_n3b.hip, mdqt_n3b_plan.hip,
// mdqt_sort.hip): the argument blocks and the launchers of the force and potential calls, the spatial order, the
// tail pass and the census.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mdqt {

// Newton-3 over block pairs (mdqt_n3b.hip k_pairs_n3b): blocks of kN3BBlock tiles, cyclic half
// shell of block distances, slots [nd + R][3][Npad] (j-slots by distance, i-slots by run).
// A rank runs the workgroups of blocks [Plo, Phi); k_n3b_reduce sums the slots it wrote.
struct N3BArgs {
    const double* Rall; // gathered positions [world][3][S]
    double* slots;      // [nd + R][3][Npad]
    int N, S, T, Npad;  // ions, slab stride, tiles, T * 64
    int NB, nd, R, runlen;   // blocks, half-shell distances NB/2 + 1, runs per block, distances per run
    int Plo, Phi;       // this rank's blocks
    double L, lDeb, Rcut, invlDeb, micT, micGuard;
    int guard;
    // spatial order (mdqt_sort.hip): tiles are 64 consecutive ions of the Hilbert order
    int use_sort;       // 1: positions from Rs, slots by sorted index, tile pairs beyond L/2 skipped;
                        // 2: the same order, nothing skipped (tests: bit-identical to 1)
    int pairs;          // 1: the paired-wave block kernel (k_pairs_n3b_pw; option "force_n3b_pairs"), 0: k_pairs_n3b
    int ax1;            // 1: the one-axis per-pair image instance where the skip radius reaches the image
                        // boundary (launch_forces_n3b; option "force_ax1"), 0: every per-pair image on all axes
    const double* Rs;   // [3][Npad] positions in sorted order
    const int* perm;    // sorted index -> ion
    const double* boxes;// [12][T]: tile center (x, y, z), half extents, raw coordinate min, max
    double Rmid;        // sub-tile groups >= Rmid apart take the mid pair form (rsq1 + table 2^t, ~2e-14
                        // relative; forces only); >= Rcut: never
    double Rfar;        // tile pairs whose boxes are >= Rfar apart take the far pair form (kFarRelErr;
                        // forces only, use_sort 1 or 2); >= Rcut: never
    double Rvfar;       // >= Rvfar apart: the very-far form (raw rsq, degree-5 2^f); >= Rcut: never
    double Rufar;       // >= Rufar apart: the ultra-far form (raw rsq, v_exp_f32); >= Rcut: never
    double Rufar32;     // >= Rufar32 apart (uniform image): the ultra-far form in f32
    double rc2;         // Rcut^2: the very-far and ultra-far forms keep a pair iff r^2 < rc2 (r^2 in f64,
                        // as exact as the exact form's r < Rcut), not on their low-precision r
    double Rskip;       // force tile pairs whose boxes are >= Rskip apart are skipped (use_sort 1):
                        // Rcut exactly (every skipped pair is beyond L/2), or the error-bounded tail
                        // radius r_t < L/2 of mdqt_force_plan.cpp tail_radius (potentials: always Rcut)
    double* tailb;      // force_tail_mode 1: per 16-ion sub-tile [4T], the sum over the pairs the call
                        // drops inside L/2 (tail-skipped tile pairs, skipped sub-tile groups) of
                        // n_b g(sub-block gap) — the measured bound on what each of its ions loses
                        // (zeroed before the launch, summed by k_n3b_plan; nullptr: not measured)
    int formm;          // force_form_mode 1 (round 6): tailb also sums, over the sub-blocks evaluated in an
                        // error-bounded form, n_b g(gap) err_form(gap) — the forms' measured bound, enforced
                        // with the tail's (k_tail_max, k_tail_fix); the tier radii come from a density model
    double u32lim2;     // formm: (Rcut (1 - 2^-20))^2 — a group takes the f32 ultra-far form only if every
                        // pair of it is closer (its boxes' far distance in the minimum image, sub_far2), so
                        // the f32 r^2 never decides the cutoff (no a-priori cutoff term)
    const double* subboxes;   // [6][4T]: the 16-ion sub-tiles' centers and half extents (use_sort)
    uint2* plan;        // force calls in spatial order: [(Phi - Plo) nd][kN3BBlock^2] tile-pair words, then
                        // [(Phi - Plo) nd] J-step masks (.x), written by k_n3b_plan (launch_forces_n3b)
                        // and read by k_pairs_n3b; nullptr: classified in the block kernel (every
                        // sub-tile group exact; no tail sums)
    unsigned long long* tmask;   // with a plan: [T][tmw] bit db of J tile's words = the block kernel wrote J's
    int tmw;                     // j-slot db (a J step with work); k_n3b_reduce reads only those (nullptr: all)
};
struct SortArgs {
    const double* Rall; // gathered positions [world][3][S]
    int N, S, Npad;
    double L;
    uint32_t *keys, *keys2;  // [N] Hilbert keys, sorted keys
    int *ion, *perm;         // [N] identity, sorted index -> ion
    void* tmp;               // hipCUB radix-sort scratch
    size_t tmp_bytes;
    double* Rs;              // out [3][Npad]
    double* boxes;           // out [12][T]
    double* subboxes;        // out [6][4T]: the 16-ion sub-tiles' centers and half extents (or null)
};
hipError_t launch_spatial_order(const SortArgs& a, hipStream_t s);
size_t spatial_order_tmp_bytes(int N);
// ev0/ev1: the block kernel's own dispatch timestamps (timing on; k_pairs_n3b alone, not the plan or
// the reduction); marks (optional, the force-call breakdown): 3 events recorded after the plan, after the
// block kernel and after the slot reduction
hipError_t launch_forces_n3b(const N3BArgs& a, int variant, double* out, hipStream_t s, hipEvent_t ev0 = nullptr,
                             hipEvent_t ev1 = nullptr, hipEvent_t* marks = nullptr);
// Epotential on the Newton-3 blocks (world 1): per-ion row sums of u into out[S]; with a.plan on the force
// call's plan (skips, sub-tile groups, error-bounded forms; tail sums into a.tailb), else exact to L/2;
// ev0/ev1 (optional) time the block kernel
hipError_t launch_potential_n3b(const N3BArgs& a, int variant, double* out, hipStream_t s, hipEvent_t ev0 = nullptr,
                                hipEvent_t ev1 = nullptr);
// force_tail_mode 1 (mdqt_n3b_plan.hip): the per-sub-tile tail sums [4T] against eps — st[0] running
// max of the tiles within eps, st[1] of all, st[2] tiles over eps (cumulative), st[3] this call's
// list length, st[4] measured calls — and the exact recomputation of the listed tiles' forces,
// written into `out` ([world][3][S], by ion) on the rank that owns the tile (0 on the others); pot: their
// potential rows U_i (component 0) instead
hipError_t launch_tail_max(const double* tailb, int T, double eps, unsigned long long* st, int* list, hipStream_t s);
hipError_t launch_tail_fix(const N3BArgs& a, const unsigned long long* st, const int* list, double* out,
                           hipStream_t s, bool pot = false);
// census of k_pairs_n3b's work by tile-pair class (mdqt_n3b_plan.hip k_n3b_census): out[2 kCensus]
constexpr int kCensus = 15;                 // (round 6: + 14 ufar_image)
// tiles per block of the Newton-3 block kernel (= its waves per workgroup): 8 (round 4, A/B vs 16:
// C3 -2.7 %, C5 -2.5 %, N = 1M -4.3 % per force call — three 8-wave workgroups per CU at 80 VGPRs
// instead of two 16-wave ones at 64: shorter J-step barriers, fewer spills; 4: slower)
constexpr int kN3BBlock = 8;
hipError_t launch_n3b_census(const N3BArgs& a, unsigned long long* out, hipStream_t s, unsigned long long* bw = nullptr,
                             unsigned long long* bal = nullptr);
hipError_t launch_sum_rank_chunks(const double* const* parts, int world, int rank, int S, double* F, hipStream_t s);

}  // namespace mdqt
