// gfx950 kernels around the Newton-3 block kernels (mdqt_n3b.hip): what decides and checks their work.
//
//   k_n3b_plan<VARIANT, GUARD>   the call's plan: every tile pair's class, image and sub-tile groups
//   k_n3b_census                 the block kernel's work by tile-pair class (diagnostic)
//   k_tail_max, k_tail_fix       force_tail_mode 1: the measured tail bound and its enforcement
#include "mdqt_n3b.hpp"
#include "mdqt_pairs.hpp"

namespace mdqt {

// force_tail_mode 1, after the call's per-sub-tile tail sums are complete (all-reduced over the
// ranks when sharded): every tile with a sub-tile sum that, with the sum's rounding (x (1 + 1e-12)),
// exceeds eps is listed for k_tail_fix (st[3] the list length; the same list on every rank); the
// other sums' largest goes into the running maximum st[0] — the bound every ion met after the fix —
// and the largest of all into st[1] (what the skip radius alone gave); st[2] counts the tiles over
// eps (the host widens r_t when it grows), st[4] the measured calls.  Positive doubles order as
// their bit patterns.
__global__ __launch_bounds__(256) void k_tail_max(const double* __restrict__ tailb, int T, double eps,
                                                  unsigned long long* st, int* list) {
    double m = 0., mr = 0.;
    unsigned long long nf = 0;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T; t += gridDim.x * 256) {
        const double v = fmax(fmax(tailb[4 * t], tailb[4 * t + 1]), fmax(tailb[4 * t + 2], tailb[4 * t + 3]));
        mr = fmax(mr, v);
        if (v * (1. + 1e-12) > eps) {
            ++nf;
            list[atomicAdd(st + 3, 1ull)] = t;
        } else {
            m = fmax(m, v);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        m = fmax(m, __shfl_xor(m, off));
        mr = fmax(mr, __shfl_xor(mr, off));
        nf += __shfl_xor(nf, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (m > 0.) atomicMax(st, (unsigned long long)__double_as_longlong(m));
        if (mr > 0.) atomicMax(st + 1, (unsigned long long)__double_as_longlong(mr));
        if (nf) atomicAdd(st + 2, nf);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(st + 4, 1ull);
}

// force_tail_mode 1, enforcement: every listed tile's ions get their force recomputed exactly —
// all pairs inside L/2 (SpeedUp:213-224: per-pair minimum image, the exact cutoff, the fast pair
// form's values), over every J tile whose box is within L/2 of the tile's box — and the result
// REPLACES their rows of `out`: on the rank that owns the tile's block (F, or its dense partial
// before the reduce-scatter; the other ranks write 0 there, so the sum over the ranks is the exact
// force).  Replacing (not adding the dropped pairs) holds whatever the block kernel skipped: whole
// tile pairs, sub-tile groups, far forms.  One workgroup of 4 waves per listed tile (grid-stride
// over the list), wave q classifying the J tiles q*64 + l + 256 k lane-parallel and walking its
// ballot; the waves' sums combined in wave order: deterministic.  Each ion belongs to one tile, so
// `out` has one writer per ion.  With an empty list (the normal case) every workgroup reads st[3]
// and returns.
// POT (Epotential on the plan): the listed tiles' U_i = sum of u over every pair inside L/2 (pair_u<1>),
// component 0 of `out` (the per-ion potential rows)
template <bool POT = false>
__global__ __launch_bounds__(256) void k_tail_fix(N3BArgs a, const unsigned long long* __restrict__ st,
                                                  const int* __restrict__ list, double* __restrict__ out) {
    __shared__ double part[4][3][64];
    const int n = (int)st[3];
    const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
    const PairC c = {a.L, a.micT, a.micGuard, a.Rcut, a.lDeb, a.invlDeb, 1. / a.L, a.rc2, nullptr};
    const double rcut2 = a.Rcut * a.Rcut;
    const N3BRadii none = {rcut2, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY};
    const int T = a.T, N = a.N, PS = a.Npad;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int I = __builtin_amdgcn_readfirstlane(list[k]);
        const bool own = I / BW >= a.Plo && I / BW < a.Phi;
        const int i = I * 64 + l;
        const bool vi = i < N;
        const double xi = vi ? a.Rs[i] : 0., yi = vi ? a.Rs[PS + i] : 0., zi = vi ? a.Rs[2 * PS + i] : 0.;
        // per J tile a 64-term partial, added with its rounding error kept (Neumaier): the exact
        // pass's sum is accurate to a few ulp of |F| rather than carrying ~1e5 rounded additions
        double fx = 0., fy = 0., fz = 0., ex = 0., ey = 0., ez = 0.;
        auto nadd = [](double& s, double& e, double v) {
            const double t = s + v;
            e += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
            s = t;
        };
        for (int j0 = q * 64; own && j0 < T; j0 += 256) {
            const int Jl = j0 + l;
            bool in = false;
            if (Jl < T) {
                double g2;
                (void)n3b_classify<false>(a, c.invL, none, I, Jl, g2);
                in = g2 < rcut2;
            }
            unsigned long long m = __ballot(in);
            while (m) {
                const int J = j0 + __builtin_ctzll(m);
                m &= m - 1;
                const int j = J * 64 + l;
                const int nj = min(64, N - J * 64);
                const double xl = j < N ? a.Rs[j] : 0., yl = j < N ? a.Rs[PS + j] : 0., zl = j < N ? a.Rs[2 * PS + j] : 0.;
                double px = 0., py = 0., pz = 0.;
                for (int t = 0; t < nj; ++t) {
                    auto lane_t = [t](double v) {
                        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), t),
                                                __builtin_amdgcn_readlane(__double2loint(v), t));
                    };
                    double dx = xi - lane_t(xl), dy = yi - lane_t(yl), dz = zi - lane_t(zl);
                    mic_r(dx, dy, dz, c);
                    if constexpr (POT) {
                        px += pair_u<1>(dx, dy, dz, c);            // 0 beyond L/2 and for i = j
                    } else {
                        const double ft = pair_ft<1>(dx, dy, dz, c);   // 0 beyond L/2 and for i = j
                        px = fma(dx, ft, px); py = fma(dy, ft, py); pz = fma(dz, ft, pz);
                    }
                }
                nadd(fx, ex, px); nadd(fy, ey, py); nadd(fz, ez, pz);
            }
        }
        part[q][0][l] = fx + ex; part[q][1][l] = fy + ey; part[q][2][l] = fz + ez;
        __syncthreads();
        if (q == 0 && vi) {
            const int ion = a.perm[i];
            const int w = ion / a.S;
            double* o = out + (size_t)w * 3 * a.S + (ion - w * a.S);
#pragma unroll
            for (int c3 = 0; c3 < (POT ? 1 : 3); ++c3)
                o[(size_t)c3 * a.S] = ((part[0][c3][l] + part[1][c3][l]) + part[2][c3][l]) + part[3][c3][l];
        }
        __syncthreads();
    }
}

// the 105 pairings of 8 tiles (pairing words as kN3BPairsDefault)
__constant__ const unsigned kN3BMatchings[105] = {0xfac688, 0xf74688, 0xd7c688, 0xfab888, 0xf73888, 0xd7b888, 0xfa3a88, 0xf33a88, 0xd3ba88, 0xf63c88, 0xf2bc88, 0xb3bc88, 0xd63e88, 0xd2be88, 0xb33e88, 0xfac650, 0xf74650, 0xd7c650, 0xfab850, 0xf73850, 0xd7b850, 0xfa3a50, 0xf33a50, 0xd3ba50, 0xf63c50, 0xf2bc50, 0xb3bc50, 0xd63e50, 0xd2be50, 0xb33e50, 0xfac458, 0xf74458, 0xd7c458, 0xfaa858, 0xf72858, 0xd7a858, 0xfa2a58, 0xf32a58, 0xd3aa58, 0xf62c58, 0xf2ac58, 0xb3ac58, 0xd62e58, 0xd2ae58, 0xb32e58, 0xfab460, 0xf73460, 0xd7b460, 0xfaa660, 0xf72660, 0xd7a660, 0xf9aa60, 0xef2a60, 0xcfaa60, 0xf5ac60, 0xeeac60, 0xafac60, 0xd5ae60, 0xceae60, 0xaf2e60, 0xfa3468, 0xf33468, 0xd3b468, 0xfa2668, 0xf32668, 0xd3a668, 0xf9a868, 0xef2868, 0xcfa868, 0xf1ac68, 0xee2c68, 0x8fac68, 0xd1ae68, 0xce2e68, 0x8f2e68, 0xf63470, 0xf2b470, 0xb3b470, 0xf62670, 0xf2a670, 0xb3a670, 0xf5a870, 0xeea870, 0xafa870, 0xf1aa70, 0xee2a70, 0x8faa70, 0xb1ae70, 0xae2e70, 0x8eae70, 0xd63478, 0xd2b478, 0xb33478, 0xd62678, 0xd2a678, 0xb32678, 0xd5a878, 0xcea878, 0xaf2878, 0xd1aa78, 0xce2a78, 0x8f2a78, 0xb1ac78, 0xae2c78, 0x8eac78};
// Census of the block kernel's work (diagnostic; bench.py's large lines): k_pairs_n3b's loop over
// this rank's block pairs without the pair terms — every tile pair classified by n3b_classify and
// its sub-tile groups by the same sub-block gaps, counted by the path the kernel takes, as
// lane-steps (its work: 64 per step of a wave, 16 steps per sub-tile group; 40 steps on a diagonal
// tile) in out[0, kCensus) and as distinct ion pairs in out[kCensus, 2 kCensus).  Classes:
// 0 skipped (boxes beyond L/2), 1 skipped by the tail radius, 2 ragged last tile (exact, per-pair
// image), 3 exact per-pair image, 4 exact uniform image, 5 far per-pair, 6 far uniform, 7 very far
// per-pair (ultra far with a per-pair image included), 8 very far uniform, 9 ultra far uniform (f64),
// 10 ultra far uniform in f32, 11 skipped sub-tile groups of evaluated tile pairs, 12 mid per-pair,
// 13 mid uniform (round 4: appended, the earlier indices kept), 14 ultra far with a one-axis per-pair image
// (round 6: the f64 ultra-far form on the AXP path).  One workgroup
// per (block P, block distance db); thread (b, q) takes tile pair (BW P + q, BW Q + b) as the
// kernel's wave q at J-step b does.
// bw (optional): the evaluated lane-steps (every class but the skipped ones) per block of this rank,
// bw[P - Plo] — the work each block's workgroups do, for the ranks' load balance (mdqt_force_block_work)
// bal (optional, round 6): the J steps' balance over the workgroup's 8 waves — each tile pair's VALU
// instructions estimated from its groups' classes (kCensusValu: per wave-step of each form, from the ISA
// counts in docs/FORCES.md) — bal[0] += sum over the waves, bal[1] += the busiest wave's, bal[2] += 1 per
// J step with work: bal[1] / (bal[0] / 8) is the barrier-bound excess of the lock-step J loop
__constant__ const unsigned kCensusValu[kCensus] = {0, 0, 52, 48, 39, 38, 31, 32, 27, 25, 9, 0, 44, 36, 28};
__global__ __launch_bounds__(256) void k_n3b_census(N3BArgs a, unsigned long long* __restrict__ out,
                                                    unsigned long long* __restrict__ bw,
                                                    unsigned long long* __restrict__ bal) {
    __shared__ unsigned long long h[2 * kCensus];
    __shared__ unsigned long long hb;
    const int t = threadIdx.x;
    if (t < 2 * kCensus) h[t] = 0;
    if (t == 0) hb = 0;
    __syncthreads();
    unsigned long long cost = 0;                    // this tile pair's estimated VALU (bal)
    auto add = [&](int k, unsigned long long steps, unsigned long long pairs) {
        atomicAdd(&h[k], steps);
        atomicAdd(&h[kCensus + k], pairs);
        if (k != 0 && k != 1 && k != 11) atomicAdd(&hb, steps);
        cost += (steps / 64) * kCensusValu[k];
    };
    const int P = a.Plo + (int)blockIdx.x / a.nd, db = (int)blockIdx.x % a.nd;
    const int q = t & (BW - 1), b = t / BW;
    const int Q = (P + db) % a.NB;
    const int I = P * BW + q, J = Q * BW + b;
    const bool half = n3b_half_covered(a.NB, P, db);
    if (!half && I < a.T && J < a.T && (db > 0 || J >= I)) {
        const N3BRadii rad = n3b_radii<1, false>(a);
        double g2;
        int sm = 0;
        const double4 t4 = n3b_classify<true>(a, 1. / a.L, rad, I, J, g2, &sm);
        const bool diag = db == 0 && J == I;
        // (a per-pair image on one axis, AXP instance: levels 4 and 5 in the f64 ultra-far form, class 14)
        constexpr bool AX1U = (kAx1Levels & 16u) != 0;
        const bool ax1p = AX1U && n3b_axp(a) && ((n3b_pack_class(t4, sm) >> 28) & 3);
        const double nI = (double)min(64, a.N - I * 64), nJ = (double)min(64, a.N - J * 64);
        const bool rag = (a.N & 63) && (I == a.T - 1 || J == a.T - 1);
        const bool uni = ((int)t4.w & 1) != 0;
        // the class of a group at far level gl (the kernel's dispatch)
        auto cls_of = [&](unsigned gl) {
            if (rag) return 2;
            if (uni) return gl == 5 ? 10 : gl == 4 ? 9 : gl == 3 ? 8 : gl == 2 ? 6 : gl == 1 ? 13 : 4;
            return (ax1p && gl >= 4) ? 14 : gl >= 3 ? 7 : gl == 2 ? 5 : gl == 1 ? 12 : 3;
        };
        if (t4.w < 0.) {
            add(t4.w == -2. ? 1 : 0, 4096ull, (unsigned long long)(nI * nJ));
        } else if (diag) {
            add(cls_of(0), 2560ull, (unsigned long long)(nI * (nI - 1) / 2));
        } else {
            const int T4 = 4 * a.T;
            const double hj2 = raw_half2(a.boxes, a.T, J);
            unsigned act = 0, mm = 0, mf = 0, mv = 0, mu = 0, m32 = 0;
            double np[4] = {0., 0., 0., 0.};       // ion pairs per group
            for (int sa = 0; sa < 4; ++sa)
                for (int sb = 0; sb < 4; ++sb) {
                    const double sg = sub_gap2(a.subboxes, T4, 4 * I + sa, 4 * J + sb, a.L, 1. / a.L);
                    const unsigned bit = 1u << (4 * sa + sb);
                    if (sg <= rad.rc2) act |= bit;
                    if (sg > rad.rm2) mm |= bit;
                    if (sg > rad.rf2) mf |= bit;
                    if (sg > rad.rv2) mv |= bit;
                    if (sg > rad.ru2) mu |= bit;
                    if (sg > rad.ru32 && sg > 4. * hj2 &&   // (k_n3b_plan's level 5)
                        (!a.formm || !uni || sub_far2(a.subboxes, T4, 4 * I + sa, 4 * J + sb, a.L, 1. / a.L) < a.u32lim2))
                        m32 |= bit;
                    np[(sb - sa) & 3] += sub_count(a.N, 4 * I + sa) * sub_count(a.N, 4 * J + sb);
                }
            const unsigned g = a.use_sort == 1 ? sub_groups_of(act) : 0xFu;   // (2: nothing skipped)
            const unsigned lv = sub_group_levels(mm, mf, mv, mu, m32);
            for (int d = 0; d < 4; ++d)
                add((g >> d) & 1u ? cls_of((lv >> (4 * d)) & 15u) : 11, 1024ull, (unsigned long long)np[d]);
        }
    }
    if (bal) {                                      // the 8 threads of J step b: lanes 8 (b mod 8) .. + 7
        unsigned long long sm = cost, mx = cost;
#pragma unroll
        for (int off = 1; off < BW; off <<= 1) {
            sm += __shfl_xor(sm, off);
            const unsigned long long o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
        }
        if (q == 0 && sm) {
            atomicAdd(bal, sm);
            atomicAdd(bal + 1, mx);
            atomicAdd(bal + 2, 1ull);
        }
        // schedules that move no work between waves (what a J-order change could reach): bal[3] the pairs
        // of J steps (b, b + 1) each run as two sub-steps with every wave on one of the two J tiles, the
        // best of the 256 choices; bal[4] the same pairs in lock-step; bal[5] per (P, db) the busiest
        // wave's sum over its 8 J steps (any J order's floor)
        const int lane = t & 63, base = lane & ~15;     // the pair's 16 costs: lanes base .. base + 15
        unsigned long long c16[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) c16[k] = __shfl(cost, base + k);
        if (lane == base) {
            unsigned long long cur = 0, m0 = 0, m1 = 0, best = ~0ull;
            for (int k = 0; k < 8; ++k) { m0 = c16[k] > m0 ? c16[k] : m0; m1 = c16[8 + k] > m1 ? c16[8 + k] : m1; }
            cur = m0 + m1;
            for (unsigned S = 0; S < 256; ++S) {        // wave k in S: J step b first, b + 1 second
                unsigned long long a1 = 0, a2 = 0;
                for (int k = 0; k < 8; ++k) {
                    const unsigned long long x = c16[k], y = c16[8 + k];
                    const bool in = (S >> k) & 1u;
                    const unsigned long long f = in ? x : y, g = in ? y : x;
                    a1 = f > a1 ? f : a1;
                    a2 = g > a2 ? g : a2;
                }
                best = a1 + a2 < best ? a1 + a2 : best;
            }
            if (cur) { atomicAdd(bal + 3, best); atomicAdd(bal + 4, cur); }
        }
        unsigned long long rw = cost;                   // wave q's sum over the workgroup's 8 J steps
#pragma unroll
        for (int off = BW; off < 64; off <<= 1) rw += __shfl_xor(rw, off);
        __shared__ unsigned long long rws[BW];
        if (lane < BW) rws[lane] = 0;
        __syncthreads();
        if (lane < BW) atomicAdd(&rws[lane], rw);
        __syncthreads();
        if (t == 0) {
            unsigned long long m = 0;
            for (int k = 0; k < BW; ++k) m = rws[k] > m ? rws[k] : m;
            if (m) atomicAdd(bal + 5, m);
        }
        // 4 waves, each on two I tiles per J step (the pair's costs add): bal[6] the pairing of the heaviest
        // row with the lightest (per (P, db)), bal[7] the fixed pairing (q, 7 - q), bal[8] (q, q + 4) — each
        // the sum over J steps of 2 x the busiest wave's pair, comparable with bal[1]
        unsigned long long c64[BW * BW];
#pragma unroll
        for (int k = 0; k < BW * BW; ++k) c64[k] = __shfl(cost, k);   // c64[q + 8 b]
        if (t == 0) {
            unsigned long long row[BW];
            int ord[BW];
            for (int k = 0; k < BW; ++k) { row[k] = 0; ord[k] = k; }
            for (int b = 0; b < BW; ++b)
                for (int k = 0; k < BW; ++k) row[k] += c64[k + BW * b];
            for (int i = 1; i < BW; ++i)                // rows by cost, descending
                for (int j = i; j > 0 && row[ord[j]] > row[ord[j - 1]]; --j) { const int x = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = x; }
            unsigned long long hl = 0, fx = 0, f4 = 0, ps = 0;
            for (int b = 0; b < BW; ++b) {
                unsigned long long m1 = 0, m2 = 0, m3 = 0, m4 = 0;
                int os[BW];                             // this J step's own heavy-light pairing (bal[9])
                for (int k = 0; k < BW; ++k) os[k] = k;
                for (int i = 1; i < BW; ++i)
                    for (int j = i; j > 0 && c64[os[j] + BW * b] > c64[os[j - 1] + BW * b]; --j) { const int x = os[j]; os[j] = os[j - 1]; os[j - 1] = x; }
                for (int k = 0; k < BW / 2; ++k) {
                    const unsigned long long p4 = c64[os[k] + BW * b] + c64[os[BW - 1 - k] + BW * b];
                    m4 = p4 > m4 ? p4 : m4;
                }
                ps += m4;
                for (int k = 0; k < BW / 2; ++k) {
                    const unsigned long long p1 = c64[ord[k] + BW * b] + c64[ord[BW - 1 - k] + BW * b];
                    const unsigned long long p2 = c64[k + BW * b] + c64[BW - 1 - k + BW * b];
                    const unsigned long long p3 = c64[k + BW * b] + c64[k + BW / 2 + BW * b];
                    m1 = p1 > m1 ? p1 : m1; m2 = p2 > m2 ? p2 : m2; m3 = p3 > m3 ? p3 : m3;
                }
                hl += m1; fx += m2; f4 += m3;
            }
            unsigned long long bm = ~0ull;          // the best of the 105 pairings of this (P, db) (bal[10])
            for (int m = 0; m < 105; ++m) {
                const unsigned pw = kN3BMatchings[m];
                unsigned long long cm = 0;
                for (int b = 0; b < BW; ++b) {
                    unsigned long long mx = 0;
                    for (int k = 0; k < BW / 2; ++k) {
                        const unsigned long long v = c64[((pw >> (6 * k)) & 7) + BW * b] + c64[((pw >> (6 * k + 3)) & 7) + BW * b];
                        mx = v > mx ? v : mx;
                    }
                    cm += mx;
                }
                bm = cm < bm ? cm : bm;
            }
            if (hl) { atomicAdd(bal + 6, hl); atomicAdd(bal + 7, fx); atomicAdd(bal + 8, f4); atomicAdd(bal + 9, ps); atomicAdd(bal + 10, bm); }
        }
    }
    __syncthreads();
    if (t < 2 * kCensus && h[t]) atomicAdd(out + t, h[t]);
    if (bw && t == 0 && hb) atomicAdd(bw + (P - a.Plo), hb);
}

// The block kernel's plan (force calls in spatial order): every tile pair of this rank's block pairs
// classified once per call, before k_pairs_n3b, so that its staging lanes read one 8-byte word per
// tile pair instead of classifying — work the block kernel's other BW - 1 waves waited out at every J
// step's barrier (the sub-tile classification there cost C5 +8 %).  plan[((P - Plo) nd
// + db) BW^2 + BW b + q] is tile pair (BW P + q, BW Q + b), Q = P + db mod NB: .x its class and
// uniform-image multiples (n3b_pack_class), .y its sub-tile groups by pair form:
//  * group d = the sub-blocks (a, (a + d) & 3) of the tile pair's 4 x 4 (16-ion sub-tiles; the block
//    kernel's lane 16 a + m runs them as its d-th 16-step group); its gap is the least of their four
//    sub-box gaps.  It runs iff that gap is within the skip radius (force_sort 1; 2 runs all), in the
//    pair form the gap allows (the far level every pair of the group reaches: each form's error
//    bound needs every pair that far apart, which the sub-boxes guarantee).  .y = groups | (the
//    groups of far level x) << (4 + 4 x), x = 0..4; 0xFF (all groups, exact form) where unused.
//  * tail sums (force_tail_mode 1, a.tailb): every pair the call drops inside L/2 — in a tile pair
//    the tail radius skips (class -2) or in a skipped group — is at least its sub-block gap apart, so
//    each ion of I sub-tile a loses at most sum_b n_b g(gap_ab) and each ion of J sub-tile b at most
//    sum_a n_a g(gap_ab); counted once per unordered tile pair, summed per sub-tile in LDS over the
//    workgroup and added to tailb (128 atomics per workgroup).
// One workgroup per (P, db), thread (b, q) — the census's decomposition.
// the plan kernel's occupancy (round 6, A/B r06p_plan_ab.txt, bit-identical): 3 waves per SIMD (168 VGPRs,
// 2 spilled) with the LDS boxes: plan stage N = 1M 9.4 -> 7.8 ms, C5 0.75 -> 0.58 ms; 4 (128 VGPRs, 37
// spilled) is slower than 2
constexpr int kPlanWpe = 3;
template <int VARIANT, bool GUARD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kPlanWpe)))
void k_n3b_plan(N3BArgs a, uint2* __restrict__ plan) {
    __shared__ double ti[BW][4], tj[BW][4];
    __shared__ unsigned jm;
    constexpr bool FARF = VARIANT == 1 && !GUARD;
    const int t = threadIdx.x, q = t & (BW - 1), b = t / BW;
    const int Pl = (int)blockIdx.x / a.nd, db = (int)blockIdx.x % a.nd;
    const int P = a.Plo + Pl, Q = (P + db) % a.NB;
    const int I = P * BW + q, J = Q * BW + b;
    const bool tmeas = a.tailb != nullptr;
    if (tmeas && t < 4 * BW) { ti[t >> 2][t & 3] = 0.; tj[t >> 2][t & 3] = 0.; }
    if (t == 0) jm = 0u;
    // the workgroup's boxes in LDS: the BW I tiles' and BW J tiles' [12] box columns and
    // their 4 BW sub-tiles' [6] — each read once, coalesced, instead of per tile pair from L2 (the kernel's
    // ~190 global loads held ~200 VGPRs: 2 waves per SIMD); the same values, the same operations
    __shared__ double bI[12][BW], bJ[12][BW], sI[6][4 * BW], sJ[6][4 * BW];
    {
        const int T4 = 4 * a.T;
        for (int k = t; k < 12 * BW; k += BW * BW) {
            const int row = k / BW, c = k % BW;
            bI[row][c] = P * BW + c < a.T ? a.boxes[(size_t)row * a.T + P * BW + c] : 0.;
            bJ[row][c] = Q * BW + c < a.T ? a.boxes[(size_t)row * a.T + Q * BW + c] : 0.;
        }
        if (a.subboxes)
            for (int k = t; k < 6 * 4 * BW; k += BW * BW) {
                const int row = k / (4 * BW), c = k % (4 * BW);
                sI[row][c] = 4 * P * BW + c < T4 ? a.subboxes[(size_t)row * T4 + 4 * P * BW + c] : 0.;
                sJ[row][c] = 4 * Q * BW + c < T4 ? a.subboxes[(size_t)row * T4 + 4 * Q * BW + c] : 0.;
            }
    }
    __syncthreads();
    // box column accessors into LDS (row stride BW / 4 BW)
    const double* const Bi = &bI[0][q];
    const double* const Bj = &bJ[0][b];
    constexpr int bld = BW;
    // (the closures also hold I and J by reference, as they did while the accessors had a global-memory
    // form: the kernel's register allocation — 168 VGPRs, 2 spilled, above — was tuned with them, and the
    // compiler schedules the kernel differently without)
    auto SBi = [&](int sa) -> const double* { (void)I; return &sI[0][4 * q + sa]; };
    auto SBj = [&](int sb) -> const double* { (void)J; return &sJ[0][4 * b + sb]; };
    constexpr int sld = 4 * BW;
    uint2 w = make_uint2(1u, 0xFFu);                // class -1 where the block kernel never looks
    double gi[4] = {0., 0., 0., 0.}, gj[4] = {0., 0., 0., 0.};   // this tile pair's tail terms per sub-tile
    // (n3b_half_covered, written out: through the function the compiler schedules this kernel differently,
    // and its register allocation — kPlanWpe above — is tuned)
    const bool half = !(a.NB & 1) && db == a.NB / 2 && P >= a.NB / 2;
    // the paired-wave kernel's work estimate of this tile pair (n3b_pair_cost: from the geometry alone, the
    // same with force_sort 1 and 2, so that both take the same pairing and stay bit-identical)
    unsigned cest = 0;
    if (!half && I < a.T && J < a.T && (db > 0 || J >= I)) {
        const N3BRadii rad = n3b_radii<VARIANT, false>(a);
        const double invL = 1. / a.L;
        double g2;
        int sm;
        const int pw = n3b_pack_class(n3b_classify_p<VARIANT == 1>(Bi, Bj, bld, a.L, invL, a.Rcut, a.use_sort, rad, g2, &sm),
                                       VARIANT == 1 ? sm : 0);
        const int cls = (pw & 15) - 2;
        w.x = (unsigned)pw;
        const bool rag = (a.N & 63) && (I == a.T - 1 || J == a.T - 1);
        const bool uni = cls >= 0 && (cls & 1);
        if (db == 0 && J == I && !(g2 > rad.rc2)) cest = (rag ? 52u : uni ? 39u : 48u) * 40u;
        if ((db > 0 || J > I) && (cls >= 0 || (tmeas && cls == -2))) {
            double sg[4][4];
#pragma unroll
            for (int sa = 0; sa < 4; ++sa)
#pragma unroll
                for (int sb = 0; sb < 4; ++sb) sg[sa][sb] = sub_gap2_p(SBi(sa), SBj(sb), sld, a.L, invL);
            unsigned groups = 0u, lvm = 0u;
            double gm[4];
#pragma unroll
            for (int d = 0; d < 4; ++d)
                gm[d] = fmin(fmin(sg[0][d & 3], sg[1][(1 + d) & 3]), fmin(sg[2][(2 + d) & 3], sg[3][(3 + d) & 3]));
            // the f32 level needs J's raw box diagonal within the group's gap (kUfar32A/B): J's extents
            // read only where a group is that far
            const double gmax = fmax(fmax(gm[0], gm[1]), fmax(gm[2], gm[3]));
            const double hj4 = FARF && gmax > rad.ru32 ? 4. * raw_half2_p(Bj, bld) : 0.;
            int xs[4];                              // the groups' levels (the measured form bound)
            // (formm) the whole tile pair within u32lim2 under its image — tile boxes: every sub-block is
            bool tile_in = false;
            if (FARF && a.formm && gmax > rad.ru32 && uni)
                tile_in = sub_far2_p(Bi, Bj, bld, a.L, invL) < a.u32lim2;   // ([12][T]: centers, half extents first)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                int x = !FARF ? 0 : n3b_level(gm[d], rad);
                if (x == 5 && !(gm[d] > hj4)) x = 4;
                if (x == 5 && a.formm && uni && !tile_in) {   // f32 only where no pair can reach the cutoff (u32lim2)
                    double f2 = 0.;
#pragma unroll
                    for (int sa = 0; sa < 4; ++sa)
                        f2 = fmax(f2, sub_far2_p(SBi(sa), SBj((sa + d) & 3), sld, a.L, invL));
                    if (!(f2 < a.u32lim2)) x = 4;
                }
                xs[d] = x;
                if (gm[d] <= rad.rc2 && !(g2 > rad.rc2)) cest += n3b_pair_cost(x, uni, rag);
                if (a.use_sort != 1 || gm[d] <= rad.rc2) {
                    groups |= 1u << d;
                    lvm |= 1u << (4 * x + d);
                }
            }
            if (cls >= 0) w.y = groups | (lvm << 4);
            if (tmeas) {
                const double rcut2 = a.Rcut * a.Rcut;
                const float invl = (float)a.invlDeb, cf = (float)(a.invlDeb * kNegLog2e);
                constexpr bool AX1U = FARF && (kAx1Levels & 16u) != 0;
                const bool ax1p = AX1U && n3b_axp(a) && ((pw >> 28) & 3);
#pragma unroll
                for (int sa = 0; sa < 4; ++sa)
#pragma unroll
                    for (int sb = 0; sb < 4; ++sb) {
                        const int d = (sb - sa) & 3;
                        const bool drop = cls == -2 || !((groups >> d) & 1u);
                        // the form the block kernel takes for the group (n3b_tile_pair): exact on a ragged
                        // tile pair; with a per-pair image levels >= 3 in the very-far form, but levels 4
                        // and 5 in the f64 ultra-far form on the one-axis path (AXP instance, LV bit 4)
                        const int e = (drop || !a.formm || rag) ? 0 : uni ? xs[d]
                                    : (ax1p && xs[d] >= 4) ? 4 : min(xs[d], 3);
                        if ((drop || e > 0) && sg[sa][sb] < rcut2) {
                            const double gd = drop ? tail_g(sg[sa][sb], invl, cf) : form_term(sg[sa][sb], invl, cf, e);
                            gi[sa] += sub_count(a.N, 4 * J + sb) * gd;
                            gj[sb] += sub_count(a.N, 4 * I + sa) * gd;
                        }
                    }
            }
        }
    }
    plan[((size_t)Pl * a.nd + db) * (BW * BW) + t] = w;
    if (tmeas) {
        // the workgroup's sums per sub-tile: I sub-tiles over b (lanes q, q + 16, q + 32, q + 48 of
        // each wave, then one LDS add per wave), J sub-tiles over q (16 consecutive lanes: b's own)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            double vi = gi[u], vj = gj[u];
#pragma unroll
            for (int off = BW; off < 64; off <<= 1) vi += __shfl_xor(vi, off);
#pragma unroll
            for (int off = BW / 2; off >= 1; off >>= 1) vj += __shfl_xor(vj, off);
            if ((t & 63) < BW && vi > 0.) atomicAdd(&ti[q][u], vi);
            if (q == 0) tj[b][u] = vj;              // (one writer per b)
        }
    }
    // the J-step mask of (P, db): J step b has work iff one of its tile pairs has a class >= 0
    // (threads BW b .. BW b + BW - 1 are lanes BW (b mod 64/BW) .. of wave b / (64/BW))
    const unsigned long long wk = __ballot((int)(w.x & 15u) >= 2);
    if ((t & 63) == 0) {
        constexpr int per = 64 / BW;
        unsigned mw = 0u;
#pragma unroll
        for (int k = 0; k < per; ++k) mw |= ((wk >> (BW * k)) & ((1ull << BW) - 1)) ? 1u << k : 0u;
        atomicOr(&jm, mw << (per * (t >> 6)));
    }
    // k_pairs_n3b_pw's pairing (.y of the J-step word): the tiles' estimated work over the 8 J steps (threads
    // q, q + 8, ... hold tile q's tile pairs), the busiest tile with the least busy, and so on
    unsigned rc = cest;
#pragma unroll
    for (int off = BW; off < 64; off <<= 1) rc += __shfl_xor(rc, off);
    // lanes 0 .. BW-1 hold the BW tiles' sums (lane t: tile t mod BW); each of them takes its tile's place in
    // the order (descending by work, ties by tile: the stable insertion sort's order) and its field of the
    // pairing word — the busiest tile with the least busy, and so on, 6 bits per pair — OR-ed over the lanes
    // (round 6: one thread's serial sort cost the plan stage ~1.5 ms of 8 at N = 1M)
    unsigned pr = 0;
    {
        unsigned row[BW];
#pragma unroll
        for (int k = 0; k < BW; ++k) row[k] = __shfl(rc, k);
        int rk = 0;
#pragma unroll
        for (int k = 0; k < BW; ++k) rk += (row[k] > rc || (row[k] == rc && k < t)) ? 1 : 0;
        if (t < BW) pr = rk < BW / 2 ? (unsigned)t << (6 * rk) : (unsigned)t << (3 + 6 * (BW - 1 - rk));
#pragma unroll
        for (int off = 1; off < BW; off <<= 1) pr |= __shfl_xor(pr, off);
    }
    __syncthreads();
    if (t == 0)
        plan[(size_t)(a.Phi - a.Plo) * a.nd * (BW * BW) + (size_t)Pl * a.nd + db] = make_uint2(jm, pr);
    // the reduction's per-J-tile masks: J step b has work -> the block kernel writes J's j-slot db
    if (a.tmask && t < BW && ((jm >> t) & 1u))
        atomicOr(a.tmask + (size_t)(Q * BW + t) * a.tmw + (db >> 6), 1ull << (db & 63));
    if (tmeas) {
        if (t < 4 * BW) {
            const int k = t >> 2, u = t & 3;
            if (ti[k][u] > 0.) atomicAdd(a.tailb + 4 * (P * BW + k) + u, ti[k][u]);
            if (tj[k][u] > 0.) atomicAdd(a.tailb + 4 * (Q * BW + k) + u, tj[k][u]);
        }
    }
}

hipError_t launch_n3b_plan(const N3BArgs& a, int variant, hipStream_t s) {
    const int nplan = (a.Phi - a.Plo) * a.nd;
    if (a.plan && nplan > 0) {
        if (!a.use_sort || !a.boxes || !a.subboxes) return hipErrorInvalidValue;   // spatial order only
        if (a.tmask && hipMemsetAsync(a.tmask, 0, (size_t)a.T * a.tmw * sizeof(unsigned long long), s) != hipSuccess)
            return hipGetLastError();
        by_variant_guard<2>(variant, a.guard, [&](auto V, auto G) {
            hipLaunchKernelGGL((k_n3b_plan<decltype(V)::value, decltype(G)::value>), dim3(nplan), dim3(BW * BW), 0, s,
                               a, a.plan);
        });
    } else if (a.tailb && !a.plan) {
        return hipErrorInvalidValue;                // the tail sums come from the plan (a rank without blocks: 0)
    }
    return hipGetLastError();
}

hipError_t launch_tail_max(const double* tailb, int T, double eps, unsigned long long* st, int* list, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tail_max, dim3((T + 255) / 256 < 64 ? (T + 255) / 256 : 64), dim3(256), 0, s, tailb, T, eps,
                       st, list);
    return hipGetLastError();
}

hipError_t launch_tail_fix(const N3BArgs& a, const unsigned long long* st, const int* list, double* out,
                           hipStream_t s, bool pot) {
    if (a.T <= 0 || !a.Rs || !a.perm || !a.boxes) return hipErrorInvalidValue;   // spatial order only
    if (pot) hipLaunchKernelGGL(k_tail_fix<true>, dim3(a.T < 512 ? a.T : 512), dim3(256), 0, s, a, st, list, out);
    else hipLaunchKernelGGL(k_tail_fix<false>, dim3(a.T < 512 ? a.T : 512), dim3(256), 0, s, a, st, list, out);
    return hipGetLastError();
}

hipError_t launch_n3b_census(const N3BArgs& a, unsigned long long* out, hipStream_t s, unsigned long long* bw,
                             unsigned long long* bal) {
    if (!a.use_sort || !a.boxes || !a.subboxes) return hipErrorInvalidValue;   // the classes need the boxes
    const int nblk = (a.Phi - a.Plo) * a.nd;
    if (hipMemsetAsync(out, 0, 2 * kCensus * sizeof(unsigned long long), s) != hipSuccess) return hipGetLastError();
    if (bw && a.Phi > a.Plo && hipMemsetAsync(bw, 0, (size_t)(a.Phi - a.Plo) * sizeof(unsigned long long), s) != hipSuccess)
        return hipGetLastError();
    if (bal && hipMemsetAsync(bal, 0, 11 * sizeof(unsigned long long), s) != hipSuccess) return hipGetLastError();
    if (nblk > 0) hipLaunchKernelGGL(k_n3b_census, dim3(nblk), dim3(BW * BW), 0, s, a, out, bw, bal);
    return hipGetLastError();
}

}  // namespace mdqt
