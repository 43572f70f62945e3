"""Exact row sums of the Yukawa force / pair potential and the per-ion error bound of a kernel.

A helper like tests/dense_qt.py (not a test file).  Everything that is *summed* here is long double
(64-bit mantissa: u_ld = 2^-64 against the kernels' u = 2^-53); only the reference's pair set is
decided in double, the way SpeedUp:213-222 decides it:

    dx = xi - xj;  dx -= L*round(dx/L)  (C round: halves away from zero);
    dr = sqrt(dx*dx + dy*dy + dz*dz);   keep the pair iff 0 < dr < L/2.

For a kept pair the separation d is the long double value of (xi - xj) - n L with the same image n
(n L is exact, the subtractions round at 2^-64), r = |d|, lam = lDeb,

    g(r) = (1/r^2 + 1/(r lam)) e^(-r/lam)            (the force is g d/r)
    u(r) = e^(-r/lam) / r                            (the pair potential)

and the row sums over the pair set S_i of ion i are

    T_i = sum g d/r       P_i = sum g       G_i = sum (|g'| + 2 g/r)       E_i = sum g (KT r/lam + KF)
    U_i = sum u           Gu_i = sum |u'|   Eu_i = sum u (KT r/lam + KU)
    |g'| = (2/r^3 + 2/(r^2 lam) + 1/(r lam^2)) e^(-r/lam),    |u'| = u (1/r + 1/lam).

Shell pairs are the pairs, in S_i or not, with |r - L/2| <= 8 L 2^-53; H_i = sum g and Hu_i = sum u
over them, and nshell counts them (ordered pairs of the requested rows).

The bound.  A kernel's F_i with summation depth D is held to

    gate_i = GEOM sqrt(3) L u G_i  +  u (D P_i + E_i)  +  [fast variant only] H_i,       u = 2^-53

and U_i to the same with Gu_i, U_i, Eu_i, Hu_i.  Every term is derived, none is measured:

* Geometry.  A kernel does not see d but d + dd.  The unscaled forms round xi - xj once (half an ulp of
  a value below 2 L) and the image once more (mic_r's fma; the threshold form's dx -+ L): two roundings
  per axis, each <= 1.25 L u for |dx| <= 1.25 L.  The box-scaled tile form (n3_terms SC) rounds both
  positions to s = x fl(1/L) (<= u in box units for |s| in [1, 9/8], u/2 below 1), rounds ds = si - sj
  (<= u for |ds| >= 1, u/2 below) and carries fl(1/L)'s own relative error u on ds (<= 1.25 u on
  |ds| <= 1.25: an image n != 0 turns it into an absolute error).  The worst case is the pair at
  |dx| = 1.25 L, one ion at 9L/8: u + u/16 + u + 1.25 u = 3.3 u; every other placement gives <= 2.7 u.
  The issue's figure for this constant is 3 (it leaves fl(1/L) out); this count is larger, so
  GEOM = 3.5 roundings of L u per axis and |dd| <= GEOM sqrt(3) L u.  To first order the force of a
  pair moves by |g'| |dd| along d and by g |dd| / r across it: <= (|g'| + 2 g/r) |dd|.  The states of
  the tests keep |dd| / r near 1e-8 at most (closest pair 1e-6, |dd| <= 1.1e-14 in the box of
  N0 = 1000), so the second-order term is about 1e-8 of the first.  Positions outside [-L/8, 9L/8] (the range-guard instances) have larger separations and so
  larger half-ulps: geom_roundings() counts them from the state.
* Per term.  In units of u, relative to the term g d_k / r:
    the scaled form (n3_terms SC): r2 by two FMAs and a product (3, all terms positive) -> 1.5 on r;
    rsq3 <= 2 (1.7e-16 measured, mdqt_math.hpp), so ri carries 3.5 and enters cubed: 10.5;
    fma(ri, sA, sB) with sA = fl(1/L)^2 and sB = fl(1/lDeb) fl(1/L), three roundings each: 3 + 1;
    the table's 2^t, <= 2 ulp: 4;  the products (.) 2^t, ri ri, (.)(ri ri), d ft: 4  -> 22.5 <= KF = 24.
    The exponent t = dr sT: sT = L (fl(1/lDeb) (64 fl(-log2 e))) carries 4, dr = r2 ri carries
    1.5 + 2 + 1, the product 1: 9.5, which enters 2^t multiplied by |t| ln 2 = r/lam.  The issue's
    figure is 8; this count is larger, so KT = 10.
    pair_ft<1> / pair_ft_cut (rows, unscaled tiles): the same without sA, sB and L: 19.5 and 8.5.
    pair_ft<0> (the reference's operations): sqrt 2.5, 1/dr + 1/lDeb 4.5, glibc / ocml exp 1 ulp = 2,
    dr dr 6, two products and the division 3 -> 15.5; the exponent -dr/lDeb carries 3.5.
    pair_u: e^(-r/lam) ri: 3.5 + 4 + 1 <= KU = 12, the same exponent.
  The weights mi mj (1.0) and m (1.0 or 0.0) of the ragged tiles are exact.
* Summation.  Any order of D dependent additions of terms |t_k| <= g is within D u sum g = D u P_i.
    rows:  D = ceil(N / nseg) + nseg + 8   (a segment's ascending-j sum, then the segments)
    tiles: D = 64 + 4 + slots + 8          (a wave's steps, the 4 waves and the j halves, the slots,
                                            slots counting the split's extra ones)
    the reference / the oracle: D = N + 8.
* The cutoff shell.  The fast variant documents that it may decide a pair within an ulp of r = L/2
  differently (mdqt_pairs.hpp, mic_r): a whole term g, so H_i.  The exact variant claims the
  reference's pair set bit for bit and gets no such allowance.

phi = max_i |dF_i|_inf / (u P_i) over ions with H_i = 0 measures an instance on the scale of its own
row sum; the tests compare it with the same figure of the reference's operations (the oracle).

The Newton-3 blocks (force_scheme 3: k_pairs_n3b, k_pairs_n3b_pw, k_n3b_reduce, k_tail_fix) are held to

    gate_i = [the gate above with D = depth_blocks(N)]  +  Form_i  +  Tail_i,

and U_i to the same with FormU_i, TailU_i.  The three block terms come from the truth's separations and
the constants the engine publishes (the radii of the call, mdqt_math.hpp's kFormErrA/B); none from a
device result.

* Summation (depth_blocks).  T = ceil(N/64) tiles, NB = ceil(T/8) blocks, nd = NB/2 + 1 block distances
  in R runs of runlen (n3b_set_range: R = min(nd, ceil(65536/NB)), runlen = ceil(nd/R), R =
  ceil(nd/runlen); N <= 5000: runlen = 1, R = nd).  A pair term reaches F_i along one of two chains:
    i side:  the tile pair's fresh sum (<= 64 steps: four 16-step groups, 40 on the diagonal tile), into
             the block distance's sum (<= 8 J tiles), into the run's sum in LDS (runlen), the i-slot;
    j side:  the wave's LDS accumulator (64 ds_add_f64 per tile pair; the paired-wave kernel adds its
             two tile pairs of a J step into one: 128), the two LDS copies (1), the fixed pairwise tree
             over the 8 or 4 waves (3 or 2), the j-slot;
  then k_n3b_reduce adds the nd j-slots and the R i-slots in one chain.  A term takes part in at most
    D = max(64 + 8 + runlen, 128 + 1 + 3) + nd + R + 8
  additions (the 8 as the rows' and tiles': the kernel's own zero starts and the negation-free combine), and
  any tree in which no term meets more than D additions is within D u sum |t_k| to first order.  The f32
  ultra-far form's 16-term f32 partial sums are part of its stated error (kUfar32B's 15u), not of D.
  k_tail_fix's replaced rows: a 64-term partial per J tile, compensated across tiles, 4 waves: below D.
  One chain over every term, N + 8, bounds any order (pad ions and masked lanes add exact zeros), so
  depth_blocks returns min(D, N + 8): the count above exceeds it only at N = 129 (142 against 137).
* Per term.  The exact instances (VARIANT 0, guarded or not) run pair_ft<0> / pair_u<0>, the fast ones
  (guarded or not) pair_ft_cut / pair_ft<1> (k_tail_fix) / pair_u<1>: counted above, within KF, KU, KT.
  n3_terms adds one product with the rotation weight (1.0 or 0.0) and, on a ragged tile, mi mj (1.0 or
  0.0): exact.  Uniform image (SHIFT) and one-axis image (AXP): the lane's xi - n L is one fma (one
  rounding, <= 1.25 L u), then sx - xj one more: two roundings per axis, what the per-pair image's
  (xi - xj) - n L has (equal bit for bit where n = 0), inside GEOM = 3.5.  No recount needed.
* Form_i.  A sub-tile group evaluated in the pair form of plan level e (1 mid, 2 far, 3 very far, 4
  ultra far, 5 ultra far in f32; n3b_level) has every sub-box gap, hence every pair, at r >= R_e; the
  kernel may take a lower level than the gap allows (ragged tiles and the diagonal: exact; a per-pair
  image: levels 4, 5 as 3 or 4; an f32 group whose J box is too wide: 4), never a higher one, and the
  stated relative errors err_e(r) = kFormErrA[e] r/lDeb + kFormErrB[e] grow with e at every r (asserted in
  tests/test_force_truth.py).  So
      Form_i = sum_j g(r_ij) err_level(r_ij)(r_ij),   level(r) = the highest enabled e with R_e <= r
  (a tier is enabled when its radius is below L/2), FormU_i the same with u (pair_u_cut's error is
  within the force form's: one factor ri instead of three).  The level is taken at r (1 + 2^-50): the
  truth's double r against the engine's double radius.  err_e is pinned to mdqt_force_plan.cpp's far_err
  through mdqt_tier_radius_model on the CPU.
  With a-priori radii (force_form_mode 0, or no measured tail) the f32 tier decides the cutoff on its f32
  r^2: fl32 relative coordinates and three f32 operations put r^2 within 11 x 2^-24 of itself
  (mdqt_math.hpp, kUfar32A/B's derivation: r within 5.5 x 2^-24, and fl32(rc2) another half), so a pair
  within F32CUT 2^-24 L/2 of L/2, F32CUT = 6, inside the reference's pair set or not, may be decided either
  way: a whole term g (u) each, added to Form_i — the analogue of H_i.  (far_radius_l's comment still
  says 3 x 2^-24, the round-3 form's count; its term (N - 1) g(L/2 (1 - 2^-20)) covers a shell 16 x 2^-24
  wide.)  The measured modes keep the f32 form off every group that can reach L/2 (u32lim2): no such term.
* Tail_i = sum g over the pairs of S_i with r >= R_skip (force_skip_radius): a skipped tile pair or sub-tile
  group has its boxes, hence its pairs, at least R_skip apart.  0 where R_skip = L/2.  Rows that k_tail_fix
  replaced hold every pair to L/2 in pair_ft<1> and are inside the gate without it.
"""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "force_truth needs a long double with a 64-bit mantissa"

U53 = 2.0 ** -53
GEOM = 3.5          # roundings of L u per axis of a separation (positions within [-L/8, 9L/8])
KT = 10.0           # roundings carried by the exponent, times r/lam
KF = 24.0           # roundings of a force term
KU = 12.0           # roundings of a potential term
SHELL = 8.0         # shell pairs: |r - L/2| <= SHELL L u


def c_round(x):
    """C round(): halves away from zero (np.round goes to even)"""
    r = np.trunc(x)
    f = x - r                          # exact
    return r + (f >= 0.5) - (f <= -0.5)


def pair_set(R, L, idx):
    """the reference's image multiples n[3][m][N] and pair set keep[m][N] of rows idx, in double"""
    R = np.asarray(R, dtype=np.float64)
    d = R[:, idx, None] - R[:, None, :]
    n = c_round(d / L)
    d = d - L * n
    dr = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return n, (dr > 0) & (dr < L / 2)


class Rows:
    """the row sums of ions idx (arrays of len(idx); T is [3][len(idx)]), all long double"""
    __slots__ = ("idx", "T", "P", "G", "E", "H", "U", "Gu", "Eu", "Hu", "nshell")


def row_sums(R, L, lDeb, idx=None, chunk=128):
    R = np.ascontiguousarray(R, dtype=np.float64)
    N = R.shape[1]
    idx = np.arange(N) if idx is None else np.asarray(idx, dtype=np.int64)
    m = len(idx)
    out = Rows()
    out.idx = idx
    out.T = np.zeros((3, m), LD)
    for k in ("P", "G", "E", "H", "U", "Gu", "Eu", "Hu"):
        setattr(out, k, np.zeros(m, LD))
    out.nshell = 0
    Rl = R.astype(LD)
    Ll, lam = LD(L), LD(lDeb)
    half, width = Ll / 2, LD(SHELL * U53) * Ll
    for a in range(0, m, chunk):
        ii = idx[a:a + chunk]
        n, keep = pair_set(R, L, ii)
        d = (Rl[:, ii, None] - Rl[:, None, :]) - Ll * n.astype(LD)
        r = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        other = r > 0                                   # not the ion itself (nor a coincident one)
        r = np.where(other, r, LD(1))
        e = np.exp(-r / lam)
        u = e / r
        g = (1 / (r * r) + 1 / (r * lam)) * e
        gp = (2 / (r * r * r) + 2 / (r * r * lam) + 1 / (r * lam * lam)) * e
        shell = other & (np.abs(r - half) <= width)
        w = np.where(keep, g, LD(0))
        wu = np.where(keep, u, LD(0))
        s = slice(a, a + len(ii))
        out.T[:, s] = (w * d / r).sum(axis=2)
        out.P[s] = w.sum(axis=1)
        out.G[s] = np.where(keep, gp + 2 * g / r, LD(0)).sum(axis=1)
        out.E[s] = (w * (KT * r / lam + KF)).sum(axis=1)
        out.U[s] = wu.sum(axis=1)
        out.Gu[s] = (wu * (1 / r + 1 / lam)).sum(axis=1)
        out.Eu[s] = (wu * (KT * r / lam + KU)).sum(axis=1)
        out.H[s] = np.where(shell, g, LD(0)).sum(axis=1)
        out.Hu[s] = np.where(shell, u, LD(0)).sum(axis=1)
        out.nshell += int(shell.sum())
    return out


def row_sums_threads(R, L, lDeb, nthreads=8):
    """row_sums of every ion, the rows split over threads (numpy's long double loops release the GIL): the
    same sums row for row, each row's in the same order"""
    from concurrent.futures import ThreadPoolExecutor
    N = np.asarray(R).shape[1]
    parts = [p for p in np.array_split(np.arange(N), nthreads) if len(p)]
    with ThreadPoolExecutor(len(parts)) as ex:
        rows = list(ex.map(lambda p: row_sums(R, L, lDeb, p), parts))
    out = Rows()
    out.idx = np.arange(N)
    out.T = np.concatenate([r.T for r in rows], axis=1)
    for k in ("P", "G", "E", "H", "U", "Gu", "Eu", "Hu"):
        setattr(out, k, np.concatenate([getattr(r, k) for r in rows]))
    out.nshell = sum(r.nshell for r in rows)
    return out


def geom_roundings(R, L):
    """roundings of L u per axis of a separation: GEOM inside [-L/8, 9L/8]; outside, the half-ulps of
    the largest separation (its subtraction) and of the largest image shift n L (the division form's
    L round(dx/L)), in units of L u, plus one for the rounding of the result"""
    R = np.asarray(R, dtype=np.float64)
    if R.min() >= -L / 8 and R.max() <= 9 * L / 8:
        return GEOM
    span = float((R.max(axis=1) - R.min(axis=1)).max()) + L / 2
    half_ulp = 2.0 ** (math.floor(math.log2(span)) - 53)
    return max(GEOM, 2 * half_ulp / (L * U53) + 1)


def force_gate(t, L, D, fast, geom=GEOM):
    g = LD(geom * math.sqrt(3.0) * L * U53) * t.G + LD(U53) * (LD(D) * t.P + t.E)
    return g + t.H if fast else g


def potential_gate(t, L, D, fast, geom=GEOM):
    g = LD(geom * math.sqrt(3.0) * L * U53) * t.Gu + LD(U53) * (LD(D) * t.U + t.Eu)
    return g + t.Hu if fast else g


def force_err(F, t):
    """|F_i - T_i|_inf per ion (F: [3][N] of all ions, or [3][len(idx)] of the rows)"""
    F = np.asarray(F)
    if F.shape[1] != len(t.idx):
        F = F[:, t.idx]
    return np.abs(F.astype(LD) - t.T).max(axis=0)


def potential_err(U, t):
    U = np.asarray(U)
    if U.shape[0] != len(t.idx):
        U = U[t.idx]
    return np.abs(U.astype(LD) - t.U)


def phi(err, scale, H):
    """max_i err_i / (u scale_i) over the ions off the cutoff shell"""
    ok = H == 0
    return float((err[ok] / (LD(U53) * scale[ok])).max())


def depth_rows(N, nseg):
    return -(-N // nseg) + nseg + 8


def depth_tiles(slots):
    return 64 + 4 + slots + 8


# ---------------------------------------------------------------------------------------------
# the Newton-3 blocks (force_scheme 3)
# ---------------------------------------------------------------------------------------------

BLOCK_TILES = 8            # kN3BBlock: tiles per block (512 ions)
BLOCK_WORKGROUPS = 65536   # n3b_set_range's workgroups per rank


def block_layout(N):
    """(T, NB, nd, R, runlen) of the block scheme at world 1 (mdqt_engine.cpp n3b_set_range)"""
    T = -(-N // 64)
    NB = -(-T // BLOCK_TILES)
    nd = NB // 2 + 1
    R = min(nd, -(-BLOCK_WORKGROUPS // NB))
    runlen = -(-nd // R)
    return T, NB, nd, -(-nd // runlen), runlen


def depth_blocks(N):
    _, _, nd, R, runlen = block_layout(N)
    return min(max(64 + BLOCK_TILES + runlen, 128 + 1 + 3) + nd + R + 8, N + 8)


# mdqt_math.hpp: kRsq1RelErr, kTab4RelErr, kFarRelErr, kRsqRawErr, kExp5RelErr, kExp2fRelErr, kUfar32A/B
_RSQ1, _TAB4, _FAR, _RSQRAW, _EXP5, _EXP2F = 2.2e-14, 4e-15, 3e-9, 2.0 ** -23, 1.1e-7, 2.0 ** -22
# kFormErrA/B by plan level (n3b_level): 0 exact, 1 mid, 2 far, 3 very far, 4 ultra far, 5 ultra far in f32
FORM_A = (0.0, _RSQ1 + 2.0 ** -52, 0.0, _RSQRAW, _RSQRAW + 2.0 ** -24, 22 * 2.0 ** -24)
FORM_B = (0.0, 3 * (_RSQ1 + 2.0 ** -52) + _TAB4, _FAR, 3 * _RSQRAW + _EXP5, 3 * _RSQRAW + _EXP2F, 52 * 2.0 ** -24)
# plan level -> the level numbering of mdqt_force_plan.cpp's far_err and mdqt_tier_radius_model
MODEL_LEVEL = {1: 5, 2: 1, 3: 2, 4: 3, 5: 4}
TIERS = {1: "mid", 2: "far", 3: "vfar", 4: "ufar", 5: "ufar32"}     # force_<name>_radius
F32CUT = 6.0               # the f32 tier's cutoff shell: |r - L/2| <= F32CUT 2^-24 L/2


def form_err(e, r, lDeb):
    """err_e(r): the stated relative error of a pair term at distance r in the form of plan level e"""
    return FORM_A[e] * (r / lDeb) + FORM_B[e]


class BlockTerms:
    """Form_i, FormU_i, Tail_i, TailU_i of ions idx (double: bounds, not truths)"""
    __slots__ = ("idx", "form", "formu", "tail", "tailu", "nform", "ntail", "ncut")


def block_terms(R, L, lDeb, radii, skip, f32cut, idx=None, chunk=256, nthreads=8):
    """the blocks' gate terms over the reference's pair set: radii = {plan level: R_e} (missing or >= L/2:
    off), skip = R_skip, f32cut: the f32 tier decides its own cutoff (a-priori radii).  nform[e], ntail, ncut
    count the ordered pairs at level e, beyond R_skip and on the f32 cutoff shell.  The rows in chunks over
    threads (numpy's loops release the GIL); each row's sum is the same whatever the split"""
    from concurrent.futures import ThreadPoolExecutor
    R = np.ascontiguousarray(R, dtype=np.float64)
    N = R.shape[1]
    idx = np.arange(N) if idx is None else np.asarray(idx, dtype=np.int64)
    m = len(idx)
    half = L / 2
    on = sorted(e for e, r in radii.items() if r < half)
    cut = f32cut and 5 in on

    def rows(a):
        ii = idx[a:a + chunk]
        n, keep = pair_set(R, L, ii)
        d = (R[:, ii, None] - R[:, None, :]) - L * n
        r = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        other = r > 0
        r = np.where(other, r, 1.0)
        e_ = np.exp(-r / lDeb)
        u = e_ / r
        g = (1 / (r * r) + 1 / (r * lDeb)) * e_
        up = r * (1 + 2.0 ** -50)
        err = np.zeros_like(r)
        lev = np.zeros(r.shape, dtype=np.int8)
        for e in on:                                    # ascending: the highest level with R_e <= r stays
            at = keep & (up >= radii[e])
            err = np.where(at, form_err(e, r, lDeb), err)
            lev[at] = e
        form, formu = (g * err).sum(axis=1), (u * err).sum(axis=1)
        ncut = 0
        if cut:
            shell = other & (np.abs(r - half) <= F32CUT * 2.0 ** -24 * half)
            form += np.where(shell, g, 0.0).sum(axis=1)
            formu += np.where(shell, u, 0.0).sum(axis=1)
            ncut = int(shell.sum())
        far = keep & (up >= skip) if skip < half else np.zeros_like(keep)
        return (a, form, formu, np.where(far, g, 0.0).sum(axis=1), np.where(far, u, 0.0).sum(axis=1),
                {e: int((lev == e).sum()) for e in on}, int(far.sum()), ncut)

    out = BlockTerms()
    out.idx = idx
    for k in ("form", "formu", "tail", "tailu"):
        setattr(out, k, np.zeros(m))
    out.nform, out.ntail, out.ncut = {e: 0 for e in on}, 0, 0
    with ThreadPoolExecutor(nthreads) as ex:
        for a, form, formu, tail, tailu, nform, ntail, ncut in ex.map(rows, range(0, m, chunk)):
            s = slice(a, a + len(form))
            out.form[s], out.formu[s], out.tail[s], out.tailu[s] = form, formu, tail, tailu
            for e in on:
                out.nform[e] += nform[e]
            out.ntail += ntail
            out.ncut += ncut
    return out


def rounding_part(t, L, D, geom=GEOM, potential=False):
    """the geometry and rounding terms of the gate: no shell, form or tail allowance"""
    return potential_gate(t, L, D, False, geom) if potential else force_gate(t, L, D, False, geom)


def block_force_gate(t, b, L, D, fast, geom=GEOM):
    return force_gate(t, L, D, fast, geom) + b.form.astype(LD) + b.tail.astype(LD)


def block_potential_gate(t, b, L, D, fast, geom=GEOM):
    return potential_gate(t, L, D, fast, geom) + b.formu.astype(LD) + b.tailu.astype(LD)


# ---------------------------------------------------------------------------------------------
# the states
# ---------------------------------------------------------------------------------------------

def random_state(N, L, seed=2024):
    return np.random.default_rng([seed, N]).uniform(0.0, L, (3, N))


def clustered_state(N, L, frac, rc, seed=2024):
    """a fraction frac of the N ions uniform in a ball of radius rc at the box centre, the rest uniform in
    the box, in random index order: far from the uniform density the skip radius's model assumes"""
    rng = np.random.default_rng([seed, N, 7])
    nc = int(frac * N)
    v = rng.normal(size=(3, nc))
    v /= np.linalg.norm(v, axis=0)
    ball = L / 2 + v * (rc * rng.uniform(0, 1, nc) ** (1 / 3))
    R = np.concatenate([rng.uniform(0.0, L, (3, N - nc)), ball], axis=1)[:, rng.permutation(N)]
    return np.ascontiguousarray(R)


def clumped_state(N, L, per=64, radius=1.0, seed=2024):
    """ions in compact clumps of `per` (the last one smaller), uniform in balls of `radius` whose centres are
    uniform in the box: in spatial order a 64-ion tile is then ~2 wide instead of the uniform density's ~6.4,
    and whole tile pairs lie beyond the cutoff at a few thousand ions already"""
    rng = np.random.default_rng([seed, N, 11])
    nc = -(-N // per)
    c = rng.uniform(radius, L - radius, (3, nc))
    v = rng.normal(size=(3, N))
    v /= np.linalg.norm(v, axis=0)
    R = np.repeat(c, per, axis=1)[:, :N] + v * (radius * rng.uniform(0, 1, N) ** (1 / 3))
    assert R.min() >= 0 and R.max() <= L
    return np.ascontiguousarray(R)


NDESIGNED = 14


def designed_state(N, L, seed=2024):
    """the random state with its first 14 ions on the edges of the geometry; every designed separation
    is the exact double difference of the stored coordinates (asserted)"""
    assert N >= 2 * NDESIGNED
    R = random_state(N, L, seed)
    # 0, 1: on the two faces x = 0 and x = L (their own y, z: no two images coincide)
    R[0, 0], R[0, 1] = 0.0, L
    # three pairs along x only, on the cutoff: exactly L/2 apart, one ulp inside, one ulp outside
    for a, x in ((2, L / 2), (4, np.nextafter(L / 2, 0.0)), (6, np.nextafter(L / 2, L))):
        R[:, a + 1] = R[:, a]
        R[0, a], R[0, a + 1] = 0.0, x
        assert R[0, a + 1] - R[0, a] == x
    # two close pairs along x, 1e-3 and 1e-6 apart, in the upper half of the box: both coordinates on
    # the grid of L's binade (every multiple of its ulp below L is a double), so that the difference is exact
    ulp = 2.0 ** (math.floor(math.log2(L)) - 52)
    for a, sep, frac in ((8, 1e-3, 0.625), (10, 1e-6, 0.875)):
        sep = round(sep / ulp) * ulp
        x = round(frac * L / ulp) * ulp
        R[:, a + 1] = R[:, a]
        R[0, a], R[0, a + 1] = x, x + sep
        assert x + sep < L and R[0, a + 1] - R[0, a] == sep
    # the ends of the allowed range: |dx| = 1.25 L - 2e-9, the limit of mic's threshold form
    R[:, 13] = R[:, 12]
    R[0, 12], R[0, 13] = -L / 8 + 1e-9, 9 * L / 8 - 1e-9
    assert R.min() >= -L / 8 and R.max() <= 9 * L / 8
    return R


SHELL_IONS = (2, 3, 4, 5, 6, 7)


def out_of_range_state(N, L, seed=2024):
    """the random state with a dozen ions outside [-L/8, 9L/8] on one or more axes"""
    R = random_state(N, L, seed)
    moves = [(0, 5, 3.7), (1, 9, -2.2), (2, 17, 2.4), (0, 33, -1.6), (1, 33, 1.9), (0, 64, 3.1),
             (1, 64, -2.7), (2, 64, 1.3), (2, 70, -0.9), (0, 100, 1.4), (1, 101, -0.3), (2, 127, 2.9),
             (0, 128, -2.05), (1, 128, 3.3), (0, 77, 1.2), (2, 12, -1.15)]
    for ax, i, f in moves:
        R[ax, i] = f * L
    return R
