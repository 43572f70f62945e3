"""The truth and the bound of output()'s numbers: <vx>, the energy sums, the velocity distributions,
the per-ion populations (SpeedUp:917-1032) and the tagged distribution and moments (QTT:1069-1138).

Written from the reference's statements in numpy long double (x87: 64-bit significand), not from the
kernels.  The inputs are the exact doubles given to the engine; the constants are formed in double as the
reference forms them (vel[j] = fl(j 0.0025), V2 = fl(1 / (2 0.002 0.002)), the normalisation
6.0 sqrt(2 pi 0.002^2)).  Every value comes with a bound B on |device - truth| that holds for any
IEEE double evaluation of the reference's operations in any summation order, and with the truth's own
error T (which B includes).  docs/OBSERVABLES.md, "The observables' per-element gate", derives each
contribution; in short, with u = 2^-53:

  a sum of n terms, any order     (n + c) u sum |t_k|, c = the roundings of one term and of what follows
                                  the sum (stated per quantity below)
  a KDE term t = exp(-x),         t expm1((E_EXP + 4 x) u) + E_EXP 2^-1074: the library exp's E_EXP ulps, the
  x = V2 (b - w)^2                argument's roundings times x <= 747 (three operations, four roundings' worth:
                                  the difference b - w enters squared, so its rounding counts twice), the
                                  subnormal floor
  the x axis, w = fl(vx - avg)    |dw| <= u (|w| + B_avg) + B_avg through t expm1(2 V2 |b - w| |dw| + V2 dw^2)
  a term left out of the truth    2^-1074 (only terms with x > 746, whose value is below 2^-1075)
  the truth itself                2^-64 relative per operation, times x in the exponent

No factor is fitted: tests/test_obs_truth.py holds the project's double restatements inside B and nine
one-defect models of the kernels outside it."""
import math

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53              # the unit roundoff of double
TINY = LD(2.0) ** -1074         # the smallest subnormal: the absolute floor of a term and of a division
ULD = LD(2.0) ** -64            # the unit roundoff of the truth's format
E_EXP = 1.0                     # the library exp's error in ulps (documented; measured: docs/OBSERVABLES.md)

NBINS, TBINS, TBIN0 = 2001, 4001, -2000
DV = 0.0025
V2 = 1. / (2. * 0.002 * 0.002)                         # SpeedUp:958, QTT:1072
NORM = 6.0 * math.sqrt(2 * math.pi * 0.002 * 0.002)    # SpeedUp:976, QTT:1121
HALF = 32                       # bins visited either side of the nearest: |b - w| <= 0.07875, so every term
                                # left out has x >= 125000 0.07875^2 = 775 > 746


def has_extended():
    return np.finfo(LD).eps <= 2.0 ** -63


def sum_bound(n, c, abs_sum):
    """a sum of n terms in any order, each term carrying c roundings of its own (or c roundings after the
    sum): (n + c) u sum|t|.  The worst case of any summation tree is (n - 1) u to first order; the 1 that
    (n + c) has on top of (n - 1 + c) covers the second order while n^2 u < 1 (n < 9e7)."""
    return (LD(n) + LD(c)) * U * abs_sum


class Kde:
    """raw[nb] the sum of the terms, err[nb] the terms' own error bound (exp, argument, dw, floors, terms
    left out), own[nb] the truth's error, nvis[nb] the terms the truth visited"""
    __slots__ = ("raw", "err", "own", "nvis")


def kde_terms(W, dW, nb, bin0, mirror, nterms):
    """the distribution's bins from the ions' abscissae W (long double; non-finite ones removed by the
    caller), dW[i] >= the device's error on W[i]; nterms = the terms the device sums per bin (for the
    floor of those the truth leaves out)"""
    W = np.asarray(W, dtype=LD)
    dW = np.broadcast_to(np.asarray(dW, dtype=LD), W.shape)
    k = Kde()
    k.raw = np.zeros(nb, dtype=LD); k.err = np.zeros(nb, dtype=LD); k.own = np.zeros(nb, dtype=LD)
    k.nvis = np.zeros(nb, dtype=np.int64)
    off = np.arange(-HALF, HALF + 1)
    for sign in ((1.0, -1.0) if mirror else (1.0,)):            # b - w, then the mirror term b + w
        Ws = W if sign > 0 else -W
        inr = np.abs(Ws.astype(np.float64) - (bin0 + (nb - 1) / 2) * DV) <= (nb / 2 + HALF + 2) * DV
        Wi, dWi = Ws[inr], dW[inr]
        for s0 in range(0, Wi.size, 4096):
            w, dw = Wi[s0:s0 + 4096, None], dWi[s0:s0 + 4096, None]
            J = np.rint(w.astype(np.float64) / DV).astype(np.int64) - bin0 + off[None, :]
            ok = (J >= 0) & (J < nb)
            b = ((J + bin0).astype(np.float64) * DV).astype(LD)   # vel[j], the double product
            d = b - w
            x = LD(V2) * d * d
            t = np.exp(-x)
            e = t * np.expm1((LD(E_EXP) + 4 * x) * U) + LD(E_EXP) * TINY
            e = e + t * np.expm1(2 * LD(V2) * np.abs(d) * dw + LD(V2) * dw * dw)
            o = t * (5 * x + 3) * ULD                            # the argument (d counts twice), expl, the addition
            jj = J[ok]
            np.add.at(k.raw, jj, t[ok]); np.add.at(k.err, jj, e[ok]); np.add.at(k.own, jj, o[ok])
            np.add.at(k.nvis, jj, 1)
    k.err = k.err + (LD(nterms) - k.nvis.astype(LD)).clip(min=0) * TINY
    return k


def normalise(k, n):
    """bins / NORM: (value, B, T).  The sum's n terms in any order and the division's rounding (c = 1: relative u
    in the normal range, at most 2^-1074 absolute below it)."""
    P = k.raw / LD(NORM)
    own = (k.own + k.raw * ULD) / LD(NORM)
    B = (sum_bound(n, 1, k.raw) + k.err) / LD(NORM) + TINY + own
    return P, B, own


def raw_bins(k, n):
    """the unnormalised bins of the sharded path: (value, B, T), c = 0"""
    return k.raw, sum_bound(n, 0, k.raw) + k.err + k.own, k.own


def vx_average(vx, N=None):
    """<vx> = (sum vx) / N: the terms are inputs (no rounding of their own), the division rounds once: c = 1.
    Returns (value, B, T)."""
    v = np.asarray(vx, dtype=LD)
    n = v.size if N is None else N
    a = v.sum() / LD(n)
    own = (LD(v.size) + 1) * ULD * np.abs(v).sum() / LD(n)
    return a, sum_bound(v.size, 1, np.abs(v).sum()) / LD(n) + own, own


def energy_sums(V, avg, B_avg, Urow):
    """the four sums over the given ions, sum 0.5 (vx - avg)^2, 0.5 vy^2, 0.5 vz^2 and sum U_i: (value[4], B[4], T[4]).
    x: w = fl(vx - avg) (relative u on w: 2 u on its square), the product (u), 0.5 exact: c = 3, one more for the
    second order of these: c = 4; and |dt| <= |w| B_avg + B_avg^2 / 2 from the device's <vx>.  y, z: the product:
    c = 1.  U: the terms are the engine's own rows: c = 0."""
    V = np.asarray(V, dtype=LD)
    n = V.shape[1]
    w = V[0] - avg
    t = [0.5 * w * w, 0.5 * V[1] * V[1], 0.5 * V[2] * V[2], np.asarray(Urow, dtype=LD)]
    val = np.array([x.sum() for x in t], dtype=LD)
    ab = np.array([np.abs(x).sum() for x in t], dtype=LD)
    own = (LD(n) + 4) * ULD * ab
    B = np.array([sum_bound(n, c, a) for c, a in zip((4, 1, 1, 0), ab)], dtype=LD) + own
    B[0] = B[0] + np.abs(w).sum() * B_avg + LD(n) * B_avg * B_avg / 2
    return val, B, own


def finish(sums, B_sums, avg, B_avg, N, t, Epot0):
    """out7 as finish_observables forms it (SpeedUp:945-954): (value[7], B[7]).  Each energy is a sum divided by N
    (one rounding; the halving of the potential is exact); out7[5] adds the four and subtracts Epot0: four
    roundings, each at most u times the largest partial sum, which the sum of the terms' magnitudes bounds —
    the scale of its terms, not of their difference."""
    n = LD(N)
    E = np.array([sums[0] / n, sums[1] / n, sums[2] / n, sums[3] / 2 / n], dtype=LD)
    BE = np.array([B_sums[0] / n, B_sums[1] / n, B_sums[2] / n, B_sums[3] / 2 / n], dtype=LD) + U * np.abs(E)
    val = np.array([LD(t), E[0], E[1], E[2], E[3], E.sum() - LD(Epot0), avg], dtype=LD)
    B5 = BE.sum() + 4 * U * (np.abs(E).sum() + BE.sum() + abs(LD(Epot0)))
    return val, np.array([LD(0), BE[0], BE[1], BE[2], BE[3], B5, B_avg], dtype=LD)


def populations(psi, model):
    """S / P / D per ion (SpeedUp:1019-1021; pumping model 3: P = 2, 3, D = 4): (value[N][3], B[N][3]).  A
    population of k states is a sum of n = 2 k non-negative terms re^2, im^2, each one product (one rounding, or
    none where the compiler fuses it into the addition): c = 1.  (No floor: the inputs' squares are normal.)"""
    p = np.asarray(psi, dtype=LD).reshape(-1, 12, 2)
    nr = (p * p).sum(axis=2)
    groups = ((0, 2), (2, 4), (4, 5)) if model == 3 else ((0, 2), (2, 6), (6, 12))
    val = np.stack([nr[:, a:b].sum(axis=1) for a, b in groups], axis=1)
    B = np.stack([sum_bound(2 * (b - a), 1, nr[:, a:b].sum(axis=1)) for a, b in groups], axis=1)
    return val, B + 16 * ULD * val


class Truth:
    pass


def observables(V, psi=None, Urow=None, model=0, t=0.0, Epot0=0.0, kde=True):
    """output() of one whole system: avg, sums, out7, P[3][NBINS], pops, each with its B (and T for the bins).
    A NaN velocity makes its axis' bins NaN (the reference's sum); an infinite one adds exact zeros."""
    V = np.asarray(V, dtype=np.float64)
    N = V.shape[1]
    r = Truth()
    r.N = N
    r.avg, r.B_avg, r.T_avg = vx_average(V[0])
    r.sums, r.B_sums, r.T_sums = energy_sums(np.where(np.isfinite(V), V, 0.0), r.avg, r.B_avg,
                                             np.zeros(N) if Urow is None else Urow)
    r.out7, r.B_out7 = finish(r.sums, r.B_sums, r.avg, r.B_avg, N, t, Epot0)
    if kde:
        r.P = np.zeros((3, NBINS), dtype=LD); r.B_P = np.zeros((3, NBINS), dtype=LD); r.T_P = np.zeros((3, NBINS), dtype=LD)
        r.nan_axis = [bool(np.isnan(V[c]).any()) for c in range(3)]
        for c in range(3):
            fin = np.isfinite(V[c])
            v = V[c][fin].astype(LD)
            if c == 0:
                w = v - r.avg
                dw = U * (np.abs(w) + r.B_avg) + r.B_avg + ULD * np.abs(v)   # (the last: the truth's own w)
            else:
                w, dw = v, LD(0)
            k = kde_terms(w, dw, NBINS, 0, True, 2 * N)
            r.P[c], r.B_P[c], r.T_P[c] = normalise(k, 2 * N)
    if psi is not None:
        r.pops, r.B_pops = populations(psi, model)
    return r


def partial(V, avg_in, Urow):
    """mdqt_partial_observables of one rank's ions with the <vx> it is given (a double, taken exactly: no dw):
    sum vx, the four sums, the unnormalised bins, each (value, B)"""
    V = np.asarray(V, dtype=np.float64)
    n = V.shape[1]
    r = Truth()
    r.n = n
    vx = V[0].astype(LD)
    r.sumvx = vx.sum()
    r.B_sumvx = sum_bound(n, 0, np.abs(vx).sum()) + LD(n) * ULD * np.abs(vx).sum()
    r.sums, r.B_sums, _ = energy_sums(V, LD(avg_in), LD(0), Urow)
    r.raw = np.zeros((3, NBINS), dtype=LD); r.B_raw = np.zeros((3, NBINS), dtype=LD)
    for c in range(3):
        w = V[c].astype(LD) - (LD(avg_in) if c == 0 else LD(0))
        dw = U * np.abs(w) if c == 0 else LD(0)
        r.raw[c], r.B_raw[c], _ = raw_bins(kde_terms(w, dw, NBINS, 0, True, 2 * n), 2 * n)
    return r


def tagged(V, tags):
    """recordTaggedParticleMoments: P[3][TBINS] over the tagged ions (bin0 = -2000, no mirror term) and the four
    moments of their vx.  v^k costs k - 1 roundings and the division by the count one: c = k.  With no ion
    tagged the bins are exactly 0 and the moments 0 / 0 (QTT:1106-1109: NaN)."""
    V = np.asarray(V, dtype=np.float64)
    on = np.asarray(tags) != 0
    nt = int(on.sum())
    r = Truth()
    r.nt = nt
    r.P = np.zeros((3, TBINS), dtype=LD); r.B_P = np.zeros((3, TBINS), dtype=LD); r.T_P = np.zeros((3, TBINS), dtype=LD)
    r.mom = np.full(4, np.nan, dtype=LD); r.B_mom = np.zeros(4, dtype=LD)
    if nt == 0:
        return r
    for c in range(3):
        k = kde_terms(V[c][on].astype(LD), LD(0), TBINS, TBIN0, False, nt)
        r.P[c], r.B_P[c], r.T_P[c] = normalise(k, nt)
    v = V[0][on].astype(LD)
    for q in range(4):
        p = v ** (q + 1)
        r.mom[q] = p.sum() / LD(nt)
        r.B_mom[q] = (sum_bound(nt, q + 1, np.abs(p).sum()) + (LD(nt) + q + 2) * ULD * np.abs(p).sum()) / LD(nt)
    return r


def to_ld(a):
    return np.asarray(a, dtype=LD)


def worst(err, B):
    """max over the elements of err / B (0 / 0 = 0: an exact value met exactly); inf where a non-zero error meets B = 0"""
    err, B = np.asarray(err, dtype=LD).ravel(), np.asarray(B, dtype=LD).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / B)
    r = np.where(np.isnan(r), LD(np.inf), r)
    i = int(np.argmax(r))
    return float(r[i]), i
