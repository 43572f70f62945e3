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
    rsq3 <= 2 (1.7e-16 measured, mdqt_internal.hpp), so ri carries 3.5 and enters cubed: 10.5;
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
# the states
# ---------------------------------------------------------------------------------------------

def random_state(N, L, seed=2024):
    return np.random.default_rng([seed, N]).uniform(0.0, L, (3, N))


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
