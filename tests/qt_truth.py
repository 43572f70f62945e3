"""Extended-precision truth of the fused substeps n x (step(); qstep()) and the per-ion bound a double
implementation of them is held to (test infrastructure; tests/test_qt_truth.py checks this module on the
CPU, tests/test_gpu_qt_accuracy.py holds the HIP substep kernels to it).

THE TRUTH.  `trajectory` evaluates the reference's dense algebra — M = I - i h H built from the operator
definitions of tests/dense_qt.py (SpeedUp:438-717, :1163-1215), tests/dense_pump.py and
tests/dense_three_state.py, four stages k = (M y / sqrt(1 - dp(y)) - y) / h, psi' = psi + (k1 + 3 k2 +
3 k3 + k4) / 8 h, the jump rule, step()'s two half drifts around the velocity kick — for all ions at once
(batched matrix-vector products) in numpy long double (64-bit significand), with exact sqrt, division, sin
and cos of that format.  The same code runs on mpmath numbers (backend MP, 40 digits) for the check that
long double is enough.  The double parameters enter exactly; a decimal literal of the reference counts as
the double the C literal is (LD(0.395)); the state (R, V, F, psi, tPart), the time t of every substep (the
double accumulation t += dtQ, a control input: it decides step()'s t > 0 branch) and the uniforms are
inputs.  tPart is carried exactly here and, next to it, as the double accumulation the kernels must match
bit for bit.  Nothing of the kernels' row chains, folded tables or reduction trees is used.

THE BOUND B (u = 2^-53; first order in u, every rounding |fl(x) - x| <= u |x|).  Counted along the
longest chain of the kernels (mdqt_qtfast.hpp: row_r, d = fma(pref, ws, -y), the stage combination, the dp
tree, rsq3, kick_term); the exact modes (mdqt_kernels.hip) and the oracle have shorter or equal chains
(cmul sums: 6 A; pref by sqrt and division: 2.5), so the count covers every arithmetic mode at its worst.

  One no-jump substep, one component of psi, Y = the largest |Re|, |Im| of psi and of the stage vectors,
  A = the largest row sum over k of sum_j |Re M_kj| + |Im M_kj| (A - 1 = O(h |H|), a few per cent):
    pref = rsq3(1 - dp)        2 (rsq3, held by tests/test_gpu_device_math.py) + 1 (the subtraction, and
                               dp's own ~10 u dp through the square root)                     3       u Y
    row_r                      seven roundings per component, each of a partial sum <= A Y    7 A     u Y
    Re M_kk = 1 + h Im hd_kk   one rounding of a number ~ 1, made on the host                 1       u Y
    psi' = fma(1/8, acc, psi)  one rounding                                                   1       u Y
    the other coefficients     host-folded: h (4 roundings), gs (3), the coupling (4): <= 12 relative;
                               Im M_kk = fma(mi1, u, mi0) 1 + u's 2; c2 = fma(dms, sin, c2re) 1 + the
                               table sincos' 2^-52 absolute: 2; together 15 u (A - 1) Y
    d = fma(pref, ws, -y)      1 u |d|, |d| <= (A - 1 + 3u) Y                                 1 (A-1) u Y
    acc                        three roundings of <= 8 max|d|, times 1/8                       3 (A-1) u Y
    y_s = fma(c, d, psi)       u Y into each later stage, whose d depends on it with slope
                               <= A - 1                                                        3 (A-1) u Y
  K = 5 + 7 A + 22 (A - 1): about 15 at the default parameters.  A vector of 2 n components each within
  K u Y has 2-norm <= sqrt(2 n) K u Y.

  The phase.  Rows 4, 5, 8, 9 of model 0 carry M_k,slot2 = c2re + dms sin(phi) (dmc cos), phi = (u cphi)
  tPart, u = vx pv2q + expDet(t).  An implementation sees phi only to the roundings of pv2q (pow and a
  product: 2), the product vx pv2q (1), the sum with expDet (1), cphi = 2 (1 + kRat) gamToE (4), the two
  products (2): c0 = 10, plus one per substep since tPart was last exact (an input, or 0 after a jump): the
  double accumulation tPart += dtQ.  So |dphi| <= |phi| (c0 + s) u + cphi pv2q tPart Bv, and the four rows
  move by |dms_k| |dphi| Y each: the phase term, 2-norm sqrt(sum_k 2 dms_k^2) |dphi| Y.  c = c0 + s.

  The velocity error Bv also moves the diagonal: h max|e1| pv2q Bv Y2 (Y2 = the 2-norm of psi).

  Accumulation.  Bpsi' = g Bpsi + local, g = pref_max (1 + x^4) + pref_max^3 h dmax Y2^2, x = h rho (rho
  the largest row sum of |H|): the propagator polynomial 1 + z + z^2/2 + 5 z^3/32 + z^4/32 has modulus
  1 + O(x^6) on z = -i x, the decay part contracts, each stage is divided by sqrt(1 - dp) <= pref_max^-1,
  and the dependence of that prefactor on y is a rank-one term of norm <= pref^3 h dmax Y2^2.  Every
  component of psi is then within Bpsi of the truth.  With renormalisation psi' / |psi'| adds 4 u Y (norm
  tree, rsq3, product) and divides the carried bound by the norm (>= 1 - dp).
  A jump resets Bpsi to 0: both sides hold the same basis state and tPart = 0.

  Velocity (x).  step_V: the product dt f and the sum, u (|dt f| + |v|); the kick's sum u |v|.  The optical
  kick: sum over its terms of |w_ab| |psi_a| |psi_b| =: kabs with 20 roundings along kick_term, the P-lane
  sum and the host-folded weight, plus psi's own error: the kick is the Hermitian form psi^H Kq psi with
  |Kq_ab| = |w_ab| / 2, so it moves by at most 2 |Kq| Y2 Bpsi, |Kq| <= the largest row sum.  (Through the
  phase this feeds back into psi: at |phi| ~ 2^20 the loop gain per substep, cphi pv2q tPart |dms| 2 |Kq|,
  reaches ~0.1 — the specification itself is that ill-conditioned there.)  A jump adds +-vKick, a constant
  made on the host in 4 roundings.  vy, vz: u (|dt f| + |v|) per substep.
  Position (every component), per half drift: the product DT v (at t = 0 also DT2 f and the inner sum), the
  sum and the wrap: 3 u (L + |DT v| + |DT2 f|), plus DT Bv.

At the default parameters this gives Bpsi ~ 8e-15 per substep per unit norm (2e-13 after 25) against the
4e-17 per substep measured for the double oracle: the worst case sits two orders above the typical error and
more than three below the 1e-9 gate of the MD-step tests.  K and c are widened only by correcting this count.
"""
import math

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
C_TAB = 12         # host-folded coefficient: relative roundings (see the count above)
C_PHI0 = 10        # roundings of the coupling phase besides tPart's accumulation


def extended_ok():
    return np.finfo(LD).eps <= 2.0 ** -63


SKIP_MESSAGE = "np.longdouble has no 64-bit significand on this platform: no extended-precision truth"


# ---------------------------------------------------------------------------------------------
# number backends: numpy long double, and mpmath numbers in object arrays (the precision check)
# ---------------------------------------------------------------------------------------------
class LDBackend:
    name = "longdouble"

    @staticmethod
    def num(x):
        return np.asarray(x, dtype=np.float64).astype(LD)        # exact

    sqrt, cos, sin = staticmethod(np.sqrt), staticmethod(np.cos), staticmethod(np.sin)

    @staticmethod
    def power(a, b):
        return np.power(a, b)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, LD)

    @staticmethod
    def lt(a, b):
        return np.less(a, b)

    @staticmethod
    def f64(a):
        return np.asarray(a, dtype=LD).astype(np.float64)


class MPBackend:
    name = "mpmath"

    def __init__(self, dps=40):
        import mpmath
        self.mp = mpmath
        mpmath.mp.dps = dps
        self._num = np.frompyfunc(lambda v: mpmath.mpf(float(v)), 1, 1)
        self._sqrt = np.frompyfunc(mpmath.sqrt, 1, 1)
        self._cos = np.frompyfunc(mpmath.cos, 1, 1)
        self._sin = np.frompyfunc(mpmath.sin, 1, 1)
        self._pow = np.frompyfunc(mpmath.power, 2, 1)
        self._f = np.frompyfunc(float, 1, 1)

    def num(self, x):
        return self._num(np.asarray(x, dtype=np.float64))

    def sqrt(self, a):
        return self._sqrt(a)

    def cos(self, a):
        return self._cos(a)

    def sin(self, a):
        return self._sin(a)

    def power(self, a, b):
        return self._pow(a, b)

    def zeros(self, shape):
        return np.full(shape, self.mp.mpf(0), dtype=object)

    @staticmethod
    def lt(a, b):
        return np.asarray(np.less(a, b)).astype(bool)

    def f64(self, a):
        return np.asarray(self._f(a), dtype=np.float64)


LDB = LDBackend()


# ---------------------------------------------------------------------------------------------
# operator sets
# ---------------------------------------------------------------------------------------------
class Program:
    """One operator set in the numbers of backend B: n states; h = dtQ gamToE; H = Hs + diag(e0 + e1 u)
    (+ the phase entries), Hs complex static (the decay term -i D / 2 included); D the decay diagonal
    (dp = h sum D_k |y_k|^2); kick terms (a, b, w): kick = sum w Im(psi_a conj psi_b); jump rule by model."""


# channel j = |a><b| of model 0 (tests/dense_qt.py cs[], SpeedUp:1163-1180)
_A0 = (1, 1, 0, 0, 1, 0, 6, 7, 8, 7, 8, 9, 8, 9, 10, 9, 10, 11)
_B0 = (2, 3, 3, 4, 4, 5, 5, 5, 5, 4, 4, 4, 3, 3, 3, 2, 2, 2)


def _ratio0(density):
    return int(math.ceil(34.81 / math.sqrt(density)))                   # :83 (an integer: double arithmetic)


def program_model0(B, Om, OmDP, detuning, detuningDP, density, fracOfSig=0.0, Te=19.0, sig0=4.0, gamToE_rel=0.0):
    """SpeedUp's 12-level Sr+ scheme.  gamToE_rel: a relative perturbation of gamToE (the teeth test)."""
    n = B.num
    P = Program()
    P.model, P.n, P.has_step = 0, 12, True
    dens = n(density)
    P.gamToE = n(174.07) / B.sqrt(dens) * (1 + n(gamToE_rel))           # :79
    P.ratio = _ratio0(density)
    P.dtQ = n(0.002) / P.ratio                                          # :84
    P.dtQ_double = 0.002 / P.ratio
    P.pv2q = n(1.1821) * B.power(dens, n(1. / 6))                       # :85
    r, kRat = n(0.0617), n(0.395)                                       # :146-147
    P.vKick = n(0.001208) / P.pv2q                                      # :148
    P.vKickDP = P.vKick * kRat
    P.h = P.dtQ * P.gamToE
    g = [n(1.), n(2.) / 3, n(1.) / 3, n(2.) / 3, n(1.) / 3, n(1.), r * 2 / 3, r * 4 / 15, r * 1 / 15, r * 2 / 5,
         r * 2 / 5, r * 1 / 5, r * 1 / 5, r * 2 / 5, r * 2 / 5, r * 1 / 15, r * 4 / 15, r * 2 / 3]   # gs^2, :1181-1198
    gs = [B.sqrt(x) for x in g]
    D = B.zeros(12)
    for j in range(18):
        D[_B0[j]] = D[_B0[j]] + g[j]                                    # :1201-1204
    P.D = D
    Hr, Hi = B.zeros((12, 12)), B.zeros((12, 12))
    Omn, OmDPn = n(Om), n(OmDP)
    sr = B.sqrt(r)
    for k in (0, 2, 4, 5):                                              # :1206-1210
        v = -gs[k] * Omn / 2
        Hr[_B0[k], _A0[k]] += v
        Hr[_A0[k], _B0[k]] += v
    for k in (6, 9, 12, 14, 15, 17):                                    # :1211-1215
        v = -gs[k] * OmDPn / 2 / sr
        Hr[_B0[k], _A0[k]] += v
        Hr[_A0[k], _B0[k]] += v
    for k in range(12):
        Hi[k, k] = -D[k] / 2                                            # hamDecayTerm
    P.Hr, P.Hi = Hr, Hi
    det, detDP = n(detuning), n(detuningDP)
    e0, e1 = B.zeros(12), B.zeros(12)
    for k in range(2, 6):
        e0[k] = -det
    for k in range(6, 12):
        e0[k] = -det + detDP
    e1[2] = e1[3] = n(-1.)
    e1[4] = e1[5] = n(1.)
    e1[6] = e1[7] = 1 - kRat
    e1[10] = e1[11] = kRat - 1
    e1[8] = e1[9] = -1 - kRat                                           # :506-510
    P.e0, P.e1 = e0, e1
    # hamCouplingTerm's time-dependent part (:508): -(OmDP/2) gs/sqrt(r) e^(i phi) |row><col|, + h.c.
    P.phase = [(8, 5, OmDPn / 2 * gs[8] / sr), (9, 4, OmDPn / 2 * gs[11] / sr)]
    P.cphi = 2 * (1 + kRat) * P.gamToE
    kS, kD = P.vKick * Omn * P.h, P.vKickDP * (OmDPn / r) * P.h         # :503
    P.kick = [(1, 2, kS * gs[0]), (0, 3, kS * gs[2]), (1, 4, -kS * gs[4]), (0, 5, -kS * gs[5]),
              (8, 5, kD * gs[8]), (9, 4, kD * gs[11]), (10, 3, kD * gs[14]), (11, 2, kD * gs[17]),
              (6, 5, -kD * gs[6]), (7, 4, -kD * gs[9]), (8, 3, -kD * gs[12]), (9, 2, -kD * gs[15])]
    P.pD = r / (r + 1)                                                  # :589
    P.thS = {1: g[2], 2: g[4]}                                          # :637-658
    P.thD = [(g[17] / r, g[17] / r + g[16] / r), (g[14] / r, g[14] / r + g[13] / r),
             (g[11] / r, g[11] / r + g[10] / r), (g[8] / r, g[8] / r + g[7] / r)]   # :612-697
    fr, Ten, sg = n(fracOfSig), n(Te), n(sig0)

    def expdet(t):                                                      # :447
        tt = n(t)
        return n(0.0126) * fr * Ten * tt / (B.sqrt(dens) * sg * B.sqrt(1 + n(0.00014314) * tt * tt * Ten / (dens * sg * sg)))
    P.expdet = expdet
    return P


def program_pump(B, model, Om, detuning, density=2.0):
    """the optical-pumping programs' qstep (tests/dense_pump.py): 1 = 408 linear, 2 = 408 quad, 3 = 422"""
    n = B.num
    P = Program()
    P.model, P.n, P.has_step = model, (5 if model == 3 else 7), True
    dens = n(density)
    if model == 3:
        P.gamToE = n(174.07) * n(.894) / B.sqrt(dens)
        P.ratio = int(math.floor(34.81 * .894 / math.sqrt(density) + 0.5))
        P.pv2q = n(1.1821) * B.power(dens, n(1. / 6)) * n(.967)
        r = n(0.0754)
    else:
        P.gamToE = n(174.07) / B.sqrt(dens)
        P.ratio = int(math.floor(34.81 / math.sqrt(density) + 0.5))
        P.pv2q = n(1.1821) * B.power(dens, n(1. / 6))
        r = n(0.0617)
    P.dtQ = n(0.002) / P.ratio
    P.dtQ_double = 0.002 / P.ratio
    P.h = P.dtQ * P.gamToE
    P.vKick = P.vKickDP = n(0.)
    t3, o3 = n(2.) / 3, n(1.) / 3
    if model == 3:
        chan = [(1, 2, t3), (1, 3, o3), (0, 3, t3), (0, 2, o3), (4, 2, r), (4, 3, r)]
        coup = [(1, 2, t3), (0, 3, t3)]
        right, left = (2,), (3,)
    else:
        chan = [(0, 2, n(1.)), (0, 3, t3), (0, 4, o3), (1, 3, o3), (1, 4, t3), (1, 5, n(1.)),
                (6, 2, r), (6, 3, r), (6, 4, r), (6, 5, r)]
        coup = [(1, 3, o3), (1, 5, n(1.)), (0, 2, n(1.)), (0, 4, o3)] if model == 1 else [(1, 5, n(1.)), (0, 4, o3)]
        right, left = (2, 3), (4, 5)
    N = P.n
    D = B.zeros(N)
    for a, b, gj in chan:
        D[b] = D[b] + gj
    P.D = D
    Hr, Hi = B.zeros((N, N)), B.zeros((N, N))
    for a, b, gj in coup:
        v = -n(Om) / 2 * B.sqrt(gj)
        Hr[a, b] += v
        Hr[b, a] += v
    for k in range(N):
        Hi[k, k] = -D[k] / 2
    P.Hr, P.Hi = Hr, Hi
    e0, e1 = B.zeros(N), B.zeros(N)
    for k in right:
        e0[k], e1[k] = -n(detuning), n(-1.)
    for k in left:
        e0[k], e1[k] = -n(detuning), n(1.)
    P.e0, P.e1 = e0, e1
    P.phase, P.cphi, P.kick = [], n(0.), []
    P.pD = r / (r + 1)
    P.t3, P.o3 = t3, o3
    P.expdet = lambda t: n(0.)
    return P


def program_three_level(B, detuning=-0.5, Om=0.5, dt=0.01, vKick=0.0012076):
    """laserCoolNoPlasmaThreeState.cpp's qstep (tests/dense_three_state.py): no positions, velQuant = vx"""
    n = B.num
    P = Program()
    P.model, P.n, P.has_step = "lc3", 3, False
    P.dtQ, P.dtQ_double, P.h = n(dt), float(dt), n(dt)
    P.gamToE, P.pv2q, P.ratio = n(1.), n(1.), 1
    P.vKick = P.vKickDP = n(vKick)
    D = B.zeros(3)
    D[1] = D[2] = n(1.)
    P.D = D
    Hr, Hi = B.zeros((3, 3)), B.zeros((3, 3))
    v = -n(Om) / 2
    for a, b in ((0, 2), (0, 1)):
        Hr[a, b] += v
        Hr[b, a] += v
    Hi[1, 1] = Hi[2, 2] = -n(1.) / 2
    P.Hr, P.Hi = Hr, Hi
    e0, e1 = B.zeros(3), B.zeros(3)
    e0[1] = e0[2] = -n(detuning)
    e1[2], e1[1] = n(-1.), n(1.)
    P.e0, P.e1 = e0, e1
    P.phase, P.cphi = [], n(0.)
    k = n(vKick) * n(Om) * n(dt)
    P.kick = [(0, 2, k), (0, 1, -k)]                                    # LC3:189, gs = 1
    P.pD = n(0.)
    P.expdet = lambda t: n(0.)
    return P


# ---------------------------------------------------------------------------------------------
# jump rules: target state, kick, and the distance of every uniform from the thresholds it meets
# ---------------------------------------------------------------------------------------------
def _jump(P, B, yr, yi, u):
    """u [N][5] (backend numbers).  Returns (target int[N], kick [N], margin float64[N][4]: rand2,
    randDOrS, randDir, rand3; inf where a draw decides nothing)."""
    N = yr.shape[0]
    inf = np.full(N, np.inf)
    if P.model == "lc3":
        up = B.lt(u[:, 1], B.num(0.5))
        return np.zeros(N, int), np.where(up, P.vKick, -P.vKick), np.stack([inf, inf, B.f64(abs(u[:, 1] - B.num(0.5))), inf], 1)
    nP = 2 if P.model == 3 else 4
    pop = [yr[:, 2 + q] * yr[:, 2 + q] + yi[:, 2 + q] * yi[:, 2 + q] for q in range(nP)]
    tot = pop[0]
    for q in range(1, nP):
        tot = tot + pop[q]
    tot = np.where(B.lt(B.num(0.) * tot, tot), tot, tot * 0 + 1)        # (no P population: never jumps)
    cum, acc = [], None
    for q in range(nP - 1):
        acc = pop[q] / tot if acc is None else acc + pop[q] / tot
        cum.append(acc)
    rand2, rds, rdir = u[:, 1], u[:, 2], u[:, 3]
    branch = np.zeros(N, int)
    m2 = inf.copy()
    for c in cum:
        branch += ~B.lt(rand2, c)
        m2 = np.minimum(m2, B.f64(abs(rand2 - c)))
    sdec = ~B.lt(rds, P.pD)
    mds = B.f64(abs(rds - P.pD))
    tgt = np.zeros(N, int)
    m3 = inf.copy()
    if P.model == 0:
        rand3 = u[:, 4]
        up = B.lt(rdir, B.num(0.5))
        mag = np.where(sdec, P.vKick, P.vKickDP)
        kick = np.where(up, mag, -mag)
        mdir = B.f64(abs(rdir - B.num(0.5)))
        for i in range(N):
            b = int(branch[i])
            if sdec[i]:
                if b in P.thS:
                    lt = bool(B.lt(rand3[i], P.thS[b]))
                    tgt[i] = (0 if lt else 1) if b == 1 else (1 if lt else 0)
                    m3[i] = float(B.f64(abs(rand3[i] - P.thS[b])))
                else:
                    tgt[i] = 1 if b == 0 else 0
            else:
                t0, t1 = P.thD[b]
                tgt[i] = (11 - b) - int(not B.lt(rand3[i], t0)) - int(not B.lt(rand3[i], t1))
                m3[i] = min(float(B.f64(abs(rand3[i] - t0))), float(B.f64(abs(rand3[i] - t1))))
        return tgt, kick, np.stack([m2, mds, mdir, m3], 1)
    kick = B.zeros(N)
    if P.model == 3:                                                    # draw 3 decides the S target
        d3 = u[:, 3]
        lt = B.lt(d3, P.t3)
        tgt = np.where(sdec, np.where(branch == 0, np.where(lt, 1, 0), np.where(lt, 0, 1)), 4)
        m3 = np.where(sdec, B.f64(abs(d3 - P.t3)), np.inf)
        return tgt, kick, np.stack([m2, mds, inf, m3], 1)
    d4 = u[:, 4]                                                        # 408: draw 3 is drawn, unused
    th = np.where(branch == 1, P.t3, P.o3)
    lt = B.lt(d4, th)
    mid = (branch == 1) | (branch == 2)
    tgt = np.where(sdec, np.where(branch == 0, 0, np.where(branch == 3, 1, np.where(lt, 0, 1))), 6)
    m3 = np.where(sdec & mid, B.f64(abs(d4 - th)), np.inf)
    return tgt, kick, np.stack([m2, mds, inf, m3], 1)


# ---------------------------------------------------------------------------------------------
# the trajectory
# ---------------------------------------------------------------------------------------------
def _matvec(Mr, Mi, yr, yi):
    a = np.matmul(Mr, yr[..., None])[..., 0] - np.matmul(Mi, yi[..., None])[..., 0]
    b = np.matmul(Mr, yi[..., None])[..., 0] + np.matmul(Mi, yr[..., None])[..., 0]
    return a, b


def trajectory(P, psi, vx, tPart, t0, uniforms, nsub, R=None, V=None, F=None, L=None, renorm=False, do_step=True,
               B=LDB, bound=True):
    """nsub x (step(); qstep()) of N ions.  psi [N][>= n][2] doubles (the first n states are used), vx [N]
    (V[0] when V is given), tPart [N], t0 the time before the first substep, uniforms [nsub][N][5] (draw
    d of substep s), R, V, F [3][N] and L for step().  Returns a dict of per-substep lists (index s = the
    state after substep s): psi_re, psi_im [N][n], V [3][N] (or vx [N]), R [3][N], tPart (exact) and
    tPart_double, jumped bool[N], target int[N] (-1: none), margin_dp [N] = |u1 - dp|, margin_draws [N][4],
    margin_pos [N] (the smallest distance of any half drift's position from 0 and L in this substep), and —
    B = LDB, bound=True — the bounds Bpsi [N], Bvx [N], Bv [N] (vy, vz), BR [N], with K [N] and c [N]."""
    n = P.n
    psi = np.asarray(psi, dtype=np.float64)
    N = psi.shape[0]
    yr, yi = B.num(psi[:, :n, 0]), B.num(psi[:, :n, 1])
    step = bool(do_step and P.has_step)
    if step:
        r, v, f, Ln = B.num(R), B.num(V), B.num(F), B.num(L)
        Lf = float(L)
    else:
        v = B.zeros((3, N))
        v[0] = B.num(vx)
        Lf = 0.0
    tp = B.num(tPart)
    tpd = np.array(tPart, dtype=np.float64)
    t = float(t0)
    dt, DT = P.dtQ, P.dtQ / 2
    DT2 = DT * DT
    eye = B.zeros((n, n))
    for k in range(n):
        eye[k, k] = B.num(1.)
    out = {k: [] for k in ("psi_re", "psi_im", "V", "R", "tPart", "tPart_double", "jumped", "target", "margin_dp",
                           "margin_draws", "margin_pos", "t", "Bpsi", "Bvx", "Bv", "BR", "K", "c", "dp")}
    bound = bound and B is LDB
    if bound:
        Bpsi, Bvx, Bv, BR = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
        since = np.zeros(N)                    # substeps since tPart was last exact
        hf, dtf = float(P.h), float(P.dtQ)
        Dmax = float(B.f64(P.D).max())
        e1max = float(np.abs(B.f64(P.e1)).max())
        pvf, cphif = float(P.pv2q), float(P.cphi)
        krow = np.zeros(n)                     # the kick is psi^H Kq psi, Kq Hermitian with |Kq_ab| = |w_ab| / 2
        for a_, b_, w in P.kick:
            krow[a_] += abs(float(w)) / 2
            krow[b_] += abs(float(w)) / 2
        knorm = float(krow.max()) if P.kick else 0.0
        vkf = max(abs(float(P.vKick)), abs(float(P.vKickDP)))
    for s in range(nsub):
        mpos = np.full(N, np.inf)
        if step:
            moving = t > 0                                                # step_R's branch (:360)
            vabs0 = np.abs(B.f64(v))
            for half in range(2):
                r = r + DT * v if moving else r + (DT * v + DT2 * f)      # :356-389
                rf = B.f64(r)
                mpos = np.minimum(mpos, np.minimum(np.abs(rf), np.abs(rf - Lf)).min(axis=0))
                r = np.where(B.lt(r, B.num(0.) * r), r + Ln, r)
                r = np.where(B.lt(Ln + 0 * r, r), r - Ln, r)
                if half == 0:
                    v = v + dt * f                                        # step_V (:398-409)
            if bound:
                ff = np.abs(B.f64(f))
                vmax = np.maximum(vabs0, np.abs(B.f64(v)))
                per_half = 3 * U53 * (Lf + float(DT) * vmax + (0 if moving else float(DT2) * ff)).max(axis=0)
                BR = BR + 2 * per_half + float(DT) * (2 * np.maximum(Bvx, Bv) + U53 * (dtf * ff + vmax).max(axis=0))
                Bvx = Bvx + U53 * (dtf * ff[0] + vmax[0])
                Bv = Bv + U53 * (dtf * ff[1:] + vmax[1:]).max(axis=0)
        # ---- qstep ----
        tp = tp + P.dtQ
        tpd = tpd + P.dtQ_double
        ueff = v[0] * P.pv2q + P.expdet(t)
        pop = yr * yr + yi * yi
        dp = P.h * np.matmul(pop, P.D)
        u = B.num(uniforms[s])
        nojump = B.lt(dp, u[:, 0])                                        # rand > dp (:487)
        Hr = np.broadcast_to(P.Hr, (N, n, n)).copy()
        Hi = np.broadcast_to(P.Hi, (N, n, n)).copy()
        ediag = P.e0[None, :] + P.e1[None, :] * ueff[:, None]
        for k in range(n):
            Hr[:, k, k] = Hr[:, k, k] + ediag[:, k]
        phi = None
        if P.phase:
            phi = P.cphi * ueff * tp                                      # 2 (vq + e)(1 + kRat) tPart gamToE
            cph, sph = B.cos(phi), B.sin(phi)
            for row, col, amp in P.phase:
                Hr[:, row, col] = Hr[:, row, col] - amp * cph
                Hi[:, row, col] = Hi[:, row, col] - amp * sph
                Hr[:, col, row] = Hr[:, col, row] - amp * cph
                Hi[:, col, row] = Hi[:, col, row] + amp * sph
        Mr = eye[None] + P.h * Hi                                         # M = I - i h H
        Mi = -P.h * Hr

        stage_y = []

        def stage(ar, ai):
            stage_y.append((ar, ai))
            dpy = P.h * np.matmul(ar * ar + ai * ai, P.D)
            pref = 1 / B.sqrt(1 - dpy)
            sr_, si_ = _matvec(Mr, Mi, ar, ai)
            return (pref[:, None] * sr_ - ar) / P.h, (pref[:, None] * si_ - ai) / P.h, pref

        hh, hhalf = P.h, P.h / 2
        k1r, k1i, p1 = stage(yr, yi)
        k2r, k2i, p2 = stage(yr + hhalf * k1r, yi + hhalf * k1i)
        k3r, k3i, p3 = stage(yr + hhalf * k2r, yi + hhalf * k2i)
        k4r, k4i, p4 = stage(yr + hh * k3r, yi + hh * k3i)
        er = yr + (k1r + 3 * k2r + 3 * k3r + k4r) / 8 * hh
        ei = yi + (k1i + 3 * k2i + 3 * k3i + k4i) / 8 * hh
        kick_nj = B.zeros(N)
        kabs = np.zeros(N)
        for a, b, w in P.kick:
            kick_nj = kick_nj + w * (yi[:, a] * yr[:, b] - yr[:, a] * yi[:, b])
            if bound:
                kabs += abs(float(w)) * B.f64(np.sqrt(pop[:, a].astype(LD)) * np.sqrt(pop[:, b].astype(LD)))
        tgt, kick_j, mdraw = _jump(P, B, yr, yi, u)
        jumped = ~nojump
        if bound:
            Y = np.max([np.maximum(np.abs(B.f64(a)), np.abs(B.f64(b))).max(axis=1) for a, b in stage_y] +
                       [np.maximum(np.abs(B.f64(er)), np.abs(B.f64(ei))).max(axis=1)], axis=0)
            Y2 = np.sqrt(B.f64(pop.sum(axis=1)))
            Mabs = np.abs(B.f64(Mr)) + np.abs(B.f64(Mi))
            A = Mabs.sum(axis=2).max(axis=1)
            Habs = np.abs(B.f64(Hr)) + np.abs(B.f64(Hi))
            x = hf * Habs.sum(axis=2).max(axis=1)
            K = 5 + 7 * A + (C_TAB + 10) * (A - 1)
            local = math.sqrt(2 * n) * K * U53 * Y
            since = since + 1
            cc = C_PHI0 + since
            if P.phase:
                dphi = np.abs(B.f64(phi)) * cc * U53 + cphif * pvf * np.abs(B.f64(tp)) * Bvx
                dms2 = sum(2 * (hf * float(amp)) ** 2 for _, _, amp in P.phase) * 2     # both rows of each entry
                local = local + math.sqrt(dms2) * dphi * Y
            local = local + hf * e1max * pvf * Bvx * Y2
            pmax = np.max([B.f64(p) for p in (p1, p2, p3, p4)], axis=0)
            g = pmax * (1 + x ** 4) + pmax ** 3 * hf * Dmax * Y2 * Y2
            Bpsi = g * Bpsi + local
            Bvx = np.where(jumped, Bvx + U53 * (4 * vkf + np.abs(B.f64(v[0])) + vkf),
                           Bvx + U53 * (np.abs(B.f64(v[0])) + 20 * kabs) + 2 * knorm * Y2 * Bpsi)
        # ---- select ----
        basis_r = B.zeros((N, n))
        for i in np.nonzero(jumped)[0]:
            basis_r[i, tgt[i]] = B.num(1.)
        yr = np.where(nojump[:, None], er, basis_r)
        yi = np.where(nojump[:, None], ei, basis_r * 0)
        tp = np.where(nojump, tp, tp * 0)
        tpd = np.where(nojump, tpd, 0.0)
        v = v.copy()
        v[0] = v[0] + np.where(nojump, kick_nj, kick_j)                   # :705
        if renorm:                                                        # :706-712
            nrm = B.sqrt((yr * yr + yi * yi).sum(axis=1))
            yr, yi = yr / nrm[:, None], yi / nrm[:, None]
        if bound:
            if renorm:
                Bpsi = Bpsi / B.f64(nrm) + 4 * U53 * Y
            Bpsi = np.where(jumped, 0.0, Bpsi)
            since = np.where(jumped, 0.0, since)
            for key, val in (("Bpsi", Bpsi), ("Bvx", Bvx), ("Bv", Bv), ("BR", BR), ("K", K), ("c", cc)):
                out[key].append(np.array(val, dtype=np.float64).copy())
        t = t + P.dtQ_double                                              # :716
        out["psi_re"].append(yr.copy()); out["psi_im"].append(yi.copy())
        out["V"].append(v.copy())
        out["R"].append(r.copy() if step else None)
        out["tPart"].append(tp.copy()); out["tPart_double"].append(tpd.copy())
        out["jumped"].append(np.asarray(jumped, bool).copy())
        out["target"].append(np.where(jumped, tgt, -1))
        out["margin_dp"].append(B.f64(abs(u[:, 0] - dp)))
        out["margin_draws"].append(np.where(jumped[:, None], mdraw, np.inf))
        out["margin_pos"].append(mpos)
        out["dp"].append(B.f64(dp))
        out["t"].append(t)
    return out


def philox_tape(orc, seed, job, N, q0, nsub, ion0=0):
    """uniforms [nsub][N][5] of the engine's Philox stream (rng_mode 1): draw d of ion i at qstep q0 + s"""
    return np.array([[[orc.philox_uniform(seed, job, ion0 + i, q0 + s, d) for d in range(5)] for i in range(N)]
                     for s in range(nsub)])


def psi_error(tr, s, psi):
    """max over the 2 n components of |psi - truth| per ion (psi [N][>= n][2] doubles), after substep s"""
    n = tr["psi_re"][s].shape[1]
    p = np.asarray(psi, dtype=np.float64)
    er = np.abs(p[:, :n, 0].astype(LD) - tr["psi_re"][s])
    ei = np.abs(p[:, :n, 1].astype(LD) - tr["psi_im"][s])
    return np.maximum(er, ei).max(axis=1).astype(np.float64)


def min_margins(tr):
    """(decision margin, position margin) over all substeps and ions"""
    d = min(min(float(np.min(a)), float(np.min(b))) for a, b in zip(tr["margin_dp"], tr["margin_draws"]))
    p = min(float(np.min(a)) for a in tr["margin_pos"])
    return d, p
