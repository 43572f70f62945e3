"""The observables' per-element gate, checked without a GPU (tests/obs_truth.py, tests/obs_cases.py;
docs/OBSERVABLES.md):

  1. the long double truth against mpmath at 50 digits: more than 200 (case, bin) pairs, bins of subnormal value
     among them, and <vx>, the four sums, the populations and the tagged moments of every small case — each
     within 1 % of B, which is what the truth's own error may take of it;
  2. the project's double restatements inside B on every element of every case: the oracle's dense
     observables() up to N = 2049, and a sparse numpy restatement of the kernels' algorithm (chunks, the
     per-wave skip, the partials' reduction) on every case, N = 16,385 and 132,000 included.  The worst
     error / B per quantity is printed (-s) and recorded in docs/OBSERVABLES.md;
  3. nine models of the kernels with one defect each, every one outside B by a factor >= 2 on some element.

The oracle's Epot (out7[4], [5]) is left out of 2: it is a pair sum of the oracle's own exponentials, not a sum
of given rows; the rows are held by tests/test_force_truth.py."""
import numpy as np
import pytest

from tests import obs_cases as oc
from tests import obs_truth as ot

LD = ot.LD
pytestmark = pytest.mark.skipif(not ot.has_extended(), reason="np.longdouble has no 64-bit significand here")
SMALL = [n for n in oc.NAMES if n != "big" and int(n.lstrip("Ndrift")) <= 2049]


# ---------------------------------------------------------------------------------------------
# numpy-double models of the kernels' algorithm, with an optional defect
# ---------------------------------------------------------------------------------------------

def sums_model(V, Urow, lost_level=False):
    """k_sum_vx and k_energy_sums: (avg, sums[4]); lost_level: block_sum without its first level, the partials of
    threads >= 512 (ions i with i mod 1024 >= 512) never added"""
    N = V.shape[1]
    keep = (np.arange(N) % 1024) < 512 if lost_level else np.ones(N, bool)
    avg = V[0][keep].sum() / N
    w = V[0][keep] - avg
    return avg, np.array([(0.5 * (w * w)).sum(), (0.5 * (V[1][keep] * V[1][keep])).sum(),
                          (0.5 * (V[2][keep] * V[2][keep])).sum(), Urow[keep].sum()])


def near_wave(v, k, skip, bin0=0):
    """the wave's ballot: some bin of indices 64 k .. 64 k + 63 within skip of v (outside the wave its end bins decide)"""
    lo, hi = (64 * k + bin0).astype(np.float64) * ot.DV, (64 * k + 63 + bin0).astype(np.float64) * ot.DV
    return ((v >= lo) & (v <= hi)) | ~(np.abs(lo - v) >= skip) | ~(np.abs(hi - v) >= skip)


def kde_model(W, nb, bin0, nch, chunk, mirror, skip=0.0773, keep=None):
    """kde_chunk + kde_reduce_bin (tagged_kde_chunk + tagged_kde_reduce_1 with mirror False) in double: chunk
    partials, the partials summed, the normalisation; an ion's terms are evaluated on the bins of a wave whose
    ballot finds it near (either of its two terms, with the mirror)"""
    N = W.size
    idx = np.arange(N)
    keep = np.ones(N, bool) if keep is None else keep
    part = np.zeros((nch, nb))
    off = np.arange(-34, 35)
    for s in ((1.0, -1.0) if mirror else (1.0,)):
        sel = idx[keep & (np.abs(s * W - (bin0 + (nb - 1) / 2) * ot.DV) <= (nb / 2 + 40) * ot.DV)]
        a = s * W[sel][:, None]                              # b + v = b - (-v)
        J = np.rint(a / ot.DV).astype(np.int64) - bin0 + off[None, :]
        ok = (J >= 0) & (J < nb)
        d = (J + bin0).astype(np.float64) * ot.DV - a
        t = np.exp(-ot.V2 * d * d)
        near = near_wave(a, J // 64, skip, bin0)
        if mirror:
            near = near | near_wave(-a, J // 64, skip, bin0)
        use = ok & near
        z = np.broadcast_to((sel // chunk)[:, None], J.shape)
        np.add.at(part, (z[use], J[use]), t[use])
    return part.sum(axis=0) / ot.NORM


def obs_model(V, Urow=None, defect=None):
    """observables_w1 in double: (avg, sums, P[3][NBINS])"""
    N = V.shape[1]
    Urow = np.zeros(N) if Urow is None else Urow
    avg, sums = sums_model(V, Urow, lost_level=defect == "tree_level")
    nch = min(max(N // 32, 1), 512)
    chunk = -(-N // nch)
    idx = np.arange(N)
    keep = np.ones(N, bool)
    if defect == "last_of_chunk":
        keep = idx != np.minimum(N, (idx // chunk + 1) * chunk) - 1
    if defect == "second_pass":
        keep = idx % chunk < 256
    P = np.zeros((3, ot.NBINS))
    for c in range(3):
        sub = (c == 0 and defect != "avg_not_on_x") or (c == 1 and defect == "avg_on_y")
        W = V[c] - avg if sub else V[c]
        P[c] = kde_model(W, ot.NBINS, 0, nch, chunk, defect != "no_mirror", 0.0760 if defect == "skip_0.0760" else 0.0773,
                         keep)
    return avg, sums, P


def pops_model(psi, model):
    p = np.asarray(psi).reshape(-1, 12, 2)
    nr = p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]
    g = ((0, 2), (2, 4), (4, 5)) if model == 3 else ((0, 2), (2, 6), (6, 12))
    return np.stack([nr[:, a:b].sum(axis=1) for a, b in g], axis=1)


def tagged_model(V, tags, defect=None):
    N = V.shape[1]
    on = tags != 0
    nch = -(-N // 256)
    if defect == "last_only_chunk":
        for z in range(nch):
            i1 = min(N, 256 * z + 256)
            if on[i1 - 1] and on[256 * z:i1].sum() == 1:
                on = on.copy(); on[i1 - 1] = False
    P = np.stack([kde_model(V[c], ot.TBINS, ot.TBIN0, nch, 256, False, keep=on) for c in range(3)])
    v, nt = V[0][tags != 0], int((tags != 0).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mom = np.array([v.sum(), (v * v).sum(), (v * v * v).sum(), (v * v * v * v).sum()]) / np.float64(nt)
    return P, mom


def ratios(avg, sums, P, tr):
    """error / B of a double result against a truth: {quantity: (worst, index)}"""
    out = {"avg": ot.worst(abs(LD(avg) - tr.avg), tr.B_avg)}
    for q, name in enumerate(("sum_x", "sum_y", "sum_z", "sum_U")):
        out[name] = ot.worst(abs(LD(sums[q]) - tr.sums[q]), tr.B_sums[q])
    for c, name in enumerate(("Px", "Py", "Pz")):
        out[name] = ot.worst(np.abs(ot.to_ld(P[c]) - tr.P[c]), tr.B_P[c])
    return out


_model_cache = {}


def model_of(name, defect=None):
    if (name, defect) not in _model_cache:
        _model_cache[(name, defect)] = obs_model(oc.case_velocities(name), defect=defect)
    return _model_cache[(name, defect)]


# ---------------------------------------------------------------------------------------------
# 1. the truth against mpmath
# ---------------------------------------------------------------------------------------------

def ld_to_mp(t):
    import mpmath
    m, e = np.frexp(LD(t))
    hi = float(m)
    return (mpmath.mpf(hi) + mpmath.mpf(float(m - LD(hi)))) * mpmath.mpf(2) ** int(e)


def mp_bin(v_mp, v_double, b, mirror):
    """one bin at 50 digits: the ions within 0.1 of it (every other term is below e^-1250)"""
    import mpmath
    s = mpmath.mpf(0)
    V2 = mpmath.mpf(ot.V2)
    for sign in ((1, -1) if mirror else (1,)):
        for i in np.nonzero(np.abs(b - sign * v_double) < 0.1)[0]:
            d = mpmath.mpf(float(b)) - sign * v_mp[i]
            s += mpmath.exp(-V2 * d * d)
    return s / mpmath.mpf(ot.NORM)


def test_truth_bins_against_mpmath():
    import mpmath
    mpmath.mp.dps = 50
    rng = np.random.default_rng(0)
    pairs = subnormal = 0
    for name in SMALL:
        V, tr = oc.case_velocities(name), oc.kinetic_truth(name)
        avg = sum(mpmath.mpf(float(x)) for x in V[0]) / V.shape[1]
        assert abs(ld_to_mp(tr.avg) - avg) <= ld_to_mp(0.01 * tr.B_avg)
        assert tr.T_avg <= 0.01 * tr.B_avg and np.all(tr.T_P <= 0.01 * tr.B_P)
        picks = [(c, int(j)) for c in range(3) for j in rng.integers(0, ot.NBINS, 3)] + oc.quiet_bins(tr)[:6] + \
                [(c, int(np.argmax(tr.P[c]))) for c in range(3)]
        for c, j in picks:
            vmp = [mpmath.mpf(float(x)) - (avg if c == 0 else 0) for x in V[c]]
            m = mp_bin(vmp, V[c] - (float(tr.avg) if c == 0 else 0.0), j * ot.DV, True)
            assert abs(ld_to_mp(tr.P[c, j]) - m) <= ld_to_mp(0.01 * tr.B_P[c, j]), (name, c, j)
            pairs += 1
            subnormal += 0 < tr.P[c, j] < LD(2.0) ** -1022
    for N in oc.TAG_SIZES:
        V, tr = oc.tagged_velocities(N), oc.tagged_truth(N, "alternate")
        on = oc.tag_pattern(N, "alternate") != 0
        for c in range(3):
            vmp = [mpmath.mpf(float(x)) for x in V[c][on]]
            for j in rng.integers(0, ot.TBINS, 3):
                m = mp_bin(vmp, V[c][on], (int(j) + ot.TBIN0) * ot.DV, False)
                assert abs(ld_to_mp(tr.P[c, j]) - m) <= ld_to_mp(0.01 * tr.B_P[c, j]), (N, c, j)
                pairs += 1
        v = [mpmath.mpf(float(x)) for x in V[0][on]]
        for q in range(4):
            m = sum(x ** (q + 1) for x in v) / len(v)
            assert abs(ld_to_mp(tr.mom[q]) - m) <= ld_to_mp(0.01 * tr.B_mom[q])
    print(f"{pairs} (case, bin) pairs against mpmath, {subnormal} of subnormal value")
    assert pairs >= 200 and subnormal >= 10


def test_truth_sums_and_populations_against_mpmath():
    import mpmath
    mpmath.mp.dps = 50
    for name in SMALL:
        V = oc.case_velocities(name)
        N = V.shape[1]
        Urow = np.random.default_rng(N).uniform(0.5, 3.0, N)
        tr = oc.with_potential(name, Urow, t=0.25, Epot0=0.125)
        avg = sum(mpmath.mpf(float(x)) for x in V[0]) / N
        s = [sum((mpmath.mpf(float(x)) - avg) ** 2 for x in V[0]) / 2, sum(mpmath.mpf(float(x)) ** 2 for x in V[1]) / 2,
             sum(mpmath.mpf(float(x)) ** 2 for x in V[2]) / 2, sum(mpmath.mpf(float(x)) for x in Urow)]
        for q in range(4):
            assert abs(ld_to_mp(tr.sums[q]) - s[q]) <= ld_to_mp(0.01 * tr.B_sums[q]), (name, q)
        o7 = [mpmath.mpf(0.25), s[0] / N, s[1] / N, s[2] / N, s[3] / 2 / N, 0, avg]
        o7[5] = o7[1] + o7[2] + o7[3] + o7[4] - mpmath.mpf(0.125)
        for q in range(1, 7):
            assert abs(ld_to_mp(tr.out7[q]) - o7[q]) <= ld_to_mp(0.01 * tr.B_out7[q]), (name, q)
        assert tr.out7[0] == 0.25 and tr.B_out7[0] == 0
    for model in (0, 1, 3):
        for N in (3, 257):
            psi = oc.random_psi(N, model)
            val, B = ot.populations(psi, model)
            g = ((0, 2), (2, 4), (4, 5)) if model == 3 else ((0, 2), (2, 6), (6, 12))
            for i in range(0, N, 16):
                for q, (a, b) in enumerate(g):
                    m = sum(mpmath.mpf(float(x)) ** 2 for x in psi[i, a:b].ravel())
                    assert abs(ld_to_mp(val[i, q]) - m) <= ld_to_mp(0.01 * B[i, q]), (model, N, i, q)


# ---------------------------------------------------------------------------------------------
# 2. the double restatements inside B
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", oc.NAMES)
def test_kernel_model_inside_B(name):
    """the defect-free model of the kernels' algorithm (the sparse numpy-double restatement): every element"""
    avg, sums, P = model_of(name)
    r = ratios(avg, sums, P, oc.kinetic_truth(name))
    print(name, "model error / B:", {k: round(v[0], 4) for k, v in r.items()})
    assert max(v[0] for v in r.values()) <= 1, (name, r)


@pytest.mark.parametrize("name", SMALL)
def test_oracle_inside_B(orc, name):
    """the oracle's dense observables() in double: <vx>, the kinetic energies, every bin, every population"""
    V = oc.case_velocities(name)
    N = V.shape[1]
    tr = oc.kinetic_truth(name)
    o = orc.OracleSim(N0=max(N, 8))
    psi = oc.random_psi(N, 0)
    o.set_state(oc.positions(N, o.const("L")), V, psi, np.zeros(N), 0.5)
    o7, P, pops = o.observables()
    o.close()
    pv, pB = ot.populations(psi, 0)
    r = {"avg": ot.worst(abs(LD(o7[6]) - tr.out7[6]), tr.B_out7[6]),
         "Ekin": ot.worst(np.abs(ot.to_ld(o7[1:4]) - tr.out7[1:4]), tr.B_out7[1:4]),
         "P": ot.worst(np.abs(ot.to_ld(P) - tr.P), tr.B_P), "pops": ot.worst(np.abs(ot.to_ld(pops) - pv), pB)}
    print(name, "oracle error / B:", {k: round(v[0], 4) for k, v in r.items()})
    assert o7[0] == 0.5
    assert max(v[0] for v in r.values()) <= 1, (name, r)


@pytest.mark.parametrize("N", oc.TAG_SIZES)
@pytest.mark.parametrize("pattern", oc.TAG_PATTERNS)
def test_tagged_model_inside_B(N, pattern):
    tr = oc.tagged_truth(N, pattern)
    P, mom = tagged_model(oc.tagged_velocities(N), oc.tag_pattern(N, pattern))
    if pattern == "none":
        assert not P.any() and not tr.P.any() and np.isnan(mom).all() and np.isnan(tr.mom).all()
        return
    rp, rm = ot.worst(np.abs(ot.to_ld(P) - tr.P), tr.B_P), ot.worst(np.abs(ot.to_ld(mom) - tr.mom), tr.B_mom)
    print(N, pattern, f"tagged model error / B: P {rp[0]:.4f}, moments {rm[0]:.4f}")
    assert rp[0] <= 1 and rm[0] <= 1


# ---------------------------------------------------------------------------------------------
# 3. the one-defect models outside B
# ---------------------------------------------------------------------------------------------

MUTANTS = [
    ("last_of_chunk", ("N65", "N257", "N1089")),
    ("second_pass", ("big",)),
    ("skip_0.0760", ("N65", "N255", "N256", "N257")),
    ("avg_not_on_x", ("N257",)),
    ("avg_on_y", ("N257",)),
    ("no_mirror", ("N257",)),
    ("tree_level", ("N1025",)),
]


@pytest.mark.parametrize("defect,names", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_outside_B(defect, names):
    best = 0.0
    for name in names:
        r = ratios(*model_of(name, defect), oc.kinetic_truth(name))
        good = ratios(*model_of(name), oc.kinetic_truth(name))
        assert max(v[0] for v in good.values()) <= 1            # the same model without the defect is inside
        w = max(r.items(), key=lambda kv: kv[1][0])
        print(f"{defect} at {name}: worst error / B = {w[1][0]:.3g} ({w[0]}, element {w[1][1]})")
        best = max(best, w[1][0])
    assert best >= 2, (defect, best)


def test_mutant_skip_radius_is_seen_in_subnormal_bins_only():
    """the defect of 0.0760 for 0.0773 drops terms of order 1e-314: no norm-wise comparison sees it"""
    seen = 0
    for name in ("N65", "N255", "N256", "N257"):
        P0, P1, tr = model_of(name)[2], model_of(name, "skip_0.0760")[2], oc.kinetic_truth(name)
        diff = np.abs(P1 - P0)
        assert diff.max() <= 1e-300 * max(P0.max(), 1.0)
        seen += int((np.abs(ot.to_ld(P1) - tr.P) > 2 * tr.B_P).sum())
    assert seen > 0


def test_mutant_model3_grouped_as_model0():
    psi = oc.random_psi(257, 3)
    val, B = ot.populations(psi, 3)
    assert ot.worst(np.abs(ot.to_ld(pops_model(psi, 3)) - val), B)[0] <= 1
    assert ot.worst(np.abs(ot.to_ld(pops_model(psi, 0)) - val), B)[0] >= 2


def test_mutant_tagged_last_only_chunk_skipped():
    best = 0.0
    for N in oc.TAG_SIZES:
        tr = oc.tagged_truth(N, "last")
        P, _ = tagged_model(oc.tagged_velocities(N), oc.tag_pattern(N, "last"), defect="last_only_chunk")
        best = max(best, ot.worst(np.abs(ot.to_ld(P) - tr.P), tr.B_P)[0])
    assert best >= 2
