"""The kernels' device math functions, each held to its stated error on the GPU.

mdqt_device_math (mdqtplasmasims_amd/csrc/mdqt_devmath.hip) evaluates, one element per thread and
through the very inline functions the kernels call, sincos_tab / sincos_fast / sincos_q2
(mdqt_device.hpp), rsq3 and exp_neg (mdqt_math.hpp) and the pair kernels' table 2^t
(mdqt_pairs.hpp exp2_neg_cut_tab).  Every other test of these functions compares one kernel that
calls them with another kernel that calls them too.

The reference is numpy long double (glibc sinl / cosl / expl / exp2l / sqrtl on the x87 format: 64-bit
significand, 2^-11 of a double ulp), itself checked against mpmath at 40 digits on a sample.  About
2e5 arguments per function: log-uniform over the binades of the stated domain, both signs, the binade
edges, the neighbours (0, +-1, +-2 ulp) of the multiples of pi/64 and pi/2 the reductions split at,
+-0, and both ends of each domain.  The limits are what the sources state or what the truth modules
assume (tests/force_truth.py's budget KF builds on rsq3 and exp_neg; tests/qt_truth.py on rsq3 and the
absolute error of sincos_tab) — none is fitted to the GPU:

  sincos_tab, sincos_q2   |error| <= 2^-52 absolute on |x| < 2^20 (a C transcription on the CPU gives
                          1.54e-16; in ulps of the result the error is unbounded near the zeros, and the
                          kernel needs only the absolute statement: c2 = c2re + dms sin);
                          sincos_q2 beyond 2^20 (the library) within 1 ulp of the result
  sincos_fast             < 1 ulp of the result away from the zeros, <= 2^-53 absolute near them
  rsq3                    relative error <= 2 x 2^-53 on [2^-20, 2^20] and on (0.9, 1]
  exp_neg                 <= 1.1 ulp on [-40, 0]
  table 2^t               <= 2 ulp on t in [-60, 0]
  library exp             <= 1 ulp on [-746.9, 0], the ulp clamped to 2^-1074 where the result is subnormal, and
                          exactly +0 at and beyond -V2 kKdeSkip^2 = -746.91 (the velocity distributions' terms and
                          their skip radius: tests/obs_truth.py takes E_EXP = 1 from this, docs/OBSERVABLES.md)

Measured on an MI355X (every test prints its maximum and where):

  sincos_tab / sincos_q2  1.514e-16 absolute (sin, x = -17.146), 1.509e-16 (cos); 2.33 ulp of the result at
                          x = 0.0494 (reported, not a limit)
  library beyond 2^20     0.74 ulp (sin), 0.76 ulp (cos)
  sincos_fast             as found: 1.34 ulp (sin), 1.38 ulp (cos) at results >= 2^-10 — above the limit.  The
                          function dropped the tail of its reduced argument, whose half ulp came on top of
                          the kernels'; it now carries the tail the way fdlibm's kernels take it
                          (mdqt_device.hpp): 0.76 ulp (sin), 0.77 ulp (cos); next to the zeros 0.50 ulp, 5.4e-20 absolute
  rsq3                    1.49 x 2^-53 on (0.9, 1], 1.46 x 2^-53 on [2^-20, 2^20]
  exp_neg                 0.95 ulp
  table 2^t               as found: 2.13 ulp at x = 64 t = -262.50000000000006 — above the limit.  The worst
                          arguments were the ties |g| = 1/2 of the reduction, where the degree-5 Taylor
                          series' truncation (0.32 ulp) came on top of the table entry's, the series' and
                          the product's roundings.  The series is now a fit (0.02 ulp) and the result one
                          FMA on the table entry, fma(te, g q, te), in the same six operations
                          (mdqt_pairs.hpp): 1.00 ulp (1.01 in a C transcription on 3e7 arguments)
  library exp             0.83 ulp on normal results (x = -113.95), 0.88 ulp on subnormal ones (x = -708.75, in
                          units of 2^-1074; none of the 44,791 subnormal results flushed); +0 at and beyond
                          -746.91 on every argument"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
NPTS = 100_000


def _need_extended():
    if np.finfo(LD).eps > 2.0 ** -63:
        pytest.skip("np.longdouble has no 64-bit significand here: no extended-precision reference")


@pytest.fixture(scope="module")
def dm():
    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd.engine import device_math
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    _need_extended()
    return device_math


def ulp_of(y):
    """the double ulp at |y| (y long double): 2^(e - 53) for |y| in [2^(e-1), 2^e)"""
    _, e = np.frexp(np.abs(y))
    return np.ldexp(LD(1), e.astype(np.int64) - 53)


def log_uniform(rng, lo_exp, hi_exp, n, signed=True):
    x = np.exp2(rng.uniform(lo_exp, hi_exp, n))
    return x * rng.choice([-1.0, 1.0], n) if signed else x


def neighbours(x, k=2):
    out = [x]
    lo, hi = x, x
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def binade_edges(lo_exp, hi_exp):
    p = np.exp2(np.arange(lo_exp, hi_exp + 1, dtype=np.float64))
    e = neighbours(p, 1)
    return np.concatenate([e, -e])


def sincos_args(rng, top=2.0 ** 20):
    """|x| < top: the binades from 2^-30, the multiples of pi/64 (the table form's split) and of pi/2
    (sincos_fast's) with their neighbours, the binade edges, +-0 and both ends of the domain"""
    mmax = int(top * 64 / (2 * np.pi)) - 2
    m = np.concatenate([rng.integers(0, mmax, 12000), np.arange(0, 700), mmax - np.arange(0, 64)]).astype(np.float64)
    # the half-way points of the reduction (m + 1/2) 2 pi/64: |r| at its largest, rint at its tie
    mult64 = np.concatenate([neighbours(m * (np.pi / 32)), neighbours((m + 0.5) * (np.pi / 32))])
    q = np.concatenate([rng.integers(0, mmax // 16, 4000), np.arange(0, 300)]).astype(np.float64)
    mult2 = np.concatenate([neighbours(q * (np.pi / 2)), neighbours((q + 0.5) * (np.pi / 2))])
    x = np.concatenate([log_uniform(rng, -30, 20, NPTS), mult64, -mult64[::3], mult2, -mult2[::3],
                        binade_edges(-30, 19), np.array([0.0, -0.0, 0.0526, np.nextafter(top, 0), -np.nextafter(top, 0)])])
    return x[np.abs(x) < top]


def check_truth_against_mpmath(x, fn_ld, fn_mp, rel=2.0 ** -60):
    """a sample of the long double reference against mpmath at 40 digits"""
    import mpmath
    mpmath.mp.dps = 40
    idx = np.linspace(0, x.size - 1, 150).astype(int)
    for i in idx:
        t = fn_ld(LD(x[i]))
        m = fn_mp(mpmath.mpf(float(x[i])))
        d = abs(mpmath.mpf(float(t)) + mpmath.mpf(float(t - LD(float(t)))) - m)
        assert d <= rel * max(abs(m), mpmath.mpf(2) ** -40), (x[i], float(d))


def report(name, x, err, unit):
    i = int(np.argmax(err))
    print(f"{name}: {x.size} arguments, max error {float(err[i]):.4g} {unit} at x = {float(x[i])!r}")
    return float(err[i])


@pytest.mark.parametrize("fn", ["sincos_tab", "sincos_q2"])
def test_table_sincos_absolute_error(dm, fn):
    """the 64-entry table form on |x| < 2^20: |error| <= 2^-52 absolute, sin and cos"""
    import mpmath
    x = sincos_args(np.random.default_rng(1))
    assert x.size > 150_000
    check_truth_against_mpmath(x, np.sin, mpmath.sin)
    check_truth_against_mpmath(x, np.cos, mpmath.cos)
    sn, cs = dm(fn, x)
    xl = x.astype(LD)
    es = np.abs(sn.astype(LD) - np.sin(xl))
    ec = np.abs(cs.astype(LD) - np.cos(xl))
    ms = report(f"{fn} sin", x, es, "absolute")
    mc = report(f"{fn} cos", x, ec, "absolute")
    ru = report(f"{fn} sin, in ulps of the result", x, np.where(np.sin(xl) != 0, es / ulp_of(np.sin(xl)), 0), "ulp")
    assert np.isfinite(ru)                               # (reported only: unbounded near the zeros)
    assert max(ms, mc) <= 2.0 ** -52
    assert sn[x == 0].tolist() == [0.0] * int((x == 0).sum()) and np.all(cs[x == 0] == 1.0)


def test_sincos_q2_library_path_beyond_2_20(dm):
    """|x| >= 2^20 takes the math library's sincos: within 1 ulp of the result"""
    rng = np.random.default_rng(2)
    x = np.concatenate([log_uniform(rng, 20, 40, 60_000), log_uniform(rng, 20, 23, 40_000),
                        np.array([2.0 ** 20, -(2.0 ** 20), np.nextafter(2.0 ** 20, np.inf), 3e6 + 343.0, 2.0 ** 40])])
    x = x[np.abs(x) >= 2.0 ** 20]
    sn, cs = dm("sincos_q2", x)
    xl = x.astype(LD)
    ts, tc = np.sin(xl), np.cos(xl)
    es = np.abs(sn.astype(LD) - ts) / ulp_of(ts)
    ec = np.abs(cs.astype(LD) - tc) / ulp_of(tc)
    ms = report("sincos_q2 (library) sin", x, es, "ulp")
    mc = report("sincos_q2 (library) cos", x, ec, "ulp")
    assert max(ms, mc) <= 1.0


def test_sincos_fast_error(dm):
    """Cody-Waite by pi/2 + the minimax kernels, |x| < 2^20: < 1 ulp of the result away from the zeros
    and <= 2^-53 absolute near them.  "Near" is |result| < 2^-10: there the reduced argument's own
    rounding (relative to r, so a fraction of an ulp of a result ~ r) is what the result carries, and
    1 ulp of the result is below 2^-63 — the consumers multiply by a coupling below 2^-6 and add."""
    x = sincos_args(np.random.default_rng(3))
    sn, cs = dm("sincos_fast", x)
    xl = x.astype(LD)
    worst_u = worst_a = 0.0
    for name, got, tru in (("sin", sn, np.sin(xl)), ("cos", cs, np.cos(xl))):
        ea = np.abs(got.astype(LD) - tru)
        eu = ea / ulp_of(np.where(tru != 0, tru, LD(1)))
        near = np.abs(tru) < 2.0 ** -10
        worst_a = max(worst_a, report(f"sincos_fast {name}, |result| < 2^-10", x, np.where(near, ea, 0), "absolute"))
        report(f"sincos_fast {name}, |result| < 2^-10 (reported only)", x, np.where(near, eu, 0), "ulp")
        worst_u = max(worst_u, report(f"sincos_fast {name}, |result| >= 2^-10", x, np.where(near, 0, eu), "ulp"))
    assert worst_u < 1.0
    assert worst_a <= 2.0 ** -53


def test_rsq3_relative_error(dm):
    """v_rsq_f64 + one third-order step: relative error <= 2 x 2^-53 on [2^-20, 2^20] and on (0.9, 1]
    (the QT prefactor 1/sqrt(1 - dp) and force_truth.py's budget)"""
    rng = np.random.default_rng(4)
    one = np.concatenate([rng.uniform(0.9, 1.0, NPTS), 1.0 - np.exp2(rng.uniform(-53, -4, 20_000)),
                          neighbours(np.array([1.0]), 2)[[0, 1, 3]], np.array([np.nextafter(0.9, 1.0)])])
    one = one[(one > 0.9) & (one <= 1.0)]
    wide = np.concatenate([log_uniform(rng, -20, 20, NPTS, signed=False), np.abs(binade_edges(-19, 19)),
                           np.array([2.0 ** -20, 2.0 ** 20])])
    wide = wide[(wide >= 2.0 ** -20) & (wide <= 2.0 ** 20)]
    import mpmath
    check_truth_against_mpmath(wide, lambda v: 1 / np.sqrt(v), lambda v: 1 / mpmath.sqrt(v))
    worst = 0.0
    for name, x in (("(0.9, 1]", one), ("[2^-20, 2^20]", wide)):
        tru = 1 / np.sqrt(x.astype(LD))
        rel = np.abs(dm("rsq3", x).astype(LD) - tru) / tru
        worst = max(worst, report(f"rsq3 on {name}", x, rel / LD(2.0 ** -53), "x 2^-53 relative"))
    assert worst <= 2.0


def test_exp_neg_error(dm):
    """Cody-Waite by ln 2 + the degree-11 minimax polynomial: <= 1.1 ulp on [-40, 0]"""
    import mpmath
    rng = np.random.default_rng(5)
    k = np.arange(0, 58, dtype=np.float64)
    x = np.concatenate([-rng.uniform(0, 40, NPTS), -log_uniform(rng, -40, 5.3, 60_000, signed=False),
                        -neighbours(k * np.log(2.0)), -neighbours((k + 0.5) * np.log(2.0)),
                        np.array([0.0, -0.0, -40.0, np.nextafter(-40.0, 0)])])
    x = x[(x >= -40) & (x <= 0)]
    check_truth_against_mpmath(x, np.exp, mpmath.exp)
    tru = np.exp(x.astype(LD))
    eu = np.abs(dm("exp_neg", x).astype(LD) - tru) / ulp_of(tru)
    assert report("exp_neg", x, eu, "ulp") <= 1.1


def test_exp2_table_error(dm):
    """the pair kernels' 2^t by the 64-entry table and a fitted series, t = x / 64 in [-60, 0]: <= 2 ulp"""
    import mpmath
    rng = np.random.default_rng(6)
    m = np.arange(0, 3841, dtype=np.float64)
    x = np.concatenate([-rng.uniform(0, 3840, NPTS), -log_uniform(rng, -40, 11.9, 60_000, signed=False),
                        -neighbours(m), -neighbours(m[:-1] + 0.5), np.array([0.0, -0.0, -3840.0])])
    x = x[(x >= -3840) & (x <= 0)]
    check_truth_against_mpmath(x, lambda v: np.exp2(v / 64), lambda v: mpmath.power(2, v / 64))
    tru = np.exp2(x.astype(LD) / 64)
    eu = np.abs(dm("exp2_tab", x).astype(LD) - tru) / ulp_of(tru)
    assert report("table 2^t", x, eu, "ulp") <= 2.0


def ld_to_mp(t):
    """a long double as an mpmath number, exactly (also below the double range)"""
    import mpmath
    m, e = np.frexp(LD(t))
    hi = float(m)
    return (mpmath.mpf(hi) + mpmath.mpf(float(m - LD(hi)))) * mpmath.mpf(2) ** int(e)


def test_library_exp_error_and_underflow(dm):
    """the math library's exp as kde_chunk and tagged_kde_chunk call it, over the whole range of their
    arguments x = -V2 d^2: <= 1 ulp of the result against expl, with the ulp clamped to 2^-1074 where the result
    is subnormal (x < -708.396), and exactly +0 at and beyond -V2 kKdeSkip^2, where the kernels skip the call"""
    import mpmath
    from tests import obs_truth as ot
    rng = np.random.default_rng(7)
    ln2 = np.log(2.0)
    first_sub, last_nonzero = -1022 * ln2, -1075 * ln2         # e^x = 2^-1022; e^x = 2^-1075, the tie to zero
    assert abs(first_sub + 708.3964185322641) < 1e-12 and abs(last_nonzero + 745.1332191019412) < 1e-12
    skip = -ot.V2 * 0.0773 * 0.0773                            # the kernels' (-V2 d) d at d = kKdeSkip
    assert -746.92 < skip < -746.90
    x = np.concatenate([-rng.uniform(0, 746.9, NPTS), -log_uniform(rng, -40, np.log2(746.9), 60_000, signed=False),
                        -rng.uniform(708.0, 746.9, 40_000), -np.abs(binade_edges(-40, 9)),
                        neighbours(np.array([first_sub, last_nonzero, skip, -745.0, -746.0])),
                        np.array([0.0, -0.0, -746.9])])
    x = x[(x >= -746.9) & (x <= 0)]
    xl = x.astype(LD)
    tru = np.exp(xl)
    mpmath.mp.dps = 40
    for i in np.concatenate([np.linspace(0, x.size - 1, 150).astype(int), np.nonzero(x < -708.4)[0][:50]]):
        m = mpmath.exp(mpmath.mpf(float(x[i])))
        assert abs(ld_to_mp(tru[i]) - m) <= mpmath.mpf(2) ** -60 * m, x[i]
    got = dm("exp", x)
    ulp = np.maximum(ulp_of(tru), LD(2.0) ** -1074)
    eu = np.abs(got.astype(LD) - tru) / ulp
    sub = x < first_sub
    report("library exp, normal results", x[~sub], eu[~sub], "ulp")
    report("library exp, subnormal results (ulp = 2^-1074)", x[sub], eu[sub], "ulp")
    assert np.count_nonzero(got[sub]) > 10_000                  # subnormal results are not flushed
    assert report("library exp", x, eu, "ulp") <= 1.0
    beyond = np.concatenate([neighbours(np.array([skip]))[[0, 1, 3]], skip * rng.uniform(1, 2, 1000),
                             np.array([-747.0, -1000.0, -1e6, -1e300, -np.inf])])
    beyond = beyond[beyond <= skip]
    z = dm("exp", beyond)
    assert beyond.size > 1000 and np.all(z == 0.0) and not np.signbit(z).any()


def test_device_math_rejects_bad_arguments(dm):
    from mdqtplasmasims_amd import MdqtError
    with pytest.raises(MdqtError, match="unknown function"):
        dm(7, np.zeros(4))
    with pytest.raises(MdqtError, match="bad arguments"):
        dm("rsq3", np.zeros(0))
