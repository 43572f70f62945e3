"""CPU checks of the QT substeps' extended-precision truth and bound (tests/qt_truth.py, tests/qt_cases.py):

  * the long double trajectory agrees with the same algebra on mpmath numbers (40 digits) to 2^-58 of |psi|,
    for every operator set (model 0, the pumping models 1-3, the three-level program), 3 ions, 8 substeps,
    one ion jumping;
  * the double oracle — OracleSim.step() and orc_qstep_ion for every ion and substep of every case the GPU
    test runs (tests/dense_three_state.py for the three-level program) — stays inside the bound B: the
    inputs are such that the reference arithmetic alone is within the gate;
  * teeth: the same oracle with gamToE off by a relative 2^-32 (orc_set_qt_constants) is outside B on
    every ion that does not jump, after 25 substeps — an error of ~1e-12 per substep that the 1e-9 gates
    of the MD-step tests cannot see;
  * every decision margin of every case is >= 2^-30 and every position margin >= 2^-30 L with no ion
    excluded (the seeds are picked from the truth alone, in qt_cases.build)."""
import numpy as np
import pytest

from tests import dense_three_state as D3
from tests import qt_cases as qc
from tests import qt_truth as qt

pytestmark = pytest.mark.skipif(not qt.extended_ok(), reason=qt.SKIP_MESSAGE)

LD = np.longdouble


def oracle_run(orc, c, seed, st, U, gamToE_rel=0.0):
    """the double reference arithmetic over a case: per substep OracleSim.step(), then orc_qstep_ion for every
    ion on the tape's uniforms.  Returns per-substep lists psi [N][12][2], V [3][N], R [3][N], tPart, jumped."""
    N, nsub = c["N"], c["nsub"]
    kw = dict(N0=N, seed=seed, job=qc.PHILOX_JOB, rng_mode=1, **c["params"])
    if c["model"] != 0:
        kw["qt_model"] = c["model"]
    o = orc.OracleSim(**kw)
    dtQ = o.const("quantumTimestep")
    if gamToE_rel:
        o.set_qt_constants(dtQ, o.const("gamToEinsteinFreq") * (1 + gamToE_rel), o.const("plasVelToQuantVel"),
                           0.0754 if c["model"] == 3 else 0.0617)
    R, V, psi, tp = st["R"].copy(), st["V"].copy(), st["psi"].copy(), st["tPart"].copy()
    t = c["t0"]
    out = dict(psi=[], V=[], R=[], tPart=[], jumped=[])
    for s in range(nsub):
        o.set_state(R, V, psi, tp, t)
        o.set_forces(st["F"])
        o.step()
        g = o.get_state()
        R, V = g["R"], g["V"]
        jumped = np.zeros(N, bool)
        for i in range(N):
            q = o.qstep_ion(t, psi[i], V[0, i], tp[i], U[s, i])
            psi[i], V[0, i], tp[i], jumped[i] = q["psi"], q["vx"], q["tPart"], q["jumped"]
        t = t + dtQ
        for k, v in (("psi", psi), ("V", V), ("R", R), ("tPart", tp), ("jumped", jumped)):
            out[k].append(v.copy())
    o.close()
    return out


def three_level_run(c, st, U):
    """tests/dense_three_state.py's double qstep_batch over a three-level case"""
    psi = st["psi"][:, :3, 0] + 1j * st["psi"][:, :3, 1]
    vx, tp = st["V"][0].copy(), st["tPart"].copy()
    out = dict(psi=[], V=[], R=[], tPart=[], jumped=[])
    for s in range(c["nsub"]):
        psi, vx, tp, j, _ = D3.qstep_batch(psi, vx, tp, U[s, :, 0], U[s, :, 1])
        p12 = np.zeros((c["N"], 12, 2))
        p12[:, :3, 0], p12[:, :3, 1] = psi.real, psi.imag
        V = st["V"].copy()
        V[0] = vx
        for k, v in (("psi", p12), ("V", V), ("R", None), ("tPart", tp.copy()), ("jumped", j.copy())):
            out[k].append(v)
    return out


def ratios(c, tr, run, st):
    """the largest err / B over the substeps, per quantity: (psi, vx, vyz, R) with the (substep, ion) of the
    psi maximum; asserts the jump sets and tPart's double accumulation on the way"""
    worst = dict(psi=0.0, vx=0.0, vyz=0.0, R=0.0)
    where = (0, 0)
    for s in range(c["nsub"]):
        assert np.array_equal(run["jumped"][s], tr["jumped"][s]), (c["name"], s)
        assert np.array_equal(run["tPart"][s], tr["tPart_double"][s]), (c["name"], s)
        ep = qt.psi_error(tr, s, run["psi"][s]) / tr["Bpsi"][s].clip(min=1e-300)
        ep = np.where(tr["jumped"][s], np.where(qt.psi_error(tr, s, run["psi"][s]) > 0, np.inf, 0.0), ep)   # a basis state: exact
        if ep.max() > worst["psi"]:
            worst["psi"], where = float(ep.max()), (s, int(np.argmax(ep)))
        Vt = tr["V"][s]
        ev = np.abs(run["V"][s].astype(LD) - Vt).astype(np.float64)
        worst["vx"] = max(worst["vx"], float((ev[0] / tr["Bvx"][s]).max()))
        if run["R"][s] is not None:
            worst["vyz"] = max(worst["vyz"], float((ev[1:].max(axis=0) / tr["Bv"][s]).max()))
            er = np.abs(run["R"][s].astype(LD) - tr["R"][s]).astype(np.float64).max(axis=0)
            worst["R"] = max(worst["R"], float((er / tr["BR"][s]).max()))
    return worst, where


def test_case_defaults_are_the_reference_defaults(orc):
    p = orc.default_params()
    for k, v in qc.DEFAULT0.items():
        assert getattr(p, k) == v, k


# ---------------------------------------------------------------------------------------------
MP_SETS = ["heavy_jump_N70_s25", "phase_ladder_heavy_N70_s17", "fracOfSig0.4_N70_s25", "renorm_N70_s25", "general_t0_N70_s2",
           "pump1_lanes_N70_s25", "pump2_lanes_N70_s25", "pump3_lanes_N70_s25", "three_level_N70_s32"]


@pytest.mark.parametrize("name", MP_SETS)
def test_truth_matches_mpmath(orc, name):
    """long double against 40-digit mpmath on 3 ions x 8 substeps, ion 0 forced to jump in substep 3: the
    two agree to 2^-58 of |psi| (and of |v|, L).  On the phase ladder long double itself sees phi only to
    2^-64 |phi| — 2^-11 / c of the bound's phase term, c >= 10 — so there the two must agree to 2^-10 of B."""
    c = dict(qc.BY_NAME[name])
    st = qc.make_state(c, 7)
    pick = [0, 5, 9]                                   # (ladder states: octaves 8, 13 and 17)
    sub = {k: (v[..., pick] if k in ("R", "V", "F") else v[pick] if k != "L" else v) for k, v in st.items()}
    c["N"], c["nsub"] = 3, 8
    U = qc.uniforms(dict(c, N=10), orc, 7)[:, pick].copy()
    U[3, 0, 0] = 1e-9                                  # u1 below any dp: the jump branch
    a = qc.run_truth(c, sub, U)
    b = qc.run_truth(c, sub, U, B=qt.MPBackend(40), bound=False)
    assert a["jumped"][3][0] and b["jumped"][3][0]
    mpb = qt.MPBackend(40)

    def diff(x, y):                                    # |x - y| as doubles, x long double (hi + lo), y mpmath
        hi = x.astype(np.float64)
        lo = (x - hi.astype(LD)).astype(np.float64)
        return mpb.f64(np.abs(mpb.num(hi) + mpb.num(lo) - y))

    worst = 0.0
    for s in range(8):
        assert np.array_equal(a["jumped"][s], b["jumped"][s]) and np.array_equal(a["target"][s], b["target"][s])
        nrm = np.sqrt((a["psi_re"][s].astype(np.float64) ** 2 + a["psi_im"][s].astype(np.float64) ** 2).sum(axis=1))
        scale = a["Bpsi"][s] * 2.0 ** 48 if "ladder" in name else nrm          # (x 2^-58 below)
        for ka in ("psi_re", "psi_im"):
            d = diff(a[ka][s], b[ka][s]).max(axis=1)
            worst = max(worst, float(np.where(d > 0, d / np.where(scale > 0, scale, 1e-300), 0.0).max()))
        assert diff(a["V"][s], b["V"][s]).max() <= 2.0 ** -58 * 3.0
        if a["R"][s] is not None:
            assert diff(a["R"][s], b["R"][s]).max() <= 2.0 ** -58 * sub["L"]
    print(f"{name}: long double vs mpmath, max |dpsi| / {'(2^48 B)' if 'ladder' in name else '|psi|'} = {worst:.3e} "
          f"(2^-58 = {2.0 ** -58:.3e})")
    assert worst <= 2.0 ** -58


@pytest.mark.parametrize("name", [c["name"] for c in qc.CASES])
def test_margins_and_oracle_inside_bound(orc, name):
    """every case: the margins hold with no ion excluded, and the double reference arithmetic is inside B"""
    c = qc.BY_NAME[name]
    seed, st, U, tr = qc.build(c, orc)
    d, p = qt.min_margins(tr)
    assert d >= qc.MARGIN
    if c["model"] != "lc3":
        assert p >= qc.MARGIN * st["L"]
    assert qc.requirements(c, tr)
    run = three_level_run(c, st, U) if c["model"] == "lc3" else oracle_run(orc, c, seed, st, U)
    worst, (s, i) = ratios(c, tr, run, st)
    print(f"{name}: seed {seed}, {int(np.array(tr['jumped']).sum())} jumps, margins {d:.2e} / {p:.2e}; oracle err/B: psi "
          f"{worst['psi']:.3g} (substep {s}, ion {i}) vx {worst['vx']:.3g} vy,vz {worst['vyz']:.3g} R {worst['R']:.3g}; "
          f"K {tr['K'][-1].max():.1f} c {tr['c'][-1].max():.0f} Bpsi <= {tr['Bpsi'][-1].max():.2e}")
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", ["prod_N70_s25", "heavy_jump_N70_s25", "fracOfSig0.4_N70_s25", "thread_N300_s25"])
def test_bound_has_teeth(orc, name):
    """gamToE off by a relative 2^-32 — h |H| 2^-32 ~ 1e-12 per substep, invisible to the 1e-9 gates — puts every
    ion that does not jump outside B"""
    c = qc.BY_NAME[name]
    seed, st, U, tr = qc.build(c, orc)
    run = oracle_run(orc, c, seed, st, U, gamToE_rel=2.0 ** -32)
    s = c["nsub"] - 1
    never = ~np.array(tr["jumped"]).any(axis=0)
    assert np.array_equal(np.array(run["jumped"]).any(axis=0), ~never)
    ratio = qt.psi_error(tr, s, run["psi"][s]) / np.where(never, tr["Bpsi"][s], 1.0)
    print(f"{name}: perturbed oracle err/B over the {int(never.sum())} ions without a jump: min {ratio[never].min():.3g}, "
          f"max {ratio[never].max():.3g}")
    assert never.sum() >= c["N"] // 2
    assert (ratio[never] > 1.0).all()
