"""The Newton-3 block scheme (force_scheme 3: k_pairs_n3b, k_pairs_n3b_pw, their plan, tail and reduce
kernels, the spatial order) held per ion to a derived bound against exact (long double) row sums, as
tests/test_gpu_force_accuracy.py holds the rows and the tiles: tests/force_truth.py, whose docstring
derives the blocks' gate_i = geometry + rounding (D = depth_blocks(N)) + Form_i + Tail_i [+ H_i, fast
variant].  Every gate term comes from the truth and from constants the engine publishes before the call
(force_skip_radius, force_*_radius, force_error_eps); none from a device result.

  a. every instance, per ion, weak screening (Ge 0.1: g(L/2) ~ 1e-3 against gates near 1e-13, so a pair
     decided, dropped or counted wrongly shows), with the error-bounded forms off (the rounding gate alone) and
     at the default exponents, random / designed / out-of-range states at the sizes that
     reach each structural path: 129 (one block of three tiles, a ragged tile of one ion), 512 (one full
     block), 513 (two blocks: the half-covered block distance, a block of one tile of one ion, an unpaired
     I tile of the paired-wave kernel), 1100 (three blocks, ragged), 2500 (five blocks), and 5000 ions in
     clumps (ten blocks; compact tiles, so that whole tile pairs and sub-tile groups are skipped);
  b. the potentials (potential_rows(), the POT instances) on the same states;
  c. one error-bounded tier at a time with its exponent lowered until its stated error dominates the
     rounding, against the truth and against the same call with the tier off;
  d. the default exponents at strong screening (N = 5000, Ge 3), where every tier and the tail engage;
  e. the enforcement (k_tail_fix) on a clustered state of 5000 ions, every ion checked.

The instances n3b_kernel_of (mdqt_n3b.hip) can return — seven per mode, forces and POT: the table in the
issue counts 16, the function's branches give 14 — and a case that launches each (a: test_forces_per_ion,
b: test_potentials_per_ion; the case ids are name-kernel-pairs-ax1-sort-tiers and name-kernel-plan-pairs-ax1-tiers):

  k_pairs_n3b_pw<1, false, false, true>    a random513-1-1-1-1-0, -1 (paired waves, one-axis image)
  k_pairs_n3b_pw<1, false, false, false>   a random513-1-1-0-1-0, random513-1-1-1-0-0 (unsorted: no plan)
  k_pairs_n3b<1, false, false, true>       a random1100-1-0-1-1-0, -1
  k_pairs_n3b<1, false, false, false>      a random1100-1-0-0-1-0, random1100-1-0-1-0-0
  k_pairs_n3b<1, true, false, false>       a outofrange1100-1-1-1-1-0 (GUARD ignores pairs and ax1)
  k_pairs_n3b<0, true, false, false>       a outofrange1100-0-1-1-1-0
  k_pairs_n3b<0, false, false, false>      a designed1100-0-1-1-1-0
  k_pairs_n3b_pw<1, false, true, true>     b random513-1-1-1-1-0, -1 (on the plan)
  k_pairs_n3b_pw<1, false, true, false>    b random513-1-1-1-0-0, random513-1-0-1-1-0 (no plan: no AXP)
  k_pairs_n3b<1, false, true, true>        b random1100-1-1-0-1-0, -1
  k_pairs_n3b<1, false, true, false>       b random1100-1-0-0-1-0
  k_pairs_n3b<1, true, true, false>        b outofrange1100-1-1-1-1-0
  k_pairs_n3b<0, true, true, false>        b outofrange1100-0-1-1-1-0
  k_pairs_n3b<0, false, true, false>       b designed1100-0-1-1-1-0

Each case prints D, phi, phi_ref and max_i |dF_i| / gate_i (run with -s)."""
import numpy as np
import pytest

from tests import force_truth as ft

pytestmark = pytest.mark.gpu

LD = np.longdouble
WEAK, STRONG = 0.1, 3.0
TIER_OPTIONS = ("force_mid_exp", "force_far_exp", "force_vfar_exp", "force_ufar_exp")
DEFAULT_EXP = 13


@pytest.fixture(scope="module")
def eng():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


@pytest.fixture(scope="module")
def sims(eng):
    """one Simulation per box (N0, Ge), made on first use: L follows N0, lDeb follows Ge"""
    made = {}

    def get(N0, Ge):
        if (N0, Ge) not in made:
            made[(N0, Ge)] = eng.Simulation(N0=N0, Ge=Ge)
        return made[(N0, Ge)]
    yield get
    for s in made.values():
        s.close()


MAKERS = {"random": ft.random_state, "designed": ft.designed_state, "outofrange": ft.out_of_range_state,
          "clustered": lambda N, L: ft.clustered_state(N, L, 0.4, 0.3), "clumped": ft.clumped_state}
_cache = {}


def state(kind, N, Ge, sim, orc=None):
    """positions, exact row sums and (with the oracle) its own phi of a state: computed once, shared, unchanged"""
    key = (kind, N, Ge)
    L, lDeb = sim.const("L"), sim.const("lDeb")
    if key not in _cache:
        R = MAKERS[kind](N, L)
        t = ft.row_sums_threads(R, L, lDeb) if N > 1500 else ft.row_sums(R, L, lDeb)
        assert t.nshell == (6 if kind == "designed" else 0)
        R.setflags(write=False)
        _cache[key] = [R, t, ft.geom_roundings(R, L), None, None]
    c = _cache[key]
    if orc is not None and c[3] is None:
        R, t = c[0], c[1]
        c[3] = ft.phi(ft.force_err(orc.forces_raw(R, L, lDeb), t), t.P, t.H)
        c[4] = ft.phi(ft.potential_err(orc.potentials_index(R, np.arange(N), L, lDeb), t), t.U, t.Hu)
    return c


def load(sim, R, kernel=1, pairs=1, ax1=1, sort=1, form_mode=2, tail_exp=12, exps=None, plan=1):
    """every option of the block scheme set, then the state: a case never inherits another's options.  The
    tail mode's round trip forgets a radius an earlier case's enforcement widened"""
    N = R.shape[1]
    sim.set_option("force_scheme", 3)
    sim.set_option("force_kernel", kernel)
    sim.set_option("force_n3b_pairs", pairs)
    sim.set_option("force_ax1", ax1)
    sim.set_option("force_sort", sort)
    sim.set_option("force_tail_mode", 0)
    sim.set_option("force_tail_mode", 1)
    sim.set_option("force_form_mode", form_mode)
    sim.set_option("force_tail_exp", tail_exp)
    for o in TIER_OPTIONS:
        sim.set_option(o, (exps or {}).get(o, 0 if exps is not None else DEFAULT_EXP))
    sim.set_option("potential_n3", 1)
    sim.set_option("potential_plan", plan)
    psi = np.zeros((N, 12, 2))
    psi[:, 0, 0] = 1.0
    sim.set_state(R, np.zeros((3, N)), psi, np.zeros(N), 0.0)
    assert sim.N == N and sim.const("force_scheme") == 3 and sim.const("force_tail_scale") == 1
    assert sim.const("n3b_block_count") == ft.block_layout(N)[1]


def block_terms(sim, R, planned=True):
    """Form_i and Tail_i of the next call from the radii the engine chose (read before the call); an
    unplanned potential call runs every pair to L/2 in the exact form: no terms"""
    L, lDeb = sim.const("L"), sim.const("lDeb")
    if not planned:
        return ft.block_terms(R, L, lDeb, {}, L / 2, False)
    radii = {e: sim.const(f"force_{name}_radius") for e, name in ft.TIERS.items()}
    return ft.block_terms(R, L, lDeb, radii, sim.const("force_skip_radius"), not sim.const("force_form_measured"))


def check(label, what, err, gate, scale, E, H, form, D, phi_ref):
    """every ion inside its gate; phi as check_forces (test_gpu_force_accuracy.py) asks of the unscaled forms,
    the error-bounded forms' stated error (Form_i, in units of u scale_i) allowed on top"""
    ratio = err / gate
    worst = int(np.argmax(ratio))
    ph = ft.phi(err, scale, H)
    line = f"{label}: D = {D}, phi = {ph:.2f}"
    bound = None
    if phi_ref is not None:
        bound = 4 * phi_ref + float(((E + form.astype(LD) / LD(ft.U53)) / scale).max())
        line += f", phi_ref = {phi_ref:.2f} (gate {bound:.1f})"
    print(line + f", max |d{what}_i|/gate_i = {float(ratio[worst]):.4f} (ion {worst}), max |d{what}_i| = {float(err.max()):.3e}")
    assert ratio[worst] <= 1, (label, worst, float(err[worst]), float(ratio[worst]))
    if bound is not None:
        assert ph <= bound, (label, ph, bound)
    return float(ratio[worst])


def check_forces(label, F, t, b, L, D, fast, geom, phi_ref=None):
    assert np.isfinite(np.asarray(F)).all()
    return check(label, "F", ft.force_err(F, t), ft.block_force_gate(t, b, L, D, fast, geom), t.P, t.E, t.H, b.form,
                 D, phi_ref)


def check_potentials(label, U, t, b, L, D, fast, geom, phi_ref=None):
    assert np.isfinite(U).all()
    return check(label, "U", ft.potential_err(U, t), ft.block_potential_gate(t, b, L, D, fast, geom), t.U, t.Eu,
                 t.Hu, b.formu, D, phi_ref)


# ---------------------------------------------------------------------------------------------
# a, b: every instance on every state, weak screening
# ---------------------------------------------------------------------------------------------

STATES = [("random", 129), ("random", 512), ("random", 513), ("random", 1100), ("random", 2500),
          ("designed", 129), ("designed", 1100), ("outofrange", 129), ("outofrange", 1100)]
# (kernel, pairs, ax1, sort, tiers): the combinations that take a distinct instance or table — the fast
# variant's four kernels on the plan, paired waves on the plan without skipping, both kernels without a plan
# (unsorted); the exact variant and the GUARD instances ignore pairs and ax1.  tiers 0: the error-bounded forms
# off, so the gate is the rounding gate alone and g(L/2) stands far above it; tiers 1: the default exponents
# (the product's call; on the one-axis image path only the error-bounded levels take the shifted i position),
# Form_i in the gate and, where the engine measures and enforces, its own budget asked too
FAST = [(1, 1, 1, 1, 0), (1, 1, 0, 1, 0), (1, 0, 1, 1, 0), (1, 0, 0, 1, 0), (1, 1, 1, 2, 0), (1, 1, 1, 0, 0),
        (1, 0, 1, 0, 0), (1, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 1, 2, 1)]
EXACT = [(0, 1, 1, 1, 0), (0, 1, 1, 2, 0), (0, 1, 1, 0, 0)]
GUARDED = [(1, 1, 1, 1, 0), (1, 1, 1, 2, 0), (1, 1, 1, 0, 0), (1, 1, 1, 1, 1)] + EXACT
FORCE_CASES = [(k, n, *c) for k, n in STATES for c in (GUARDED if k == "outofrange" else FAST + EXACT)]
# Skipping proper.  A tile of 64 ions is ~6.4 wide and a sub-tile of 16 ~4 at the uniform density, whatever N, so
# up to 5000 ions (L/2 <= 13.8) no tile pair and hardly a sub-tile group lies wholly beyond the cutoff (N = 5000:
# 0.08 % of the pairs): a build whose skip radius was 5 % short passed every uniform case.  In clumps of 64 ions
# of radius 1 the tiles are ~2 wide, and at 5000 ions whole tile pairs are skipped — asserted from the census —
# while g(L/2) = 2.5e-5 still stands far above the gate.
SKIP_N = 5000
FORCE_CASES += [("clumped", SKIP_N, *c)
                for c in ((1, 1, 1, 1, 0), (1, 0, 1, 1, 0), (1, 1, 1, 2, 0), (1, 1, 1, 1, 1), (0, 1, 1, 1, 0))]
# (kernel, plan, pairs, ax1, tiers)
POT_FAST = [(1, 1, 1, 1, 0), (1, 1, 0, 1, 0), (1, 1, 1, 0, 0), (1, 0, 1, 1, 0), (1, 0, 0, 1, 0), (1, 1, 1, 1, 1),
            (1, 1, 0, 1, 1), (0, 1, 1, 1, 0), (0, 0, 1, 1, 0)]
POT_GUARDED = [(1, 1, 1, 1, 0), (1, 0, 1, 1, 0), (1, 1, 1, 1, 1), (0, 1, 1, 1, 0), (0, 0, 1, 1, 0)]
POT_CASES = [(k, n, *c) for k, n in STATES for c in (POT_GUARDED if k == "outofrange" else POT_FAST)]
POT_CASES += [("clumped", SKIP_N, *c) for c in ((1, 1, 1, 1, 0), (1, 0, 1, 1, 0), (1, 1, 1, 1, 1), (0, 1, 1, 1, 0))]


def case_id(c):
    return f"{c[0]}{c[1]}-" + "-".join(str(x) for x in c[2:])


def budget_check(label, what, sim, err, rp, scale=1.0):
    """where the engine measures and enforces its error-bounded parts (force_error_eps > 0): every ion within
    that budget + the rounding part, whatever Form_i allows"""
    eps = sim.const("force_error_eps")
    if sim.const("force_form_measured") and eps > 0:
        eps_check(label, what, err, scale * eps, rp)


@pytest.mark.parametrize("case", FORCE_CASES, ids=case_id)
def test_forces_per_ion(sims, orc, case):
    kind, N, kernel, pairs, ax1, sort, tiers = case
    sim = sims(N, WEAK)
    R, t, geom, phi_ref, _ = state(kind, N, WEAK, sim, orc)
    L, D = sim.const("L"), ft.depth_blocks(N)
    guard = kind == "outofrange"
    load(sim, R, kernel, pairs, ax1, sort, exps=None if tiers else {})
    assert sim.const("range_guard") == (1 if guard else 0) and sim.const("force_sort") == sort
    assert sim.const("force_n3b_pairs") == pairs and sim.const("force_ax1") == ax1
    assert sim.const("force_skip_radius") == L / 2          # weak screening: nothing skipped inside the cutoff
    b = block_terms(sim, R)
    assert not b.tail.any()
    if N == SKIP_N and sort == 1:                            # the case's own sharpness: the plan does skip
        census = sim.force_census()
        assert census["skip_cut"][1] > 0 and census["skip_sub"][1] > 0     # whole tile pairs, and groups
        print(f"{case_id(case)}: {census['skip_cut'][1]:.0f} ion pairs in skipped tile pairs, {census['skip_sub'][1]:.0f} "
              f"in culled sub-tile groups, of {N * (N - 1) // 2}")
    if not tiers or guard:                                   # (the error-bounded forms: the fast plan's, no guard)
        assert not b.form.any() and sim.const("force_error_eps") == 0
    sim.forces()
    F = sim.get_state()["F"]
    # no shell allowance with force_kernel 0: the exact variant claims the reference's pair set, through
    # tile-pair skipping (sort 1) too
    check_forces(case_id(case), F, t, b, L, D, kernel == 1, geom, phi_ref)
    if tiers and not guard:
        budget_check(case_id(case), "F", sim, ft.force_err(F, t), ft.force_gate(t, L, D, True, geom))
    assert sim.const("force_scheme") == 3 and sim.const("range_guard") == (1 if guard else 0)


@pytest.mark.parametrize("case", POT_CASES, ids=case_id)
def test_potentials_per_ion(sims, orc, case):
    """potential_rows() on the blocks: on the force call's plan (potential_plan 1, fast variant, no guard) or
    every pair to L/2 in the exact form"""
    kind, N, kernel, plan, pairs, ax1, tiers = case
    sim = sims(N, WEAK)
    R, t, geom, _, phi_ref = state(kind, N, WEAK, sim, orc)
    L, D = sim.const("L"), ft.depth_blocks(N)
    guard = kind == "outofrange"
    load(sim, R, kernel, pairs, ax1, 1, exps=None if tiers else {}, plan=plan)
    assert sim.const("range_guard") == (1 if guard else 0)
    assert sim.const("potential_plan") == plan and sim.const("potential_n3") == 1
    planned = plan == 1 and kernel == 1 and not guard
    b = block_terms(sim, R, planned=planned)
    if not tiers or not planned:
        assert not b.formu.any() and not b.tailu.any()
    U = sim.potential_rows()
    check_potentials(case_id(case), U, t, b, L, D, kernel == 1, geom, phi_ref)
    if tiers and planned:
        budget_check(case_id(case), "U", sim, ft.potential_err(U, t), ft.potential_gate(t, L, D, True, geom),
                     sim.const("lDeb"))
    assert sim.const("force_scheme") == 3 and sim.const("range_guard") == (1 if guard else 0)


# ---------------------------------------------------------------------------------------------
# c: one tier at a time, its stated error made visible
# ---------------------------------------------------------------------------------------------

# tier: (plan level, option, exponent, census classes).  N = 1100, Ge 0.1, a-priori radii (force_form_mode
# 0), no tail.  The exponents are chosen on the CPU from the truth and the radius model alone (asserted
# below).  A form runs on a sub-tile group only when all four of its sub-box gaps reach the radius, and a
# 16-ion sub-tile is ~4 wide in a box of L/2 = 8.3: at far 8 (r_far = 6.5, Form_i >= 230 x the rounding part
# of every ion's gate) the census finds no such group and F_on = F_off, so the radii are brought inside one
# sub-tile width: far 5 (r = 0.56), very far 3 (0.73), ultra far 3 (0.83) — Form_i >= 5,000 x the rounding
# part.  The f32 level comes with ultra far; at weak screening its cutoff term keeps it off.  The mid form's
# stated error, (r/lDeb + 3) 2.2e-14 + 4e-15 ~ 1e-13, is ~900 roundings of a term where the gate's rounding
# part already allows D + KF + KT r/lDeb ~ 200 of them: no exponent brings Form_i to 100 x the rounding part
# (its supremum over r is below 10).  Its sharpness condition is instead the same 100 on the scale of the
# ion's own row sum, Form_i >= 100 u P_i, with r_mid = 0.9 (exponent 10: exact-form and mid-form pairs both
# present).
TIER_N = 1100
TIERS = {"mid": (1, "force_mid_exp", 10, ("mid_image", "mid_uniform")),
         "far": (2, "force_far_exp", 5, ("far_image", "far_uniform")),
         "vfar": (3, "force_vfar_exp", 3, ("vfar_image", "vfar_uniform")),
         "ufar": (4, "force_ufar_exp", 3, ("ufar_image", "ufar_uniform", "ufar32_uniform"))}


@pytest.mark.parametrize("tier", list(TIERS))
def test_one_tier_at_a_time(sims, tier):
    level, option, k, classes = TIERS[tier]
    N = TIER_N
    sim = sims(N, WEAK)
    R, t, geom, _, _ = state("random", N, WEAK, sim)
    L, D = sim.const("L"), ft.depth_blocks(N)
    # the tier off: the exact form on every pair inside L/2
    load(sim, R, form_mode=0, tail_exp=0, exps={})
    assert all(sim.const(f"force_{n}_radius") == L / 2 for n in ft.TIERS.values())
    sim.forces()
    F_off = sim.get_state()["F"]
    U_off = sim.potential_rows()
    none = block_terms(sim, R)
    assert not none.form.any() and not none.tail.any()
    check_forces(f"{tier} off", F_off, t, none, L, D, True, geom)
    # the tier on
    load(sim, R, form_mode=0, tail_exp=0, exps={option: k})
    assert sim.const("force_form_measured") == 0 and sim.const("force_skip_radius") == L / 2
    radius = sim.const(f"force_{ft.TIERS[level]}_radius")
    assert 0 < radius < L / 2
    assert all(sim.const(f"force_{n}_radius") == L / 2 for e, n in ft.TIERS.items() if e not in (level, 5))
    b = block_terms(sim, R)
    assert not b.tail.any() and b.nform[level] > 0
    census = sim.force_census()
    in_class = sum(census[c][1] for c in classes)
    sim.forces()
    F_on = sim.get_state()["F"]
    U_on = sim.potential_rows()
    for what, on, off, form, scale, checker in (("F", F_on, F_off, b.form, t.P, check_forces),
                                                ("U", U_on, U_off, b.formu, t.U, check_potentials)):
        pot = what == "U"
        rp = ft.rounding_part(t, L, D, geom, potential=pot)
        # the test's own sharpness: the stated error dominates the rounding, the class has pairs, the tier ran
        sharp = float((form / (LD(ft.U53) * scale)).min()) if tier == "mid" else float((form / rp).min())
        worst = checker(f"{tier} 1e-{k} ({what})", on, t, b, L, D, True, geom)
        diff = np.abs(np.asarray(on, dtype=np.float64) - off)
        diff = diff.max(axis=0) if diff.ndim == 2 else diff
        print(f"{tier} ({what}): radius {radius:.3f} of L/2 = {L / 2:.3f}, {in_class:.0f} ion pairs in its census classes, "
              f"min_i Form_i / {'(u P_i)' if tier == 'mid' else 'rounding_i'} = {sharp:.1f}, "
              f"max_i |d{what}_i(on - off)| / Form_i = {float((diff / form).max()):.4f}, "
              f"max_i |d{what}_i| / gate_i = {worst:.4f}")
        assert sharp >= 100
        assert in_class > 0
        assert (diff <= form + 2 * rp).all()
        assert (diff > 0).any()


# ---------------------------------------------------------------------------------------------
# d, e: the default exponents at strong screening; the enforcement
# ---------------------------------------------------------------------------------------------

STRONG_N = 5000


def eps_check(label, what, err, eps, rp):
    """every ion within the engine's own budget (force_error_eps: the tail's and the tiers') + the rounding
    part, which covers the distance between the exact sum to L/2 in double and the long double truth"""
    ratio = err / (LD(eps) + rp)
    worst = int(np.argmax(ratio))
    print(f"{label}: max |d{what}_i| / (eps + rounding_i) = {float(ratio[worst]):.4f} (ion {worst}; eps {eps:.2e})")
    assert ratio[worst] <= 1, (label, worst, float(err[worst]))


@pytest.mark.parametrize("form_mode", [2, 0])
def test_default_exponents_strong_screening(sims, form_mode):
    N = STRONG_N
    sim = sims(N, STRONG)
    R, t, geom, _, _ = state("random", N, STRONG, sim)
    L, lDeb, D = sim.const("L"), sim.const("lDeb"), ft.depth_blocks(N)
    load(sim, R, form_mode=form_mode)
    assert sim.const("force_form_measured") == (1 if form_mode else 0)
    skip = sim.const("force_skip_radius")
    radii = {n: sim.const(f"force_{n}_radius") for n in ft.TIERS.values()}
    assert skip < L / 2 and all(r < skip for r in radii.values())      # every tier and the tail engage
    eps = sim.const("force_error_eps")
    assert 0 < eps <= 1.5e-12 * (1 + 1e-9)
    b = block_terms(sim, R)
    assert b.ntail > 0 and all(n > 0 for n in b.nform.values()) and len(b.nform) == 5
    print(f"N = {N}, Ge {STRONG}, form mode {form_mode}: L/2 = {L / 2:.3f}, r_t = {skip:.3f}, radii "
          + ", ".join(f"{n} {r:.3f}" for n, r in radii.items()) + f"; f32 cutoff-shell pairs {b.ncut}")
    sim.forces()
    F = sim.get_state()["F"]
    check_forces(f"strong, form mode {form_mode}", F, t, b, L, D, True, geom)
    eps_check(f"strong, form mode {form_mode}", "F", ft.force_err(F, t), eps, ft.rounding_part(t, L, D, geom))
    U = sim.potential_rows()
    check_potentials(f"strong, form mode {form_mode}", U, t, b, L, D, True, geom)
    eps_check(f"strong, form mode {form_mode}", "U", ft.potential_err(U, t), lDeb * eps,
              ft.rounding_part(t, L, D, geom, potential=True))
    print(f"strong, form mode {form_mode}: tiles recomputed exactly {sim.const('force_tail_fixed_tiles'):.0f}")


def test_enforcement_on_clustered_ions(sims):
    """40 % of 5000 ions in a ball of radius 0.3 at strong screening: the ions a skip radius away from the
    ball lose 2000 partners at once.  From the truth: the sum of g over the pairs beyond the model's radius
    exceeds the call's eps on some ions (Tail_i bounds what a call can drop; the plan drops the sub-blocks
    whose boxes are that far apart).  That the plan's sums then list a tile and k_tail_fix runs is asserted
    on the call itself; every ion, on the ball and off it, stays inside its gate and the engine's budget"""
    N = STRONG_N
    sim = sims(N, STRONG)
    R, t, geom, _, _ = state("clustered", N, STRONG, sim)
    L, D = sim.const("L"), ft.depth_blocks(N)
    load(sim, R)
    skip0, eps = sim.const("force_skip_radius"), sim.const("force_error_eps")
    b = block_terms(sim, R)
    assert skip0 < L / 2 and (b.tail > eps).sum() > 0           # the condition, from the truth's separations
    rp = ft.rounding_part(t, L, D, geom)
    sim.forces()
    F = sim.get_state()["F"]                                     # (a synchronisation: the host reacts)
    fixed = sim.const("force_tail_fixed_tiles")
    print(f"clustered N = {N}: r_t = {skip0:.3f} of L/2 = {L / 2:.3f}, {(b.tail > eps).sum()} ions with an exact tail over "
          f"eps = {eps:.2e} (largest {b.tail.max():.3e}); tiles recomputed {fixed:.0f}")
    assert fixed > 0                                             # the exact pass ran
    check_forces("clustered, first call", F, t, b, L, D, True, geom)
    eps_check("clustered, first call", "F", ft.force_err(F, t), eps, rp)
    # the next call: a wider radius, nothing to fix
    skip1 = sim.const("force_skip_radius")
    assert sim.const("force_tail_scale") > 1 and skip0 < skip1 <= L / 2
    b1 = block_terms(sim, R)
    eps1 = sim.const("force_error_eps")
    sim.forces()
    F1 = sim.get_state()["F"]
    assert sim.const("force_tail_fixed_tiles") == fixed
    assert sim.const("force_tail_bound") <= eps1
    check_forces(f"clustered, second call (r_t {skip1:.3f})", F1, t, b1, L, D, True, geom)
    eps_check("clustered, second call", "F", ft.force_err(F1, t), eps1, rp)
