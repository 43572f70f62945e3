"""The force and potential kernels that run at N <= 65,536 — the owner-computes rows and the Newton-3
tiles — held per ion to a derived bound against exact (long double) row sums: tests/force_truth.py,
whose docstring derives gate_i.  Where tests/test_gpu_parity.py asks max|dF| / max|F| < 1e-13 against the
oracle's double sum on init()'s uniform positions, these ask of every ion

  1. |F_i - T_i|_inf <= gate_i and |U_i - U_i^truth| <= gate^U_i;
  2. with force_kernel 0 no allowance for the cutoff shell: a pair decided against the reference shows
     as g(L/2) ~ 1e-3 against a gate near 3e-13;
  3. phi = max_i |dF_i|_inf / (2^-53 P_i) <= 4 phi_ref + max_i E_i / P_i for every instance but the
     box-scaled tile form (n3_terms SC: scheme 2, fast kernel, no range guard), phi_ref the same figure of
     the oracle (the reference's operations) on the same state.  The margin 4: the fast forms' 2^t is
     <= 2 ulp where glibc's exp is <= 1, and the maximum over ~1000 ions of a rounding sum moves by about a
     factor of two with the summation order.

on random states at the tile kernel's sizes (63: one tile; 64: a full tile, the diagonal's 32nd step; 65: a
ragged tile of one ion; 129: three tiles; 1000: sixteen), on a designed state (ions on the box faces, pairs
exactly L/2 apart and one ulp either side, close pairs, the ends of the allowed range), on a state outside the
range (the GUARD instances) and once on C2's own launch.  Each case prints phi, phi_ref and
max_i |dF_i| / gate_i (run with -s)."""
import numpy as np
import pytest

from tests import force_truth as ft

pytestmark = pytest.mark.gpu

SPLIT_CUS = 115          # N = 1000: 136 tile pairs on 115 CUs leave 21 in the last round, 5 of them whole


@pytest.fixture(scope="module")
def eng():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


@pytest.fixture(scope="module")
def sim(eng):
    s = eng.Simulation(N0=1000)
    s.default_split = int(s.const("force_tile_split"))
    yield s
    s.close()


STATES = {
    "random63": (ft.random_state, 63), "random64": (ft.random_state, 64), "random65": (ft.random_state, 65),
    "random129": (ft.random_state, 129), "random1000": (ft.random_state, 1000),
    "designed129": (ft.designed_state, 129), "designed1000": (ft.designed_state, 1000),
    "outofrange129": (ft.out_of_range_state, 129),
}
_cache = {}


def state(name, sim, orc):
    """positions, exact row sums and the oracle's own phi of a state: computed once, shared, unchanged"""
    if name not in _cache:
        L, lDeb = sim.const("L"), sim.const("lDeb")
        make, N = STATES[name]
        R = make(N, L)
        t = ft.row_sums(R, L, lDeb)
        assert t.nshell == (6 if name.startswith("designed") else 0)
        phi_f = ft.phi(ft.force_err(orc.forces_raw(R, L, lDeb), t), t.P, t.H)
        phi_u = ft.phi(ft.potential_err(orc.potentials_index(R, np.arange(N), L, lDeb), t), t.U, t.Hu)
        R.setflags(write=False)
        _cache[name] = (R, t, ft.geom_roundings(R, L), phi_f, phi_u)
    return _cache[name]


def load(sim, R, scheme, kernel, split=None, split_cus=0, potential_n3=1):
    N = R.shape[1]
    sim.set_option("force_scheme", scheme)
    sim.set_option("force_kernel", kernel)
    sim.set_option("force_tile_split", sim.default_split if split is None else split)
    sim.set_option("force_split_cus", split_cus)
    sim.set_option("potential_n3", potential_n3)
    psi = np.zeros((N, 12, 2))
    psi[:, 0, 0] = 1.0
    sim.set_state(R, np.zeros((3, N)), psi, np.zeros(N), 0.0)
    assert sim.N == N and sim.const("force_scheme") == scheme


def depth(sim, scheme, N):
    if scheme == 1:
        assert sim.const("force_slots") == 0
        return ft.depth_rows(N, int(sim.const("force_segments")))
    assert sim.const("force_slots") == (N + 63) // 64
    extra = 0
    if sim.const("force_tile_split_pairs") > 0:
        extra = 4 if sim.const("force_tile_split") == 2 else 1
    return ft.depth_tiles(int(sim.const("force_slots")) + extra)


def check_forces(label, F, t, L, D, fast, geom, scaled, phi_ref):
    err = ft.force_err(F, t)
    ratio = err / ft.force_gate(t, L, D, fast, geom)
    worst = int(np.argmax(ratio))
    ph = ft.phi(err, t.P, t.H)
    bound = 4 * phi_ref + float((t.E / t.P).max())
    print(f"{label}: D = {D}, phi = {ph:.2f}, phi_ref = {phi_ref:.2f} (gate {'none: scaled form' if scaled else f'{bound:.1f}'}), "
          f"max |dF_i|/gate_i = {float(ratio[worst]):.4f} (ion {worst}), max |dF_i| = {float(err.max()):.3e}")
    assert np.isfinite(np.asarray(F)).all()
    assert ratio[worst] <= 1, (label, worst, float(err[worst]), float(ratio[worst]))
    if not scaled:
        assert ph <= bound, (label, ph, bound)
    return ph


FORCE_CASES = [(1, 0, None), (1, 1, None), (2, 0, None), (2, 1, None)]
SPLIT_CASES = [(2, 0, 1), (2, 0, 2), (2, 1, 1), (2, 1, 2)]
CASES = [(n, *c) for n in STATES for c in FORCE_CASES] + \
        [(n, *c) for n in ("random1000", "designed1000") for c in SPLIT_CASES]


@pytest.mark.parametrize("name,scheme,kernel,split", CASES)
def test_forces_per_ion(sim, orc, name, scheme, kernel, split):
    R, t, geom, phi_ref, _ = state(name, sim, orc)
    N, L = R.shape[1], sim.const("L")
    guard = name.startswith("outofrange")
    load(sim, R, scheme, kernel, split, SPLIT_CUS if split else 0)
    assert sim.const("range_guard") == (1 if guard else 0)
    if split:
        assert sim.const("force_tile_split") == split and sim.const("force_tile_split_pairs") > 0
    elif scheme == 2 and sim.const("device_cus") >= 136:
        assert sim.const("force_tile_split_pairs") == 0          # one round of workgroups: nothing to split
    D = depth(sim, scheme, N)
    sim.forces()
    F = sim.get_state()["F"]
    scaled = scheme == 2 and kernel == 1 and not guard
    check_forces(f"{name} scheme {scheme} kernel {kernel} split {split}", F, t, L, D, kernel == 1, geom, scaled, phi_ref)
    assert sim.const("force_scheme") == scheme and sim.const("range_guard") == (1 if guard else 0)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("potential_n3", [1, 0])
@pytest.mark.parametrize("name", list(STATES))
def test_potential_rows_per_ion(sim, orc, name, potential_n3, kernel):
    """potential_rows(): the tile kernel's potential mode (k_pairs_n3_pot, so far checked as a total only) and
    the rows, both pair forms"""
    R, t, geom, _, phi_ref = state(name, sim, orc)
    N, L = R.shape[1], sim.const("L")
    guard = name.startswith("outofrange")
    load(sim, R, 2, kernel, potential_n3=potential_n3)
    assert sim.const("potential_n3") == potential_n3 and sim.const("range_guard") == (1 if guard else 0)
    if potential_n3:                                   # the plain tile-pair table into the potential's own slots
        assert sim.const("force_slots") == (N + 63) // 64
        D = ft.depth_tiles(int(sim.const("force_slots")))
    else:
        D = ft.depth_rows(N, int(sim.const("force_segments")))
    U = sim.potential_rows()
    err = ft.potential_err(U, t)
    ratio = err / ft.potential_gate(t, L, D, kernel == 1, geom)
    worst = int(np.argmax(ratio))
    ph = ft.phi(err, t.U, t.Hu)
    bound = 4 * phi_ref + float((t.Eu / t.U).max())
    print(f"{name} potential_n3 {potential_n3} kernel {kernel}: D = {D}, phi = {ph:.2f}, phi_ref = {phi_ref:.2f} "
          f"(gate {bound:.1f}), max |dU_i|/gate_i = {float(ratio[worst]):.4f} (ion {worst})")
    assert np.isfinite(U).all()
    assert ratio[worst] <= 1, (name, worst, float(err[worst]), float(ratio[worst]))
    assert ph <= bound


def test_c2_launch_per_ion(eng, orc):
    """BASELINE configs[1] (C2) as bench.py runs it: N = 3,573, 56 Newton-3 tile slots and the split's extra one
    on 256 CUs, the box-scaled fast form — the instance the headline times — every row against its exact sum"""
    s = eng.Simulation(N0=3500, seed=12346, job=1).init()
    assert s.N == 3573
    s.forces()
    st = s.get_state()
    L, lDeb = s.const("L"), s.const("lDeb")
    assert s.const("force_scheme") == 2 and s.const("force_slots") == 56 and s.const("range_guard") == 0
    split = s.const("force_tile_split_pairs") > 0
    if s.const("device_cus") == 256:
        assert split
    D = ft.depth_tiles(56 + (0 if not split else 4 if s.const("force_tile_split") == 2 else 1))
    s.close()
    t = ft.row_sums(st["R"], L, lDeb)
    assert t.nshell == 0
    phi_ref = ft.phi(ft.force_err(orc.forces_raw(st["R"], L, lDeb, nthreads=8), t), t.P, t.H)
    check_forces("C2 launch (scheme 2, fast kernel, scaled form)", st["F"], t, L, D, True, ft.GEOM, True, phi_ref)
