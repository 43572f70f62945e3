"""The kernels behind every number the programs write — k_sum_vx, k_energy_sums, k_kde / k_kde_reduce and
k_output_pack (bodies: mdqt_obs_device.hpp) and the tagged distribution and moments (tagged_kde_chunk,
tagged_kde_reduce_1 in mdqt_pump_device.hpp; tag_moments_body) — held per element to a derived bound B against an
extended-precision truth (tests/obs_truth.py; derivation and the measured figures: docs/OBSERVABLES.md).  Where
tests/test_gpu_parity.py compares the bins norm-wise at one size, these ask |device - truth| <= B of every bin
of P[3][2001], every entry of out7, every ion's three populations and every bin of the tagged P[3][4001], at
the sizes where the kernels' shapes change (tests/obs_cases.py), with velocities at the skip radius' edges.
Sum U_i is held against the exact sum of the potential_rows() the same context returns.  No tolerance here
is a number of its own: each is B.  Every test prints its worst error / B per quantity (run with -s).

As measured on an MI355X (worst error / B per quantity, all cases): docs/OBSERVABLES.md."""
import os

import numpy as np
import pytest

from tests import force_truth as ft
from tests import obs_cases as oc
from tests import obs_truth as ot

pytestmark = pytest.mark.gpu
LD = ot.LD


@pytest.fixture(scope="module")
def eng():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    if not ot.has_extended():
        pytest.skip("np.longdouble has no 64-bit significand here: no extended-precision reference")
    return M


def load(eng, V, psi=None, t=0.0, **kw):
    N = V.shape[1]
    s = eng.Simulation(N0=N, **kw)
    if psi is None:
        psi = np.zeros((N, 12, 2))
        psi[:, 0, 0] = 1.0
    s.set_state(oc.positions(N, s.const("L")), V, psi, np.zeros(N), t)
    assert s.N == N
    return s


def check(label, got, val, B, report):
    got, val = ot.to_ld(got), ot.to_ld(val)
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), label
    w, i = ot.worst(np.abs(got - val), B)
    report.append(f"{label} {w:.4f}")
    assert w <= 1, (label, i, float(np.ravel(got)[i]), float(np.ravel(val)[i]), float(np.ravel(B)[i]), w)


@pytest.mark.parametrize("name", oc.NAMES)
def test_observables_inside_B(eng, name):
    """observables_w1 at every size where a shape changes, the drifting plasma and N = 132,000 (the second
    staging pass; the potential on the Newton-3 blocks): out7, every bin, every ion's populations"""
    V = oc.case_velocities(name)
    N = V.shape[1]
    psi = oc.random_psi(N, 0)
    s = load(eng, V, psi, t=0.75)
    Urow = s.potential_rows()
    o7, P, pops = s.observables()
    Epot0 = s.counters()["Epot0"]
    s.close()
    tr = oc.with_potential(name, Urow, t=0.75, Epot0=Epot0)
    rep = []
    assert o7[0] == 0.75
    for q, lab in ((1, "EkinX"), (2, "EkinY"), (3, "EkinZ"), (4, "Epot"), (5, "Etot-Epot0"), (6, "<vx>")):
        check(lab, o7[q], tr.out7[q], tr.B_out7[q], rep)
    for c, lab in enumerate(("Px", "Py", "Pz")):
        check(lab, P[c], tr.P[c], tr.B_P[c], rep)
    pv, pB = ot.populations(psi, 0)
    check("pops", pops, pv, pB, rep)
    print(f"{name} (N = {N}) error / B: " + ", ".join(rep))


@pytest.mark.parametrize("N", [3, 257])
@pytest.mark.parametrize("model", [0, 1, 3])
def test_populations_inside_B(eng, model, N):
    """k_output_pack for SpeedUp's grouping (models 0 - 2) and the 422 pumping program's (model 3: P = 2, 3;
    D = 4; states 5..11 non-zero in the input and ignored), unnormalised ions among them"""
    V = oc.case_velocities(f"N{N}")
    psi = oc.random_psi(N, model)
    s = load(eng, V, psi, **({"pump_program": model} if model else {}))
    assert int(s.params.qt_model) == model
    _, _, pops = s.observables(kde=False)
    s.close()
    val, B = ot.populations(psi, model)
    rep = []
    check(f"model {model} N {N} pops", pops, val, B, rep)
    if model == 3:
        other, _ = ot.populations(psi, 0)
        assert ot.worst(np.abs(other - val), B)[0] > 2          # (the two groupings differ on these inputs)
    print(rep[0])


@pytest.mark.parametrize("N", [3, 257])
def test_vx_column_is_the_input(eng, tmp_path, N):
    """output()'s vx column (k_output_pack's first array) is the input bit for bit: through the one interface that
    shows it, statePopulationsVsVTime's first column, whose text is that of the input doubles"""
    V = oc.case_velocities(f"N{N}")
    psi = oc.random_psi(N, 0)
    s = load(eng, V, psi, saveDirectory=str(tmp_path) + "/")
    s.setup_directories()
    s.output()
    s.flush_files()
    rows = [ln.split("\t") for ln in open(os.path.join(s.save_directory, "statePopulationsVsVTime000000.dat"))]
    s.close()
    assert len(rows) == N and [r[0] for r in rows] == ["%g" % v for v in V[0]]


def test_nan_velocity_poisons_its_axis_only(eng):
    """one ion with vy = NaN: all 2001 y bins are NaN, as the reference's sum makes them; x and z stay inside B"""
    V = oc.case_velocities("N257").copy()
    V[1, 100] = np.nan
    s = load(eng, V)
    _, P, _ = s.observables(pops=False)
    s.close()
    tr = ot.observables(V)
    assert tr.nan_axis == [False, True, False]
    assert np.isnan(P[1]).all()
    rep = []
    check("Px", P[0], tr.P[0], tr.B_P[0], rep)
    check("Pz", P[2], tr.P[2], tr.B_P[2], rep)
    print("vy = NaN, error / B: " + ", ".join(rep))


def test_infinite_velocity_adds_exact_zeros(eng):
    """one ion with vz = +inf (the last of 258: the 257 before it keep their chunks of 33) leaves every z bin
    bit-identical to the run without that ion"""
    V257 = oc.case_velocities("N257")
    V = np.concatenate([V257, np.array([[0.1], [0.2], [np.inf]])], axis=1)
    assert -(-258 // (258 // 32)) == -(-257 // (257 // 32)) == 33
    out = []
    for v in (V, V257):
        s = load(eng, v)
        out.append(s.observables(pops=False)[1])
        s.close()
    assert np.isfinite(out[0][2]).all() and np.array_equal(out[0][2], out[1][2])
    tr = oc.kinetic_truth("N257")
    check("Pz", out[0][2], tr.P[2], tr.B_P[2], [])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("N", [70, 257])
def test_sharded_partial_observables_inside_B(eng, N, world):
    """mdqt_partial_observables on an in-process rank group (slabs of unequal length, <vx> passed in, partial P):
    the ranks' sums and bins added on the host in long double, inside the sum of the ranks' bounds — each rank's
    with its own term counts.  Sum U_i: against the exact rows, each inside the force gate's potential bound."""
    from mdqtplasmasims_amd.engine import comm_init_local
    V = oc.velocities(N, 60 + N)
    avg_in = float(ot.vx_average(V[0])[0])
    psi = np.zeros((N, 12, 2))
    psi[:, 0, 0] = 1.0
    sims = [eng.Simulation(N0=N, world_size=world, rank=r) for r in range(world)]
    L, lDeb = sims[0].const("L"), sims[0].const("lDeb")
    R = oc.positions(N, L)
    for s in sims:
        s.set_option("force_scheme", 1)
        s.set_option("force_kernel", 1)
        s.set_state(R, V, psi, np.zeros(N), 0.0)
    comm_init_local(sims)
    for s in sims:
        s.allgather_positions()
    rows = ft.row_sums(R, L, lDeb)
    tot = np.zeros(5, dtype=LD); Btot = np.zeros(5, dtype=LD)
    P = np.zeros((3, ot.NBINS), dtype=LD); BP = np.zeros((3, ot.NBINS), dtype=LD)
    val = np.zeros(5, dtype=LD); valP = np.zeros((3, ot.NBINS), dtype=LD)
    lens = []
    for s in sims:
        lo, hi = s.slab_bounds()
        lens.append(hi - lo)
        o5, Pr = s.partial_observables(avg_in)
        nseg = max(int(s.const("force_segments")), 1)
        gate = ft.potential_gate(rows, L, ft.depth_rows(N, nseg), True, ft.geom_roundings(R, L))
        tr = ot.partial(V[:, lo:hi], avg_in, rows.U[lo:hi])
        tot += ot.to_ld(o5); P += ot.to_ld(Pr)
        val += np.concatenate([[tr.sumvx], tr.sums]); valP += tr.raw
        Btot += np.concatenate([[tr.B_sumvx], tr.B_sums]); BP += tr.B_raw
        Btot[4] += gate[lo:hi].sum()
    for s in sims:
        s.close()
    assert sum(lens) == N and len(set(lens)) > 1                 # unequal slabs
    rep = []
    for q, lab in enumerate(("sum vx", "sum_x", "sum_y", "sum_z", "sum_U")):
        check(lab, tot[q], val[q], Btot[q] + ot.ULD * world * abs(val[q]), rep)
    for c, lab in enumerate(("Px", "Py", "Pz")):
        check(lab, P[c], valP[c], BP[c] + ot.ULD * world * valP[c], rep)
    print(f"sharded N = {N} world {world} (slabs {lens}) error / B: " + ", ".join(rep))


# ---------------------------------------------------------------------------------------------
# the tagged distribution and moments
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def taggers(eng):
    from mdqtplasmasims_amd import mdmc
    made = {}

    def get(N, model):
        if (N, model) not in made:
            e = mdmc.MonteCarloMD(qt_model=model, N=N)      # (no init(): it asks for a lattice's N)
            e.set_state(V=oc.tagged_velocities(N))
            made[(N, model)] = e
        return made[(N, model)]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("pattern", oc.TAG_PATTERNS)
@pytest.mark.parametrize("N,model", [(255, 1), (256, 1), (257, 1), (513, 1), (257, 3)])
def test_tagged_distribution_and_moments_inside_B(taggers, N, model, pattern):
    """recordTaggedParticleMoments over the ragged last chunk of 256: tags set through psi, every bin of
    P[3][4001] inside B and the four moments inside their sum bounds; no ion tagged: the bins are exactly 0 and
    the moments the reference's 0 / 0"""
    e = taggers(N, model)
    want = oc.tag_pattern(N, pattern)
    e.set_psi(oc.tag_psi(want))
    tags, cnt = e.tag_qt()
    assert np.array_equal(tags, want) and cnt == want.sum()
    mom, P = e.tagged_moments_qt()
    tr = oc.tagged_truth(N, pattern)
    if pattern == "none":
        assert tr.nt == 0 and not P.any() and not np.signbit(P).any()
        assert np.isnan(mom).all()                               # firstMom /= numTagged with numTagged = 0
        return
    rep = []
    for c, lab in enumerate(("Px", "Py", "Pz")):
        check(lab, P[c], tr.P[c], tr.B_P[c], rep)
    check("moments", mom, tr.mom, tr.B_mom, rep)
    print(f"tagged N = {N} model {model} {pattern} ({tr.nt} tagged) error / B: " + ", ".join(rep))
