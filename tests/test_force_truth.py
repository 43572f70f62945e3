"""tests/force_truth.py itself: the exact row sums against 50-digit arithmetic and against the reference's
own compiled force, the oracle (the reference's operations in double) inside the per-ion bound, and the
conditions the designed inputs must meet.  The GPU tests (test_gpu_force_accuracy.py) hold the kernels
to the same bound on the same states."""
import os

import numpy as np
import pytest

from tests import force_truth as ft

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_md_n4096.npz")
LD = np.longdouble


@pytest.fixture(scope="module")
def box(orc):
    o = orc.OracleSim(N0=1000)
    L, lDeb = o.const("L"), o.const("lDeb")
    o.close()
    return L, lDeb


def states(L):
    out = [(f"random N={N}", ft.random_state(N, L)) for N in (63, 64, 65, 129, 1000)]
    out += [(f"designed N={N}", ft.designed_state(N, L)) for N in (129, 1000)]
    out.append(("out of range N=129", ft.out_of_range_state(129, L)))
    return out


def mp_rows(R, L, lDeb):
    """T_i and U_i at 50 digits over the pair set and images of force_truth.pair_set"""
    import mpmath as mp
    mp.mp.dps = 50
    N = R.shape[1]
    n, keep = ft.pair_set(R, L, np.arange(N))
    Lm, lam = mp.mpf(L), mp.mpf(lDeb)
    T = [[mp.mpf(0)] * N for _ in range(3)]
    U = [mp.mpf(0)] * N
    for i in range(N):
        for j in range(N):
            if not keep[i, j]:
                continue
            d = [mp.mpf(R[k, i]) - mp.mpf(R[k, j]) - Lm * int(n[k, i, j]) for k in range(3)]
            r = mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
            e = mp.exp(-r / lam)
            g = (1 / r ** 2 + 1 / (r * lam)) * e
            for k in range(3):
                T[k][i] += g * d[k] / r
            U[i] += e / r
    return T, U


@pytest.mark.parametrize("state", ["random", "designed"])
def test_truth_matches_mpmath(box, state):
    """N = 12 against mpmath at 50 digits: U_i within 2^-60 of itself, every component of T_i within
    2^-60 of the row's P_i = sum g.  P_i is the scale of the bound the truth serves (gate_i is in units
    of 2^-53 P_i) and the only one on which a sum of signed terms has a relative accuracy: each long
    double term carries about a dozen roundings of 2^-64, and a component whose terms cancel to
    |T_ki| = P_i / 36 (ion 2 of the random state) is off by 55 x 2^-64 = 2^-58.2 of its own value while
    it is within 1.5 x 2^-64 of P_i.  The figure relative to the component's own value is printed.
    (The designed state needs 28 ions for its 14 designed ones: its first 12 are the faces, the three
    cutoff pairs and the two close pairs.)"""
    import mpmath as mp
    L, lDeb = box
    R = ft.random_state(12, L) if state == "random" else np.ascontiguousarray(ft.designed_state(28, L)[:, :12])
    t = ft.row_sums(R, L, lDeb)
    T, U = mp_rows(R, L, lDeb)
    def to_mp(a):                           # long double -> mpmath exactly: the high and low double halves
        hi = float(a)
        return mp.mpf(hi) + mp.mpf(float(a - LD(hi)))

    worst_t = worst_u = worst_own = 0.0
    for i in range(12):
        if t.P[i] == 0:
            assert not t.T[:, i].any() and t.U[i] == 0 and U[i] == 0
            continue
        worst_u = max(worst_u, float(abs(to_mp(t.U[i]) - U[i]) / U[i]))
        for k in range(3):
            d = abs(to_mp(t.T[k, i]) - T[k][i])
            worst_t = max(worst_t, float(d / to_mp(t.P[i])))
            if T[k][i] != 0:
                worst_own = max(worst_own, float(d / abs(T[k][i])))
    print(f"{state}: max |dU_i|/U_i = {worst_u:.2e}, max |dT_ki|/P_i = {worst_t:.2e}, max |dT_ki|/|T_ki| = "
          f"{worst_own:.2e} (2^-60 = {2.0 ** -60:.2e})")
    assert worst_u <= 2.0 ** -60 and worst_t <= 2.0 ** -60


@pytest.mark.parametrize("case", [0, 1])
def test_truth_matches_reference_golden(case):
    """the reference's own compiled force and potential (N = 4096, 512 sampled rows): inside the bound
    with D = N + 8 and no shell allowance — this pins the truth's pair set and constants to the reference"""
    g = np.load(GOLD)
    L, lDeb = float(g["L"]), 1.0 / float(g["kappa"])
    R = g[f"R{case}"]
    N = R.shape[1]
    idx = np.sort(np.random.default_rng(case).choice(N, 512, replace=False))
    t = ft.row_sums(R, L, lDeb, idx)
    assert t.nshell == 0
    rf = ft.force_err(g[f"A{case}"], t) / ft.force_gate(t, L, N + 8, fast=False)
    ru = ft.potential_err(g[f"U{case}"], t) / ft.potential_gate(t, L, N + 8, fast=False)
    print(f"golden case {case}: max |dA_i|/gate_i = {float(rf.max()):.4f}, max |dU_i|/gate_i = {float(ru.max()):.4f}, "
          f"phi = {ft.phi(ft.force_err(g[f'A{case}'], t), t.P, t.H):.2f}")
    assert rf.max() <= 1 and ru.max() <= 1


def test_oracle_inside_the_bound(orc, box):
    """the reference's operations in double (the oracle) on every state of the GPU tests, D = N + 8, no
    shell allowance: the largest |dF_i| / gate_i must be <= 1.  The printed figures are what the GPU
    tests' instances are compared with."""
    L, lDeb = box
    for name, R in states(L):
        N = R.shape[1]
        t = ft.row_sums(R, L, lDeb)
        geom = ft.geom_roundings(R, L)
        ef = ft.force_err(orc.forces_raw(R, L, lDeb), t)
        eu = ft.potential_err(orc.potentials_index(R, np.arange(N), L, lDeb), t)
        rf = float((ef / ft.force_gate(t, L, N + 8, fast=False, geom=geom)).max())
        ru = float((eu / ft.potential_gate(t, L, N + 8, fast=False, geom=geom)).max())
        print(f"{name}: oracle max |dF_i|/gate_i = {rf:.4f} (phi_ref = {ft.phi(ef, t.P, t.H):.2f}, max |dF_i| = "
              f"{float(ef.max()):.2e}), max |dU_i|/gate_i = {ru:.4f} (phi_ref = {ft.phi(eu, t.U, t.Hu):.2f})")
        assert rf <= 1 and ru <= 1, name


def test_input_conditions(box):
    """random states have no pair on the cutoff shell; the designed state has exactly its three (6 ordered
    pairs, on ions 2-7), one of them outside the reference's pair set and two inside"""
    L, lDeb = box
    for name, R in states(L):
        t = ft.row_sums(R, L, lDeb)
        if name.startswith("designed"):
            assert t.nshell == 6, name
            on = np.nonzero(t.H)[0]
            assert len(on) <= 6 and set(on) == set(ft.SHELL_IONS)
            _, keep = ft.pair_set(R, L, np.arange(R.shape[1]))
            # exactly L/2: whichever image, r = L/2 is not < L/2.  One ulp inside: dx/L = 1/2 - 2^-53/m for
            # L = m 2^e lies strictly between the doubles 1/2 - 2^-53 and 1/2 - 2^-54, so fl(dx/L) < 1/2 for
            # every L: no image, inside.  One ulp outside: round gives 1, the image is dx - L, an ulp inside.
            assert not keep[2, 3] and not keep[3, 2]
            assert keep[4, 5] and keep[5, 4]
            assert keep[6, 7] and keep[7, 6]
            n, _ = ft.pair_set(R, L, np.array([5, 7]))
            assert n[0, 0, 4] == 0 and n[0, 1, 6] == 1
            assert ft.geom_roundings(R, L) == ft.GEOM
            d = R[:, :, None] - R[:, None, :]
            r = np.sqrt((d ** 2).sum(axis=0)) + np.eye(R.shape[1])
            assert 0.99e-6 < r.min() < 1.01e-6         # |dd| / r stays near 1e-8
        else:
            assert t.nshell == 0 and not t.H.any() and not t.Hu.any(), name
        if name.startswith("out of range"):
            assert ft.geom_roundings(R, L) > ft.GEOM
            assert (np.abs(R) > 2 * L).sum() >= 6 and ((R < -L / 8) | (R > 9 * L / 8)).any(axis=0).sum() >= 12


# ---------------------------------------------------------------------------------------------
# the Newton-3 blocks' gate terms (tests/test_gpu_block_accuracy.py)
# ---------------------------------------------------------------------------------------------

BLOCK_SIZES = (129, 512, 513, 1100, 2500, 5000)


def test_block_depth_within_one_chain():
    """depth_blocks: the layout n3b_set_range gives at the block tests' sizes, and never more than the one
    chain over every term, N + 8"""
    want = {129: (3, 1, 1, 1, 1), 512: (8, 1, 1, 1, 1), 513: (9, 2, 2, 2, 1), 1100: (18, 3, 2, 2, 1),
            2500: (40, 5, 3, 3, 1), 5000: (79, 10, 6, 6, 1)}
    for N in BLOCK_SIZES:
        assert ft.block_layout(N) == want[N], N
        T, NB, nd, R, runlen = want[N]
        D = ft.depth_blocks(N)
        assert D <= N + 8
        assert D == min(132 + nd + R + 8, N + 8)
        print(f"N = {N}: T {T}, NB {NB}, nd {nd}, R {R}: D = {D} (N + 8 = {N + 8})")
    assert ft.depth_blocks(129) == 137 and ft.depth_blocks(5000) == 152
    for N in range(1, 5001, 7):
        assert ft.depth_blocks(N) <= N + 8


def test_form_err_pinned_to_the_engine():
    """err_e(r) = kFormErrA[e] r/lDeb + kFormErrB[e] as force_truth states it against mdqt_force_plan.cpp's
    far_err: the a-priori radius model returns bound = (N - 1) g(radius) err(radius) (for the f32 level
    without its constant cutoff term: apriori 2)"""
    from mdqtplasmasims_amd.engine import tier_radius_model
    N, L, lDeb = 5000, (5000 * 4 * np.pi / 3) ** 0.333333333, 1 / 3.0
    for e in (1, 2, 3, 4, 5):
        for k in (13, 9):
            r, bound = tier_radius_model(N, L, lDeb, k, ft.MODEL_LEVEL[e], apriori=2 if e == 5 else 1)
            assert 0 < r < L / 2, (e, k)
            g = (1 / r + 1 / lDeb) * np.exp(-r / lDeb) / r
            err = bound / ((N - 1) * g)
            print(f"level {e} ({ft.TIERS[e]}), 1e-{k}: radius {r:.4f}, err {err:.6e}, force_truth {ft.form_err(e, r, lDeb):.6e}")
            assert abs(err - ft.form_err(e, r, lDeb)) <= 1e-12 * err


def test_form_err_grows_with_the_level():
    """Form_i charges a pair the error of the highest level its distance allows; the kernel may take a lower
    one: the stated errors must grow with the level at every distance"""
    x = np.concatenate([[0.0], np.logspace(-6, 4, 400)])          # r / lDeb
    for e in (1, 2, 3, 4):
        assert (ft.form_err(e + 1, x, 1.0) > ft.form_err(e, x, 1.0)).all(), e


def test_block_terms_match_a_plain_loop(box):
    """Form_i, FormU_i, Tail_i, TailU_i and the f32 cutoff shell on 40 ions, against a double loop over the
    reference's pair set (SpeedUp:213-222), radii that put pairs in every level"""
    import math
    L, lDeb = box
    R = ft.designed_state(40, L)
    half = L / 2
    R[:, 21] = R[:, 20]                                # a pair on the f32 tier's cutoff shell, outside L/2
    R[0, 20], R[0, 21] = 0.25 * L, 0.25 * L + half * (1 + 2.0 ** -23)
    radii = {1: 0.2 * half, 2: 0.4 * half, 3: 0.6 * half, 4: 0.7 * half, 5: 0.8 * half}
    skip = 0.9 * half
    for on, f32cut in (((1, 2, 3, 4, 5), True), ((1, 2, 3, 4, 5), False), ((2, 4), True), ((), False)):
        rad = {e: (radii[e] if e in on else half) for e in radii}
        b = ft.block_terms(R, L, lDeb, rad, skip, f32cut, chunk=16)
        form, formu, tail, tailu = (np.zeros(40) for _ in range(4))
        nform, ntail, ncut = {e: 0 for e in on}, 0, 0
        for i in range(40):
            for j in range(40):
                if i == j:
                    continue
                d = [R[k, i] - R[k, j] for k in range(3)]
                d = [x - L * float(ft.c_round(np.float64(x / L))) for x in d]
                r = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                g = (1 / (r * r) + 1 / (r * lDeb)) * math.exp(-r / lDeb)
                u = math.exp(-r / lDeb) / r
                if f32cut and 5 in on and abs(r - half) <= ft.F32CUT * 2.0 ** -24 * half:
                    form[i] += g
                    formu[i] += u
                    ncut += 1
                if not 0 < r < half:
                    continue
                lev = max([e for e in on if rad[e] <= r * (1 + 2.0 ** -50)], default=0)
                if lev:
                    nform[lev] += 1
                    form[i] += g * ft.form_err(lev, r, lDeb)
                    formu[i] += u * ft.form_err(lev, r, lDeb)
                if r * (1 + 2.0 ** -50) >= skip:
                    tail[i] += g
                    tailu[i] += u
                    ntail += 1
        assert b.nform == nform and b.ntail == ntail and b.ncut == ncut
        assert ncut == (2 + 6 if f32cut and 5 in on else 0)        # the new pair and the designed state's three
        assert ntail > 0 and all(v > 0 for v in nform.values())
        for got, ref in ((b.form, form), (b.formu, formu), (b.tail, tail), (b.tailu, tailu)):
            assert np.allclose(got, ref, rtol=1e-12, atol=0)
    # no tier, no tail: nothing
    b = ft.block_terms(R, L, lDeb, {}, half, True)
    assert not b.form.any() and not b.tail.any() and not b.formu.any() and not b.tailu.any()


def test_block_gate_sees_one_cutoff_pair(orc):
    """what test_gpu_block_accuracy.py's weak-screening cases rest on: in the box of 129 ions at Ge 0.1 one
    pair term at the cutoff, dropped from the designed state's exact row sums, stands 1e9 gates above the
    blocks' gate; the fast variant's shell allowance covers the pair one ulp inside L/2 and no other"""
    o = orc.OracleSim(N0=129, Ge=0.1)
    L, lDeb = o.const("L"), o.const("lDeb")
    o.close()
    R = ft.designed_state(129, L)
    t = ft.row_sums(R, L, lDeb)
    none = ft.block_terms(R, L, lDeb, {}, L / 2, False)
    D = ft.depth_blocks(129)
    r = R[0, 5] - R[0, 4]                               # one ulp inside L/2, along x: in the pair set
    assert r < L / 2 and ft.pair_set(R, L, np.array([4]))[1][0, 5]
    g = (1 / (r * r) + 1 / (r * lDeb)) * np.exp(-r / lDeb)
    F = t.T.astype(np.float64)
    assert (ft.force_err(F, t) <= ft.block_force_gate(t, none, L, D, False)).all()
    F[0, 4] += g                                        # ion 4 loses its partner at +x: its force moves by +g
    ratio = ft.force_err(F, t) / ft.block_force_gate(t, none, L, D, False)
    print(f"g(L/2) = {g:.3e}: |dF_4| / gate_4 = {float(ratio[4]):.3e} (the exact variant's gate)")
    assert ratio[4] > 1e9 and (np.delete(ratio, 4) <= 1).all()
    # the fast variant's gate allows exactly that pair (H_4 = g: mic_r may decide it either way), and no other:
    # ion 20's farthest partner inside the cutoff, off the shell
    assert ft.force_err(F, t)[4] <= ft.block_force_gate(t, none, L, D, True)[4]
    n, keep = ft.pair_set(R, L, np.array([20]))
    d = (R[:, 20, None] - R) - L * n[:, 0, :]
    rr = np.where(keep[0], np.sqrt((d * d).sum(axis=0)), 0.0)
    j = int(np.argmax(rr))
    assert t.H[20] == 0 and 0.9 * L / 2 < rr[j] < L / 2
    gj = (1 / (rr[j] ** 2) + 1 / (rr[j] * lDeb)) * np.exp(-rr[j] / lDeb)
    F = t.T.astype(np.float64)
    F[:, 20] -= gj * d[:, j] / rr[j]
    ratio = ft.force_err(F, t) / ft.block_force_gate(t, none, L, D, True)
    print(f"ion 20 without its partner at r = {rr[j]:.3f}: |dF_20| / gate_20 = {float(ratio[20]):.3e} (the fast variant's gate)")
    assert ratio[20] > 1e8 and (np.delete(ratio, 20) <= 1).all()
