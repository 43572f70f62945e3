"""The Python restatements of the MC + MD program in oracle/oracle.py (mcmd_*), which take any N,
pinned to the reference program itself at its one size, N = 4096: the reference's source built
unmodified into oracle/_ref/libmdref.so (oracle.RefMCMD).  tests/test_gpu_mdmc_sizes.py then uses
the restatements where the reference build cannot go (N != 4096).  CPU only.

Tolerances:
  * potentials and the Metropolis chain: positions and the accepted count bit for bit, U within
    1e-12 max|U| (the project's, tests/test_mdmc.py); the chain's smallest decision margin must be
    >= 1e-9, four orders above the rounding of an energy difference, so equality is not luck;
  * MD steps: 16 x the difference measured here between the long-double restatement and the
    reference's sequential float64 sums (see test_md_steps_match_reference);
  * g(r): every bin equal after %lg; temperatures and moments: equal after %lg / the file's digits;
  * direct autocorrelations against the FFT restatement: 1e-9 of the largest term (test_mdmc.py).
"""
import math
import os
import tempfile

import numpy as np
import pytest

N = 4096
KAPPA, GAMMA, MAXRSTEP, DT = 0.5, 3.0, 0.3, 0.005


@pytest.fixture(scope="module")
def refmc(orc):
    if not orc.ref_available():
        pytest.fail("oracle/_ref/libmdref.so not built (oracle/ref/Makefile)")
    return orc


@pytest.fixture(scope="module")
def consts(refmc):
    L, rCut, nbins = refmc.mcmd_constants(N)
    assert L == refmc.ref().mdref_L() and rCut == refmc.ref().mdref_rcut()
    return L, rCut, nbins


def _cols(path):
    return np.loadtxt(path, ndmin=2)


def test_potentials_match_reference(refmc, consts):
    L, rCut, _ = consts
    with tempfile.TemporaryDirectory() as tmp:
        ref = refmc.RefMCMD(seed=12, save_directory=tmp + "/")
        ref.init()
        R, _, _, U0 = ref.get_state()
    U = refmc.mcmd_potentials(R, L, KAPPA, rCut)
    assert np.abs(U - U0).max() <= 1e-12 * np.abs(U0).max()


def test_metropolis_matches_reference(refmc, consts):
    """1500 steps from the lattice, then 500 more: the same stream (mt19937(seed) less the one
    uniform of MCMD:55), the same decisions"""
    L, rCut, _ = consts
    with tempfile.TemporaryDirectory() as tmp:
        ref = refmc.RefMCMD(seed=77, save_directory=tmp + "/")
        ref.init()
        R, V, A, U = ref.get_state()
        ref.L.mdref_seed(77)
        ref.set_state(R, V, A, U)
        mt = refmc.MT19937(77)
        mt.uniform()
        R = R.copy(); U = U.copy()
        total = 0
        for n in (1500, 500):
            ref.monte_carlo(n)
            acc, margin = refmc.mcmd_monte_carlo(R, U, mt, n, L, KAPPA, rCut, MAXRSTEP, GAMMA)
            R1, _, _, U1 = ref.get_state()
            total += acc
            assert margin >= 1e-9, margin
            assert np.array_equal(R, R1)
            assert np.abs(U - U1).max() <= 1e-12 * np.abs(U1).max()
        assert 0 < total <= 2000


def test_md_steps_match_reference(refmc, consts):
    """3 plain steps and 3 with the laser term, collisions off, after a short anneal.  Measured
    here (restatement in long double vs the reference's sequential float64 sums, N = 4096):
    max|dA| = 9.68e-15, max|dV| = 4.44e-16, max|dR| = 3.55e-15 (one ulp of a position) over the
    six steps; asserted at 16 x that (summation orders differ), far below the project's 1e-10
    (tests/test_mdmc.py)."""
    L, rCut, _ = consts
    with tempfile.TemporaryDirectory() as tmp:
        ref = refmc.RefMCMD(seed=13, save_directory=tmp + "/")
        ref.init()
        ref.monte_carlo(300)
        ref.set_collision_freq(0.0)
        R, V, A, _ = ref.get_state()
        worst = np.zeros(3)
        for laser in (False, True):
            ref.set_laser_force(laser)
            for _ in range(3):
                ref.md_steps(1)
                R, V, A, _ = refmc.mcmd_md_step(R, V, A, L, KAPPA, rCut, DT, laser=laser, oneAxis=False)
                R1, V1, A1, _ = ref.get_state()
                worst = np.maximum(worst, [np.abs(A - A1).max(), np.abs(V - V1).max(), np.abs(R - R1).max()])
        ref.set_laser_force(False)
    print("md restatement vs reference: max|dA| %.3e max|dV| %.3e max|dR| %.3e" % tuple(worst))
    assert worst[0] <= 16 * 9.68e-15 and worst[1] <= 16 * 4.44e-16 and worst[2] <= 16 * 3.55e-15


def test_pair_corr_temperatures_and_moments_match_reference(refmc, consts):
    L, rCut, nbins = consts
    with tempfile.TemporaryDirectory() as tmp:
        ref = refmc.RefMCMD(seed=14, save_directory=tmp + "/")
        ref.init()
        ref.monte_carlo(400)
        R, V, _, _ = ref.get_state()
        ref.pair_corr_file(7)
        gref = _cols(os.path.join(tmp, "pairPairCorrStepNum7.dat"))
        g = refmc.mcmd_pair_corr(R, L, 0.05)
        assert g.size == gref.shape[0] == nbins
        assert np.array_equal(np.array([float("%lg" % x) for x in g]), gref[:, 1])
        ref.record_temperature(); ref.record_temp_axes(3)
        t = refmc.mcmd_temperatures(V)
        assert float("%lg" % t[0]) == _cols(os.path.join(tmp, "temperature.dat"))[0, 0]
        ax = _cols(os.path.join(tmp, "tempAxes.dat"))[0]
        assert np.array_equal([float("%lg" % x) for x in t[1:]], ax[1:])
        tags = ref.tag_particles()
        ref.tagged_moments_file(5)
        m, mag, cnt = refmc.mcmd_tagged_moments(V, tags, GAMMA)
        assert np.array_equal(cnt, tags.sum(axis=1)) and cnt.min() > 0
        for k, name in enumerate(["One", "Two", "Three", "Four"]):
            row = _cols(os.path.join(tmp, f"taggedV{name}Moments.dat"))[0]
            np.testing.assert_allclose(m[k], row[1:], rtol=2e-5, atol=1e-6)   # the %lg file's digits
        # tagParticles on a known stream: reseeded (which zeroes the state), the velocities put back
        ref.L.mdref_seed(31)
        ref.set_state(V=V)
        mt = refmc.MT19937(31)
        mt.uniform()
        assert np.array_equal(ref.tag_particles(), refmc.mcmd_tag_particles(V, mt, GAMMA))


def test_direct_autocorrelations_match_fft_restatement(orc):
    """a small store: the direct long-double lag sums against the FFT restatement that the
    committed reference golden pins (test_autocorrelation_restatement_matches_reference_golden)"""
    rng = np.random.default_rng(3)
    vs = rng.standard_normal((3, 40, 64)) * math.sqrt(1 / GAMMA)
    out, mag = orc.mcmd_autocorrelations_direct(vs, GAMMA)
    fft = orc.mcmd_autocorrelations(vs, GAMMA)
    assert mag.shape == out.shape == (4, 64) and np.all(mag > 0)
    for f in range(4):
        scale = np.abs(fft[f]).max() + (3 / 9.0 if f == 1 else 27 / 81.0 if f == 3 else 0)
        assert np.abs(out[f] - fft[f]).max() <= 1e-9 * scale, f
