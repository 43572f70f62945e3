"""The lane QT kernels' substep body chooses wave-uniformly between the no-jump block and one
straight-line block for a substep in which an ion of the wave jumps (mdqt_qtfast.hip, lane_substeps).
The thread-per-ion kernel (k_substeps_r) performs the same operations in the same order and is the
bit-level yardstick: every instance of the lane body must equal it bit for bit under heavy jumping,
and the oracle (stepped qstep by qstep on the same Philox stream) says which ions jump and when, so
that no comparison here passes without the jump variant having run.

Ions 4w .. 4w+3 share a wave of the lane kernels (16 lanes per ion)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QTK_LANES_IM_EDZ = 1         # mdqt_internal.hpp QTKernel: the production instance (FAST + IM01 + EDZ, no renorm)
QTK_LANES_R = 4              # k_substeps_lanes_r<true, false>: the general model-0 instance
QTK_LANES_R_PUMP_FAST = 5    # k_substeps_lanes_r<false, true>: the pump models' fused launch (LDS gather)
RATIO = 25                   # substeps per MD step (the reference's default)
SEED = 22                    # chosen against the oracle (the conditions asserted below; 21 gives no same-wave
                             # pair), never against the kernels
HEAVY = dict(N0=300, seed=SEED, rng_mode=1, Om=3.0, OmDP=2.0)
Q0 = 1000


@pytest.fixture(scope="module")
def eng():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


def heavy_state(orc, pure_s=()):
    """an evolved N0 = 300 configuration with a random normalised psi, ~95 % of it in the P states (a
    jump per ion and substep with probability dp ~ 0.7 %), every tPart >= 1 (a small final tPart proves a
    jump inside the run) and t > 0; the ions in `pure_s` start in a pure S superposition (dp = 0)"""
    o = orc.OracleSim(N0=300, seed=SEED, rng_mode=1, nthreads=4).init()
    o.md_steps(1)
    st = o.get_state()
    n = st["psi"].shape[0]
    rng = np.random.default_rng(1)
    z = rng.normal(size=(n, 12)) + 1j * rng.normal(size=(n, 12))
    z[:, 2:6] *= 5.
    for i in pure_s:
        z[i, 2:] = 0.
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    psi = np.zeros_like(st["psi"])
    psi[:, :, 0], psi[:, :, 1] = z.real, z.imag
    return dict(R=st["R"], V=st["V"], psi=psi, tPart=st["tPart"] + 1.0, t=0.3)


def load(x, st, q0=Q0):
    x.set_state(st["R"], st["V"], st["psi"], st["tPart"], st["t"])
    x.qstep_index = q0
    return x


def oracle_jumps(o, nmd):
    """nmd MD steps of the oracle, substep by substep: J[m, s, i] = ion i jumped in substep s of MD
    step m (a jump zeroes tPart; without one it grows from a positive value), and the state
    populations [m, s, i, state] before and after every qstep"""
    n = o.N
    J = np.zeros((nmd, RATIO, n), bool)
    pop = np.zeros((2, nmd, RATIO, n, 12))
    for m in range(nmd):
        o.forces()
        for s in range(RATIO):
            o.step()
            pop[0, m, s] = (o.get_state()["psi"] ** 2).sum(-1)
            o.qstep()
            st = o.get_state()
            pop[1, m, s] = (st["psi"] ** 2).sum(-1)
            J[m, s] = st["tPart"] == 0.
    return J, pop


def same_wave_pair(J):
    """a substep in which two ions of one wave jump together"""
    n = J.shape[-1]
    pad = (-n) % 4
    w = np.concatenate([J, np.zeros(J.shape[:-1] + (pad,), bool)], -1).reshape(J.shape[:-1] + (-1, 4))
    return bool((w.sum(-1) >= 2).any())


def run_kernels(eng, st, kw, run, opts=()):
    """the same run with the thread-per-ion (1) and the lane (2) substep kernels -> states, lane qt_kernel"""
    out, inst = [], None
    for mode in (1, 2):
        s = load(eng.Simulation(**kw), st)
        s.set_option("qt_math", 2)
        s.set_option("substep_kernel", mode)
        for k, v in opts:
            s.set_option(k, v)
        run(s)
        out.append(s.get_state())
        inst = int(s.const("qt_kernel"))
        s.close()
    return out[0], out[1], inst


def assert_bit_identical(a, b):
    for k in ("R", "V", "psi", "tPart"):
        assert np.array_equal(a[k], b[k]), k


def test_heavy_jumps_production_instance(eng, orc):
    """md_steps(2) on the production instance: lane == thread bit for bit, the jumped set is the
    oracle's; the oracle shows >= N/4 jumping ions, two ions of one wave jumping in the same substep,
    and a jump in the first and in the last substep of a launch"""
    st = heavy_state(orc)
    o = load(orc.OracleSim(nthreads=4, **HEAVY), st)
    J, _ = oracle_jumps(o, 2)
    b = o.get_state()
    n = J.shape[-1]
    jumped = J.any(axis=(0, 1))
    print(f"oracle: N={n} jumping ions={int(jumped.sum())} jumps={int(J.sum())} "
          f"first-substep={int(J[:, 0].sum())} last-substep={int(J[:, -1].sum())} same-wave pair={same_wave_pair(J)}")
    assert jumped.sum() >= n / 4
    assert same_wave_pair(J)
    assert J[:, 0].any() and J[:, -1].any()
    thr, lane, inst = run_kernels(eng, st, HEAVY, lambda s: s.md_steps(2))
    assert inst == QTK_LANES_IM_EDZ, inst
    assert_bit_identical(thr, lane)
    assert np.array_equal(b["tPart"] < 1.0, jumped)            # (tPart started >= 1)
    assert np.array_equal(lane["tPart"] < 1.0, jumped)
    dpsi, dV = np.abs(lane["psi"] - b["psi"]).max(), np.abs(lane["V"] - b["V"]).max()
    print(f"lane vs oracle: |dpsi|={dpsi:.2e} |dV|={dV:.2e}")
    assert dpsi < 1e-10
    assert dV < 1e-12


@pytest.mark.parametrize("renorm", [0, 1])
def test_heavy_jumps_stepwise_general_instance(eng, orc, renorm):
    """forces() then 25 x (step(); qstep()): the general (non-FAST) instance, one substep per launch"""
    kw = dict(HEAVY, reNormalizewvFns=renorm)
    st = heavy_state(orc)
    o = load(orc.OracleSim(nthreads=4, **kw), st)
    J, _ = oracle_jumps(o, 1)
    jumped = J.any(axis=(0, 1))
    assert jumped.sum() >= 10 and same_wave_pair(J)

    def run(s):
        s.forces()
        for _ in range(RATIO):
            s.step()
            s.qstep()
    thr, lane, inst = run_kernels(eng, st, kw, run)
    assert inst == QTK_LANES_R, inst
    assert_bit_identical(thr, lane)
    assert np.array_equal(lane["tPart"] < 1.0, jumped)


def test_heavy_jumps_pump_model(eng, orc):
    """qt_model 1 (lane = state, coupling slots gathered through LDS, jump_target_pump), 2 MD steps"""
    kw = dict(N0=300, seed=SEED, rng_mode=1, qt_model=1, Om=0.7, detuning=-2.5)
    o = orc.OracleSim(nthreads=4, **kw).init()
    st = o.get_state()
    n = st["psi"].shape[0]
    rng = np.random.default_rng(1)
    z = np.zeros((n, 12), complex)
    z[:, :7] = rng.normal(size=(n, 7)) + 1j * rng.normal(size=(n, 7))
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    st = dict(R=st["R"], V=st["V"], psi=np.stack([z.real, z.imag], -1), tPart=st["tPart"] + 1.0, t=0.3)
    load(o, st)
    J, pop = oracle_jumps(o, 2)
    # a spin-changing jump: the ion lands on the S state (0 / 1) that held the smaller part of its S
    # population before the substep
    landed = pop[1].argmax(-1)
    other = np.take_along_axis(pop[0], (1 - np.minimum(landed, 1))[..., None], -1)[..., 0]
    mine = np.take_along_axis(pop[0], landed[..., None], -1)[..., 0]
    flips = (J & (landed <= 1) & (mine < other)).sum()
    print(f"oracle: jumps={int(J.sum())} spin-changing={int(flips)}")
    assert J.sum() >= 20 and flips >= 1
    thr, lane, inst = run_kernels(eng, st, kw, lambda s: s.md_steps(2))
    assert inst == QTK_LANES_R_PUMP_FAST, inst
    assert_bit_identical(thr, lane)
    assert np.array_equal(lane["tPart"] < 1.0, J.any(axis=(0, 1)))


def test_wave_without_jump_next_to_jumping_waves(eng, orc):
    """ions 0-7 (waves 0 and 1) start in pure S (dp = 0): the oracle shows them not jumping while
    other waves do, so they run the wave-uniform no-jump variant throughout"""
    quiet = range(8)
    st = heavy_state(orc, pure_s=quiet)
    o = load(orc.OracleSim(nthreads=4, **HEAVY), st)
    J, _ = oracle_jumps(o, 2)
    assert not J[:, :, :8].any()
    assert J[:, :, 8:].any(axis=2).sum() >= 25         # jumps elsewhere in at least half of the substeps
    thr, lane, inst = run_kernels(eng, st, HEAVY, lambda s: s.md_steps(2))
    assert inst == QTK_LANES_IM_EDZ, inst
    assert_bit_identical(thr, lane)
    for k in ("psi", "tPart"):
        assert np.array_equal(thr[k][:8], lane[k][:8]), k
    assert np.all(lane["tPart"][:8] >= 1.0)
