"""GPU tests of the three-level laser-cooling engine (include/mdlc.h, mdlc_kernels.hip) against
the dense numpy checker tests/dense_three_state.py.  The checker's uniforms are the engine's own
Philox stream through the oracle's restatement: philox_uniform(seed, job, ion, qstep, draw), u1 =
draw 0, randDir = draw 1."""
import os
import subprocess

import numpy as np
import pytest

from tests import dense_three_state as D

pytestmark = pytest.mark.gpu

VKICK = 0.0012076


def draws(orc, seed, job, n, q):
    """(u1[n], randDir[n]) of qstep q"""
    u1 = np.array([orc.philox_uniform(seed, job, i, q, 0) for i in range(n)])
    rd = np.array([orc.philox_uniform(seed, job, i, q, 1) for i in range(n)])
    return u1, rd


def random_states(rng, n):
    a = rng.normal(size=(n, 3)) + 1j * rng.normal(size=(n, 3))
    return a / np.sqrt((np.abs(a) ** 2).sum(1))[:, None]


def bits(a):                                           # (complex: two words per element)
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


def make(**kw):
    from mdqtplasmasims_amd import LaserCooling
    kw.setdefault("device", 0)
    return LaserCooling(**kw)


def checker_run(orc, seed, job, N0, steps):
    """qstep_batch from init() for `steps` steps: per-step (psi, vx, tPart, jumped) and min |u1 - dp|"""
    from mdqtplasmasims_amd.mdlc import sample_velocities
    vx = sample_velocities(seed + job, N0, 0.01)[0].copy()
    psi = np.zeros((N0, 3), complex)
    psi[:, 0] = 1
    tp = np.zeros(N0)
    hist, margin = [], np.inf
    for q in range(steps):
        u1, rd = draws(orc, seed, job, N0, q)
        psi, vx, tp, j, dp = D.qstep_batch(psi, vx, tp, u1, rd)
        margin = min(margin, np.abs(u1 - dp).min())
        hist.append((psi, vx, tp, j))
    return hist, margin


# ---- 1. one step, no-jump branch ----
def test_one_step_no_jump(orc):
    """(a 1e-12 gate against the double checker; tests/test_gpu_qt_accuracy.py holds the same kernel per ion to
    a derived rounding bound against an extended-precision truth, over 17 and 32 steps)"""
    N0, seed, job = 70, 4242, 3                        # 70 ions: neither a whole wave nor a whole workgroup
    rng = np.random.default_rng(11)
    psi = random_states(rng, N0)
    V = np.zeros((1, 3, N0))
    V[0, 0] = rng.normal(0, 0.105, N0)
    tp = rng.uniform(0, 2, N0)
    with make(N0=N0, seed=seed, job=job) as s:
        s.set_state(V=V, psi=psi[None], tPart=tp[None], q=5)
        s.qsteps(1)
        g = s.get_state()
    assert g["q"] == 6
    u1, rd = draws(orc, seed, job, N0, 5)
    nojump = 0
    for i in range(N0):
        p, v, t, j = D.qstep_ion(psi[i], V[0, 0, i], tp[i], u1[i], rd[i])
        nojump += not j
        dpsi, dv = np.abs(g["psi"][0, i] - p).max(), abs(g["V"][0, 0, i] - v)
        assert dpsi <= 1e-12 and dv <= 1e-15, (i, j, dpsi, dv)
        assert g["tPart"][0, i] == t
    assert nojump >= 60
    assert same_bits(g["V"][0, 1:], V[0, 1:])          # V[1], V[2] are carried, never touched


# ---- 2. one step, jump branch ----
def test_one_step_jump_branch(orc):
    N0, job = 2000, 1
    psi = np.tile(np.array([0, 1 / np.sqrt(2), 1 / np.sqrt(2)], complex), (N0, 1))     # dp = 0.01
    rng = np.random.default_rng(5)
    V = np.zeros((1, 3, N0))
    V[0, 0] = rng.normal(0, 0.105, N0)
    tp = np.full(N0, 0.37)
    for seed in range(100, 140):                       # chosen on the CPU, from the checker alone
        u1, rd = draws(orc, seed, job, N0, 0)
        cp, cv, ct, cj, dp = D.qstep_batch(psi, V[0, 0], tp, u1, rd)
        if cj.sum() >= 10 and (rd[cj] < 0.5).any() and (rd[cj] >= 0.5).any():
            break
    else:
        pytest.fail("no seed with >= 10 jumps of both kick signs")
    print(f"seed {seed}: {cj.sum()} jumps, min |u1 - dp| = {np.abs(u1 - dp).min():.3e}")
    with make(N0=N0, seed=seed, job=job) as s:
        s.set_state(V=V, psi=psi[None], tPart=tp[None], q=0)
        s.qsteps(1)
        g = s.get_state()
    gj = g["tPart"][0] == 0
    assert (gj == cj).all()
    assert (g["psi"][0][cj] == np.array([1, 0, 0])).all()
    up = rd[cj] < 0.5
    assert same_bits(g["V"][0, 0][cj], np.where(up, V[0, 0][cj] + VKICK, V[0, 0][cj] - VKICK))
    assert np.abs(g["psi"][0][~cj] - cp[~cj]).max() <= 1e-12
    assert np.abs(g["V"][0, 0][~cj] - cv[~cj]).max() <= 1e-15


# ---- 3. trajectory from init() ----
def test_trajectory_matches_checker(orc):
    N0, job, steps = 70, 2, 300
    for seed in range(7000, 7040):                     # chosen on the CPU, from the checker alone
        hist, margin = checker_run(orc, seed, job, N0, steps)
        njumps = sum(int(h[3].sum()) for h in hist)
        if njumps >= 15 and margin > 1e-9:
            break
    else:
        pytest.fail("no seed with >= 15 jumps and a decision margin above 1e-9")
    norm = (np.abs(hist[-1][0]) ** 2).sum(1)
    print(f"seed {seed}: {njumps} jumps, min |u1 - dp| = {margin:.3e}, final norm in [{norm.min():.6f}, {norm.max():.6f}]")
    with make(N0=N0, seed=seed, job=job) as s:
        s.init()
        dpsi = dv = 0.
        for q in range(steps):
            s.qsteps(1)
            g = s.get_state()
            cp, cv, ct, cj = hist[q]
            assert ((g["tPart"][0] == 0) == cj).all(), q
            dpsi = max(dpsi, np.abs(g["psi"][0] - cp).max())
            dv = max(dv, np.abs(g["V"][0, 0] - cv).max())
        assert g["q"] == steps
    print(f"max |dpsi| = {dpsi:.3e}, max |dv| = {dv:.3e}")
    assert dpsi <= 1e-9 and dv <= 1e-10
    gn = (np.abs(g["psi"][0]) ** 2).sum(1)
    assert np.abs(gn - norm).max() <= 1e-9             # psi is not renormalised: the kernel follows the drift


# ---- 4. launch splitting ----
def test_launch_splitting_is_bit_identical():
    kw = dict(N0=70, seed=99, job=4)
    with make(**kw) as a, make(**kw) as b:
        a.init(); b.init()
        a.qsteps(50)
        b.qsteps(7); b.qsteps(43)
        ga, gb = a.get_state(), b.get_state()
    assert ga["q"] == gb["q"] == 50
    for k in ("V", "psi", "tPart"):
        assert same_bits(ga[k], gb[k]), k


# ---- 5. an ensemble equals its single jobs ----
@pytest.mark.parametrize("N0", [70, 300])              # 300: two workgroups per job, the second partly idle
def test_ensemble_equals_singles(N0):
    seed, job = 31, 5
    with make(N0=N0, seed=seed, job=job, njobs=3) as e:
        e.init()
        e.qsteps(50)
        ge, ee = e.get_state(), e.ekin_x()
    assert ge["V"].shape == (3, 3, N0)
    for k in range(3):
        with make(N0=N0, seed=seed, job=job + k) as s:
            s.init()
            s.qsteps(50)
            gs, es = s.get_state(), s.ekin_x()
        assert same_bits(ge["V"][k], gs["V"][0])
        assert same_bits(ge["psi"][k], gs["psi"][0])
        assert same_bits(ge["tPart"][k], gs["tPart"][0])
        assert same_bits(ee[k:k + 1], es)
    assert not same_bits(ge["V"][0], ge["V"][1])       # the jobs differ


# ---- 6. EkinX ----
@pytest.mark.parametrize("N0,njobs", [(70, 1), (1000, 2), (20000, 1)])
def test_ekin_x(N0, njobs):
    with make(N0=N0, seed=8, job=1, njobs=njobs) as s:
        s.init()
        s.qsteps(3)
        e1, e2 = s.ekin_x(), s.ekin_x()
        V = s.get_state()["V"]
    assert same_bits(e1, e2)
    ref = 0.5 * (V[:, 0] ** 2).mean(axis=1)
    assert np.abs(e1 / ref - 1).max() <= 1e-14


# ---- 7. applyForce = 0 ----
def test_apply_force_off():
    with make(N0=70, seed=8, job=1, applyForce=0) as s:
        s.init()
        g0 = s.get_state()
        s.qsteps(20)
        g1 = s.get_state()
    assert same_bits(g0["V"], g1["V"])
    assert np.abs(g1["psi"] - g0["psi"]).max() > 1e-4


# ---- 8. run(): main()'s loop, directories and energies.dat ----
def test_run_writes_the_reference_files(tmp_path, orc):
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    N0, seed, job = 70, 77, 6
    base = str(tmp_path / "a") + "/"
    outs, iterations = D.main_loop(0.35, 10, 0.01)
    assert iterations == 35
    kw = dict(N0=N0, seed=seed, job=job, njobs=2, tmax=0.35, sampleFreq=10, saveDirectory=base)
    with make(**kw) as s:
        assert s.const("iterations") == 35 and s.const("outputs") == 3
        s.run()
        assert s.get_state()["q"] == 35
        dirs = [s.save_directory(k) for k in range(2)]
        texts = []
        for k, d in enumerate(dirs):
            assert d == f"{base}Om50/Det-50NumIons70InitialTemp10000uK/job{job + k}/"
            lines = open(d + "energies.dat").read().splitlines()
            assert len(lines) == 3
            hist, _ = checker_run(orc, seed, job + k, N0, 29)
            for (c0, t), line in zip(outs, lines):
                ts, es = line.split("\t")
                assert ts == D.lg(t)
                ek = 0.5 * (hist[c0 - 1][1] ** 2).sum() / N0      # after c0 qsteps
                assert abs(float(es) / ek - 1) <= 2e-6, (k, c0, es, ek)
            texts.append(open(d + "energies.dat").read())
        s.run()                                                    # appends, as the reference's "a" mode
        for d, tx in zip(dirs, texts):
            assert open(d + "energies.dat").read() == tx + tx
    base2 = str(tmp_path / "b") + "/"
    r = subprocess.run([MDLC_CLI_PATH, str(job), f"--N0={N0}", f"--seed={seed}", "--njobs=2", "--tmax=0.35",
                        "--sampleFreq=10", f"--saveDirectory={base2}", "--device=0", "--quiet=1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for k, tx in enumerate(texts):
        d = f"{base2}Om50/Det-50NumIons70InitialTemp10000uK/job{job + k}/"
        assert open(d + "energies.dat").read() == tx
    assert os.listdir(d) == ["energies.dat"]
