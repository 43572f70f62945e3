"""GPU tests of the three-level laser-cooling program's parameter scan (mdlc_create_sweep, include/mdlc.h;
k_lc_steps_sweep, mdlc_sweep_kernels.hip): every member against the single-job context of its own parameters bit
for bit, the scan's kernel against the dense numpy checker tests/dense_three_state.py at a laser setting that is
not the default, and the files of run() and of the command line."""
import os
import subprocess

import numpy as np
import pytest

from tests import dense_three_state as D

pytestmark = pytest.mark.gpu

# (detuning, Om): the default, a point that differs in both, and the default's blue mirror
POINTS = [dict(detuning=-0.5, Om=0.5), dict(detuning=-1.25, Om=1.5), dict(detuning=0.5, Om=0.5)]


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


def make(params=None, **kw):
    from mdqtplasmasims_amd import LaserCooling
    if params is not None:
        params.device = 0
        return LaserCooling(params)
    kw.setdefault("device", 0)
    return LaserCooling(**kw)


# ---- 1. every member equals the single job of its parameters ----
# 1: one lane; 70: neither a whole wave nor a whole workgroup; 256: exactly one workgroup; 300: the second partly idle
@pytest.mark.parametrize("N0", [1, 70, 256, 300])
def test_members_equal_their_singles(N0):
    seed, job, R = 31, 5, 2
    with make(N0=N0, seed=seed, job=job, njobs=R, sweep=POINTS) as e:
        assert (e.npoints, e.njobs, e.members) == (3, 2, 6)
        assert (e.const("npoints"), e.const("njobs"), e.const("members")) == (3, 2, 6)
        e.init()
        g0 = e.get_state()
        e.qsteps(50)
        ge, ee = e.get_state(), e.ekin_x()
        member = [e.member_params(k) for k in range(6)]
    assert ge["V"].shape == (6, 3, N0) and ge["psi"].shape == (6, N0, 3) and ee.shape == (6,)
    for k, p in enumerate(member):
        q, r = divmod(k, R)
        assert (p.detuning, p.Om, p.job, p.njobs) == (POINTS[q]["detuning"], POINTS[q]["Om"], job + r, 1)
        with make(p) as s:
            assert (s.const("npoints"), s.const("njobs"), s.const("members")) == (1, 1, 1)
            s.init()
            s.qsteps(50)
            gs, es = s.get_state(), s.ekin_x()
        assert gs["q"] == ge["q"] == 50
        assert same_bits(ge["V"][k], gs["V"][0]), k
        assert same_bits(ge["psi"][k], gs["psi"][0]), k
        assert same_bits(ge["tPart"][k], gs["tPart"][0]), k
        assert same_bits(ee[k:k + 1], es), k
    for r in range(R):
        # common random numbers: replica r starts from the same velocities at every point ...
        assert same_bits(g0["V"][r], g0["V"][R + r]) and same_bits(g0["V"][r], g0["V"][2 * R + r])
        # ... and the points' lasers then drive it apart
        assert not same_bits(ge["psi"][r], ge["psi"][R + r])
        assert not same_bits(ge["psi"][r], ge["psi"][2 * R + r])
        assert not same_bits(ge["psi"][R + r], ge["psi"][2 * R + r])
    if N0 > 1:
        assert not same_bits(g0["V"][0], g0["V"][1])   # the replicas differ


# ---- 2. the temperature axis ----
def test_temperature_axis():
    from mdqtplasmasims_amd.mdlc import sample_velocities
    N0, seed, job, R = 70, 17, 3, 2
    temps = [0.01, 0.0025, 0.]
    with make(N0=N0, seed=seed, job=job, njobs=R, sweep={"temperature": temps}) as e:
        e.init()
        V0 = e.get_state()["V"]
        e.qsteps(200)
        g1 = e.get_state()
        V1, tp = g1["V"], g1["tPart"]
        dirs = [e.save_directory(k) for k in range(6)]
    for k in range(6):
        q, r = divmod(k, R)
        assert same_bits(V0[k], sample_velocities(seed + job + r, N0, temps[q])), k
        assert dirs[k].endswith(f"InitialTemp{(10000, 2500, 0)[q]}uK/job{job + r}/")
        assert same_bits(V1[k, 1:], V0[k, 1:])           # V[1], V[2] are carried, never touched
    for k in (4, 5):
        # T = 0: at v = 0 the two beams balance exactly, so an ion rests until its first jump's recoil, and moves
        # along x only
        assert (V0[k] == 0).all()
        never = tp[k] == tp[k].max()                     # tPart was never reset
        assert 0 < never.sum() < N0
        assert (V1[k, 0][never] == 0).all() and (V1[k, 0][~never] != 0).any()
        assert (V1[k, 1:] == 0).all()
    assert 0.09 < V0[0].std() < 0.12 and 0.045 < V0[2].std() < 0.06     # 1.0508 sqrt(T)


# ---- 3. the scan's kernel against the dense checker, away from the default laser ----
def test_one_step_no_jump_off_default(orc):
    """test_gpu_mdlc.py::test_one_step_no_jump, its gates, through the scan's kernel at (detuning, Om) =
    (-1.25, 1.5): the existing suite checks the defaults only"""
    N0, job, R, q0 = 70, 3, 2, 5
    det, Om = POINTS[1]["detuning"], POINTS[1]["Om"]
    rng = np.random.default_rng(11)
    psi = random_states(rng, N0)
    vx = rng.normal(0, 0.105, N0)
    tp = rng.uniform(0, 2, N0)
    dp = 0.01 * ((np.abs(psi[:, 1]) ** 2) + (np.abs(psi[:, 2]) ** 2))
    for seed in range(4242, 4282):                     # chosen on the CPU, from the checker alone
        ok = True
        for r in range(R):
            u1, _ = draws(orc, seed, job + r, N0, q0)
            ok = ok and (u1 > dp).sum() >= 60 and np.abs(u1 - dp).min() > 1e-9
        if ok:
            break
    else:
        pytest.fail("no seed with >= 60 no-jump ions and a decision margin above 1e-9 in both replicas")
    V = np.zeros((6, 3, N0))
    V[:, 0] = vx
    with make(N0=N0, seed=seed, job=job, njobs=R, sweep=POINTS) as e:
        e.set_state(V=V, psi=np.tile(psi, (6, 1, 1)), tPart=np.tile(tp, (6, 1)), q=q0)
        e.qsteps(1)
        g = e.get_state()
    assert g["q"] == q0 + 1
    for r in range(R):
        k = R + r                                      # point 1
        u1, rd = draws(orc, seed, job + r, N0, q0)
        nojump, worst = 0, (0., 0.)
        for i in range(N0):
            p, v, t, j = D.qstep_ion(psi[i], vx[i], tp[i], u1[i], rd[i], detuning=det, Om=Om)
            nojump += not j
            dpsi, dv = np.abs(g["psi"][k, i] - p).max(), abs(g["V"][k, 0, i] - v)
            worst = max(worst[0], dpsi), max(worst[1], dv)
            assert dpsi <= 1e-12 and dv <= 1e-15, (r, i, j, dpsi, dv)
            assert g["tPart"][k, i] == t
            assert (g["tPart"][k, i] == 0) == j        # the jump set
        print(f"seed {seed} replica {r}: {nojump} no-jump ions, max |dpsi| = {worst[0]:.3e}, max |dv| = {worst[1]:.3e}")
        assert nojump >= 60
    # the default point would fail this point's gates: the comparison can see the laser
    assert np.abs(g["psi"][0] - g["psi"][R]).max() > 1e-4


# ---- 4. launch splitting ----
def test_launch_splitting_is_bit_identical():
    kw = dict(N0=70, seed=99, job=4, njobs=2, sweep=POINTS)
    with make(**kw) as a, make(**kw) as b:
        a.init(); b.init()
        a.qsteps(50)
        b.qsteps(7); b.qsteps(43)
        ga, gb, ea, eb = a.get_state(), b.get_state(), a.ekin_x(), b.ekin_x()
    assert ga["q"] == gb["q"] == 50
    for k in ("V", "psi", "tPart"):
        assert same_bits(ga[k], gb[k]), k
    assert same_bits(ea, eb)


# ---- 5. a scan of one point is the ordinary ensemble ----
def test_one_point_equals_the_ordinary_ensemble():
    kw = dict(N0=300, seed=31, job=5, njobs=3)
    with make(sweep={"detuning": [-0.5]}, **kw) as a, make(**kw) as b:
        assert (a.npoints, a.members, b.npoints, b.members) == (1, 3, 1, 3)
        assert (b.const("npoints"), b.const("njobs"), b.const("members")) == (1, 3, 3)
        a.init(); b.init()
        e0a, e0b = a.ekin_x(), b.ekin_x()                # (the partial-sum launch alone)
        a.qsteps(50); b.qsteps(50)
        ga, gb, ea, eb = a.get_state(), b.get_state(), a.ekin_x(), b.ekin_x()
        assert [a.save_directory(k) for k in range(3)] == [b.save_directory(k) for k in range(3)]
    for k in ("V", "psi", "tPart"):
        assert same_bits(ga[k], gb[k]), k
    assert same_bits(e0a, e0b) and same_bits(ea, eb)


# ---- 6. run() and the command line ----
def tree(base):
    """{path below base: bytes} of every file"""
    out = {}
    for d, _, files in os.walk(base):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, base)] = open(p, "rb").read()
    return out


def test_run_and_cli_write_each_members_files(tmp_path):
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    N0, seed, job, R = 70, 77, 6, 2
    dets, oms = [-0.5, -1.0], [0.5, 1.0]
    a, b, c = (str(tmp_path / x) + "/" for x in "abc")
    kw = dict(N0=N0, seed=seed, job=job, njobs=R, tmax=0.35, sampleFreq=10)
    want = [f"Om{int(o * 100)}/Det{int(d * 100)}NumIons70InitialTemp10000uK/job{job + r}/"
            for d in dets for o in oms for r in range(R)]
    with make(saveDirectory=a, sweep={"detuning": dets, "Om": oms}, **kw) as e:
        assert e.members == 8 and e.const("iterations") == 35 and e.const("outputs") == 3
        e.run()
        assert e.get_state()["q"] == 35
        assert [e.save_directory(k) for k in range(8)] == [a + w for w in want]
        fresh = tree(a)
        e.run()                                          # appends, as the reference's "a" mode
        twice = tree(a)
        member = [e.member_params(k) for k in range(8)]
    assert sorted(fresh) == sorted(w + "energies.dat" for w in want) and len(set(want)) == 8
    for k, p in enumerate(member):
        p.saveDirectory = b.encode()
        with make(p) as s:
            s.run()
            one = open(b + want[k] + "energies.dat", "rb").read()
            s.run()
            two = open(b + want[k] + "energies.dat", "rb").read()
        assert len(one.splitlines()) == 3 and two == one + one
        assert fresh[want[k] + "energies.dat"] == one, k
        assert twice[want[k] + "energies.dat"] == two, k
    # the replicas of a point differ in print (in 35 steps the points of a replica move EkinX by less than %lg shows)
    assert all(fresh[want[k] + "energies.dat"] != fresh[want[k + 1] + "energies.dat"] for k in range(0, 8, 2))
    assert tree(b) == twice
    r = subprocess.run([MDLC_CLI_PATH, str(job), f"--N0={N0}", f"--seed={seed}", f"--njobs={R}", "--tmax=0.35",
                        "--sampleFreq=10", f"--saveDirectory={c}", "--device=0", "--quiet=1",
                        "--sweep=detuning:-0.5,-1", "--sweep=Om:0.5,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert tree(c) == fresh


# ---- 7. the scan sees the physics ----
def test_red_cools_and_blue_heats():
    """1024 ions at v = +0.2: the red-detuned point slows them, the blue-detuned point speeds them up.  The dense
    checker alone gives mean dv = -3.1e-3, z = -28 (red) and +2.9e-3, z = +26 (blue) at these settings."""
    n, steps, v0 = 1024, 5000, 0.2
    V = np.zeros((2, 3, n))
    V[:, 0] = v0
    psi = np.zeros((2, n, 3), complex)
    psi[:, :, 0] = 1
    with make(N0=n, seed=7, job=1, sweep={"detuning": [-0.5, 0.5]}) as e:
        e.set_state(V=V, psi=psi, tPart=np.zeros((2, n)), q=0)
        e.qsteps(steps)
        dv = e.get_state()["V"][:, 0] - v0
    z = dv.mean(1) / (dv.std(1, ddof=1) / np.sqrt(n))
    print(f"red: mean dv = {dv[0].mean():.3e}, z = {z[0]:.1f}; blue: mean dv = {dv[1].mean():.3e}, z = {z[1]:.1f}")
    assert dv[0].mean() < 0 < dv[1].mean()
    assert abs(z[0]) >= 5 and abs(z[1]) >= 5
