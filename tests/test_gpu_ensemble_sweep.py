"""A sweep ensemble (mdqt_ensemble_create_sweep, Ensemble(sweep=...), mdqt --sweep: parameter points x replicas in
one set of batched launches) against the same jobs on contexts of their own: every member is bit for bit and
byte for byte the job it is alone — array_equal and equal files throughout, no tolerances.

Sizes (init()'s N for seeds 501, 502 at density 0.5): N0 = 62 -> 64, 64 (one tile each; force_scheme 2 puts them
through the batched force kernel), N0 = 120 -> 107, 136 (either side of the 128-ion rule: the first keeps its
own row launch), N0 = 300 -> 288, 299 (five tiles; 19 groups of 16, the last ragged).  density 0.5: 50 substeps
per MD step, two QT launches (MAXSUB 32)."""
import os
import subprocess

import numpy as np
import pytest

from tests.ensemble_helpers import assert_same, assert_same_trees, snapshot

pytestmark = pytest.mark.gpu

BASE = dict(seed=501, job=1, rng_mode=1, density=0.5, tmax=0.25)
RATIO = 50
POINTS3 = [dict(detuningDP=0.0, Om=0.5), dict(detuningDP=1.0, Om=0.0), dict(detuningDP=1.0, Om=1.0)]
POINTS2 = [dict(detuningDP=0.0), dict(detuningDP=1.0)]
# QTKernel codes (mdqt_internal.hpp)
IM_EDZ, IM, R_FAST, R_GENERAL, IM_EDZ_RN = 1, 2, 3, 4, 7


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as M
    return M


def member_params(params, points, njobs, k):
    """member k (point-major): the point's values, job + r and seed + r"""
    q, r = divmod(k, njobs)
    return dict(params, **points[q], seed=params["seed"] + r, job=params["job"] + r)


def seam_then_ahead(x):
    """init() has run: forces() + substeps(ratio) three times, then md_steps(3)"""
    for _ in range(3):
        x.forces()
        x.substeps(RATIO)
    x.md_steps(3)


_singles = {}


def single(M, params, options, calls):
    """one job on a context of its own after init() and `calls`; computed once per (parameters, options, calls)"""
    key = (tuple(sorted(params.items())), tuple(sorted(options.items())), calls.__name__)
    if key not in _singles:
        with M.Simulation(**params) as s:
            for name, v in options.items():
                s.set_option(name, v)
            s.init()
            calls(s)
            _singles[key] = snapshot(s)
    return _singles[key]


def check_members(M, e, params, points, njobs, options, calls):
    assert len(e.jobs) == len(points) * njobs
    for k, j in enumerate(e.jobs):
        want = single(M, member_params(params, points, njobs, k), options, calls)
        assert_same(snapshot(j), want, f"point {k // njobs} replica {k % njobs}")


# ---- 1. core identity ----
@pytest.mark.parametrize("N0, scheme, sizes", [(62, 2, [64, 64]), (120, 0, [107, 136]), (300, 0, [288, 299])])
def test_core_identity(M, N0, scheme, sizes):
    params, options = dict(BASE, N0=N0), {"force_scheme": scheme}
    with M.Ensemble(njobs=2, sweep=POINTS3, **params) as e:
        assert e.points == POINTS3 and M._lib.lib().mdqt_ensemble_points(e.h) == 3
        e.set_option("force_scheme", scheme)
        e.init()
        assert e.N == sizes * 3                                 # every point's replicas: the same init()
        first = [e.member(q, 0).get_state() for q in range(3)]
        for q in (1, 2):                                        # replica 0 of every point starts from the same state
            assert np.array_equal(first[q]["R"], first[0]["R"]) and np.array_equal(first[q]["V"], first[0]["V"])
        seam_then_ahead(e)
        check_members(M, e, params, POINTS3, 2, options, seam_then_ahead)
        assert e.member(2, 1) is e.jobs[5]
        psi = [e.member(q, 0).get_state()["psi"] for q in range(3)]
        assert not np.array_equal(psi[0], psi[1]) and not np.array_equal(psi[1], psi[2])   # ... and the laser told them apart
        assert e.member(0, 0).counters()["c0"] == e.member(2, 1).counters()["c0"]
        assert e.member(0, 0).qstep_index == 6 * RATIO


# ---- 2. every launch instance ----
def first_then_steps(x):
    x.forces()
    x.substeps(RATIO)            # from t = 0: not all-moving
    x.md_steps(2)


@pytest.mark.parametrize("what, extra, points, member_opts, ens_opts, instance", [
    ("production", {}, POINTS2, {}, {}, IM_EDZ),
    ("renormalised", dict(reNormalizewvFns=1), POINTS2, {}, {}, IM_EDZ_RN),
    ("expanding", {}, [dict(fracOfSig=0.5), dict(fracOfSig=1.0)], {}, {}, IM),
    ("general couplings", {}, POINTS2, {"qt_im01": 0}, {}, R_FAST),
    ("three waves", {}, POINTS2, {}, {"qt_waves": 3}, IM_EDZ),
])
def test_every_instance(M, what, extra, points, member_opts, ens_opts, instance):
    params = dict(BASE, N0=62, **extra)
    options = dict({"force_scheme": 2}, **member_opts)
    seen = []

    def calls(e):
        e.forces()
        e.substeps(RATIO)
        seen.append([j.const("qt_kernel") for j in e.jobs])
        e.md_steps(2)

    with M.Ensemble(njobs=2, sweep=points, **params) as e:
        for name, v in dict(options, **ens_opts).items():
            e.set_option(name, v)
        e.init()
        calls(e)
        # the first chunk from t = 0 is not all-moving (the general lane instance), the second and the rest are
        assert seen[0] == [instance] * 4
        assert [j.const("qt_kernel") for j in e.jobs] == [instance] * 4, what
        check_members(M, e, params, points, 2, options, first_then_steps)


def test_not_all_moving_instance(M):
    """the very first substeps from t = 0 (one chunk: t[0] = 0 is not moving): the general lane instance"""
    params, options = dict(BASE, N0=62), {"force_scheme": 2}
    with M.Ensemble(njobs=2, sweep=POINTS2, **params) as e:
        e.set_option("force_scheme", 2)
        e.init()
        first_seven(e)
        assert [j.const("qt_kernel") for j in e.jobs] == [R_GENERAL] * 4
        check_members(M, e, params, POINTS2, 2, options, first_seven)


def first_seven(x):
    x.forces()
    x.substeps(7)


# ---- 3. the backstop: one instance per launch ----
def test_an_option_on_one_member_is_refused_before_any_launch(M):
    with M.Ensemble(njobs=2, sweep=POINTS2, **dict(BASE, N0=62)) as e:
        e.set_option("force_scheme", 2)
        e.init()
        e.md_steps(1)
        e.jobs[2].set_option("qt_im01", 0)
        e.synchronize()
        e.enable_timing()
        before = [snapshot(j) for j in e.jobs]
        for call in (lambda: e.substeps(3), lambda: e.md_steps(2)):
            with pytest.raises(M.MdqtError, match=r"job index 2 differs from job index 0 in qt_im01"):
                call()
        t = e.kernel_times()
        assert t["n_substep"] == 0 and t["n_force"] == 0        # nothing was launched
        for k, j in enumerate(e.jobs):
            assert_same(snapshot(j), before[k], f"member {k}")
        e.jobs[2].set_option("qt_im01", 1)                      # in step again: the ensemble goes on
        e.md_steps(1)
        assert e.member(1, 0).counters()["c0"] == before[2]["c0"] + 1


# ---- 4. one point: the sweep kernels against the uniform ones ----
def test_one_point_equals_the_uniform_ensemble(M):
    params = dict(BASE, N0=300)
    with M.Ensemble(njobs=3, **params) as u, M.Ensemble(njobs=3, sweep={"Om": [1.0]}, **params) as s:
        lib = M._lib.lib()
        assert lib.mdqt_ensemble_points(u.h) == 1 and lib.mdqt_ensemble_points(s.h) == 1
        assert u.points == [{}] and s.points == [{"Om": 1.0}]
        for e in (u, s):
            e.init()
            seam_then_ahead(e)
        assert [j.const("qt_kernel") for j in s.jobs] == [IM_EDZ] * 3
        for k in range(3):
            assert_same(snapshot(s.jobs[k]), snapshot(u.jobs[k]), f"job index {k}")


# ---- 5. lockstep ----
def test_lockstep_names_the_member(M):
    with M.Ensemble(njobs=2, sweep=POINTS2, **dict(BASE, N0=62)) as e:
        e.init()
        e.md_steps(1)
        e.member(1, 0).md_steps(1)
        before = [snapshot(j) for j in e.jobs]
        for call in (lambda: e.md_steps(1), e.forces, lambda: e.substeps(1)):
            with pytest.raises(M.MdqtError, match=r"job index 2 is out of step"):
                call()
        for k, j in enumerate(e.jobs):
            assert_same(snapshot(j), before[k], f"member {k}")


# ---- 6. run(): fresh and resumed, both output paths ----
RUN = dict(BASE, N0=300, tmax=0.1)


@pytest.fixture(scope="module")
def single_runs(M, tmp_path_factory):
    """the four jobs' own runs, fresh (tmax 0.1) and resumed (to 0.16): (tree root, c0 after it) per stage"""
    out = []
    c0 = None
    for stage, kw in enumerate((dict(), dict(tmax=0.16, newRun=0))):
        root = str(tmp_path_factory.mktemp(f"singles{stage}")) + "/"
        if stage:
            kw = dict(kw, c0=c0)
            subprocess.run(["cp", "-r", out[0][0] + ".", root], check=True)
        dirs = []
        for k in range(4):
            with M.Simulation(saveDirectory=root, **member_params(dict(RUN, **kw), POINTS2, 2, k)) as s:
                s.run()
                dirs.append(os.path.relpath(s.save_directory, root))
                c0 = s.counters()["c0"]
        assert len(set(dirs)) == 4
        out.append((root, c0, dirs))
    return out


@pytest.mark.parametrize("output_batch", [0, 1])
def test_run_writes_the_singles_trees(M, single_runs, tmp_path, output_batch):
    root = str(tmp_path / "ens") + "/"
    kw = dict()
    for stage, (want_root, want_c0, want_dirs) in enumerate(single_runs):
        with M.Ensemble(njobs=2, sweep=POINTS2, saveDirectory=root, **dict(RUN, **kw)) as e:
            e.set_option("output_batch", output_batch)
            e.run()
            assert [os.path.relpath(j.save_directory, root) for j in e.jobs] == want_dirs
            assert [j.counters()["c0"] for j in e.jobs] == [want_c0] * 4
        assert_same_trees(root, want_root)
        kw = dict(tmax=0.16, newRun=0, c0=want_c0)
    assert single_runs[1][1] > single_runs[0][1]


# ---- 7. the command line ----
def test_cli_sweep(M, tmp_path):
    def run(base, *args):
        r = subprocess.run([M.CLI_PATH, *args, "--N0=62", "--tmax=0.1", "--density=0.5", f"--saveDirectory={base}/"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.split()

    assert run(tmp_path / "ens", "1", "--njobs=2", "--seed=501", "--sweep=detuningDP:0,1") == ["64", "64", "64", "64"]
    for dp in ("0", "1"):
        for r in (0, 1):
            assert run(tmp_path / "one", str(1 + r), f"--seed={501 + r}", f"--detuningDP={dp}") == ["64"]
    assert_same_trees(tmp_path / "ens", tmp_path / "one")
    d = subprocess.run(["diff", "-r", str(tmp_path / "ens"), str(tmp_path / "one")], capture_output=True, text=True)
    assert d.returncode == 0 and d.stdout == "", d.stdout[-2000:]


# ---- 8. launches per MD step do not grow with the points ----
@pytest.mark.parametrize("points", [[dict(Om=1.0)], POINTS2, POINTS3])
def test_launches_per_md_step(M, points):
    with M.Ensemble(njobs=2, sweep=points, **dict(BASE, N0=62)) as e:
        e.set_option("force_scheme", 2)                         # every member on the tiles
        e.init()
        e.enable_timing()
        e.md_steps(4)                                           # built ahead
        t = e.kernel_times()
        assert (t["n_force"], t["n_substep"]) == (4, 4 * -(-RATIO // 32))
        for _ in range(3):                                      # step by step
            e.forces()
            e.substeps(RATIO)
        t = e.kernel_times()
        assert (t["n_force"], t["n_substep"]) == (3, 3 * -(-RATIO // 32))
