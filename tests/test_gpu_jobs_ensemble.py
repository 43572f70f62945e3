"""An ensemble of jobs stepped in batched launches (include/mdqt.h "ensembles", mdqt --njobs=J) against the
same jobs on contexts of their own: bit-identity throughout, no tolerances — the single-job path is what
the rest of the suite pins to the oracle and the reference.

Below 128 ions a context takes the owner-computes rows by default (an ensemble member keeps that: its own
small force launch inside the batched call), so the small cases run twice: with the default scheme, and
with force_scheme 2 on the members and the singles alike, which puts the one-tile (slot = F, nothing
pending) and two-tile jobs through the batched force kernel."""
import os
import subprocess

import numpy as np
import pytest

from tests.ensemble_helpers import assert_same, member_params, snapshot, tree

pytestmark = pytest.mark.gpu

SMALL = dict(N0=62, seed=501, job=1, rng_mode=1)            # the oracle's init(): N = SMALL_N for jobs 1 .. 6
SMALL_N = [64, 64, 62, 70, 67, 47]
C2 = dict(N0=3500, seed=12346, job=1, rng_mode=1)
C2_N = [3573, 3399, 3496]                                   # 56 / 54 / 55 tiles


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as M
    return M


def single(M, params, k, options, calls):
    """job k of an ensemble of `params`, on a context of its own, after `calls`"""
    with M.Simulation(**member_params(params, k)) as s:
        for name, v in options.items():
            s.set_option(name, v)
        s.init()
        calls(s)
        return snapshot(s)


def ensemble(M, params, njobs, options, calls):
    with M.Ensemble(njobs=njobs, **params) as e:
        for name, v in options.items():
            e.set_option(name, v)
        e.init()
        calls(e)
        return [snapshot(j) for j in e.jobs], [j.const("qt_kernel") for j in e.jobs]


_singles = {}


def small_single(M, k, scheme, nsteps=3):
    """the small jobs' single runs, computed once"""
    key = (k, scheme, nsteps)
    if key not in _singles:
        _singles[key] = single(M, SMALL, k, {"force_scheme": scheme}, lambda s: s.md_steps(nsteps))
    return _singles[key]


# ---- 1. one-tile edge: full / ragged single tiles and two-tile jobs in one launch ----
@pytest.mark.parametrize("scheme", [0, 2])
def test_one_tile_edge(M, scheme):
    got, _ = ensemble(M, SMALL, 6, {"force_scheme": scheme}, lambda e: e.md_steps(3))
    assert [g["N"] for g in got] == SMALL_N
    for k, g in enumerate(got):
        assert g["c0"] == 2 and g["qstep"] == 75
        assert_same(g, small_single(M, k, scheme), f"scheme {scheme} job index {k}")


# ---- 2. the production instance: N0 = 3500, split and plain tile-pair tables, quantum jumps ----
def test_production_instance(M):
    opts = {"force_split_cus": 256}
    seen = {}

    def calls(e):
        e.md_steps(1)
        seen["first"] = [j.const("qt_kernel") for j in e.jobs]
        seen["split"] = [j.const("force_tile_split_pairs") for j in e.jobs]
        e.md_steps(2)

    got, kernels = ensemble(M, C2, 3, opts, calls)
    assert [g["N"] for g in got] == C2_N
    assert seen["split"] == [4, 0, 0]                       # job 0 on the split table, the others plain
    assert seen["first"] == [4, 4, 4] and kernels == [1, 1, 1]   # t = 0: the general lane instance; then the headline one
    jumps = 0
    for k, g in enumerate(got):
        assert_same(g, single(M, C2, k, opts, lambda s: s.md_steps(3)), f"job index {k}")
        jumps += int((g["tPart"] < g["tPart"].max()).sum())   # tPart restarts at a jump
    assert jumps > 0, "no quantum jump in 75 substeps of 10,468 ions: the jump tail did not run"


def test_production_instance_three_waves(M):
    """option qt_waves 3 (the tighter register budget of the batched production instance): same bits"""
    opts = {"force_split_cus": 256}
    with M.Ensemble(njobs=2, **C2) as e:
        e.set_option("force_split_cus", 256)
        e.set_option("qt_waves", 3)
        with pytest.raises(M.MdqtError, match="qt_waves"):
            e.set_option("qt_waves", 2)
        e.init()
        e.md_steps(3)
        got = [snapshot(j) for j in e.jobs]
        assert [j.const("qt_kernel") for j in e.jobs] == [1, 1]
    for k, g in enumerate(got):
        assert_same(g, single(M, C2, k, opts, lambda s: s.md_steps(3)), f"job index {k}")


# ---- 3. alone and together: job 2 (seed 502) in ensembles of 1, 2 and 6 ----
@pytest.mark.parametrize("scheme", [0, 2])
def test_alone_and_together(M, scheme):
    ref = small_single(M, 1, scheme)
    alone, _ = ensemble(M, dict(SMALL, seed=502, job=2), 1, {"force_scheme": scheme}, lambda e: e.md_steps(3))
    assert_same(alone[0], ref, "njobs 1")
    for nj in (2, 6):
        got, _ = ensemble(M, SMALL, nj, {"force_scheme": scheme}, lambda e: e.md_steps(3))
        assert_same(got[1], ref, f"njobs {nj}")


# ---- 4. seam-level calls, and a member read between them ----
@pytest.mark.parametrize("peek", [False, True])
def test_seam_calls_equal_md_steps(M, peek):
    opts = {"force_scheme": 2}
    ratio = 25

    def seam(e):
        assert e.jobs[0].const("plasmaToQuantumTimestepRatio") == ratio
        for _ in range(2):
            e.forces()
            if peek:                                        # settles job 3's slots (two tiles) only
                st = e.jobs[3].get_state()
                assert np.isfinite(st["F"]).all() and np.abs(st["F"]).max() > 0
                e.jobs[0].get_state()                       # a one-tile job: nothing pending
            e.substeps(7)
            e.substeps(ratio - 7)

    got, _ = ensemble(M, SMALL, 6, opts, seam)
    for k, g in enumerate(got):                             # c0 is md_steps' own count: the seam calls leave it
        assert g["c0"] == -1                                # to the caller, as mdqt_forces / mdqt_substeps do
        assert_same(dict(g, c0=1), small_single(M, k, 2, nsteps=2), f"job index {k}")


# ---- 5. ratio above MAXSUB: two launches per interval ----
def test_ratio_above_maxsub(M):
    params = dict(SMALL, density=0.5)
    opts = {"force_scheme": 2}
    got, _ = ensemble(M, params, 2, opts, lambda e: e.md_steps(2))
    for k, g in enumerate(got):
        assert g["qstep"] == 100
        assert_same(g, single(M, params, k, opts, lambda s: s.md_steps(2)), f"job index {k}")


# ---- 6. MD only ----
def test_md_only(M):
    params = dict(SMALL, qt_enabled=0)
    opts = {"force_scheme": 2}
    got, kernels = ensemble(M, params, 3, opts, lambda e: e.md_steps(3))
    assert kernels == [4, 4, 4]                             # the general lane instance with do_qt = 0
    for k, g in enumerate(got):
        assert_same(g, single(M, params, k, opts, lambda s: s.md_steps(3)), f"job index {k}")


# ---- 6a. more argument uploads in a row than the pinned ring has slots (8) ----
def test_more_launches_than_ring_slots(M):
    """every substeps() call takes a slot for its QT blocks: 12 of them go once and a half round the ring"""
    opts = {"force_scheme": 2}

    def calls(x):
        for _ in range(12):
            x.forces()
            x.substeps(1)
        x.md_steps(3)

    got, _ = ensemble(M, SMALL, 3, opts, calls)
    for k, g in enumerate(got):
        assert g["qstep"] == 12 + 75
        assert_same(g, single(M, SMALL, k, opts, calls), f"job index {k}")


def test_md_steps_built_ahead_round_the_ring(M):
    """md_steps' built-ahead path: 1024 device blocks / 64 jobs / 1 QT launch per MD step = 16 MD steps per upload,
    so 130 = 8 x 16 + 2 MD steps are 9 uploads, one more than the ring has slots (the force blocks, unchanged from
    step to step, took one more slot before the first)"""
    opts = {"force_scheme": 2}
    njobs, seen = 64, {}

    def calls(e):
        ratio = e.jobs[0].const("plasmaToQuantumTimestepRatio")
        per_step = -(-int(ratio) // 32)                     # QT launches per MD step (MAXSUB 32)
        ahead = min(64, 1024 // (njobs * per_step))
        assert ahead >= 2 and 64 % ahead == 0               # the built-ahead path, whole batches up to step 64 k
        seen["steps"] = 8 * ahead + 2                       # 9 uploads
        e.md_steps(seen["steps"])

    got, _ = ensemble(M, SMALL, njobs, opts, calls)
    assert seen["steps"] == 130
    for k in (0, 31, 63):
        assert got[k]["c0"] == 129
        assert_same(got[k], single(M, SMALL, k, opts, lambda s: s.md_steps(seen["steps"])), f"job index {k}")


# ---- 6b. the timing contract: exact launch counts, then a reset ----
def test_kernel_times_count_the_batched_launches(M):
    with M.Ensemble(njobs=3, **SMALL) as e:
        e.set_option("force_scheme", 2)                     # every member on the tiles: one force launch per MD step
        e.init()
        e.enable_timing()
        e.md_steps(4)
        t = e.kernel_times()
        assert t["n_force"] == 4 and t["n_substep"] == 4    # ratio 25 <= MAXSUB: one QT launch per MD step
        for k in ("force", "substep"):
            assert 0 < t[k + "_median_ms"] <= t[k + "_ms"]
        again = e.kernel_times()
        assert all(v == 0 for v in again.values()), again
    with M.Simulation(**SMALL) as s:
        s.set_option("force_scheme", 2)
        s.init()
        s.enable_timing()
        s.md_steps(4)
        t = s.kernel_times()
        assert t["n_force"] > 0 and t["n_substep"] > 0 and t["force_ms"] > 0 and t["substep_ms"] > 0
        again = s.kernel_times()                            # a single context's: the same reset
        assert all(v == 0 for v in again.values()), again


# ---- 7. lockstep ----
def test_lockstep_names_the_job(M):
    with M.Ensemble(njobs=3, **SMALL) as e:
        e.init()
        e.md_steps(1)
        e.jobs[1].md_steps(1)
        before = [snapshot(j) for j in e.jobs]
        for call in (lambda: e.md_steps(1), e.forces, lambda: e.substeps(1)):
            with pytest.raises(M.MdqtError, match=r"job index 1 is out of step"):
                call()
        for k, j in enumerate(e.jobs):                      # nothing was launched
            assert_same(snapshot(j), before[k], f"job index {k}")


# ---- 8. refusals ----
@pytest.mark.parametrize("param, word", [(dict(rng_mode=0), "rng_mode"), (dict(qt_model=1), "qt_model"),
                                          (dict(world_size=2), "world_size")])
def test_refused_at_creation(M, param, word):
    with pytest.raises(M.MdqtError, match=word):
        M.Ensemble(njobs=2, **dict(SMALL, **param))


@pytest.mark.parametrize("njobs", [0, -3, 1025])
def test_refused_sizes(M, njobs):
    with pytest.raises(M.MdqtError, match="njobs"):
        M.Ensemble(njobs=njobs, **SMALL)


def test_refused_options(M):
    with M.Ensemble(njobs=2, **SMALL) as e:
        e.init()
        e.jobs[1].set_option("fused_step", 1)
        with pytest.raises(M.MdqtError, match="job index 1 has the option"):
            e.md_steps(1)
        e.jobs[1].set_option("fused_step", 0)
        e.jobs[0].set_option("qt_math", 0)
        with pytest.raises(M.MdqtError, match="job index 0 has qt_math"):
            e.md_steps(1)


# ---- 9. run() ----
def test_run_writes_the_singles_files(M, tmp_path):
    a, b = str(tmp_path / "ens") + "/", str(tmp_path / "one") + "/"
    nj = 3

    def both(**kw):
        with M.Ensemble(njobs=nj, saveDirectory=a, **dict(SMALL, **kw)) as e:
            e.run()
            dirs = [os.path.relpath(j.save_directory, a) for j in e.jobs]
            c0 = [j.counters()["c0"] for j in e.jobs]
        for k in range(nj):
            with M.Simulation(saveDirectory=b, **dict(SMALL, seed=SMALL["seed"] + k, job=SMALL["job"] + k, **kw)) as s:
                s.run()
                assert os.path.relpath(s.save_directory, b) == dirs[k]
                assert s.counters()["c0"] == c0[k]
        ta, tb = tree(a), tree(b)
        assert sorted(ta) == sorted(tb)
        assert [k for k in ta if ta[k] != tb[k]] == []
        return ta, c0[0]

    files, c0 = both(tmax=0.1)
    for k in range(nj):
        job = [f for f in files if f"/job{1 + k}/" in f]
        assert sum("statePopulationsVsVTime" in f for f in job) == 1          # output() at c0 = 39
        assert sum("wvFns_timestep" in f for f in job) == 1 and any(f.endswith("energies.dat") for f in job)
    files2, c1 = both(tmax=0.16, newRun=0, c0=c0)
    assert c1 > c0 and len(files2) > len(files)


# ---- 10. the command line ----
def test_cli_njobs(M, tmp_path):
    def run(base, *args):
        r = subprocess.run([M.CLI_PATH, *args, "--N0=62", "--tmax=0.1", f"--saveDirectory={base}/"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.split()

    assert run(tmp_path / "ens", "1", "--njobs=2", "--seed=501") == ["64", "64"]
    assert run(tmp_path / "one", "2", "--seed=502") == ["64"]
    te, to = tree(tmp_path / "ens"), tree(tmp_path / "one")
    job2 = {k: v for k, v in te.items() if "/job2/" in k}
    assert job2 and sorted(job2) == sorted(to)
    assert [k for k in job2 if job2[k] != to[k]] == []
    assert any("/job1/" in k for k in te)
    assert run(tmp_path / "alone", "2", "--njobs=1", "--seed=502") == ["64"]
    ta = tree(tmp_path / "alone")
    assert sorted(ta) == sorted(to) and [k for k in ta if ta[k] != to[k]] == []
