"""An ensemble of optical-pumping jobs stepped in batched launches (include/mdqt.h "ensembles of the
optical-pumping programs", `mdqt --pump_program=m --pump_jobs=J`) against the same jobs on contexts of their
own: bit-identical state, byte-identical files, no tolerances — the single-job path is what
test_gpu_pump_main.py pins to the oracle.

The members' N come from the host-side init() (the oracle's, on the CPU): SMALL has a one-tile member below
64 ions, a full single tile, and two-tile members between 64 and 128 (ragged last tiles; below 128 ions a
context takes the owner-computes rows by default, so SMALL also runs with force_scheme 2, which puts them
through the batched force kernel); MID has five- and six-tile members with ragged last tiles, so that the
grids' "past my last tile / group / chunk" exits run."""
import subprocess

import numpy as np
import pytest

from tests.ensemble_helpers import assert_same, assert_same_trees, member_params, snapshot, tree

pytestmark = pytest.mark.gpu

SMALL = dict(N0=62, seed=501, job=1, rng_mode=1)            # the oracle's init(): SMALL_N for jobs 1 .. 5
SMALL_N = [64, 64, 62, 70, 67]
MID = dict(N0=300, seed=5, job=2, rng_mode=1)               # MID_N for jobs 2 .. 6: 5 / 6 / 5 / 5 / 5 tiles
MID_N = [313, 327, 296, 290, 287]
SIZES = {"small": (SMALL, SMALL_N), "mid": (MID, MID_N)}
T1 = 0.37                                                   # a time past 0 for the moving form of step()

# test_gpu_pump_main.py's SMALL run and its three programs' parameters
RUN = dict(N0=300, seed=5, job=2, rng_mode=1, tmax=0.3, sampleFreq=10, tpumpreal=5.2e-8, tstartV0=0.1, Ge=0.1)
PROGRAM = {1: dict(Om=0.7, detuning=-2.5), 2: dict(Om=2.0, detuning=0.0), 3: dict(Om=1.3, detuning=-1.0)}
# strong drive for the QT-only steps: quantum jumps and mixed tags within 66 qsteps of ~300 ions
QT = {1: dict(Om=4.0, detuning=0.0), 2: dict(Om=6.0, detuning=0.0), 3: dict(Om=4.0, detuning=0.0)}


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as M
    return M


# ---- 1. MD steps: the t == 0 form, then five steps at t > 0 (leading drift, folded drifts, the last unfolded) ----
_md_singles = {}


def md_single(M, size, k, scheme):
    key = (size, k, scheme)
    if key not in _md_singles:
        with M.Simulation(pump_program=1, **member_params(SIZES[size][0], k)) as s:
            s.set_option("force_scheme", scheme)
            s.init()
            s.pump_md_steps(1)
            first = snapshot(s)
            s.t = T1
            s.pump_md_steps(5)
            _md_singles[key] = (first, snapshot(s))
    return _md_singles[key]


@pytest.mark.parametrize("njobs", [1, 3, 5])
@pytest.mark.parametrize("size,scheme", [("small", 0), ("small", 2), ("mid", 0)])
def test_md_steps(M, size, scheme, njobs):
    params, want_N = SIZES[size]
    with M.PumpEnsemble(njobs, pump_program=1, **params) as e:
        e.set_option("force_scheme", scheme)
        e.init()
        assert e.N == want_N[:njobs]
        e.md_steps(1)
        first = [snapshot(j) for j in e.jobs]
        for j in e.jobs:
            j.t = T1
        e.md_steps(5)
        last = [snapshot(j) for j in e.jobs]
    for k in range(njobs):
        a, b = md_single(M, size, k, scheme)
        assert last[k]["c0"] == first[k]["c0"] + 5
        assert_same(first[k], a, f"{size} scheme {scheme} job index {k}, the t == 0 step")
        assert_same(last[k], b, f"{size} scheme {scheme} job index {k}, five steps at t > 0")


# ---- 2. two launches per MD step for any J ----
@pytest.mark.parametrize("njobs", [1, 5])
def test_launch_count(M, njobs):
    n = 4
    with M.PumpEnsemble(njobs, pump_program=1, **MID) as e:
        e.init()
        assert min(e.N) >= 128                              # every member on the Newton-3 tiles
        for j in e.jobs:
            j.t = T1
        before = e.launches()
        e.md_steps(n)
        e.synchronize()
        assert e.launches() - before == 2 * n + 1           # the leading drift, then (force, kick-drift[-drift]) x n


# ---- 3. QT-only steps (1, 25 and 40: the last crosses MAXSUB) and 4. the tagging after them ----
QSTEPS = (1, 25, 40)
_qt_singles = {}


def qt_single(M, model, k):
    key = (model, k)
    if key not in _qt_singles:
        with M.Simulation(pump_program=model, **member_params(dict(MID, **QT[model]), k)) as s:
            s.init()
            snaps = []
            for n in QSTEPS:
                for _ in range(n):
                    s.qstep()
                snaps.append(snapshot(s))
            _qt_singles[key] = (snaps, s.tag_spin_up())
    return _qt_singles[key]


@pytest.mark.parametrize("model", [1, 2, 3])
def test_qsteps_and_tagging(M, model):
    njobs = 3
    with M.PumpEnsemble(njobs, pump_program=model, **dict(MID, **QT[model])) as e:
        e.init()
        snaps = []
        for n in QSTEPS:
            e.qsteps(n)
            snaps.append([snapshot(j) for j in e.jobs])
        kernels = [j.const("qt_kernel") for j in e.jobs]
        tags = e.tag_spin_up()
    assert kernels == [6] * njobs                           # QTK_LANES_R_PUMP
    jumps = 0
    for k in range(njobs):
        want, (wtags, wn) = qt_single(M, model, k)
        for i, n in enumerate(QSTEPS):
            assert snaps[i][k]["qstep"] == sum(QSTEPS[:i + 1])
            assert_same(snaps[i][k], want[i], f"model {model} job index {k} after {n} more qsteps")
        tp = want[-1]["tPart"]
        jumps += int((tp < tp.max()).sum())                 # tPart restarts at a jump
        assert 0 < wn < want[-1]["N"], "the single job's tags are all equal: the tagging shows nothing"
        assert tags[k][1] == wn and np.array_equal(tags[k][0], wtags), f"model {model} job index {k}: tags"
    assert jumps > 0, "no quantum jump on the single contexts: the jump path did not run"


# ---- 4a. more QT launches in a row than the pinned ring has slots (8), and the tagging's slot after them ----
def test_more_qt_launches_than_ring_slots(M):
    njobs = 3
    params = dict(MID, **QT[1])
    with M.PumpEnsemble(njobs, pump_program=1, **params) as e:
        e.init()
        for _ in range(12):
            e.qsteps(1)
        got = [snapshot(j) for j in e.jobs]
        tags = e.tag_spin_up()
    for k in range(njobs):
        with M.Simulation(pump_program=1, **member_params(params, k)) as s:
            s.init()
            for _ in range(12):
                s.qstep()
            assert_same(got[k], snapshot(s), f"job index {k} after twelve launches of one qstep")
            wtags, wn = s.tag_spin_up()
        assert tags[k][1] == wn and np.array_equal(tags[k][0], wtags), f"job index {k}: tags"


# ---- 4b. the timing contract: exact launch counts, then a reset ----
def test_kernel_times_count_the_batched_launches(M):
    with M.PumpEnsemble(3, pump_program=1, **MID) as e:
        e.init()
        assert min(e.N) >= 128                              # every member on the Newton-3 tiles
        for j in e.jobs:
            j.t = T1
        e.enable_timing()
        e.md_steps(4)                                       # (force, kick-drift) x 4
        e.qsteps(40)                                        # 32 + 8: two QT launches
        t = e.kernel_times()
        assert (t["n_force"], t["n_kick"], t["n_qt"]) == (4, 4, 2)
        for k in ("force", "kick", "qt"):
            assert 0 < t[k + "_median_ms"] <= t[k + "_ms"]
        again = e.kernel_times()
        assert all(v == 0 for v in again.values()), again


# ---- 5. run() and 6. the resume, against run_pump() of every job into another directory ----
def run_both(M, model, njobs, params, da, db, launches=None):
    """the ensemble's run into da, the singles' into db: (final states, spin-up lists, c0) of both sides"""
    p = dict(params, **PROGRAM[model])
    with M.PumpEnsemble(njobs, pump_program=model, saveDirectory=str(da) + "/", **p) as e:
        e.run()
        assert launches is None or e.launches() == launches
        got = [(snapshot(j), j.spin_up_list()) for j in e.jobs]
    want = []
    for k in range(njobs):
        with M.Simulation(pump_program=model, saveDirectory=str(db) + "/", **member_params(p, k)) as s:
            s.run_pump()
            want.append((snapshot(s), s.spin_up_list()))
    for k in range(njobs):
        assert_same(got[k][0], want[k][0], f"model {model} job index {k}: final state")
        assert got[k][1][1] == want[k][1][1] and np.array_equal(got[k][1][0], want[k][1][0]), f"job index {k}: spin_up_list"
    assert_same_trees(da, db)
    return got


@pytest.mark.parametrize("model", [1, 2, 3])
def test_run_and_resume(M, tmp_path, model):
    got = run_both(M, model, 3, RUN, tmp_path / "ens", tmp_path / "one")
    assert [g[0]["N"] for g in got] == MID_N[:3]
    assert all(0 < g[1][1] < g[0]["N"] for g in got)
    names = tree(tmp_path / "ens")
    for k in range(3):
        assert any(f"job{2 + k}/vel_distX_timestep" in n for n in names)
    # newRun = 0 from those files (readConditions of every member), a little further
    c0 = got[0][0]["c0"]
    run_both(M, model, 3, dict(RUN, newRun=0, c0=c0, tmax=RUN["tmax"] + 0.05), tmp_path / "ens", tmp_path / "one")
    assert len(tree(tmp_path / "ens")) > len(names)


# The run's launches, so that a fold the loop asks for and the driver drops shows (the files would not change).
# RUN's schedule (tests/test_main_loops.py's loop at ratio 25, tendV0 = 0.1 + 0.0598...): 151 MD steps, 30 QT
# launches, the tagging; with sampleFreq 1, 72 outputs and 72 led / 79 folded steps; with none, the tagging's
# output and 2 led / 149 folded steps.  A step is a force and a kick launch, a led one a drift launch more, the
# t == 0 step its forces() first, an output two launches: 2 x 151 + led + 1 + 30 + 1 + 2 x outputs.
RUN_LAUNCHES = {1: 550, 100000: 338}


@pytest.mark.parametrize("sampleFreq", [1, 100000])
def test_run_every_step_an_output_and_none(M, tmp_path, sampleFreq):
    """sampleFreq 1: an output after every MD step once tagged, no folded drift there; sampleFreq beyond the
    run: every step but the measurement's and the last is folded"""
    run_both(M, 1, 3, dict(RUN, sampleFreq=sampleFreq), tmp_path / "ens", tmp_path / "one", RUN_LAUNCHES[sampleFreq])


# ---- 7. a member stepped on its own ends the ensemble's stepping, before anything is launched ----
def test_desynchronised_member_is_refused(M):
    with M.PumpEnsemble(3, pump_program=1, **MID) as e:
        e.init()
        for j in e.jobs:
            j.t = T1
        e.md_steps(2)
        e.jobs[1].pump_md_steps(1)                          # its own step: c0 runs ahead
        before = [snapshot(j) for j in e.jobs]
        n0 = e.launches()
        for call in (lambda: e.md_steps(1), lambda: e.qsteps(1), e.tag_spin_up):
            with pytest.raises(M.MdqtError, match="job index 1 is out of step"):
                call()
        assert e.launches() == n0
        for k, j in enumerate(e.jobs):
            assert_same(snapshot(j), before[k], f"job index {k} after the refused calls")
        with M.Simulation(pump_program=1, **member_params(MID, 1)) as s:   # the member alone did what a context does
            s.init()
            s.t = T1
            s.pump_md_steps(3)
            assert_same(before[1], snapshot(s), "the member stepped on its own")


# ---- 8. the command line ----
def test_cli_pump_jobs(M, tmp_path):
    common = ["--pump_program=3", "--N0=300", "--tmax=0.3", "--sampleFreq=10", "--tpumpreal=5.2e-8", "--tstartV0=0.1"]
    r = subprocess.run([M.CLI_PATH, "2", *common, "--pump_jobs=2", "--seed=5", f"--saveDirectory={tmp_path}/ens/"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(n) for n in MID_N[:2]]
    for k in range(2):
        s = subprocess.run([M.CLI_PATH, str(2 + k), *common, f"--seed={5 + k}", f"--saveDirectory={tmp_path}/one/"],
                           capture_output=True, text=True, timeout=120)
        assert s.returncode == 0, s.stderr
        assert s.stdout.split() == [str(MID_N[k])]
    assert_same_trees(tmp_path / "ens", tmp_path / "one")
    assert subprocess.run(["diff", "-r", str(tmp_path / "ens"), str(tmp_path / "one")], capture_output=True).returncode == 0
