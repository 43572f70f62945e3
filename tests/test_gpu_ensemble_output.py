"""The SpeedUp ensemble's batched output() (include/mdqt.h "ensembles": mdqt_ensemble_output, _observables,
_epotential; mdqt --njobs=J --output_batch=0|1) against the same jobs on contexts of their own: every number
array_equal, every file byte-equal, no tolerances.

A member is batched when its own pass takes the Newton-3 tile potential (N >= 128 by default, or force_scheme
2); any other member takes its own call inside the batched one.  Ensemble.output_launches counts the batched
path's kernel launches only: 6 per output() or observables(), 3 per epotential(), 0 when no member is batched.
Member sizes are the CPU oracle's init()."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.ensemble_helpers import assert_same, tree

pytestmark = pytest.mark.gpu

SEED = dict(seed=501, job=1, rng_mode=1)
SMALL = dict(N0=62, **SEED)
SMALL_N = [64, 64, 62, 70, 67, 47]          # full and ragged single tiles, two-tile jobs; N // 32 = 1 and 2 chunks
MID = dict(N0=120, **SEED)
MID_N = [107, 136, 119, 128, 116, 116]      # both sides of the 128-ion rule; 128 = two full tiles, 136 = three
LARGE = dict(N0=300, **SEED)
LARGE_N = [288, 299, 313, 320, 314, 300]    # five tiles, ragged and full; 9 and 10 KDE chunks in one launch
C2 = dict(N0=3500, seed=12346, job=1, rng_mode=1)
C2_N = [3573, 3399, 3496]


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as M
    return M


def job_of(params, k):
    return dict(params, seed=params["seed"] + k, job=params["job"] + k)


def record(obs, epot_after_obs, ep, epot_after_ep):
    o, P, pops = obs
    return dict(o=np.array(o), P=np.array(P), pops=np.array(pops), Epot_obs=epot_after_obs, ep=ep, Epot_ep=epot_after_ep)


def probe_single(s):
    obs = s.observables()
    c = s.counters()["Epot"]
    ep = s.epotential()
    return record(obs, c, ep, s.counters()["Epot"])


def probe_ensemble(e):
    obs = e.observables()
    c = [j.counters()["Epot"] for j in e.jobs]
    ep = e.epotential()
    return [record(obs[k], c[k], ep[k], j.counters()["Epot"]) for k, j in enumerate(e.jobs)]


def state(sim):              # this file's own: ensemble_helpers.snapshot has Epot0 as well, which these tests never compared
    st = sim.get_state()
    c = sim.counters()
    return dict(st, qstep=sim.qstep_index, c0=c["c0"], counter=c["counter"], Epot=c["Epot"], N=sim.N)


_singles = {}


def single_probes(M, params, k, options, tail=0):
    """job k on a context of its own: the probes after init() and after md_steps(3) [and the state `tail` MD steps on]"""
    key = (tuple(sorted(params.items())), k, tuple(sorted(options.items())), tail)
    if key not in _singles:
        with M.Simulation(**job_of(params, k)) as s:
            for name, v in options.items():
                s.set_option(name, v)
            s.init()
            first = probe_single(s)
            s.md_steps(3)
            second = probe_single(s)
            end = None
            if tail:
                s.md_steps(tail)
                end = state(s)
            _singles[key] = (first, second, end)
    return _singles[key]


def ensemble_probes(M, params, njobs, options, output_batch=1, tail=0, first_job=0):
    with M.Ensemble(njobs=njobs, **job_of(params, first_job)) as e:
        for name, v in options.items():
            e.set_option(name, v)
        e.set_option("output_batch", output_batch)
        e.init()
        first = probe_ensemble(e)
        e.md_steps(3)                                       # leaves force slots pending
        second = probe_ensemble(e)
        launches = e.output_launches
        end = None
        if tail:
            e.md_steps(tail)
            end = [state(j) for j in e.jobs]
        return dict(N=e.N, first=first, second=second, launches=launches, end=end,
                    scheme=[int(j.const("force_scheme")) for j in e.jobs])


def check_against_singles(M, params, got, options, tail=0, first_job=0):
    for k in range(len(got["N"])):
        a, b, end = single_probes(M, params, first_job + k, options, tail)
        assert_same(got["first"][k], a, f"job index {k} after init()")
        assert_same(got["second"][k], b, f"job index {k} after md_steps(3)")
        if tail:
            assert_same(got["end"][k], end, f"job index {k}, {tail} MD steps after the observables")


# ---- 1. observables() and epotential() against the singles' ----
@pytest.mark.parametrize("scheme", [2, 0])
def test_small_members(M, scheme):
    opts = {"force_scheme": scheme}
    got = ensemble_probes(M, SMALL, 6, opts)
    assert got["N"] == SMALL_N
    assert got["scheme"] == ([2] * 6 if scheme else [1] * 6)
    assert got["launches"] == (2 * (6 + 3) if scheme else 0)     # all batched / every member its own fallback
    check_against_singles(M, SMALL, got, opts)


def test_both_sides_of_the_128_ion_rule(M):
    got = ensemble_probes(M, MID, 6, {})
    assert got["N"] == MID_N
    assert got["scheme"] == [1, 2, 1, 2, 1, 1]              # rows below 128 ions: job indices 1 and 3 are batched
    assert got["launches"] == 2 * (6 + 3)
    check_against_singles(M, MID, got, {})
    with M.Ensemble(njobs=6, **MID) as e:                    # ... and only those: taken off the tile potential,
        e.set_option("output_batch", 1)                      # nothing is left for the batched path
        e.init()
        for k in (1, 3):
            e.jobs[k].set_option("potential_n3", 0)
        obs = e.observables()
        assert e.output_launches == 0
        e.jobs[3].set_option("potential_n3", 1)
        e.epotential()
        assert e.output_launches == 3
    for k in (1, 3):                                         # potential_n3 changes the summation order, not these
        assert np.array_equal(obs[k][0][:4], got["first"][k]["o"][:4])


def test_five_tiles_and_two_chunk_counts(M):
    got = ensemble_probes(M, LARGE, 6, {})
    assert got["N"] == LARGE_N
    assert sorted({n // 32 for n in LARGE_N}) == [9, 10]
    assert got["launches"] == 2 * (6 + 3)
    check_against_singles(M, LARGE, got, {})


def test_production_size_split_table_slots_stay_pending(M):
    opts = {"force_split_cus": 256}
    got = ensemble_probes(M, C2, 3, opts, tail=2)
    assert got["N"] == C2_N
    assert got["launches"] == 2 * (6 + 3)
    check_against_singles(M, C2, got, opts, tail=2)


# ---- 2. both output_batch values, J = 1, 3, 6; job 2 alone and together ----
@pytest.mark.parametrize("njobs", [1, 3, 6])
def test_output_batch_values_agree(M, njobs):
    opts = {"force_scheme": 2}
    a = ensemble_probes(M, SMALL, njobs, opts, output_batch=1)
    b = ensemble_probes(M, SMALL, njobs, opts, output_batch=0)
    assert a["launches"] == 2 * (6 + 3) and b["launches"] == 0
    for k in range(njobs):
        assert_same(a["first"][k], b["first"][k], f"job index {k} after init()")
        assert_same(a["second"][k], b["second"][k], f"job index {k} after md_steps(3)")
    check_against_singles(M, SMALL, a, opts)


@pytest.mark.parametrize("njobs", [1, 2])
def test_job_2_alone_and_together(M, njobs):
    """job 2 (seed 502) first in ensembles of 1 and 2 (index 1 of 6: test_small_members)"""
    opts = {"force_scheme": 2}
    got = ensemble_probes(M, SMALL, njobs, opts, first_job=1)
    check_against_singles(M, SMALL, got, opts, first_job=1)


# ---- 3. launch counts ----
@pytest.mark.parametrize("njobs", [1, 6])
def test_launch_counts(M, tmp_path, njobs):
    with M.Ensemble(njobs=njobs, saveDirectory=str(tmp_path) + "/", **SMALL) as e:
        e.set_option("force_scheme", 2)
        e.set_option("output_batch", 1)
        e.init()
        e.md_steps(1)
        for j in e.jobs:
            j.setup_directories()
        assert e.output_launches == 0
        e.output()
        assert e.output_launches == 6
        e.observables(pops=False)
        assert e.output_launches == 6 + 5
        e.epotential()
        assert e.output_launches == 6 + 5 + 3
        e.set_option("output_batch", 0)
        e.output()
        e.observables()
        e.epotential()
        assert e.output_launches == 6 + 5 + 3
        with pytest.raises(M.MdqtError, match="output_batch"):
            e.set_option("output_batch", 2)


def test_kernel_times_keep_their_six_and_grow(M):
    from mdqtplasmasims_amd._lib import lib
    with M.Ensemble(njobs=3, **SMALL) as e:
        e.set_option("force_scheme", 2)
        e.set_option("output_batch", 1)
        e.init()
        e.enable_timing()
        e.md_steps(2)
        e.observables()
        e.epotential()
        t = e.output_kernel_times()
        assert t["n_force"] == 2 and t["n_substep"] == 2
        assert t["n_potential"] == 2 and t["n_kde"] == 1
        assert 0 < t["potential_median_ms"] <= t["potential_ms"] and 0 < t["kde_median_ms"] <= t["kde_ms"]
        e.md_steps(1)
        six = e.kernel_times()
        assert sorted(six) == sorted(["force_ms", "n_force", "substep_ms", "n_substep", "force_median_ms", "substep_median_ms"])
        assert six["n_force"] == 1 and six["n_substep"] == 1
        e.md_steps(1)
        e.epotential()
        out = (C.c_double * 12)(*([-1.] * 12))                  # a caller that passes 6 gets its six
        assert lib().mdqt_ensemble_kernel_times(e.h, out, 6) == 0
        assert out[1] == 1 and out[3] == 1 and list(out[6:]) == [-1.] * 6


# ---- 4. output() files ----
@pytest.mark.parametrize("params, scheme", [(SMALL, 2), (MID, 0)])
def test_output_files(M, tmp_path, params, scheme):
    a, b = str(tmp_path / "ens") + "/", str(tmp_path / "one") + "/"
    nj = 6

    def calls(x):
        x.md_steps(2); x.output(); x.md_steps(1); x.output()

    with M.Ensemble(njobs=nj, saveDirectory=a, **params) as e:
        e.set_option("force_scheme", scheme)
        e.set_option("output_batch", 1)
        for j in e.jobs:
            j.setup_directories()
        e.init()
        calls(e)
        assert e.output_launches == 12
        counters = [j.counters() for j in e.jobs]
    for k in range(nj):
        with M.Simulation(saveDirectory=b, **job_of(params, k)) as s:
            s.set_option("force_scheme", scheme)
            s.setup_directories()
            s.init()
            calls(s)
            assert s.counters() == counters[k] and counters[k]["counter"] == 2
    ta, tb = tree(a), tree(b)
    assert sorted(ta) == sorted(tb)
    assert [k for k in ta if ta[k] != tb[k]] == []
    for k in range(nj):
        job = sorted(os.path.basename(f) for f in ta if f"/job{1 + k}/" in f)
        assert job == sorted(["energies.dat"] + [f"vel_dist{x}_time{c:06d}.dat" for x in "XYZ" for c in (0, 1)] +
                             [f"statePopulationsVsVTime{c:06d}.dat" for c in (0, 1)])
        assert ta[[f for f in ta if f"/job{1 + k}/" in f and f.endswith("energies.dat")][0]].count(b"\n") == 2


# ---- 5. run(), fresh and resumed ----
def test_run_both_output_batch_values(M, tmp_path):
    nj = 3
    bases = {ob: str(tmp_path / f"ens{ob}") + "/" for ob in (0, 1)}
    one = str(tmp_path / "one") + "/"

    def both(counter0=0, **kw):
        c0 = None
        for ob, base in bases.items():
            with M.Ensemble(njobs=nj, saveDirectory=base, **dict(SMALL, **kw)) as e:
                e.set_option("force_scheme", 2)
                e.set_option("output_batch", ob)
                before = [j.counters()["counter"] for j in e.jobs]
                e.run()
                cs = [j.counters() for j in e.jobs]
                outputs = cs[0]["counter"] - counter0
                assert outputs >= 1 and before == [0] * nj
                assert e.output_launches == (6 * outputs if ob else 0)
                assert c0 in (None, cs[0]["c0"])
                c0 = cs[0]["c0"]
        for k in range(nj):
            with M.Simulation(saveDirectory=one, **job_of(dict(SMALL, **kw), k)) as s:
                s.set_option("force_scheme", 2)
                s.run()
                assert s.counters()["c0"] == c0
        t1 = tree(one)
        for base in bases.values():
            te = tree(base)
            assert sorted(te) == sorted(t1)
            assert [k for k in te if te[k] != t1[k]] == []
        return c0, cs[0]["counter"]

    c0, counter = both(tmax=0.1)
    assert counter == 1                                          # output() at c0 = 39
    c1, counter1 = both(counter0=counter, tmax=0.16, newRun=0, c0=c0)
    assert c1 > c0 and counter1 > counter


# ---- 6. the command line ----
def test_cli_output_batch(M, tmp_path):
    for ob in (0, 1):
        r = subprocess.run([M.CLI_PATH, "1", "--njobs=2", "--N0=62", "--tmax=0.1", "--seed=501", f"--output_batch={ob}",
                            f"--saveDirectory={tmp_path}/ob{ob}/"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == ["64", "64"]
    t0, t1 = tree(tmp_path / "ob0"), tree(tmp_path / "ob1")
    assert t0 and sorted(t0) == sorted(t1)
    assert [k for k in t0 if t0[k] != t1[k]] == []
    assert any("statePopulationsVsVTime" in k for k in t0)


# ---- 6a. the pump ensemble's output(): Epotential() from the batched potential path ----
PUMP_RUN = dict(N0=300, seed=5, job=2, rng_mode=1, tmax=0.3, sampleFreq=10, tpumpreal=5.2e-8, tstartV0=0.1, Ge=0.1,
                Om=0.7, detuning=-2.5)                  # tests/test_gpu_pump_ensemble.py's RUN with PROGRAM[1]


def test_pump_ensemble_output_takes_the_batched_potential(M, tmp_path):
    nj = 3
    launches, outputs, after_run = {}, {}, {}
    for ob in (0, 1):
        base = tmp_path / f"ens{ob}"
        with M.PumpEnsemble(nj, pump_program=1, saveDirectory=str(base) + "/", **PUMP_RUN) as e:
            e.set_option("output_batch", ob)
            e.run()
            after_run[ob] = tree(base)
            launches[ob], c0 = e.launches(), [j.counters()["counter"] for j in e.jobs]
            outputs[ob] = c0[0]
            e.output()                                           # one more, on its own
            assert e.launches() - launches[ob] == (2 + 3 if ob else 2)   # the tagged KDE's two, the potential path's three
            assert [j.counters()["counter"] for j in e.jobs] == [c + 1 for c in c0]
    assert outputs[0] == outputs[1] >= 2
    assert launches[1] - launches[0] == 3 * outputs[1]
    for k in range(nj):
        with M.Simulation(pump_program=1, saveDirectory=str(tmp_path / "one") + "/", **job_of(PUMP_RUN, k)) as s:
            s.run_pump()
    t1 = tree(tmp_path / "one")
    for ob in (0, 1):                                            # run_pump's members' files, byte for byte
        assert sorted(after_run[ob]) == sorted(t1)
        assert [k for k in t1 if after_run[ob][k] != t1[k]] == []
    a, b = tree(tmp_path / "ens0"), tree(tmp_path / "ens1")      # ... and the extra output()'s under both values
    assert len(a) > len(t1) and sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == []


# ---- 7. refusals ----
def test_desynchronised_member_and_null_arguments(M):
    from mdqtplasmasims_amd._lib import lib
    with M.Ensemble(njobs=3, **SMALL) as e:
        e.set_option("force_scheme", 2)
        e.set_option("output_batch", 1)
        e.init()
        e.md_steps(1)
        L = lib()
        for rc in (L.mdqt_ensemble_observables(e.h, None, None, None), L.mdqt_ensemble_epotential(e.h, None)):
            assert rc != 0 and b"NULL argument" in L.mdqt_last_error()
        for rc in (L.mdqt_ensemble_output(None), L.mdqt_ensemble_observables(None, None, None, None),
                   L.mdqt_ensemble_epotential(None, None)):
            assert rc != 0 and b"NULL ensemble" in L.mdqt_last_error()
        assert L.mdqt_ensemble_output_launches(None) == 0
        e.jobs[1].md_steps(1)
        n0 = e.output_launches
        for call in (e.output, e.observables, e.epotential):
            with pytest.raises(M.MdqtError, match=r"job index 1 is out of step"):
                call()
        assert e.output_launches == n0                      # nothing was launched
