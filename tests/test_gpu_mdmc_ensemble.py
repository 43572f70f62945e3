"""An ensemble of Monte-Carlo + MD jobs (include/mdmc.h "ensembles", mdmc --njobs=J) against the same jobs
run alone: member k of MonteCarloEnsemble(seed, job) and MonteCarloMD(seed=seed + k, job=job + k) driven by
the same calls give the same bits — np.array_equal on the state (R, V, A, U), the wavefunctions and tags of
the QT tagging variant, the accepted counts, and byte-equal files.  No tolerances: the batched anneal kernel
is the single-job kernel's body on each member's own argument block, and the MD stages are the single
context's code on the member's own stream.
"""
import os
import subprocess

import numpy as np
import pytest

from tests.ensemble_helpers import tree

pytestmark = pytest.mark.gpu

BASE = dict(numVelAutoCorrsSteps=8, seed=41, job=5)
# the reduced MCMD main() of test_mdmc.py::test_run_writes_the_reference_files and the reduced QTT main() of
# test_mdmc_qt.py::test_qtt_run_writes_the_reference_files
MCMD_RUN = dict(N=512, monteCarloSteps=20000, numPreRecordMDSteps=20, numVelAutoCorrsSteps=150,
                numInstantaneousAnisotropySteps=30, numReestablishEquilSteps=10, anisotropyEstablishmentTime=1,
                anisotropyFromForcesRelaxSteps=25, job=3, seed=9)
QTT_RUN = dict(qt_model=1, N=512, monteCarloSteps=20000, numPreRecordMDSteps=20, numVelAutoCorrsSteps=40, job=4, seed=3)


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


def single(k, **kw):
    from mdqtplasmasims_amd.mdmc import MonteCarloMD
    kw = dict(kw, seed=kw["seed"] + k, job=kw["job"] + k)
    return MonteCarloMD(**kw)


def assert_same_state(a, b, what=""):
    for name, x, y in zip("RVAU", a.get_state(), b.get_state()):
        assert np.array_equal(x, y), (what, name)


# ---- 1. the anneal: both passes of the per-thread loop, both pair-energy forms ----
@pytest.mark.parametrize("force_kernel", [0, 1])
@pytest.mark.parametrize("N", [512, 1728])       # NPT = 1 with half the threads idle; NPT = 2, ragged second pass of 704
def test_anneal_matches_the_jobs_run_alone(M, N, force_kernel):
    kw = dict(BASE, N=N, force_kernel=force_kernel)
    with M.MonteCarloEnsemble(3, **kw) as ens:
        ens.init()
        acc = ens.monte_carlo(3000)
        assert len(acc) == 3 and all(0 < a < 3000 for a in acc), acc
        assert not np.array_equal(ens.jobs[0].get_state()[0], ens.jobs[1].get_state()[0])
        for k in range(3):
            with single(k, **kw) as s:
                s.init()
                assert s.monte_carlo(3000) == acc[k], k
                assert_same_state(ens.jobs[k], s, k)


# ---- 2. chunking ----
def test_anneal_calls_add_up_and_cross_the_chunk(M):
    kw = dict(BASE, N=512)
    with M.MonteCarloEnsemble(2, **kw) as ens, M.MonteCarloEnsemble(2, **kw) as big:
        ens.init()
        a1, a2 = ens.monte_carlo(1000), ens.monte_carlo(1500)
        big.init()
        ab = big.monte_carlo(12000)                    # one full chunk of 10,000 and a last one of 2,000
        for k in range(2):
            with single(k, **kw) as s:
                s.init()
                assert s.monte_carlo(2500) == a1[k] + a2[k]
                assert_same_state(ens.jobs[k], s, ("2500", k))
            with single(k, **kw) as s:
                s.init()
                assert s.monte_carlo(12000) == ab[k]
                assert_same_state(big.jobs[k], s, ("12000", k))


# ---- 3. alone and together ----
def test_a_job_does_not_depend_on_the_ensemble_size(M):
    kw = dict(BASE, N=512)
    with M.MonteCarloEnsemble(2, **kw) as two, M.MonteCarloEnsemble(5, **kw) as five, M.MonteCarloEnsemble(1, **kw) as one:
        for e in (two, five, one):
            e.init()
        a2, a5, a1 = two.monte_carlo(1000), five.monte_carlo(1000), one.monte_carlo(1000)
        assert a2[1] == a5[1]
        assert_same_state(two.jobs[1], five.jobs[1], "job index 1")
        with single(0, **kw) as s:
            s.init()
            assert [s.monte_carlo(1000)] == a1
            assert_same_state(one.jobs[0], s, "J = 1")


# ---- 4. MD steps ----
def test_md_steps_with_collisions_laser_force_and_a_member_stepped_alone(M):
    kw = dict(BASE, N=512)
    with M.MonteCarloEnsemble(3, **kw) as ens:
        ens.init()
        ens.monte_carlo(500)
        ens.md_steps(12)                               # collisionFreq 0.25: host-drawn collisions
        for j in ens.jobs:
            j.set_collision_freq(0)
        ens.jobs[1].set_laser_force(True)
        ens.md_steps(12)
        ens.jobs[2].md_steps(3)                        # a member on its own between two ensemble calls
        ens.jobs[2].monte_carlo(50)
        ens.md_steps(4)
        for k in range(3):
            with single(k, **kw) as s:
                s.init()
                s.monte_carlo(500)
                s.md_steps(12)
                s.set_collision_freq(0)
                if k == 1:
                    s.set_laser_force(True)
                s.md_steps(12)
                if k == 2:
                    s.md_steps(3)
                    s.monte_carlo(50)
                s.md_steps(4)
                assert_same_state(ens.jobs[k], s, k)
        assert not np.array_equal(ens.jobs[0].get_state()[1], ens.jobs[1].get_state()[1])


# ---- 5. the QT tagging variant ----
def test_qt_tagging_members(M):
    kw = dict(BASE, qt_model=1, N=512)

    def drive(md_steps, mc, members):
        mc(500)
        md_steps(5)
        for m in members:
            m.qsteps(20)
        md_steps(2)

    with M.MonteCarloEnsemble(2, **kw) as ens:
        ens.init()
        drive(ens.md_steps, ens.monte_carlo, ens.jobs)
        for k in range(2):
            with single(k, **kw) as s:
                s.init()
                drive(s.md_steps, s.monte_carlo, [s])
                assert np.array_equal(ens.jobs[k].get_psi(), s.get_psi()), k
                assert_same_state(ens.jobs[k], s, k)
                te, ne = ens.jobs[k].tag_qt()
                ts, ns = s.tag_qt()
                assert ne == ns and np.array_equal(te, ts), k
        assert not np.array_equal(ens.jobs[0].get_psi(), ens.jobs[1].get_psi())


# ---- 6. run(): every stage and file ----
@pytest.mark.parametrize("cfg", [MCMD_RUN, QTT_RUN], ids=["mcmd", "qtt"])
def test_run_writes_each_jobs_own_files(M, tmp_path, cfg):
    with M.MonteCarloEnsemble(2, saveDirectory=str(tmp_path / "ens") + "/", **cfg) as ens:
        ens.run()
    for k in range(2):
        with single(k, saveDirectory=str(tmp_path / "alone") + "/", **cfg) as s:
            s.run()
    te, ta = tree(tmp_path / "ens"), tree(tmp_path / "alone")
    assert sorted(te) == sorted(ta) and len(te) > 20
    assert {p.split(os.sep)[1] for p in te} == {f"job{cfg['job']}", f"job{cfg['job'] + 1}"}
    for p in te:
        assert te[p] == ta[p], p


# ---- 7. refusals ----
@pytest.mark.parametrize("njobs", [0, -3, 1025])
def test_refuses_njobs_out_of_range(M, njobs):
    with pytest.raises(M.MdqtError, match="njobs"):
        M.MonteCarloEnsemble(njobs, **dict(BASE, N=512))


def test_refuses_n_beyond_the_lds_kernel(M):
    with pytest.raises(M.MdqtError, match="N = 6859"):
        M.MonteCarloEnsemble(2, **dict(BASE, N=6859))


# ---- 8. the command line ----
def test_cli_njobs(M, tmp_path):
    from mdqtplasmasims_amd._lib import MDMC_CLI_PATH
    cfg = {k: v for k, v in MCMD_RUN.items() if k not in ("job", "seed")}

    def cli(sub, job, seed, *more):
        r = subprocess.run([MDMC_CLI_PATH, str(job), f"--seed={seed}", "--quiet=1", "--device=0",
                            f"--saveDirectory={tmp_path / sub}/", *[f"--{k}={v}" for k, v in cfg.items()], *more],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout == "", (r.stdout, r.stderr)
        return tree(tmp_path / sub)

    ens = cli("ens", 3, 9, "--njobs=2")
    four = cli("four", 4, 10)
    sub = {p: b for p, b in ens.items() if p.split(os.sep)[1] == "job4"}
    assert sub == four and len(four) > 10
    assert len(ens) == 2 * len(four)
    assert cli("one", 3, 9, "--njobs=1") == cli("plain", 3, 9)
