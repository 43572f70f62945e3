"""The batched QT calls of an ensemble of QT tagging jobs (include/mdmc.h, "ensembles of the QT tagging variants":
qsteps, tag_qt, tagged_moments_qt, qt_launches; the pump and recorded stage of run() under md_batch 1) against the
same jobs on MonteCarloMD contexts of their own (mdmc_job_params(base, k): job + k, seed + k), and between md_batch 1
and md_batch 0.  Every comparison is np.array_equal / byte-equal: a batched kernel is the single-job kernel's body
on the member's own argument block, and the X distribution is component 0 of the three-component kernel with the
same terms in the same order.

Sizes (perfect cubes: init() takes only those): N = 27 (one ragged 16-ion lane group pair, one ragged 256-ion chunk),
343 (22 lane groups with a last one of 7; two chunks, the second of 87), 1331 (six chunks).  J = 1, 3, 5; models
1, 2, 3.  A QT call of n = 70 substeps splits into 32 + 32 + 6.

The members of a test start from the same positions, velocities and wavefunctions (heavy P populations on the first
40 ions, as tests/test_mdmc_qt.py's qstep test has them), so they differ in their Philox key (seed + k, job + k)
alone: the no-jump evolution is deterministic, and two members ending with different wavefunctions have jumped.
"""

import numpy as np
import pytest

from tests.ensemble_helpers import tree

pytestmark = pytest.mark.gpu

SEED, JOB = 41, 5
SIZES, JOBS, MODELS = [27, 343, 1331], [1, 3, 5], [1, 2, 3]
QTT_RUN = dict(N=216, monteCarloSteps=2000, numPreRecordMDSteps=5, numVelAutoCorrsSteps=101, job=4, seed=3)


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


def params(N, model, **kw):
    return dict(dict(qt_model=model, N=N, numVelAutoCorrsSteps=8, seed=SEED, job=JOB), **kw)


def alone(M, J, **kw):
    """the jobs of an ensemble on contexts of their own, from mdmc_job_params"""
    from mdqtplasmasims_amd.mdmc import MonteCarloMD, default_params
    from mdqtplasmasims_amd.mdmc_ensemble import mdmc_job_params
    base = default_params(**kw)
    out = []
    for k in range(J):
        p = mdmc_job_params(base, k)
        assert (p.job, p.seed) == (kw["job"] + k, kw["seed"] + k)
        out.append(MonteCarloMD(**dict(kw, seed=p.seed, job=p.job)))
    return out


class Groups:
    """the same jobs three ways: one ensemble per md_batch mode (1, 0), and contexts of their own"""

    def __init__(self, M, J, **kw):
        self.ens = [M.MonteCarloEnsemble(J, md_batch=mode, **kw) for mode in (1, 0)]
        self.lone = alone(M, J, **kw)
        self.groups = [self.lone, self.ens[0].jobs, self.ens[1].jobs]
        self.J = J

    def each(self, f, only=None):
        for g in self.groups:
            for k, m in enumerate(g):
                if only is None or k == only:
                    f(m)

    def md_steps(self, n):
        for e in self.ens:
            e.md_steps(n)
        for m in self.lone:
            m.md_steps(n)

    def qsteps(self, n):
        """n qsteps every way; the batched ensemble issues ceil(n / 32) launches, the other none"""
        before = [e.qt_launches() for e in self.ens]
        for e in self.ens:
            e.qsteps(n)
        for m in self.lone:
            m.qsteps(n)
        grown = [e.qt_launches() - b for e, b in zip(self.ens, before)]
        assert grown == [(n + 31) // 32, 0], (n, self.J, grown)

    def close(self):
        for e in self.ens:
            e.close()
        for m in self.lone:
            m.close()


def heavy_p(N, model):
    """normalised random wavefunctions with heavy P populations on the first 40 ions (tests/test_mdmc_qt.py:92-99)"""
    rng = np.random.default_rng(model)
    n = 5 if model == 3 else 7
    z = np.zeros((N, 12), complex)
    z[:, :n] = rng.normal(size=(N, n)) + 1j * rng.normal(size=(N, n))
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    z[:40, 2:2 + (2 if model == 3 else 4)] *= 30.0
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    return z


def prepare(G, N, model):
    """a short anneal and two MD steps, then member 0's state and the same wavefunctions for every member"""
    G.each(lambda m: m.init())
    for e in G.ens:
        e.monte_carlo(200)
    for m in G.lone:
        m.monte_carlo(200)
    G.md_steps(2)
    state = G.lone[0].get_state()
    z = heavy_p(N, model)
    G.each(lambda m: (m.set_state(*state), m.set_psi(z)))


def same(G, what):
    for g in G.groups[1:]:
        for k, (a, b) in enumerate(zip(G.lone, g)):
            assert np.array_equal(a.get_psi(), b.get_psi()), (what, k, "psi")
            for name, x, y in zip("RVAU", a.get_state(), b.get_state()):
                assert np.array_equal(x, y), (what, k, name)


# ---- 1. qsteps: 1, 32, 33 and 70 (32 + 32 + 6) substeps ----
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("J", JOBS)
@pytest.mark.parametrize("N", SIZES)
def test_qsteps_match_the_jobs_run_alone_and_the_other_mode(M, N, J, model):
    G = Groups(M, J, **params(N, model))
    try:
        prepare(G, N, model)
        assert [e.qt_launches() for e in G.ens] == [0, 0]
        start = G.lone[0].get_psi()
        for n in (1, 32, 33, 70):
            G.qsteps(n)
            same(G, n)
        assert not np.array_equal(G.lone[0].get_psi(), start)
        if J > 1:       # the same start, another Philox key: different only through a jump
            assert not np.array_equal(G.lone[0].get_psi(), G.lone[1].get_psi())
    finally:
        G.close()


# ---- 2. a member out of step with its neighbours ----
def test_member_stepped_alone_between_two_calls(M):
    N, model = 343, 2
    G = Groups(M, 3, **params(N, model))
    try:
        prepare(G, N, model)
        G.qsteps(5)
        G.each(lambda m: m.qsteps(3), only=1)            # its qstep index runs ahead of the others'
        G.qsteps(33)
        same(G, "a member three qsteps ahead")
        assert not np.array_equal(G.lone[0].get_psi(), G.lone[2].get_psi())
    finally:
        G.close()


# ---- 3. tag_qt and tagged_moments_qt ----
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("J", JOBS)
@pytest.mark.parametrize("N", SIZES)
def test_tags_moments_and_x_distribution(M, N, J, model):
    G = Groups(M, J, **params(N, model))
    try:
        prepare(G, N, model)
        G.qsteps(7)
        before = [e.qt_launches() for e in G.ens]
        tags = [e.tag_qt() for e in G.ens]
        assert [e.qt_launches() - b for e, b in zip(G.ens, before)] == [1, 0]          # one launch for any J
        lone = [m.tag_qt() for m in G.lone]
        for t, cnt in tags:
            assert t.shape == (J, N) and cnt.shape == (J,)
            for k in range(J):
                assert np.array_equal(t[k], lone[k][0]) and cnt[k] == lone[k][1] == lone[k][0].sum(), k
        for k in range(J):
            assert 0 < lone[k][1] < N, (k, lone[k][1])                                  # both values
        if J > 1:
            assert any(not np.array_equal(lone[0][0], lone[k][0]) for k in range(1, J))

        def moments(dist):
            before = [e.qt_launches() for e in G.ens]
            got = [e.tagged_moments_qt(dist=dist) for e in G.ens]
            assert [e.qt_launches() - b for e, b in zip(G.ens, before)] == [3 if dist else 1, 0]
            ref = [m.tagged_moments_qt(dist=dist) for m in G.lone]
            for g in got:
                mom, d = g if dist else (g, None)
                assert mom.shape == (J, 4)
                for k in range(J):
                    rm, rd = ref[k] if dist else (ref[k], None)
                    assert np.array_equal(mom[k], rm, equal_nan=True), (k, mom[k], rm)
                    if dist:
                        assert d.shape == (J, 4001) and np.array_equal(d[k], rd[0]), k
            return got[0], ref

        (mom, d), ref = moments(True)
        assert np.isfinite(mom).all() and (d.max(axis=1) > 0).all()
        moments(False)
        # the last member with no spin-up weight (all of it in state 1): none of its ions is tagged
        z = np.zeros((N, 12), complex)
        z[:, 1] = 1.0
        G.each(lambda m: m.set_psi(z), only=J - 1)
        tags = [e.tag_qt() for e in G.ens]
        lone = [m.tag_qt() for m in G.lone]
        for t, cnt in tags:
            assert cnt[J - 1] == 0 == lone[J - 1][1] and not t[J - 1].any()
            for k in range(J):
                assert np.array_equal(t[k], lone[k][0]), k
        (mom, d), ref = moments(True)
        assert np.isnan(mom[J - 1]).all() and np.isnan(ref[J - 1][0]).all()
        assert not d[J - 1].any()
        same(G, "tags and moments leave the state alone")
    finally:
        G.close()


# ---- 4. MD steps, QT steps, MD steps: the fences and the pre-advanced positions survive the QT call ----
def test_md_and_qt_steps_interleaved(M):
    N, model = 343, 2
    G = Groups(M, 3, **params(N, model))
    try:
        prepare(G, N, model)
        G.md_steps(3)
        G.qsteps(33)
        G.md_steps(3)
        same(G, "md, qt, md")
        G.qsteps(2)
        G.md_steps(1)
        same(G, "qt, md")
    finally:
        G.close()


# ---- 5. the timing entries ----
def test_kernel_times_count_the_qt_and_distribution_launches(M):
    N, model = 343, 2
    with M.MonteCarloEnsemble(2, md_batch=1, **params(N, model)) as ens:
        ens.init()
        ens.enable_timing(True)
        ens.qsteps(70)
        ens.tag_qt()
        ens.tagged_moments_qt()
        ens.tagged_moments_qt(dist=False)
        assert ens.qt_launches() == 3 + 1 + 3 + 1
        t = ens.kernel_times()
        assert t["n_qt"] == 3 and t["n_qt_dist"] == 1 and t["n_md_force"] == 0 and t["n_anneal"] == 0
        for k in ("qt", "qt_dist"):
            assert 0 < t[k + "_min_ms"] <= t[k + "_median_ms"] <= t[k + "_max_ms"] <= t[k + "_ms"]
        assert ens.kernel_times()["n_qt"] == 0            # reset


# ---- 6. an ensemble without QT refuses every call, by name ----
def test_an_ensemble_without_qt_refuses_the_calls(M):
    with M.MonteCarloEnsemble(2, N=27, numVelAutoCorrsSteps=8) as ens:
        for mode in (0, 1):
            ens.md_batch = mode
            for name, call in (("mdmc_ensemble_qsteps", lambda: ens.qsteps(1)), ("mdmc_ensemble_tag_qt", ens.tag_qt),
                               ("mdmc_ensemble_tagged_moments_qt", ens.tagged_moments_qt),
                               ("mdmc_ensemble_qt_launches", ens.qt_launches)):
                with pytest.raises(M.MdqtError, match=name + r".*no QT \(qt_model 0\)"):
                    call()


# ---- 7. run(): the pump and recorded stage in batched launches, every file ----
@pytest.mark.parametrize("model", [2, 3])
def test_qtt_run_writes_the_same_files_in_both_modes_and_alone(M, tmp_path, model):
    J, T, pre = 3, QTT_RUN["numVelAutoCorrsSteps"], QTT_RUN["numPreRecordMDSteps"]
    counts = {}
    for mode, jobs in ((1, J), (0, J), (1, 1)):
        kw = dict(QTT_RUN, qt_model=model, saveDirectory=f"{tmp_path}/mode{mode}_{jobs}/")
        if jobs == 1:
            kw["collisionFreq"] = 0.0                    # no collision scatter launches: md_launches is predictable
        with M.MonteCarloEnsemble(jobs, md_batch=mode, **kw) as ens:
            pump = int(ens.jobs[0].const("pumpMDTimeSteps"))
            ratio = int(ens.jobs[0].const("plasmaToQuantumTimestepRatio"))
            assert pump > 0 and ratio > 32
            ens.run()
            counts[mode, jobs] = (ens.qt_launches(), ens.md_launches())
    for m in alone(M, J, **dict(QTT_RUN, qt_model=model, saveDirectory=f"{tmp_path}/alone/")):
        m.run()
        m.close()
    # the QT launches: the pump stage's, the tagging, three per recorded step; whatever J is
    want = pump * ((ratio + 31) // 32) + 1 + 3 * T
    assert counts[1, J][0] == want == counts[1, 1][0], (counts, want)
    assert counts[0, J][0] == 0
    # with the MD launches (one stale-position launch per member, two per collisionless step, the temperatures and the
    # velocity store): seven launches per recorded step
    assert counts[1, 1][1] == 1 + 2 * pre + 2 * pump + 4 * T, (counts, pump)
    t1, t0, ta = tree(tmp_path / f"mode1_{J}"), tree(tmp_path / f"mode0_{J}"), tree(tmp_path / "alone")
    assert sorted(t1) == sorted(t0) == sorted(ta) and len(t1) >= J * (T + 8)
    assert any("pairPairCorrStepNum100.dat" in p for p in t1)        # a g(r) inside the recorded stage
    assert sum("vel_distX_timestep" in p for p in t1) == J * T
    for p in t1:
        assert t1[p] == t0[p] == ta[p], p
