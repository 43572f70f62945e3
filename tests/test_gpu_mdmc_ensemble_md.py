"""The batched MD stages of an MC + MD ensemble (include/mdmc.h, md_batch 1; mdmc --njobs=J --md_batch=1) against
the same jobs on MonteCarloMD contexts of their own (job + k, seed + k), and against the member-by-member mode
(md_batch 0).  Every comparison is np.array_equal / byte-equal: a batched kernel is the single-job kernel's body
on jobs[blockIdx.<job axis>], so there is nothing to tune.

Sizes: N = 27 (below one tile, ragged, one slot), 64 (exactly one tile: seven of k_vv_step's eight waves sum
nothing), 100 (two tiles, ragged last), 1025 (17 slots: the waves get 3, 2, 2, ... slots; a last tile of one
ion).  The non-cubes start from set_state, as tests/test_gpu_mdmc_sizes.py does.  run() begins with the
reference's lattice init (MCMD:182-201), which takes perfect cubes only, so the run() tests use the cubes that
reach the same paths: N = 125 (two tiles, ragged last) and N = 1331 (21 slots: the waves get 3, 3, 3, 3, 3, 2,
2, 2; a ragged last tile of 51).

The host rng (a member's own Mt32 and normal_distribution) has no getter: its state is compared through what it
produces next — tag_particles() (uniforms) and a further monte_carlo (the chain starts from the handed-over
state), both equal only if the stream position is.
"""
import math
import subprocess

import numpy as np
import pytest

from tests.ensemble_helpers import tree

pytestmark = pytest.mark.gpu

SEED, JOB, DT = 41, 5, 0.005
COLL = 0.25 / DT * 0.2                   # dt collisionFreq = 0.05: some members have no hit on some steps at N = 27
RUN = dict(monteCarloSteps=200, numPreRecordMDSteps=3, numVelAutoCorrsSteps=101, numInstantaneousAnisotropySteps=3,
           numReestablishEquilSteps=3, anisotropyEstablishmentTime=1, anisotropyFromForcesRelaxSteps=3, job=3, seed=9)
QTT_RUN = dict(qt_model=2, N=216, monteCarloSteps=2000, numPreRecordMDSteps=5, numVelAutoCorrsSteps=20, job=4, seed=3)


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


def params(N, **kw):
    return dict(dict(N=N, numVelAutoCorrsSteps=8, seed=SEED, job=JOB), **kw)


def alone(M, J, **kw):
    from mdqtplasmasims_amd.mdmc import MonteCarloMD
    return [MonteCarloMD(**dict(kw, seed=kw["seed"] + k, job=kw["job"] + k)) for k in range(J)]


def start(members, N):
    """seeded ions in [0, L] and Maxwellian velocities, different for every member (no lattice: any N)"""
    L = members[0].const("L")
    for k, m in enumerate(members):
        g = np.random.default_rng(7000 + 10 * N + k)
        m.set_state(R=g.uniform(0, L, (3, N)), V=g.normal(0, math.sqrt(1 / 3.), (3, N)), A=np.zeros((3, N)), U=np.zeros(N))


def same(a, b, what):
    for name, x, y in zip("RVAU", a.get_state(), b.get_state()):
        assert np.array_equal(x, y), (what, name)


def same_all(groups, what):
    ref = groups[0]
    for g in groups[1:]:
        for k, (a, b) in enumerate(zip(ref, g)):
            same(a, b, (what, k))


def same_rng(groups, what):
    """the members' host rng streams, through the next things drawn from them"""
    tags = [[m.tag_particles() for m in g] for g in groups]
    accs = [[m.monte_carlo(100) for m in g] for g in groups]
    for t, a in zip(tags[1:], accs[1:]):
        assert all(np.array_equal(x, y) for x, y in zip(tags[0], t)), what
        assert a == accs[0], what
    same_all(groups, (what, "after the next draws"))


class Groups:
    """the same jobs three ways: one ensemble per md_batch mode, and contexts of their own"""

    def __init__(self, M, J, **kw):
        self.ens = [M.MonteCarloEnsemble(J, md_batch=mode, **kw) for mode in (1, 0)]
        self.lone = alone(M, J, **kw)
        self.groups = [self.lone, self.ens[0].jobs, self.ens[1].jobs]

    def md_steps(self, n):
        for e in self.ens:
            e.md_steps(n)
        for m in self.lone:
            m.md_steps(n)

    def each(self, f, only=None):
        for g in self.groups:
            for k, m in enumerate(g):
                if only is None or k == only:
                    f(m)

    def monte_carlo(self, n):
        accs = [e.monte_carlo(n) for e in self.ens] + [[m.monte_carlo(n) for m in self.lone]]
        assert accs[0] == accs[1] == accs[2], accs

    def close(self):
        for e in self.ens:
            e.close()
        for m in self.lone:
            m.close()


def hit_counts(orc, seed, N, steps, p):
    """the hits of `steps` collisional steps of a fresh context (no init(): set_state) from the reference's own
    draws (MCMD:474-482): mt19937(seed) less the uniform of MCMD:55, one uniform per ion, three
    normal_distribution draws per hit (libstdc++: Marsaglia's polar method, two values per accepted point)"""
    mt = orc.MT19937(seed)
    mt.uniform()
    saved, out = False, []
    for _ in range(steps):
        n = 0
        for _ in range(N):
            if mt.uniform() < p:
                n += 1
                for _ in range(3):
                    if saved:
                        saved = False
                        continue
                    while True:
                        x, y = 2.0 * mt.uniform() - 1.0, 2.0 * mt.uniform() - 1.0
                        r2 = x * x + y * y
                        if not (r2 > 1.0 or r2 == 0.0):
                            break
                    saved = True
        out.append(n)
    return out


# ---- 1. six steps of each kind: with collisions, collisionless, under the laser force ----
@pytest.mark.parametrize("force_kernel", [0, 1])
@pytest.mark.parametrize("J", [1, 3, 5])
@pytest.mark.parametrize("N", [27, 64, 100, 1025])
def test_md_steps_match_the_jobs_run_alone_and_the_other_mode(M, N, J, force_kernel):
    from oracle import oracle as orc
    kw = params(N, force_kernel=force_kernel, collisionFreq=COLL)
    G = Groups(M, J, **kw)
    try:
        assert [e.md_batch for e in G.ens] == [1, 0]
        for g in G.groups:
            start(g, N)
        G.md_steps(6)                                    # collisional first: the draws are predictable from the seed
        same_all(G.groups, "collisions")
        if N == 27 and J > 1:
            hits = [hit_counts(orc, SEED + k, N, 6, DT * COLL) for k in range(J)]
            # a step on which one member has hits and another has none: k_collide_ens's h >= a.nhits row
            assert any(any(h[s] > 0 for h in hits) and any(h[s] == 0 for h in hits) for s in range(6)), hits
        G.monte_carlo(300)
        G.each(lambda m: m.set_collision_freq(0))
        G.md_steps(6)
        same_all(G.groups, "collisionless")
        G.each(lambda m: m.set_laser_force(True))
        G.md_steps(6)
        same_all(G.groups, "laser force")
        if J > 1:
            assert not np.array_equal(G.lone[0].get_state()[1], G.lone[1].get_state()[1])
        same_rng(G.groups, "rng")
    finally:
        G.close()


@pytest.mark.parametrize("force_kernel", [0, 1])
@pytest.mark.parametrize("N", [27, 1025])
def test_laser_force_along_one_axis(M, N, force_kernel):
    G = Groups(M, 3, **params(N, force_kernel=force_kernel, collisionFreq=0, applyForceAlongOneAxisOnly=1))
    try:
        for g in G.groups:
            start(g, N)
        G.monte_carlo(300)
        G.each(lambda m: m.set_laser_force(True))
        G.md_steps(6)
        same_all(G.groups, "one axis")
        G.each(lambda m: m.set_collision_freq(COLL))      # the collided ions take the laser term too (k_collide)
        G.md_steps(6)
        same_all(G.groups, "one axis, collisions")
    finally:
        G.close()


# ---- 2. a member out of step with its neighbours ----
def test_member_stepped_alone_restated_and_set_apart(M):
    N = 100
    G = Groups(M, 3, **params(N, collisionFreq=0))
    try:
        for g in G.groups:
            start(g, N)
        G.monte_carlo(300)
        G.md_steps(2)
        G.each(lambda m: m.md_steps(1), only=1)          # the other buffer parity from here on
        G.md_steps(3)
        same_all(G.groups, "parity")
        G.each(lambda m: m.set_state(*m.get_state()), only=2)   # clears the pre-advanced positions (rnValid)
        G.md_steps(2)
        same_all(G.groups, "set_state")
        G.each(lambda m: m.set_collision_freq(COLL), only=0)
        G.each(lambda m: m.set_laser_force(True), only=1)
        G.md_steps(4)
        same_all(G.groups, "one member's collision frequency, another's laser force")
        same_rng(G.groups, "rng")
    finally:
        G.close()


# ---- 2a. more uploads in flight than the pinned rings have slots: 64 collisional steps, 4 stretches ----
def test_more_steps_and_stretches_than_ring_slots(M):
    N = 27
    G = Groups(M, 3, **params(N, collisionFreq=COLL))
    try:
        for g in G.groups:
            start(g, N)
        G.md_steps(70)                                   # one stretch of 70 collisional steps: 70 VVArgs uploads
        same_all(G.groups, "70 collisional steps in one stretch")
        for _ in range(6):                               # six stretches: six header uploads
            G.md_steps(1)
        same_all(G.groups, "six stretches of one step")
        same_rng(G.groups, "rng")
    finally:
        G.close()


# ---- 3. the launch count: 2 per collisionless step, whatever J ----
@pytest.mark.parametrize("J", [1, 5])
def test_two_launches_per_collisionless_step(M, J):
    N = 64
    with M.MonteCarloEnsemble(J, md_batch=1, **params(N, collisionFreq=0)) as ens:
        start(ens.jobs, N)
        assert ens.md_launches() == 0
        ens.md_steps(1)                                  # J stale members: their k_vv_positions, then 2
        assert ens.md_launches() == J + 2
        for n in (6, 1, 3):
            before = ens.md_launches()
            ens.md_steps(n)
            assert ens.md_launches() - before == 2 * n, (J, n)
        ens.md_batch = 0
        before = ens.md_launches()
        ens.md_steps(3)
        assert ens.md_launches() == before
        with pytest.raises(M.MdqtError, match="mode must be 0"):
            ens.md_batch = 2
        assert ens.md_batch == 0


def test_kernel_times_report_the_batched_launches(M):
    N = 100
    with M.MonteCarloEnsemble(2, md_batch=1, **params(N, collisionFreq=0)) as ens:
        start(ens.jobs, N)
        ens.enable_timing(True)
        ens.md_steps(4)
        t = ens.kernel_times()
        assert t["n_md_force"] == 4 and t["n_md_vv"] == 4 and t["n_anneal"] == 0
        for k in ("md_force", "md_vv"):
            assert 0 < t[k + "_min_ms"] <= t[k + "_median_ms"] <= t[k + "_max_ms"] <= t[k + "_ms"]
        assert list(t["stage_ms"]) == list(ens.STAGES)
        assert ens.kernel_times()["n_md_force"] == 0     # reset


# ---- 4. run(): the batched observables, every stage and file ----
@pytest.mark.parametrize("N", [125, 1331])
def test_run_writes_the_same_files_in_both_modes_and_alone(M, tmp_path, N):
    J = 3
    for mode in (1, 0):
        with M.MonteCarloEnsemble(J, md_batch=mode, N=N, saveDirectory=f"{tmp_path}/mode{mode}/", **RUN) as ens:
            before = ens.md_launches()
            ens.run()
            assert (ens.md_launches() > before) == (mode == 1)
    for m in alone(M, J, N=N, saveDirectory=f"{tmp_path}/alone/", **RUN):
        m.run()
        m.close()
    t1, t0, ta = tree(tmp_path / "mode1"), tree(tmp_path / "mode0"), tree(tmp_path / "alone")
    assert sorted(t1) == sorted(t0) == sorted(ta) and len(t1) > 3 * 12
    assert any("pairPairCorrStepNum100.dat" in p for p in t1)        # a g(r) inside the recorded stage
    for p in t1:
        assert t1[p] == t0[p] == ta[p], p


def test_qt_tagging_run_in_both_modes(M, tmp_path):
    for mode in (1, 0):
        with M.MonteCarloEnsemble(2, md_batch=mode, saveDirectory=f"{tmp_path}/mode{mode}/", **QTT_RUN) as ens:
            ens.run()
            assert (ens.md_launches() > 0) == (mode == 1)            # its pre-record stage only
    t1, t0 = tree(tmp_path / "mode1"), tree(tmp_path / "mode0")
    assert sorted(t1) == sorted(t0) and len(t1) > 20
    for p in t1:
        assert t1[p] == t0[p], p


# ---- 5. the command line ----
def test_cli_md_batch(M, tmp_path):
    from mdqtplasmasims_amd._lib import MDMC_CLI_PATH
    cfg = {k: v for k, v in RUN.items() if k not in ("job", "seed")}
    for mode in (1, 0):
        r = subprocess.run([MDMC_CLI_PATH, "1", "--njobs=2", f"--md_batch={mode}", "--seed=9", "--quiet=1", "--device=0",
                            "--N=125", f"--saveDirectory={tmp_path}/mode{mode}/", *[f"--{k}={v}" for k, v in cfg.items()]],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout == "", (r.stdout, r.stderr)
    r = subprocess.run(["diff", "-r", f"{tmp_path}/mode1", f"{tmp_path}/mode0"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stdout[:2000]
    assert len(tree(tmp_path / "mode1")) > 2 * 12
