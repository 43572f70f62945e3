"""Every context and ensemble gives back the device and pinned memory it took: mdqt_live_bytes(0 / 1) (the bytes
mdqt_devbuf.hpp's buffers hold, process-wide) is above its start value while an object lives and back at it once
the object is destroyed.  The counters are the library's own, so other work on the device does not move them.
Each case creates, uses once the paths that allocate, and destroys; no case forces an allocation failure (that
path: tests/test_devbuf.py)."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as m
    if m.device_count() < 1:
        pytest.skip("no GPU")
    return m


def live():
    from mdqtplasmasims_amd._lib import lib
    return lib().mdqt_live_bytes(0), lib().mdqt_live_bytes(1)


@contextlib.contextmanager
def returned():
    """the body's objects are destroyed by its end: both counters are then where they were"""
    start = live()
    yield start
    assert live() == start, (live(), start)


def held(start, pinned=True):
    """an object lives: device bytes (and pinned ones) above the start value; returns the counters"""
    now = live()
    assert now[0] > start[0] and (now[1] > start[1] if pinned else now[1] >= start[1]), (now, start)
    return now


def state_of(s, N, seed=3):
    """a state of N ions in s's box for set_state"""
    g = np.random.default_rng(seed)
    psi = np.zeros((N, 12, 2))
    psi[:, 0, 0] = 1.
    return g.uniform(0., s.const("L"), (3, N)), g.normal(0., 0.01, (3, N)), psi, np.zeros(N), 0.


def test_counter_arguments():
    from mdqtplasmasims_amd._lib import lib
    assert lib().mdqt_live_bytes(2) == -1 and lib().mdqt_live_bytes(-1) == -1


def test_mdqt_context_resized_both_ways(M):
    with returned() as start:
        s = M.Simulation(N0=200, seed=12346, rng_mode=1).init()
        s.md_steps(1)
        small = held(start)
        s.set_state(*state_of(s, 700))                 # S != capS: everything sized by it is allocated anew
        s.md_steps(1)
        big = held(start)
        assert big[0] > small[0]
        s.set_state(*state_of(s, 200))                 # ... and again on the way down
        s.md_steps(1)
        assert held(start)[0] < big[0]
        s.close()


def test_mdqt_context_overlapped_step(M):
    with returned() as start:
        s = M.Simulation(N0=200, seed=12346, rng_mode=1).init()
        plain = held(start)
        s.set_option("overlap", 1)                     # dArrive, the QT stream and its events
        s.md_steps(1)
        assert held(start)[0] > plain[0]
        s.close()


def test_mdqt_context_drand48_order(M):
    with returned() as start:
        s = M.Simulation(N0=200, seed=12346, rng_mode=0).init()   # dX48, dU
        s.md_steps(1)
        held(start)
        s.close()


def test_mdqt_context_block_scheme(M):
    with returned() as start:
        s = M.Simulation(N0=66000, seed=7, rng_mode=1)
        s.set_state(*state_of(s, 66000))               # just above the 65,536 switch to the blocks
        assert s.const("force_scheme") == 3
        before = held(start)
        s.forces()                                     # the sort buffers, boxes, plan, slots and tail arrays
        s.Epotential()
        assert held(start)[0] > before[0]
        s.close()


def test_mdqt_rank_group(M):
    from mdqtplasmasims_amd.engine import comm_init_local
    with returned() as start:
        st = M.Simulation(N0=400, seed=9).init().get_state()
        assert live() == start                         # (that one went at once)
        sims = [M.Simulation(world_size=2, rank=r, N0=400, seed=9) for r in range(2)]
        for s in sims:
            s.set_option("force_scheme", 3)            # the blocks: dFr, and dPeerParts for the group's sum
            s.set_state(st["R"], st["V"], st["psi"], st["tPart"], st["t"])
        comm_init_local(sims)
        before = held(start)
        for s in sims:
            s.allgather_positions()
        for s in sims:
            s.forces()
        for s in sims:
            s.get_state()                              # settles the forces: the ranks' partials summed
        assert held(start)[0] > before[0]
        for s in sims:
            s.close()


PUMP = dict(N0=200, seed=5, job=2, rng_mode=1, tstartV0=0., tpumpreal=0., sampleFreq=1)


def test_pump_context_tag_buffers_regrow(M, tmp_path):
    """measureSpinUps() and output() run inside the program's main() only (mdqt_run_pump): a new run at N0 = 200
    tags and writes one output; a resumed context reads that run's files (200 ions), then the same files rewritten
    for 700 ions — readConditions and output() then regrow the tag array and the tagged distribution's partials"""
    base = str(tmp_path) + "/"
    with returned() as start:
        a = M.Simulation(pump_program=1, saveDirectory=base, tmax=0., **PUMP)
        a.run_pump()                                   # t = 0: measureSpinUps, output(), one step, writeConditions
        assert a.spin_up_list()[0].size == a.N
        held(start)
        c0, N, d = a.counters()["c0"], a.N, a.save_directory
        a.close()
        assert live() == start
        t0 = (c0 - 9) * 0.002 + 0.02                   # readConditions' t of step c0
        b = M.Simulation(pump_program=1, saveDirectory=base, newRun=0, c0=c0, tmax=t0 + 0.003, **PUMP)
        b.run_pump()
        assert b.N == N
        small = held(start)
        n, L, g = 700, b.const("L"), np.random.default_rng(1)
        with open(f"{d}ions_timestep{c0:06d}.dat", "w") as f:
            f.write(f"{n}\t0")
        with open(f"{d}spinUpIonsList_timestep{c0:06d}.dat", "w") as f:
            f.write("".join(f"{k % 2}\n" for k in range(n)))
        with open(f"{d}conditions_timestep{c0:06d}.dat", "w") as f:
            for r, v in zip(g.uniform(0., L, (n, 3)), g.normal(0., 0.01, (n, 3))):
                f.write("\t".join(f"{x:.17g}" for x in (*r, *v)) + "\t\n")
        b.run_pump()
        assert b.N == n and b.spin_up_list()[1] == n // 2
        assert held(start)[0] > small[0]
        b.close()


def test_mdqt_ensemble_batched_output(M, tmp_path):
    with returned() as start:
        e = M.Ensemble(njobs=2, saveDirectory=str(tmp_path) + "/", N0=62, seed=11, job=1, rng_mode=1)
        e.set_option("force_scheme", 2)
        e.set_option("output_batch", 1)
        e.init()
        e.md_steps(1)
        for j in e.jobs:
            j.setup_directories()
        before = held(start)
        e.output()
        assert e.output_launches == 6                  # the batched path: its blocks, rows and columns
        assert held(start)[0] > before[0]
        e.close()


def test_pump_ensemble_tagged_output(M, tmp_path):
    with returned() as start:
        e = M.PumpEnsemble(2, pump_program=1, saveDirectory=str(tmp_path) + "/", N0=200, seed=5, job=2, rng_mode=1)
        e.init()
        for j in e.jobs:
            j.setup_directories()
        e.md_steps(1)
        before = held(start)
        tags = e.tag_spin_up()
        assert all(t.size == n for (t, _), n in zip(tags, e.N))
        e.output()
        assert held(start)[0] > before[0]              # the members' tag arrays and distribution partials
        e.close()


def mc_state(c, seed=3):
    """positions in c's box and small velocities for MonteCarloMD.set_state (256 is no cube: init() has no lattice for it)"""
    g = np.random.default_rng(seed)
    N = int(c.const("N"))
    return g.uniform(0., c.const("L"), (3, N)), g.normal(0., 0.1, (3, N))


def test_mdmc_context_qt(M):
    from mdqtplasmasims_amd.mdmc import MonteCarloMD
    with returned() as start:
        c = MonteCarloMD(qt_model=1, N=256, numVelAutoCorrsSteps=1, seed=5)
        c.set_state(*mc_state(c))
        c.md_steps(1)
        held(start)
        c.close()


def test_mdmc_ensemble_batched_stretch(M):
    with returned() as start:
        e = M.MonteCarloEnsemble(2, md_batch=1, N=256, numVelAutoCorrsSteps=1, seed=5, job=1)
        for k, j in enumerate(e.jobs):
            j.set_state(*mc_state(j, seed=k))
        launches = e.md_launches()
        e.md_steps(2)                                  # one stretch
        assert e.md_launches() > launches
        held(start)
        e.close()


def test_mdlc_context(M):
    from mdqtplasmasims_amd import LaserCooling
    with returned() as start:
        c = LaserCooling(N0=100, njobs=2, device=0)
        c.init()
        c.qsteps(4)
        held(start)
        c.close()
