"""The SpeedUp ensemble's pooled output() (include/mdqt.h "Pooled output()": the options pool and member_files,
mdqt_ensemble_pool_observables, mdqt --pool / --member_files) against a Python restatement of its definitions on the
members' published values: every number array_equal, every file's text equal, no tolerances.  The one bound is the
independent check of the slot sums against math.fsum: sum_bound(n, 0, sum|t|) of tests/obs_truth.py (n terms in any
order, no roundings of their own).  Member sizes are the CPU oracle's init()."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import obs_truth
from tests.ensemble_helpers import assert_same, snapshot, tree

pytestmark = pytest.mark.gpu

SEED = dict(seed=501, job=1, rng_mode=1)
SMALL = dict(N0=62, **SEED)
SMALL_N = [64, 64, 62]                      # one and two KDE chunks, a ragged tile
LARGE = dict(N0=300, **SEED)
LARGE_N = [288, 299, 313]                   # 9 chunks of 32 / 34 / 35 ions: chunk ends inside the 256-ion staging
SLOTS = 1002
NBINS = 2001
POOL_FILES = sorted(["energies.dat", "energies_sem.dat", "populations.dat", "vel_distX_time%06d.dat", "vel_distY_time%06d.dat",
                     "vel_distZ_time%06d.dat", "statePopulationsVsV_time%06d.dat"])


@pytest.fixture(scope="module")
def M():
    import mdqtplasmasims_amd as M
    return M


def scan(M, params, replicas, scheme=None, **kw):
    """2 points (detuningDP 0 / 1) x `replicas`, on the batched pass"""
    e = M.Ensemble(njobs=replicas, sweep={"detuningDP": [0.0, 1.0]}, **dict(params, **kw))
    if scheme is not None:
        e.set_option("force_scheme", scheme)
    e.set_option("output_batch", 1)
    return e


# ---- the restatement: the definitions of include/mdqt.h on the members' published values ----
def slots_of(vx):
    r = np.rint(vx * 100.0)
    with np.errstate(invalid="ignore"):
        inside = np.abs(r) <= 500                    # NaN: False
    return np.where(inside, 500 + np.where(inside, r, 0.0), SLOTS - 1).astype(np.int64)


def restate_rows(rows):
    R = len(rows)
    mean, sem = [float(rows[0][0])], []
    for c in range(1, 7):
        s = 0.0
        for r in range(R):
            s = s + float(rows[r][c])
        m = s / float(R)
        ss = 0.0
        for r in range(R):
            d = float(rows[r][c]) - m
            ss = ss + d * d
        mean.append(m)
        sem.append(math.sqrt(ss / (float(R) * float(R - 1))) if R > 1 else 0.0)
    return np.array(mean), np.array(sem)


def restate_member_slots(vx, pops):
    """a member's slot sums: its KDE chunks, each chunk's ions in ascending order onto 0, the chunks in ascending order onto 0"""
    N = len(vx)
    nch = min(max(N // 32, 1), 512)
    chunk = -(-N // nch)
    slot = slots_of(vx)
    cnt, tot = np.zeros(SLOTS, dtype=np.int64), np.zeros((3, SLOTS))
    for z in range(nch):
        c, s = np.zeros(SLOTS, dtype=np.int64), np.zeros((3, SLOTS))
        for i in range(z * chunk, min(N, (z + 1) * chunk)):
            c[slot[i]] += 1
            s[:, slot[i]] = s[:, slot[i]] + pops[i]
        cnt, tot = cnt + c, tot + s
    return cnt, tot


def restate(e, replicas):
    """pool_observables() from e.observables() and the members' vx"""
    obs = e.observables()
    vx = [j.get_state()["V"][0] for j in e.jobs]
    P = len(e.jobs) // replicas
    out = dict(mean7=np.zeros((P, 7)), sem6=np.zeros((P, 6)), Pvel=np.zeros((P, 3, NBINS)), count=np.zeros((P, SLOTS), dtype=np.int64),
               spd=np.zeros((P, 3, SLOTS)))
    terms = [[[] for _ in range(SLOTS)] for _ in range(P)]      # the slots' terms (S, P, D rows), for the order-free check
    for q in range(P):
        members = range(q * replicas, (q + 1) * replicas)
        out["mean7"][q], out["sem6"][q] = restate_rows([obs[k][0] for k in members])
        for k in members:
            assert np.isfinite(vx[k]).all() and np.isfinite(obs[k][2]).all(), f"job index {k}: a non-finite velocity or population"
            out["Pvel"][q] = out["Pvel"][q] + obs[k][1]
            cnt, tot = restate_member_slots(vx[k], obs[k][2])
            out["count"][q] = out["count"][q] + cnt
            out["spd"][q] = out["spd"][q] + tot
            for i, b in enumerate(slots_of(vx[k])):
                terms[q][b].append(obs[k][2][i])
    return out, terms


def assert_pooled_equal(got, want, what):
    assert sorted(got) == sorted(want) == ["Pvel", "count", "mean7", "sem6", "spd"]
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs"        # a NaN on either side fails this


def assert_slot_sums_within_bound(got, terms, what):
    for q, point in enumerate(terms):
        for b, t in enumerate(point):
            assert got["count"][q, b] == len(t), (what, q, b)
            if not t:
                assert np.array_equal(got["spd"][q, :, b], np.zeros(3)), (what, q, b)
                continue
            t = np.array(t)
            for c in range(3):
                exact = math.fsum(t[:, c])
                B = obs_truth.sum_bound(len(t), 0, obs_truth.LD(math.fsum(np.abs(t[:, c]))))
                assert abs(obs_truth.LD(got["spd"][q, c, b]) - obs_truth.LD(exact)) <= B, (what, q, b, c)


# ---- 1. the restatement, bit for bit ----
@pytest.mark.parametrize("params, scheme, sizes", [(SMALL, 2, SMALL_N), (LARGE, None, LARGE_N)])
def test_pool_observables_restated(M, params, scheme, sizes):
    with scan(M, params, 3, scheme) as e:
        e.init()
        e.md_steps(3)                                            # psi non-trivial, force slots pending
        assert e.N == sizes + sizes                              # the points share job and seed
        n0 = e.output_launches
        got = e.pool_observables()
        assert e.output_launches == n0 + 8
        again = e.pool_observables()
        want, terms = restate(e, 3)
        assert_pooled_equal(got, want, "pool_observables()")
        assert_pooled_equal(again, got, "the second call")
        assert_slot_sums_within_bound(got, terms, "pool_observables()")
        assert list(got["count"].sum(axis=1)) == [sum(sizes)] * 2
        assert np.isfinite(got["spd"]).all() and np.isfinite(got["mean7"]).all() and np.isfinite(got["Pvel"]).all()
        assert not np.array_equal(got["spd"][0], got["spd"][1])          # the points' populations differ after three MD steps
        assert (got["sem6"] > 0).all() and got["count"][:, :SLOTS - 1].sum() > 0


# ---- 2. crafted velocities ----
def test_crafted_velocities(M):
    edges = [(s - 500) / 100.0 for s in (255, 256, 511, 512, 767, 768, 1000, 0)]
    ties = [0.125, 0.375, -0.125, -0.375, 0.625, 0.875] + [(b + 0.5) / 100.0 for b in (2, 3, -2, -3, 254, 255, 499, -500)]
    rim = [5.0, -5.0, 5.01, -5.01, 5.0049, 5.0051, 5.005, -5.005, np.nextafter(5.005, 0.0), np.nextafter(5.005, 10.0),
           np.nextafter(-5.005, 0.0), np.nextafter(-5.005, -10.0)]
    crafted = np.array(edges + ties + [-0.0, 0.0] + rim)
    expect = {0.125: 512, 0.375: 538, -0.125: 488, -0.375: 462, 0.625: 562, 0.875: 588, -0.0: 500, 5.0: 1000, -5.0: 0,
              5.01: 1001, -5.01: 1001, 5.0051: 1001, 5.0049: 1000}          # exact products: round half to even
    s = slots_of(crafted)
    for v, b in expect.items():
        assert s[list(crafted).index(v)] == b, v
    assert set((255, 256, 511, 512, 767, 768, 1000, 0)) <= set(s)
    with M.Ensemble(njobs=3, **SMALL) as e:
        e.set_option("force_scheme", 2)
        e.set_option("output_batch", 1)
        e.init()
        e.md_steps(3)
        assert e.N == SMALL_N
        for k, j in enumerate(e.jobs):
            st = j.get_state()
            V = st["V"].copy()
            if k == 0:
                V[0, :len(crafted)] = crafted
            else:
                V[0, :] = 0.5 if k == 1 else 7.0             # every ion in slot 550; every ion outside
            j.set_state(st["R"], V, st["psi"], st["tPart"], st["t"])
        got = e.pool_observables()
        want, terms = restate(e, 3)
        assert_pooled_equal(got, want, "crafted velocities")
        assert_slot_sums_within_bound(got, terms, "crafted velocities")
        pops = e.observables()
        assert got["count"][0].sum() == sum(SMALL_N)
        s0 = slots_of(e.jobs[0].get_state()["V"][0])        # the crafted ions and the replica's other 28
        assert int((s0 == SLOTS - 1).sum()) >= int((s == SLOTS - 1).sum()) >= 5
        assert got["count"][0, SLOTS - 1] == 62 + int((s0 == SLOTS - 1).sum())
        own = int((s0 == 550).sum())
        assert got["count"][0, 550] == 64 + own
        if own == 0:                                         # the one-slot replica's sums: its ions in one chunk order
            assert np.array_equal(got["spd"][0, :, 550], restate_member_slots(np.full(64, 0.5), pops[1][2])[1][:, 550])
        for b in (255, 256, 511, 512, 767, 768, 1000, 0, 500):
            assert got["count"][0, b] >= 1, b


# ---- 3., 4. members untouched; the pooled files ----
def fmt(*cols):
    return "\t".join("%g" % c for c in cols) + "\n"


def pooled_text(p, q, counter):
    """the pooled files of point q from pool_observables()'s values: name -> text"""
    m, se, cnt, spd = p["mean7"][q], p["sem6"][q], p["count"][q], p["spd"][q]
    total, tot = 0, [0.0, 0.0, 0.0]
    for b in range(SLOTS):
        total += int(cnt[b])
        for c in range(3):
            tot[c] = tot[c] + float(spd[c, b])
    vel = [float(j) * 0.0025 for j in range(NBINS)]
    out = {"energies.dat": fmt(*m), "energies_sem.dat": fmt(m[0], *se),
           "populations.dat": fmt(m[0], tot[0] / float(total), tot[1] / float(total), tot[2] / float(total), float(total),
                                  float(cnt[SLOTS - 1]))}
    for a, axis in enumerate("XYZ"):
        shift = float(m[6]) if a == 0 else 0.0
        out["vel_dist%s_time%06d.dat" % (axis, counter)] = "".join(fmt(vel[j] + shift, p["Pvel"][q, a, j]) for j in range(NBINS))
    out["statePopulationsVsV_time%06d.dat" % counter] = "".join(
        fmt(float(b - 500) * 0.01, float(cnt[b]), *[(float(spd[c, b]) / float(cnt[b]) if cnt[b] else 0.0) for c in range(3)])
        for b in range(SLOTS - 1))
    return out


def test_members_untouched_and_pooled_files(M, tmp_path):
    rec = {}
    for pool in (0, 1):
        base = str(tmp_path / f"pool{pool}") + "/"
        with scan(M, SMALL, 3, 2, saveDirectory=base) as e:
            e.set_option("pool", pool)
            for j in e.jobs:
                j.setup_directories()
            e.init()
            e.md_steps(3)
            obs = e.observables()
            pooled = [e.pool_observables()]
            n0 = e.output_launches
            e.output()
            assert e.output_launches == n0 + (8 if pool else 6)
            e.md_steps(1)
            pooled.append(e.pool_observables())
            e.output()
            dirs = [e.pool_directory(q) for q in range(2)]
            e.md_steps(2)                                    # force slots pending across the passes stayed pending
            rec[pool] = dict(obs=obs, pooled=pooled, dirs=dirs, end=[snapshot(j) for j in e.jobs], tree=tree(base))
    a, b = rec[0], rec[1]
    for k in range(6):                                       # 3. the members: numbers, files, the state two MD steps on
        for x, y, what in zip(a["obs"][k], b["obs"][k], ("out7", "Pvel", "pops")):
            assert np.array_equal(x, y), (k, what)
        assert_same(a["end"][k], b["end"][k], f"job index {k}")
    assert_pooled_equal(a["pooled"][0], b["pooled"][0], "pool_observables() under pool 0 and 1")
    members = {f: t for f, t in b["tree"].items() if "/pool_job" not in "/" + f}
    assert sorted(members) == sorted(a["tree"]) and a["tree"]
    assert [f for f in members if members[f] != a["tree"][f]] == []
    assert not [f for f in a["tree"] if "pool_job" in f]
    for q in range(2):                                       # 4. the pooled files of the two outputs
        d = os.path.relpath(b["dirs"][q], str(tmp_path / "pool1"))
        assert d.endswith("/pool_job1to3") and ("DetDP%d" % (100 * q)) in d
        assert os.path.dirname(d) == os.path.dirname(os.path.dirname([f for f in members if f"DetDP{100 * q}O" in f][0]))
        files = {os.path.basename(f): t.decode() for f, t in b["tree"].items() if os.path.dirname(f) == d}
        assert sorted(files) == sorted({n % c if "%" in n else n for n in POOL_FILES for c in (0, 1)})
        first, second = pooled_text(b["pooled"][0], q, 0), pooled_text(b["pooled"][1], q, 1)
        for name in POOL_FILES:
            if "%" in name:
                assert files[name % 0] == first[name % 0], name % 0
                assert files[name % 1] == second[name % 1], name % 1
            else:                                            # appended: one line per output
                assert files[name] == first[name] + second[name], name
                assert files[name].count("\n") == 2


# ---- 5. member_files 0: run(), fresh and resumed ----
RUN = dict(LARGE, sampleFreq=10)


def test_member_files_0_run_and_resume(M, tmp_path):
    bases = {mf: str(tmp_path / f"mf{mf}") + "/" for mf in (1, 0)}

    def run(mf, **kw):
        with scan(M, RUN, 2, saveDirectory=bases[mf], **kw) as e:
            e.set_option("member_files", mf)
            e.set_option("pool", 1)
            e.run()
            assert e.N == LARGE_N[:2] * 2
            return [snapshot(j) for j in e.jobs], e.output_launches, [e.pool_directory(q) for q in range(2)]

    def pooled(t):
        return {f: x for f, x in t.items() if "/pool_job1to2/" in f}

    ends = {mf: run(mf, tmax=0.05) for mf in (1, 0)}
    counter, c0 = ends[0][0][0]["counter"], ends[0][0][0]["c0"]
    assert 2 <= counter <= 3
    assert ends[0][1] == ends[1][1] == 8 * counter
    for k in range(4):
        assert_same(ends[0][0][k], ends[1][0][k], f"job index {k} after run()")
    t1, t0 = tree(bases[1]), tree(bases[0])
    assert pooled(t1) and sorted(pooled(t1)) == sorted(pooled(t0))
    assert [f for f in pooled(t1) if pooled(t1)[f] != t0[f]] == []
    assert len(pooled(t1)) == 2 * (3 + 4 * counter)
    kinds = {os.path.basename(f).split("_")[0] for f in t0 if "/pool_job" not in f}
    assert kinds == {"conditions", "ions", "wvFns", "VZERO"}                     # writeConditions' files only
    assert {f for f in t1 if "/pool_job" not in f} > {f for f in t0 if "/pool_job" not in f}
    assert [f for f in t0 if "/pool_job" not in f and t0[f] != t1[f]] == []
    before = {f: x for f, x in t0.items() if f.endswith("/pool_job1to2/energies.dat")}
    assert len(before) == 2 and all(x.count(b"\n") == counter for x in before.values())

    ends2 = {mf: run(mf, tmax=0.09, newRun=0, c0=c0) for mf in (1, 0)}           # resumed: appended to, not truncated
    counter2 = ends2[0][0][0]["counter"]
    assert counter2 > counter and ends2[0][0][0]["c0"] > c0
    for k in range(4):
        assert_same(ends2[0][0][k], ends2[1][0][k], f"job index {k} after the resumed run()")
    t1, t0 = tree(bases[1]), tree(bases[0])
    assert [f for f in pooled(t1) if pooled(t1)[f] != t0[f]] == [] and sorted(pooled(t1)) == sorted(pooled(t0))
    for f, x in before.items():
        assert t0[f][:len(x)] == x and t0[f].count(b"\n") == counter2
    for d in ends2[0][2]:
        assert os.path.isdir(d)


# ---- 6. launch counts ----
def test_launch_counts(M, tmp_path):
    with M.Ensemble(njobs=3, saveDirectory=str(tmp_path) + "/", **SMALL) as e:
        e.set_option("force_scheme", 2)
        e.set_option("output_batch", 1)
        e.init()
        e.md_steps(1)
        for j in e.jobs:
            j.setup_directories()
        e.enable_timing()
        seen = []
        for pool in (0, 1, 0, 1):
            e.set_option("pool", pool)
            n0 = e.output_launches
            e.output()
            seen.append(e.output_launches - n0)
        assert seen == [6, 8, 6, 8]
        t = e.output_kernel_times()
        assert t["n_potential"] == 4 and t["n_kde"] == 4 and t["n_popv"] == 2 and t["n_pool"] == 2
        assert 0 < t["popv_median_ms"] <= t["popv_ms"] and 0 < t["pool_median_ms"] <= t["pool_ms"]
        assert sorted(e.kernel_times()) == sorted(["force_ms", "n_force", "substep_ms", "n_substep", "force_median_ms",
                                                   "substep_median_ms"])
        for name in ("pool", "member_files"):
            with pytest.raises(M.MdqtError, match=name):
                e.set_option(name, 2)


# ---- 7. refusals ----
MID_FROM_2 = dict(N0=120, seed=502, job=2, rng_mode=1)      # 136, 119, 128 ions: job index 1 on the owner-computes rows


def test_refusals(M, tmp_path):
    with M.Ensemble(njobs=3, saveDirectory=str(tmp_path) + "/", **MID_FROM_2) as e:
        for j in e.jobs:
            j.setup_directories()
        e.init()
        e.md_steps(1)
        assert e.N == [136, 119, 128]
        e.set_option("pool", 1)
        n0 = e.output_launches
        for call in (e.output, e.pool_observables):                          # output_batch 0 (the default)
            with pytest.raises(M.MdqtError, match=r"output_batch 1"):
                call()
        e.set_option("output_batch", 1)
        for call in (e.output, e.pool_observables):
            with pytest.raises(M.MdqtError, match=r"job index 1 has 119 ions on the owner-computes rows: set force_scheme 2"):
                call()
        e.set_option("pool", 0)
        e.set_option("member_files", 0)
        with pytest.raises(M.MdqtError, match=r"member_files 0 with pool 0"):
            e.output()
        assert e.output_launches == n0 and tree(tmp_path) == {}              # no launch, no file
        assert [j.counters()["counter"] for j in e.jobs] == [0, 0, 0]
        e.set_option("member_files", 1)
        e.set_option("pool", 1)
        e.set_option("force_scheme", 2)                                      # the same ensemble pools
        got = e.pool_observables()
        want, _ = restate(e, 3)
        assert_pooled_equal(got, want, "after force_scheme 2")
        n1 = e.output_launches
        e.output()
        assert e.output_launches == n1 + 8
        assert sorted(os.listdir(e.pool_directory(0))) == sorted(n % 0 if "%" in n else n for n in POOL_FILES)
        assert e.pool_directory(0).endswith("/pool_job2to4/")


def test_pump_ensemble_refuses_the_options(M):
    with M.PumpEnsemble(2, pump_program=1, N0=300, seed=5, job=2, rng_mode=1) as e:
        for name in ("pool", "member_files"):
            for v in (0, 1):
                with pytest.raises(M.MdqtError, match=name + r" is an option of the SpeedUp ensemble"):
                    e.set_option(name, v)


# ---- 8. the command line ----
def test_cli_pool(M, tmp_path):
    def run(name, *args):
        r = subprocess.run([M.CLI_PATH, "1", "--njobs=2", "--sweep=detuningDP:0,1", "--N0=300", "--tmax=0.05", "--sampleFreq=10",
                            "--seed=501", f"--saveDirectory={tmp_path}/{name}/", *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == [str(n) for n in LARGE_N[:2] * 2]
        return tree(tmp_path / name)

    plain, pooled, only = run("plain"), run("pool", "--pool=1"), run("only", "--pool=1", "--member_files=0")
    pool_of = lambda t: {f: x for f, x in t.items() if "/pool_job1to2/" in f}
    rest_of = lambda t: {f: x for f, x in t.items() if "/pool_job" not in f}
    assert not pool_of(plain) and any("statePopulationsVsVTime" in f for f in plain)
    assert len({os.path.dirname(f) for f in pool_of(pooled)}) == 2
    assert {os.path.basename(f) for f in pool_of(pooled)} >= {"energies.dat", "energies_sem.dat", "populations.dat"}
    assert sorted(rest_of(pooled)) == sorted(plain) and [f for f in plain if plain[f] != pooled[f]] == []
    assert sorted(pool_of(only)) == sorted(pool_of(pooled)) and [f for f in pool_of(only) if only[f] != pooled[f]] == []
    assert not any("statePopulationsVsVTime" in f or "vel_dist" in os.path.basename(f) or f.endswith("/energies.dat")
                   for f in rest_of(only))
