#!/usr/bin/env python3
"""Rate of an ensemble of MDQT jobs stepped in batched launches (mdqtplasmasims_amd.Ensemble) on one GPU,
against one Simulation alone and against k Simulations on k streams (the pattern of bench.py's
replicas_line, re-implemented here with the same synchronise placement: warm-up, synchronise, timed MD
steps issued from one host thread, synchronise).

Configs: c2 = N0 3500 full MDQT (bench.py's C2), n500 = N0 500 full MDQT.  Jobs k = 1 .. are seeded
12345 + k, job = k, as replicas_line seeds them, so the three patterns step the same systems.

Prints ONE JSON line:
  single:    the rate of job 1 alone, its two kernels' mean launch durations (event timestamps)
  streams:   per k in --streams: the aggregate rate of k Simulations round-robin on their own streams
  ensemble:  per J in --jobs: the aggregate wall-clock rate of one md_steps(--steps) call (timing off;
             value), of --steps calls of md_steps(1) (value_call_per_step: the argument blocks copied
             before every QT launch instead of ahead), then from a timed pass with the kernels' dispatch
             timestamps: median force / QT launch (us), and their FP64 roof
             fractions as the project counts them (QT 1,750 flop per particle-qstep, force 30 flop per
             pair, N (N - 1) / 2 pairs per job; against 78.6 TF)
Rates are particle-qsteps/s summed over the jobs.  Any error exits non-zero; there is no CPU fallback.
--sweep NAME:v1,v2 makes the ensembles sweep ensembles (parameter points x jobs, J members in all): one value times
the sweep QT kernels on the uniform ensemble's own jobs, two or more a scan of the same J.

--mode output measures output() of all members instead: per J in --jobs, --outputs outputs --every MD steps
apart after --skip uncounted ones, the wall time (ms, median / min / max over the outputs) of
  members_observables:  for j in e.jobs: j.observables()   each member's device pass and synchronisation, no files
  members_output:       for j in e.jobs: j.output()        ... and its files, formatted and flushed
and, where the library has the batched output (this is skipped under MDQT_LIB with an older build), for
output_batch 0 and 1: e.observables() and e.output() (files flushed inside), with the batched potential and
KDE launches' own median durations.  The observables / output pairs split an output into the device pass with
its synchronisations and the files' formatting.  --pool adds the pooled output (ensemble option pool 1 on the batched
pass): pool_observables (e.pool_observables(): the pooled pass, no files) and output_pool_files<m> (e.output() with
pool 1 and member_files m, for each m of --member-files), with the two pooled launches' own median durations beside
the KDE launch's.  --sweep applies here too (J members in all, J / points per point: the pooled pass pools each
point), and --paths keeps only the named paths.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12
QT_FLOP = 1750.0          # per particle-qstep
PAIR_FLOP = 30.0          # per evaluated pair
CONFIGS = {"c2": dict(N0=3500), "n500": dict(N0=500)}


def timed(step, sync, steps, warmup):
    for _ in range(warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    return time.perf_counter() - t0


def stats_ms(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2] * 1e3, min=xs[0] * 1e3, max=xs[-1] * 1e3)


def output_mode(M, a, params, jobs, out, sweep=None, npoints=1):
    """the wall time of one output() of all members, by path (see the module docstring)"""
    from mdqtplasmasims_amd._lib import lib
    batched = hasattr(lib(), "mdqt_ensemble_output")
    out["mode"] = "output"
    out["outputs"], out["every"], out["skip"] = a.outputs, a.every, a.skip
    out["output"] = []
    for J in jobs:
        paths = {"members_observables": (None, lambda e: [j.observables() for j in e.jobs]),
                 "members_output": (None, lambda e: [j.output() for j in e.jobs])}
        if batched:
            for ob in (0, 1):
                paths[f"observables_batch{ob}"] = (ob, lambda e: e.observables())
                paths[f"output_batch{ob}"] = (ob, lambda e: e.output())
        options = {}
        if a.pool:
            paths["pool_observables"] = (1, lambda e: e.pool_observables())
            for mf in a.member_files:
                paths[f"output_pool_files{mf}"] = (1, lambda e: e.output())
                options[f"output_pool_files{mf}"] = dict(pool=1, member_files=mf)
        if a.paths:
            unknown = [n for n in a.paths if n not in paths]
            if unknown:
                raise SystemExit(f"--paths: {unknown} not among {sorted(paths)}")
            paths = {n: paths[n] for n in a.paths}
        row = dict(jobs=J)
        for name, (ob, call) in paths.items():
            base = tempfile.mkdtemp(prefix="mdqt_output_")
            try:
                with (M.Ensemble(njobs=J // npoints, sweep=sweep, seed=12346, job=1, saveDirectory=base + "/", **params) if sweep
                      else M.Ensemble(njobs=J, seed=12346, job=1, saveDirectory=base + "/", **params)) as e:
                    if ob is not None:
                        e.set_option("output_batch", ob)
                    for option, v in options.get(name, {}).items():
                        e.set_option(option, v)
                    for j in e.jobs:
                        j.setup_directories()
                    e.init()
                    if ob == 1:
                        e.enable_timing(True)
                    ts = []
                    for k in range(a.skip + a.outputs):
                        e.md_steps(a.every)
                        e.synchronize()
                        t0 = time.perf_counter()
                        call(e)
                        ts.append(time.perf_counter() - t0)
                    row["N_total"] = sum(e.N)
                    row[name] = stats_ms(ts[a.skip:])
                    if ob == 1:
                        kt = e.output_kernel_times()
                        row[name]["potential_us"] = kt["potential_median_ms"] * 1e3
                        row[name]["kde_us"] = kt["kde_median_ms"] * 1e3
                        if kt.get("n_popv"):
                            row[name]["popv_us"] = kt["popv_median_ms"] * 1e3
                            row[name]["pool_us"] = kt["pool_median_ms"] * 1e3
            finally:
                shutil.rmtree(base, ignore_errors=True)
        out["output"].append(row)


def main():
    ap = argparse.ArgumentParser(formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c2")
    ap.add_argument("--jobs", default="1,2,4,8,16,32,64", help="ensemble sizes J")
    ap.add_argument("--streams", default="2,4,8", help="k of the k-streams pattern ('' = skip)")
    ap.add_argument("--steps", type=int, default=1000, help="timed MD steps (the window has to be long: a 100-step\n"
                    "window of one C2 job is 4 ms and measures the clock ramp as much as the kernels)")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--qt-waves", type=int, default=0, help="Ensemble option qt_waves (0, 3)")
    ap.add_argument("--sweep", action="append", default=[], metavar="NAME:v1,v2",
                    help="the ensembles are sweep ensembles (Ensemble(sweep=...)) of J members in all: the\n"
                    "points are the product of the lists (may be given per NAME), J / points jobs each; one value\n"
                    "= the sweep kernels on the uniform ensemble's jobs")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--mode", choices=["rate", "output"], default="rate")
    ap.add_argument("--outputs", type=int, default=25, help="--mode output: timed outputs")
    ap.add_argument("--every", type=int, default=40, help="--mode output: MD steps between outputs (sampleFreq)")
    ap.add_argument("--skip", type=int, default=5, help="--mode output: uncounted outputs first")
    ap.add_argument("--pool", action="store_true", help="--mode output: also the pooled output (option pool 1)")
    ap.add_argument("--member-files", default="1,0", help="--mode output --pool: the member_files values to measure")
    ap.add_argument("--paths", default="", help="--mode output: only these paths (comma-separated names of the result's keys)")
    ap.add_argument("--json", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd._sweep import parse_sweep_args
    params = dict(CONFIGS[a.config], device=a.device)
    jobs = [int(x) for x in a.jobs.split(",") if x]
    streams = [int(x) for x in a.streams.split(",") if x]
    try:
        sweep = parse_sweep_args(a.sweep)
    except ValueError as e:
        ap.error(str(e))
    npoints = 1
    for values in sweep.values():
        npoints *= len(values)
    a.member_files = [int(x) for x in a.member_files.split(",") if x]
    a.paths = [x for x in a.paths.split(",") if x]
    if any(J % npoints for J in jobs) and sweep:
        ap.error(f"--sweep: every J of --jobs must be a multiple of the {npoints} points")
    out = dict(tool="mdqt_ensemble_rate", config=a.config, steps=a.steps, warmup=a.warmup, qt_waves=a.qt_waves,
               unit="particle-qsteps/s", fp64_peak=FP64_PEAK)
    if sweep:
        out["sweep"] = sweep
    if a.mode == "output":
        output_mode(M, a, params, jobs, out, sweep, npoints)
        out["unit"] = "ms per output of all members"
        line = json.dumps(out)
        print(line)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                f.write(line + "\n")
        return

    # one Simulation alone
    with M.Simulation(seed=12346, job=1, **params) as s:
        s.init()
        ratio = int(s.const("plasmaToQuantumTimestepRatio"))
        el = timed(lambda: s.md_steps(1), s.synchronize, a.steps, a.warmup)
        s.enable_timing(1)
        timed(lambda: s.md_steps(1), s.synchronize, min(a.steps, 200), 0)
        kt = s.kernel_times()
        out["single"] = dict(N=s.N, ms_per_md_step=el / a.steps * 1e3, value=s.N * ratio * a.steps / el,
                             force_us=kt["force_ms"] / max(kt["n_force"], 1) * 1e3,
                             qt_us=kt["substep_ms"] / max(kt["n_substep"], 1) * 1e3)
    out["ratio"] = ratio

    # k Simulations on k streams, round-robin from this thread
    out["streams"] = []
    for k in streams:
        sims = [M.Simulation(seed=12345 + j, job=j, **params).init() for j in range(1, k + 1)]
        try:
            def step():
                for x in sims:
                    x.md_steps(1)

            def sync():
                for x in sims:
                    x.synchronize()
            el = timed(step, sync, a.steps, a.warmup)
            ntot = sum(x.N for x in sims)
        finally:
            for x in sims:
                x.close()
        out["streams"].append(dict(jobs=k, N_total=ntot, ms_per_md_step=el / a.steps * 1e3,
                                   value=ntot * ratio * a.steps / el))

    # the ensemble
    out["ensemble"] = []
    for J in jobs:
        with (M.Ensemble(njobs=J // npoints, sweep=sweep, seed=12346, job=1, **params) if sweep else
              M.Ensemble(njobs=J, seed=12346, job=1, **params)) as e:
            if a.qt_waves:
                e.set_option("qt_waves", a.qt_waves)
            e.init()
            # one md_steps call: the argument blocks of the steps are built ahead, one copy per <= 64 steps
            e.md_steps(a.warmup)
            el = timed(lambda: e.md_steps(a.steps), e.synchronize, 1, 0)
            # one call per MD step (the k-streams pattern's call shape): a copy before every QT launch
            el1 = timed(lambda: e.md_steps(1), e.synchronize, a.steps, 0)
            e.enable_timing(True)
            e.md_steps(min(a.steps, 200))
            kt = e.kernel_times()
            Ns = e.N
        ntot = sum(Ns)
        pairs = sum(n * (n - 1) / 2 for n in Ns)
        f_us, q_us = kt["force_median_ms"] * 1e3, kt["substep_median_ms"] * 1e3
        out["ensemble"].append(dict(
            jobs=J, N_total=ntot, ms_per_md_step=el / a.steps * 1e3, value=ntot * ratio * a.steps / el,
            value_call_per_step=ntot * ratio * a.steps / el1,
            force_us=f_us, qt_us=q_us, n_force=kt["n_force"], n_qt=kt["n_substep"],
            force_roof=(pairs * PAIR_FLOP / (f_us * 1e-6) / FP64_PEAK) if f_us > 0 else None,
            qt_roof=(ntot * ratio * QT_FLOP / (q_us * 1e-6) / FP64_PEAK) if q_us > 0 else None))

    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
