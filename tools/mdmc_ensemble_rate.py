#!/usr/bin/env python3
"""Rates of the MC + MD ensemble (docs/PROGRAMS.md, "Ensembles of the MC + MD programs").  One process, one GPU.

    python tools/mdmc_ensemble_rate.py anneal [--jobs 1,8,64,256]
        the batched anneal launch (N = 4096, force_kernel 1, 10,000 steps per launch): 20 launches after 5
        warm-ups, from the launches' own timestamps: median (min-max), us per step, ratio to the first J,
        chain-steps/s summed over the jobs
    python tools/mdmc_ensemble_rate.py single
        25 single-job launches of 10,000 steps at N = 4096 (--N: another perfect cube; mdmc_monte_carlo; host wall time per call).  Run it
        under `rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 ...` for the kernels' own
        timestamps, with MDQT_LIB naming another build of the library to compare two builds
    python tools/mdmc_ensemble_rate.py trace DIR
        the k_monte_carlo_lds dispatches of such a trace: the 20 after the first 5, median (min-max)
    python tools/mdmc_ensemble_rate.py e2e --bin A/bin/mdmc --seq-bin B/bin/mdmc --njobs 8 [--qt_model 2] [--runs 3]
        wall clock with process start of `mdmc 1 --njobs=J --seed=777 --quiet=1` (build A) against J sequential
        `mdmc k --seed=777+k-1 --quiet=1` (build B), and `diff -r` of the two trees; --no-seq: the ensemble only; --plain: build A without --njobs (J = 1);
        --keep DIR keeps the last ensemble tree, --same-as DIR compares it with one kept before (another build or --md_batch)
    python tools/mdmc_ensemble_rate.py stages --njobs 8 [--qt_model 2] [--md_batch 1]
        wall time by stage of one ensemble run (host timers around the stage helpers); with --md_batch 1 also the
        batched force and velocity-Verlet launches' own time and, with --qt_model, the batched QT launches' and the
        X distribution's chunk kernel's
    python tools/mdmc_ensemble_rate.py md [--jobs 1,8,64] [--md_batch 0|1] [--steps 300]
        the MD step of the ensemble (N = 4096, force_kernel 1, collisionless, after 2,000 Metropolis steps): wall us
        per ensemble step of one md_steps(--steps) call after a warm-up call of 50; with --md_batch 1 also, from a
        second call with timing on, the batched force and velocity-Verlet launches' own median (min-max) and the force launch's FP64 roof
        fraction (30 flop x N(N-1)/2 per member against 78.6 TF).  Without --md_batch the switch is left alone
        (MDQT_LIB naming a build that predates it).  e2e and stages take --md_batch too
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS, WARM, REPS = 10000, 5, 20


def cmd_anneal(a):
    import mdqtplasmasims_amd as M
    rows = []
    for J in [int(x) for x in a.jobs.split(",")]:
        with M.MonteCarloEnsemble(J, N=4096, force_kernel=1, numVelAutoCorrsSteps=8, seed=777, job=1) as e:
            e.init()
            e.enable_timing(True)
            for _ in range(WARM):
                e.monte_carlo(STEPS)
            e.kernel_times()
            for _ in range(REPS):
                e.monte_carlo(STEPS)
            t = e.kernel_times()
        assert t["n_anneal"] == REPS, t
        rows.append(dict(J=J, median_ms=t["anneal_median_ms"], min_ms=t["anneal_min_ms"], max_ms=t["anneal_max_ms"]))
    for r in rows:
        r["us_per_step"] = r["median_ms"] * 1e3 / STEPS
        r["ratio"] = r["median_ms"] / rows[0]["median_ms"]
        r["chain_steps_per_s"] = r["J"] * STEPS / (r["median_ms"] * 1e-3)
        print("J = {J:4d}: {median_ms:8.3f} ms ({min_ms:.3f}-{max_ms:.3f})  {us_per_step:6.3f} us/step  x{ratio:5.3f}  "
              "{chain_steps_per_s:.4g} chain-steps/s".format(**r))
    print(json.dumps({"anneal": rows}))


def cmd_single(a):
    from mdqtplasmasims_amd._lib import LIB_PATH
    from mdqtplasmasims_amd.mdmc import MonteCarloMD
    with MonteCarloMD(N=a.N, force_kernel=1, numVelAutoCorrsSteps=8, seed=777, job=1) as s:
        s.init()
        ms = []
        for _ in range(WARM + REPS):
            t0 = time.perf_counter()
            s.monte_carlo(STEPS)
            ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[WARM:]
    print(json.dumps({"single_host_ms": dict(lib=LIB_PATH, N=a.N, median=statistics.median(ms), min=min(ms), max=max(ms))}))


def cmd_trace(a):
    files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {a.dir}")
    d = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "k_monte_carlo_lds" in r["Kernel_Name"]:
                d.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    ms = [x for _, x in sorted(d)][WARM:WARM + REPS]
    if len(ms) != REPS:
        sys.exit(f"{len(d)} anneal dispatches in the trace, need {WARM + REPS}")
    print(json.dumps({"single_kernel_ms": dict(dir=a.dir, median=statistics.median(ms), min=min(ms), max=max(ms),
                                               us_per_step=statistics.median(ms) * 1e3 / STEPS)}))


MD_N, MD_WARM, ROOF_TF = 4096, 50, 78.6


def cmd_md(a):
    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd._lib import LIB_PATH
    rows = []
    for J in [int(x) for x in a.jobs.split(",")]:
        with M.MonteCarloEnsemble(J, md_batch=a.md_batch, N=MD_N, force_kernel=1, collisionFreq=0, numVelAutoCorrsSteps=8,
                                  seed=777, job=1) as e:
            e.init()
            e.monte_carlo(2000)
            e.md_steps(MD_WARM)
            t0 = time.perf_counter()
            e.md_steps(a.steps)                          # the wall window: timing off, no events on the launches
            wall = time.perf_counter() - t0
            r = dict(J=J, md_batch=a.md_batch, steps=a.steps, us_per_step=wall * 1e6 / a.steps,
                     us_per_member_step=wall * 1e6 / a.steps / J)
            if a.md_batch == 1:                          # a second window for the launches' own timestamps
                e.enable_timing(True)
                e.md_steps(a.steps)
            if a.md_batch == 1:
                t = e.kernel_times()
                assert t["n_md_force"] == a.steps and t["n_md_vv"] == a.steps, t
                flop = 30. * MD_N * (MD_N - 1) / 2 * J
                r.update(force_us=[t["md_force_median_ms"] * 1e3, t["md_force_min_ms"] * 1e3, t["md_force_max_ms"] * 1e3],
                         vv_us=[t["md_vv_median_ms"] * 1e3, t["md_vv_min_ms"] * 1e3, t["md_vv_max_ms"] * 1e3],
                         force_roof=flop / (t["md_force_median_ms"] * 1e-3) / (ROOF_TF * 1e12))
        rows.append(r)
        print("J = {J:3d} md_batch {md_batch}: {us_per_step:9.1f} us / ensemble step  {us_per_member_step:7.2f} us / member-step".format(**r)
              + ("  force {0[0]:.1f} ({0[1]:.1f}-{0[2]:.1f}) us  vv {1[0]:.1f} ({1[1]:.1f}-{1[2]:.1f}) us  roof {2:.3f}".format(
                  r["force_us"], r["vv_us"], r["force_roof"]) if a.md_batch == 1 else ""))
    print(json.dumps({"md": dict(lib=LIB_PATH, rows=rows)}))


def timed(cmd, limit):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return time.perf_counter() - t0


def cmd_e2e(a):
    more = [f"--qt_model={a.qt_model}"] if a.qt_model else []
    batch = [f"--md_batch={a.md_batch}"] if a.md_batch is not None and not a.plain else []
    work = tempfile.mkdtemp(prefix="mdmc_e2e_")
    res = dict(bin=a.bin, njobs=a.njobs, qt_model=a.qt_model, md_batch=a.md_batch, ens_s=[], seq_s=[])
    try:
        for _ in range(a.runs):
            shutil.rmtree(work + "/ens", ignore_errors=True)
            res["ens_s"].append(timed([a.bin, "1"] + ([] if a.plain else [f"--njobs={a.njobs}"]) + ["--seed=777", "--quiet=1",
                                       f"--saveDirectory={work}/ens/"] + more + batch, a.limit))
        for _ in range(0 if a.no_seq else a.runs):
            shutil.rmtree(work + "/seq", ignore_errors=True)
            tot = 0.
            for k in range(a.njobs):
                tot += timed([a.seq_bin or a.bin, str(1 + k), f"--seed={777 + k}", "--quiet=1",
                              f"--saveDirectory={work}/seq/"] + more, a.limit)
            res["seq_s"].append(tot)
        if not a.no_seq:
            r = subprocess.run(["diff", "-r", work + "/ens", work + "/seq"], capture_output=True, text=True)
            res["diff_r_identical"] = r.returncode == 0 and r.stdout == ""
            res["files"] = sum(len(f) for _, _, f in os.walk(work + "/ens"))
            res["done"] = max(res["ens_s"]) < min(res["seq_s"]) and res["diff_r_identical"]
        if a.same_as:                                    # the tree of another build or mode, kept by its --keep
            r = subprocess.run(["diff", "-r", work + "/ens", a.same_as], capture_output=True, text=True)
            res["same_as"] = dict(tree=a.same_as, identical=r.returncode == 0 and r.stdout == "")
        if a.keep:
            shutil.rmtree(a.keep, ignore_errors=True)
            shutil.move(work + "/ens", a.keep)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps({"e2e": res}))


def cmd_stages(a):
    import mdqtplasmasims_amd as M
    work = tempfile.mkdtemp(prefix="mdmc_stages_")
    try:
        kw = dict(qt_model=a.qt_model) if a.qt_model else {}
        with M.MonteCarloEnsemble(a.njobs, md_batch=a.md_batch, seed=777, job=1, saveDirectory=work + "/", **kw) as e:
            e.enable_timing(True)
            t0 = time.perf_counter()
            e.run()
            wall = time.perf_counter() - t0
            t = e.kernel_times()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    res = dict(njobs=a.njobs, qt_model=a.qt_model, md_batch=a.md_batch, run_s=wall, stage_ms=t["stage_ms"],
               anneal_launch_ms=t["anneal_ms"], n_anneal=t["n_anneal"])
    if a.md_batch == 1:
        res.update(md_force_ms=t["md_force_ms"], n_md_force=t["n_md_force"], md_force_median_us=t["md_force_median_ms"] * 1e3,
                   md_vv_ms=t["md_vv_ms"], n_md_vv=t["n_md_vv"], md_vv_median_us=t["md_vv_median_ms"] * 1e3)
        if a.qt_model:                                   # zeros from a build that predates the batched QT stages
            res.update(qt_ms=t["qt_ms"], n_qt=t["n_qt"], qt_median_us=t["qt_median_ms"] * 1e3,
                       qt_dist_ms=t["qt_dist_ms"], n_qt_dist=t["n_qt_dist"], qt_dist_median_us=t["qt_dist_median_ms"] * 1e3)
    print(json.dumps({"stages": res}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("anneal"); p.add_argument("--jobs", default="1,8,64,256"); p.set_defaults(f=cmd_anneal)
    p = sub.add_parser("single"); p.add_argument("--N", type=int, default=4096); p.set_defaults(f=cmd_single)
    p = sub.add_parser("trace"); p.add_argument("dir"); p.set_defaults(f=cmd_trace)
    p = sub.add_parser("e2e")
    p.add_argument("--bin", required=True); p.add_argument("--seq-bin"); p.add_argument("--njobs", type=int, default=8)
    p.add_argument("--qt_model", type=int, default=0); p.add_argument("--runs", type=int, default=3)
    p.add_argument("--no-seq", action="store_true"); p.add_argument("--plain", action="store_true")
    p.add_argument("--limit", type=float, default=300.); p.add_argument("--md_batch", type=int, choices=[0, 1])
    p.add_argument("--keep"); p.add_argument("--same-as")
    p.set_defaults(f=cmd_e2e)
    p = sub.add_parser("stages"); p.add_argument("--njobs", type=int, default=8)
    p.add_argument("--qt_model", type=int, default=0); p.add_argument("--md_batch", type=int, choices=[0, 1])
    p.set_defaults(f=cmd_stages)
    p = sub.add_parser("md"); p.add_argument("--jobs", default="1,8,64"); p.add_argument("--md_batch", type=int, choices=[0, 1])
    p.add_argument("--steps", type=int, default=300); p.set_defaults(f=cmd_md)
    a = ap.parse_args()
    a.f(a)


if __name__ == "__main__":
    main()
