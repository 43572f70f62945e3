#!/usr/bin/env python3
"""Step times of an ensemble of optical-pumping jobs stepped in batched launches
(mdqtplasmasims_amd.PumpEnsemble) on one GPU, against the same jobs on contexts of their own — stepped one
after the other on one stream, and on a stream each — with the synchronise placement of
tools/mdqt_ensemble_rate.py: warm-up, synchronise, timed steps issued from one host thread, synchronise.

Job k = 0 .. J-1 has seed 777 + k and job 1 + k on every side, so the patterns step the same systems.  The
contexts' MD step is Simulation.pump_md_steps(1) — mdqt_run_pump's own step (four launches: half drift,
forces, slot sum, kick + half drift).

Prints ONE JSON line:
  md:      per J: wall us per MD-only step of all J jobs (t > 0) for the ensemble (one md_steps(--steps) call),
           the contexts on one stream and on J streams; the batched force and kick-drift launches' median
           durations (dispatch timestamps, a timed pass of their own)
  window:  per J: wall us per pump-window step (ratio qsteps in one fused launch + one MD step) of the
           ensemble; the QT launch's median duration and its FP64 roof fraction as the project counts it
           (1,750 flop per particle-qstep against 78.6 TF)
Any error exits non-zero; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12
QT_FLOP = 1750.0          # per particle-qstep
T1 = 1.0                  # a time past 0: the moving form of step()


def timed(step, sync, steps, warmup):
    for _ in range(warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--jobs", default="1,8,64", help="ensemble sizes J")
    ap.add_argument("--N0", type=int, default=3500)
    ap.add_argument("--program", type=int, default=1, choices=(1, 2, 3))
    ap.add_argument("--steps", type=int, default=1000, help="timed steps (a 100-step window misleads by 10-15 %%)")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--contexts", type=int, default=1, help="0: skip the contexts' baselines")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd._lib import lib
    params = dict(N0=a.N0, device=a.device, rng_mode=1)
    out = dict(tool="pump_ensemble_rate", N0=a.N0, program=a.program, steps=a.steps, warmup=a.warmup, md=[], window=[])

    for J in [int(x) for x in a.jobs.split(",") if x]:
        row = dict(jobs=J)
        with M.PumpEnsemble(J, pump_program=a.program, seed=777, job=1, **params) as e:
            e.init()
            ratio = int(e.jobs[0].const("plasmaToQuantumTimestepRatio"))
            for j in e.jobs:
                j.t = T1
            e.md_steps(a.warmup)
            el = timed(lambda: e.md_steps(a.steps), e.synchronize, 1, 0)
            e.enable_timing(True)
            e.md_steps(min(a.steps, 200))
            kt = e.kernel_times()
            e.enable_timing(False)
            ntot = sum(e.N)
            row.update(N_total=ntot, ensemble_us=el / a.steps * 1e6, force_us=kt["force_median_ms"] * 1e3,
                       kick_us=kt["kick_median_ms"] * 1e3, n_force=kt["n_force"], n_kick=kt["n_kick"])

            # the pump window's step: ratio qsteps (one fused launch), then the MD step
            def wstep():
                e.qsteps(ratio)
                e.md_steps(1)
            elw = timed(wstep, e.synchronize, a.steps, a.warmup)
            e.enable_timing(True)
            for _ in range(min(a.steps, 200)):
                wstep()
            kw = e.kernel_times()
            q_us = kw["qt_median_ms"] * 1e3
            out["window"].append(dict(jobs=J, N_total=ntot, ratio=ratio, ensemble_us=elw / a.steps * 1e6, qt_us=q_us,
                                      force_us=kw["force_median_ms"] * 1e3, kick_us=kw["kick_median_ms"] * 1e3,
                                      qt_roof=(ntot * ratio * QT_FLOP / (q_us * 1e-6) / FP64_PEAK) if q_us > 0 else None))
        if a.contexts:
            for shared in (True, False):
                sims = [M.Simulation(pump_program=a.program, seed=777 + k, job=1 + k, **params).init() for k in range(J)]
                try:
                    if shared:
                        st = lib().mdqt_get_stream(sims[0].h)
                        for x in sims[1:]:
                            x.set_stream(st)
                    for x in sims:
                        x.t = T1

                    def step():
                        for x in sims:
                            x.pump_md_steps(1)

                    def sync():
                        for x in sims:
                            x.synchronize()
                    el = timed(step, sync, a.steps, a.warmup)
                    if shared:                              # the streams go back before their owner is destroyed
                        for x in sims[1:]:
                            x.set_stream(None)
                finally:
                    for x in reversed(sims):
                        x.close()
                row["contexts_one_stream_us" if shared else "contexts_own_streams_us"] = el / a.steps * 1e6
        out["md"].append(row)

    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
