#!/usr/bin/env python3
"""Rate of the three-level laser-cooling kernel (k_lc_steps, mdlc_kernels.hip) on one GPU.

For N0 = 1000 and njobs = 1, 8 and 64: 5 warm-up launches of 1000 steps, then 20 timed launches
(each kernel's own dispatch timestamps, mdlc_time_qsteps).  Prints ONE JSON line:

  per njobs: median / min / max ms per launch, us per step, ion-steps/s, the launch time relative
             to njobs = 1
  fp64_per_ion_step: FP64 vector instructions inside k_lc_steps' step loop (both branches), counted
             in build/mdlc_kernels.s (`make -C mdqtplasmasims_amd/csrc asm`); an FMA counts as one
             instruction and two FLOP
  roof_fraction: ion-steps/s x FP64 FLOP per ion-step / 78.6e12 (the FP64 vector peak)

--sweep NAME:v1,v2,... (NAME one of detuning, Om, temperature; once per name) times a parameter scan instead
(k_lc_steps_sweep, mdlc_sweep_kernels.hip): each njobs value J is then the members in all, the points (the
product of the lists) x J / points replicas.  One value runs the scan's kernel on the uniform ensemble's own jobs.

There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12
ASM = os.path.join(ROOT, "mdqtplasmasims_amd", "build", "mdlc_kernels.s")


def count_loop_fp64(path=ASM):
    """(FP64 instructions, FP64 FLOP, all vector ALU instructions) in the step loop of k_lc_steps:
    the basic blocks the compiler's comments place inside the kernel's loop"""
    txt = open(path).read()
    m = re.search(r"^(_ZN4mdqt10k_lc_steps\w*):.*?^\s+s_endpgm", txt, flags=re.S | re.M)
    if not m:
        raise RuntimeError(f"k_lc_steps not found in {path}")
    in_loop = False
    n64 = flop = valu = 0
    for line in m.group(0).splitlines():
        if re.match(r"^\.LBB\d+_\d+:", line):
            in_loop = "Loop" in line
            continue
        if not in_loop:
            continue
        ins = line.split(";")[0].split()
        if not ins or not ins[0].startswith("v_"):
            continue
        valu += 1
        if re.search(r"_f64(_|$)", ins[0]) and not ins[0].startswith(("v_cmp", "v_cvt")):
            n64 += 1
            flop += 2 if re.match(r"v_(fma|fmac|mad)_f64", ins[0]) else 1
    return n64, flop, valu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N0", type=int, default=1000)
    ap.add_argument("--njobs", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sweep", action="append", default=[], metavar="NAME:v1,v2,...",
                    help="time a scan of J members in all: the points are the product of the axes")
    ap.add_argument("--asm", default=ASM, help="assembly of mdlc_kernels.hip (made with `make asm` if missing)")
    a = ap.parse_args()

    import numpy as np
    from mdqtplasmasims_amd import LaserCooling
    from mdqtplasmasims_amd._sweep import parse_sweep_args

    if not os.path.exists(a.asm):
        subprocess.run(["make", "-C", os.path.join(ROOT, "mdqtplasmasims_amd", "csrc"), "asm"], check=True,
                       stdout=subprocess.DEVNULL)
    n64, flop, valu = count_loop_fp64(a.asm)
    try:
        sweep = parse_sweep_args(a.sweep)
    except ValueError as e:
        ap.error(str(e))
    npoints = int(np.prod([len(v) for v in sweep.values()])) if sweep else 1
    rows = {}
    base = None
    for J in a.njobs:
        if J % npoints:
            ap.error(f"--njobs {J} is not a multiple of the scan's {npoints} points")
        with LaserCooling(N0=a.N0, njobs=J // npoints, seed=12345, job=1, device=a.device, sweep=sweep or None) as s:
            assert s.members == J
            s.init()
            ms = s.time_qsteps(a.steps, a.warmup, a.launches)
        med = float(np.median(ms))
        base = med if base is None else base
        rate = a.N0 * J * a.steps / (med * 1e-3)
        rows[str(J)] = dict(ms_median=round(med, 5), ms_min=round(float(ms.min()), 5), ms_max=round(float(ms.max()), 5),
                            us_per_step=round(med * 1e3 / a.steps, 5), ion_steps_per_s=round(rate, 1),
                            launch_vs_first=round(med / base, 4), roof_fraction=round(rate * flop / FP64_PEAK, 6))
    try:
        tree = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        tree = ""
    print(json.dumps(dict(tool="mdlc_rate", N0=a.N0, steps=a.steps, warmup=a.warmup, launches=a.launches,
                          fp64_per_ion_step=n64, fp64_flop_per_ion_step=flop, valu_per_ion_step=valu,
                          fp64_peak=FP64_PEAK, tree=tree or None, sweep=sweep or None, njobs=rows)))


if __name__ == "__main__":
    main()
