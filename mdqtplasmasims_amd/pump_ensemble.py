"""An ensemble of independent optical-pumping jobs on one MI355X, stepped in batched launches.

The reference's pump programs (randomFrozenStartTag408Linear.cpp, 408Quad, 422Linear) are run as a Slurm
array of independent jobs like every other program (exampleSlurmFile.slurm:3, ``exe <job>``).
:class:`PumpEnsemble` owns ``njobs`` such jobs — job k has ``job + k`` and ``seed + k`` — and steps them
together (include/mdqt.h, "ensembles of the optical-pumping programs"): at t > 0 one MD step of all of
them is two launches.  Every job's state and files are bit for bit / byte for byte what
``Simulation(pump_program=m, ...).run_pump()`` gives for that job alone.

    ===================================  ============================  ===============================
    reference (408Linear), per job       here, all jobs                C ABI (include/mdqt.h)
    ===================================  ============================  ===============================
    init()              :289-315         PumpEnsemble.init()           mdqt_pump_ensemble_init
    step(); c0++ x n    :377-394         PumpEnsemble.md_steps(n)      mdqt_pump_ensemble_md_steps
    qstep() x n         :396-598         PumpEnsemble.qsteps(n)        mdqt_pump_ensemble_qsteps
    measureSpinUps()    :600-665         PumpEnsemble.tag_spin_up()    mdqt_pump_ensemble_tag_spin_up
    output()            :799-935         PumpEnsemble.output()         mdqt_pump_ensemble_output
    main()              :981-1076        PumpEnsemble.run()            mdqt_pump_ensemble_run
    ===================================  ============================  ===============================
"""
from __future__ import annotations

import ctypes as C

from ._ensemble_base import _EnsembleBase
from ._lib import check, lib
from .engine import default_params_pump
from .ensemble import _Member, job_params


class PumpEnsemble(_EnsembleBase):
    """``njobs`` independent jobs (job + k, seed + k) of pump program 1 / 2 / 3, stepped together."""

    _DESTROY = "mdqt_pump_ensemble_destroy"

    def __init__(self, njobs: int, pump_program: int = 1, **params):
        self.params = default_params_pump(pump_program, **params)
        h = C.c_void_p()
        check(lib().mdqt_pump_ensemble_create(C.byref(self.params), int(njobs), C.byref(h)),
              "mdqt_pump_ensemble_create")
        self.h = h
        self.jobs = [_Member(self, lib().mdqt_pump_ensemble_job(h, k), job_params(self.params, k))
                     for k in range(lib().mdqt_pump_ensemble_size(h))]

    @property
    def N(self):
        """every job's ion number"""
        return [j.N for j in self.jobs]

    def set_option(self, name: str, value: int):
        """any Simulation option, on every job"""
        check(lib().mdqt_pump_ensemble_set_option(self.h, name.encode(), int(value)), "pump_ensemble_set_option")

    # ---- the reference's function seam, for every job at once ----
    def init(self):
        check(lib().mdqt_pump_ensemble_init(self.h), "pump_ensemble_init")
        return self

    def md_steps(self, n: int):
        """n x (step(); c0++) at the jobs' t"""
        check(lib().mdqt_pump_ensemble_md_steps(self.h, int(n)), "pump_ensemble_md_steps")

    def qsteps(self, n: int):
        """n x qstep() (QT only), fused in launches of at most 32"""
        check(lib().mdqt_pump_ensemble_qsteps(self.h, int(n)), "pump_ensemble_qsteps")

    def tag_spin_up(self):
        """measureSpinUps() of every job: [(tags[N], n_up), ...]"""
        check(lib().mdqt_pump_ensemble_tag_spin_up(self.h), "pump_ensemble_tag_spin_up")
        return [j.spin_up_list() for j in self.jobs]

    def output(self):
        check(lib().mdqt_pump_ensemble_output(self.h), "pump_ensemble_output")

    def run(self):
        """main() of every job (newRun 0 and 1): each job's directory tree as ``run_pump()`` writes it"""
        check(lib().mdqt_pump_ensemble_run(self.h), "pump_ensemble_run")

    def synchronize(self):
        check(lib().mdqt_pump_ensemble_synchronize(self.h), "pump_ensemble_synchronize")

    def launches(self) -> int:
        """kernel launches the batched path has issued since creation"""
        return int(lib().mdqt_pump_ensemble_launches(self.h))

    # ---- timing ----
    def enable_timing(self, on: bool = True):
        """record the batched kernels' dispatch timestamps at every launch"""
        check(lib().mdqt_pump_ensemble_enable_timing(self.h, 1 if on else 0))

    def kernel_times(self):
        """force, QT and kick-drift launches since the last call (synchronises and resets): summed ms, counts,
        median ms"""
        out = (C.c_double * 9)()
        check(lib().mdqt_pump_ensemble_kernel_times(self.h, out, 9), "pump_ensemble_kernel_times")
        return self._times(out, ("force_ms", "n_force", "qt_ms", "n_qt", "kick_ms", "n_kick", "force_median_ms",
                                 "qt_median_ms", "kick_median_ms"))


__all__ = ["PumpEnsemble"]
