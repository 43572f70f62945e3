"""An ensemble of independent MDQT jobs on one MI355X, stepped in batched launches.

The reference is run as a Slurm array of independent jobs of laserCoolingPlusExpansionMDQTSpeedUp.cpp
(exampleSlurmFile.slurm:3, ``exe <job>``, srand48(time + job) at SpeedUp:1219) whose results are
averaged.  :class:`Ensemble` owns ``njobs`` such jobs — job k has ``job + k`` and ``seed + k`` — and steps
them with one force launch and one QT launch per MD step (include/mdqt.h, "ensembles").  Every job's
state is bit for bit what :class:`~mdqtplasmasims_amd.engine.Simulation` gives for that job alone.

    =================================  ===========================  ==========================
    reference (SpeedUp), per job       here, all jobs               C ABI (include/mdqt.h)
    =================================  ===========================  ==========================
    init()            :289-348         Ensemble.init()              mdqt_ensemble_init
    forces()          :192-236         Ensemble.forces()            mdqt_ensemble_forces
    step();qstep() x n  :1376-1377     Ensemble.substeps(n)         mdqt_ensemble_substeps
    forces + ratio substeps, x n       Ensemble.md_steps(n)         mdqt_ensemble_md_steps
    main()            :1139-1383       Ensemble.run()               mdqt_ensemble_run
    output()          :917-1032        Ensemble.output()            mdqt_ensemble_output
    output()'s numbers                 Ensemble.observables()       mdqt_ensemble_observables
    Epotential()      :244-281         Ensemble.epotential()        mdqt_ensemble_epotential
    the job array's averages           Ensemble.pool_observables()  mdqt_ensemble_pool_observables
    =================================  ===========================  ==========================
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ensemble_base import _EnsembleBase
from ._lib import MdqtParams, check, dptr, lib
from ._sweep import sweep_points
from .engine import NBINS, Simulation, default_params


def job_params(base: MdqtParams, k: int) -> MdqtParams:
    """job k's parameters of an ensemble created from `base` (job + k, seed + k; host only)"""
    out = MdqtParams()
    check(lib().mdqt_ensemble_job_params(C.byref(base), int(k), C.byref(out)), "ensemble_job_params")
    return out


SWEEP_FIELDS = ("detuning", "detuningDP", "Om", "OmDP", "fracOfSig")


def sweep_params(base: MdqtParams, sweep, njobs: int, k: int) -> MdqtParams:
    """member k's parameters of a sweep ensemble of `njobs` replicas per point (point k // njobs, replica k % njobs:
    job + r, seed + r), after the checks mdqt_ensemble_create_sweep makes of the points (host only)"""
    _, arr = sweep_points(base, sweep, SWEEP_FIELDS)
    out = MdqtParams()
    check(lib().mdqt_ensemble_sweep_params(arr, len(arr), int(njobs), int(k), C.byref(out)), "ensemble_sweep_params")
    return out


POOL_SLOTS = 1002   # the velocity-resolved populations' slots: 1,001 of width 0.01 centred on -5 .. 5, and "outside"


def pool_directory(points, njobs: int, p: int = 0) -> str:
    """the pooled directory of point p of an ensemble of len(points) x njobs members (points: MdqtParams, one or
    an array; host only)"""
    arr = (MdqtParams * 1)(points) if isinstance(points, MdqtParams) else points
    buf = C.create_string_buffer(1400)
    check(lib().mdqt_ensemble_pool_directory(arr, len(arr), int(njobs), int(p), buf, len(buf)), "ensemble_pool_directory")
    return buf.value.decode()


class _Member(Simulation):
    """a job of an ensemble: the whole Simulation interface on a context the ensemble owns"""

    def __init__(self, ensemble, handle, params):  # no mdqt_create
        self._ensemble = ensemble                  # keeps the owner alive
        self.params = params
        self.h = C.c_void_p(handle)

    def close(self):                               # not this view's to destroy
        self.h = None


class Ensemble(_EnsembleBase):
    """``njobs`` independent jobs (job + k, seed + k) resident on one MI355X, stepped together.

    ``sweep={"detuningDP": [0.0, 1.0], "Om": [0.5, 1.0]}`` makes it a parameter scan (mdqt_ensemble_create_sweep):
    the points are the product of the lists (the first name slowest) — or, given as a list of dicts, those points —
    each with ``njobs`` replicas; ``jobs`` is flat in member order (point-major), ``points`` lists the swept
    values, ``member(p, r)`` is replica r of point p.
    """

    _DESTROY = "mdqt_ensemble_destroy"

    def __init__(self, njobs: int, sweep=None, **params):
        self.params = default_params(**params)
        self.njobs = int(njobs)
        h = C.c_void_p()
        if sweep is None:
            self.points = [{}]
            self._point_params = (MdqtParams * 1)(self.params)
            check(lib().mdqt_ensemble_create(C.byref(self.params), self.njobs, C.byref(h)), "mdqt_ensemble_create")
            member = [job_params(self.params, k) for k in range(lib().mdqt_ensemble_size(h))]
        else:
            self.points, arr = sweep_points(self.params, sweep, SWEEP_FIELDS)
            self._point_params = arr
            check(lib().mdqt_ensemble_create_sweep(arr, len(arr), self.njobs, C.byref(h)), "mdqt_ensemble_create_sweep")
            member = [job_params(arr[k // self.njobs], k % self.njobs) for k in range(lib().mdqt_ensemble_size(h))]
        self.h = h
        self.jobs = [_Member(self, lib().mdqt_ensemble_job(h, k), p) for k, p in enumerate(member)]

    def member(self, p: int, r: int):
        """replica r of point p (``jobs[p * njobs + r]``)"""
        if not (0 <= p < len(self.points) and 0 <= r < self.njobs):
            raise IndexError(f"member({p}, {r}) of {len(self.points)} points x {self.njobs} replicas")
        return self.jobs[p * self.njobs + r]

    @property
    def N(self):
        """every job's ion number"""
        return [j.N for j in self.jobs]

    def set_option(self, name: str, value: int):
        """"qt_waves" (the batched QT kernel's register budget), "output_batch" (1: output() of all jobs in one
        device pass, 0: job after job, the default), "pool" (1: every output() also writes each point's pooled
        observables; needs output_batch 1), "member_files" (0: output() writes the pooled files only) or any
        Simulation option, on every job"""
        check(lib().mdqt_ensemble_set_option(self.h, name.encode(), int(value)), "ensemble_set_option")

    # ---- the reference's function seam, for every job at once ----
    def init(self):
        check(lib().mdqt_ensemble_init(self.h), "ensemble_init")
        return self

    def forces(self):
        check(lib().mdqt_ensemble_forces(self.h), "ensemble_forces")

    def substeps(self, n: int):
        check(lib().mdqt_ensemble_substeps(self.h, int(n)), "ensemble_substeps")

    def md_steps(self, n: int):
        check(lib().mdqt_ensemble_md_steps(self.h, int(n)), "ensemble_md_steps")

    def run(self):
        check(lib().mdqt_ensemble_run(self.h), "ensemble_run")

    def synchronize(self):
        check(lib().mdqt_ensemble_synchronize(self.h), "ensemble_synchronize")

    # ---- output() of every job in one device pass (option "output_batch") ----
    def output(self):
        """output() of every job; returns when the files are on disk"""
        check(lib().mdqt_ensemble_output(self.h), "ensemble_output")

    def observables(self, kde: bool = True, pops: bool = True):
        """a list of what Simulation.observables() returns, job by job"""
        n = self.N
        o = np.zeros((len(n), 7))
        P = np.zeros((len(n), 3, NBINS)) if kde else None
        pp = np.zeros((sum(n), 3)) if pops else None
        check(lib().mdqt_ensemble_observables(self.h, dptr(o), dptr(P), dptr(pp)), "ensemble_observables")
        at = np.concatenate(([0], np.cumsum(n)))
        return [(o[k], P[k] if kde else None, pp[at[k]:at[k + 1]] if pops else None) for k in range(len(n))]

    def epotential(self):
        """Epotential() of every job: [njobs]"""
        out = np.zeros(len(self.jobs))
        check(lib().mdqt_ensemble_epotential(self.h, dptr(out)), "ensemble_epotential")
        return out

    # ---- the pooled output(): each point's observables over its replicas (option "pool") ----
    def pool_observables(self):
        """one pooled pass, no files: {mean7 [P, 7], sem6 [P, 6], Pvel [P, 3, NBINS], count [P, 1002] (int64), spd
        [P, 3, 1002] (the slots' sums of S, P, D)} for the P points (include/mdqt.h has the definitions)"""
        P = len(self.points)
        out = dict(mean7=np.zeros((P, 7)), sem6=np.zeros((P, 6)), Pvel=np.zeros((P, 3, NBINS)),
                   count=np.zeros((P, POOL_SLOTS), dtype=np.int64), spd=np.zeros((P, 3, POOL_SLOTS)))
        check(lib().mdqt_ensemble_pool_observables(self.h, dptr(out["mean7"]), dptr(out["sem6"]), dptr(out["Pvel"]),
                                                   out["count"].ctypes.data_as(C.POINTER(C.c_longlong)), dptr(out["spd"])),
              "ensemble_pool_observables")
        return out

    def pool_directory(self, p: int = 0) -> str:
        """the directory of point p's pooled files (host only): beside its replicas' job<k>/"""
        return pool_directory(self._point_params, self.njobs, p)

    @property
    def output_launches(self):
        """kernel launches the batched output path has issued (a member's own fallback calls are not counted)"""
        return int(lib().mdqt_ensemble_output_launches(self.h))

    # ---- timing ----
    def enable_timing(self, on: bool = True):
        """record the two batched kernels' dispatch timestamps at every launch"""
        check(lib().mdqt_ensemble_enable_timing(self.h, 1 if on else 0))

    def kernel_times(self):
        """{force_ms, n_force, substep_ms, n_substep, force_median_ms, substep_median_ms} of the batched
        launches since the last call (synchronises and resets)"""
        return {k: v for k, v in self.output_kernel_times().items() if "force" in k or "substep" in k}

    def output_kernel_times(self):
        """kernel_times() and the batched output's potential and KDE launches: potential_ms, n_potential, kde_ms,
        n_kde, potential_median_ms, kde_median_ms; then the pooled pass's two launches: popv_ms, n_popv, pool_ms,
        n_pool, popv_median_ms, pool_median_ms"""
        out = (C.c_double * 18)()
        check(lib().mdqt_ensemble_kernel_times(self.h, out, 18), "ensemble_kernel_times")
        return self._times(out, ("force_ms", "n_force", "substep_ms", "n_substep", "force_median_ms", "substep_median_ms",
                                 "potential_ms", "n_potential", "kde_ms", "n_kde", "potential_median_ms", "kde_median_ms",
                                 "popv_ms", "n_popv", "pool_ms", "n_pool", "popv_median_ms", "pool_median_ms"))


__all__ = ["Ensemble", "job_params", "sweep_params", "pool_directory", "SWEEP_FIELDS", "POOL_SLOTS"]
