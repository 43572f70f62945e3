"""An ensemble of independent Monte-Carlo + MD jobs on one MI355X.

The reference runs its MC + MD programs as a Slurm array of independent jobs (exampleSlurmFile.slurm:3,16,
``srun tagQuad $SLURM_ARRAY_TASK_ID``).  :class:`MonteCarloEnsemble` owns ``njobs`` such jobs — job k has
``job + k`` and ``seed + k`` — anneals all their Metropolis chains with one launch (one workgroup per chain)
and steps their MD either member by member on the members' own streams (``md_batch=0``, the default) or with one
force launch and one velocity-Verlet launch per step for all jobs (``md_batch=1``; include/mdmc.h, "ensembles").
Every job's state and files are bit for bit what :class:`~mdqtplasmasims_amd.mdmc.MonteCarloMD` gives for that
job alone, in either mode.  For the QT tagging programs (``qt_model`` 1..3) the QT substeps, the spin-up tagging
and the tagged ions' moments and X distribution follow ``md_batch`` too: member by member, or one launch for all
jobs (``qt_launches()`` counts those).

    =================================  ================================  ============================
    reference (MCMD), per job          here, all jobs                    C ABI (include/mdmc.h)
    =================================  ================================  ============================
    init()             :173-245        MonteCarloEnsemble.init()         mdmc_ensemble_init
    MonteCarloStep() x n  :315-382     MonteCarloEnsemble.monte_carlo(n) mdmc_ensemble_monte_carlo
    MDStep() x n       :504-511        MonteCarloEnsemble.md_steps(n)    mdmc_ensemble_md_steps
    main()             :1030-1167      MonteCarloEnsemble.run()          mdmc_ensemble_run
    qstep() x n        QTT:555-756     .qsteps(n)                        mdmc_ensemble_qsteps
    tagParticles       QTT:1022-1067   .tag_qt()                         mdmc_ensemble_tag_qt
    recordTaggedParticleMoments        .tagged_moments_qt(dist=True)     mdmc_ensemble_tagged_moments_qt
                       QTT:1069-1138   (the X distribution only)
    (launch counter)                   .qt_launches()                    mdmc_ensemble_qt_launches
    =================================  ================================  ============================
"""
from __future__ import annotations

import ctypes as C

from ._ensemble_base import _EnsembleBase
import numpy as np

from ._lib import MdmcParams, check, dptr, lib
from .mdmc import MonteCarloMD, default_params


def mdmc_job_params(base: MdmcParams, k: int) -> MdmcParams:
    """job k's parameters of an ensemble created from `base` (job + k, seed + k; host only)"""
    out = MdmcParams()
    check(lib().mdmc_ensemble_job_params(C.byref(base), int(k), C.byref(out)), "mdmc_ensemble_job_params")
    return out


class _Member(MonteCarloMD):
    """a job of an ensemble: the whole MonteCarloMD interface on a context the ensemble owns"""

    def __init__(self, ensemble, handle, params):  # no mdmc_create
        self._ensemble = ensemble                  # keeps the owner alive
        self.p = params
        self._h = C.c_void_p(handle)
        self.N = int(params.N)
        self.T = int(params.numVelAutoCorrsSteps)

    def close(self):                               # not this view's to destroy
        self._h = None


class MonteCarloEnsemble(_EnsembleBase):
    """``njobs`` independent jobs (job + k, seed + k) resident on one MI355X."""

    _DESTROY = "mdmc_ensemble_destroy"

    STAGES = ("anneal", "pre_record_md", "qt_pump", "recorded_md", "autocorrelations", "rest")

    def __init__(self, njobs: int, md_batch=None, **params):
        self.p = default_params(**params)
        h = C.c_void_p()
        check(lib().mdmc_ensemble_create(C.byref(self.p), int(njobs), C.byref(h)), "mdmc_ensemble_create")
        self.h = h
        self.jobs = [_Member(self, lib().mdmc_ensemble_job(h, k), mdmc_job_params(self.p, k))
                     for k in range(lib().mdmc_ensemble_size(h))]
        if md_batch is not None:
            self.md_batch = md_batch

    # ---- how the MD stages are stepped: 0 member by member, 1 batched launches (the same bits) ----
    @property
    def md_batch(self) -> int:
        mode = lib().mdmc_ensemble_md_batch(self.h)
        if mode < 0:
            check(mode, "mdmc_ensemble_md_batch")
        return mode

    @md_batch.setter
    def md_batch(self, mode: int):
        check(lib().mdmc_ensemble_set_md_batch(self.h, int(mode)), "mdmc_ensemble_set_md_batch")

    def md_launches(self) -> int:
        """kernel launches the batched MD path has issued since creation (md_batch 0 leaves it unchanged)"""
        n = C.c_ulonglong(0)
        check(lib().mdmc_ensemble_md_launches(self.h, C.byref(n)), "mdmc_ensemble_md_launches")
        return int(n.value)

    # ---- the reference's function seam, for every job at once ----
    def init(self):
        check(lib().mdmc_ensemble_init(self.h), "mdmc_ensemble_init")
        return self

    def monte_carlo(self, nsteps: int) -> list:
        """nsteps Metropolis steps of every chain (batched launches); the accepted counts by job"""
        acc = (C.c_longlong * len(self.jobs))()
        check(lib().mdmc_ensemble_monte_carlo(self.h, int(nsteps), acc), "mdmc_ensemble_monte_carlo")
        return [int(a) for a in acc]

    def md_steps(self, nsteps: int):
        check(lib().mdmc_ensemble_md_steps(self.h, int(nsteps)), "mdmc_ensemble_md_steps")

    def run(self, verbose: bool = False):
        check(lib().mdmc_ensemble_run(self.h, int(bool(verbose))), "mdmc_ensemble_run")

    # ---- the QT tagging variants (qt_model 1..3), for every job at once ----
    def qsteps(self, n: int):
        """qstep() x n of every job (QTT:555-756): ceil(n / 32) launches under md_batch 1, whatever njobs is"""
        check(lib().mdmc_ensemble_qsteps(self.h, int(n)), "mdmc_ensemble_qsteps")

    def tag_qt(self):
        """tagParticles of every job (QTT:1022-1067) -> (tags [njobs][N], counts [njobs])"""
        J = len(self.jobs)
        t = np.zeros((J, int(self.p.N)), dtype=np.int32)
        cnt = np.zeros(J, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        check(lib().mdmc_ensemble_tag_qt(self.h, t.ctypes.data_as(ip), cnt.ctypes.data_as(ip)), "mdmc_ensemble_tag_qt")
        return t, cnt

    def tagged_moments_qt(self, dist: bool = True):
        """recordTaggedParticleMoments of every job (QTT:1069-1138): the moments [njobs][4] and, with `dist`, the X
        distributions [njobs][4001] — X only, the row the programs write; row 0 of MonteCarloMD.tagged_moments_qt"""
        J = len(self.jobs)
        out = np.zeros((J, 4))
        d = np.zeros((J, 4001)) if dist else None
        check(lib().mdmc_ensemble_tagged_moments_qt(self.h, dptr(out), dptr(d)), "mdmc_ensemble_tagged_moments_qt")
        return (out, d) if dist else out

    def qt_launches(self) -> int:
        """kernel launches the batched QT, tagging, moment and distribution paths have issued since creation
        (md_batch 0 leaves it unchanged; md_launches() does not count them)"""
        n = C.c_ulonglong(0)
        check(lib().mdmc_ensemble_qt_launches(self.h, C.byref(n)), "mdmc_ensemble_qt_launches")
        return int(n.value)

    # ---- timing ----
    def enable_timing(self, on: bool = True):
        """record the batched launches' dispatch timestamps, and time the stages of run()"""
        check(lib().mdmc_ensemble_enable_timing(self.h, 1 if on else 0))

    def kernel_times(self):
        """{anneal_ms, n_anneal, anneal_median_ms, anneal_min_ms, anneal_max_ms} of the batched launches since
        the last call (synchronises and resets), the same five as md_force_* and md_vv_* for the batched force
        and velocity-Verlet launches (md_batch 1), as qt_* and qt_dist_* for the batched QT launches and the X
        distribution's chunk kernel, and stage_ms: the wall time of the last run()'s stages"""
        out = (C.c_double * 31)()
        check(lib().mdmc_ensemble_kernel_times(self.h, out, 31), "mdmc_ensemble_kernel_times")
        d = {}
        for i, k in ((0, "anneal"), (11, "md_force"), (16, "md_vv"), (21, "qt"), (26, "qt_dist")):
            d.update(self._times(out, (k + "_ms", "n_" + k, k + "_median_ms", k + "_min_ms", k + "_max_ms"), i))
        d["stage_ms"] = {k: out[5 + i] for i, k in enumerate(self.STAGES)}
        return d


__all__ = ["MonteCarloEnsemble", "mdmc_job_params"]
