"""Python mirror of laserCoolNoPlasmaThreeState.cpp ("LC3", tlangin/MDQTPlasmaSims): Doppler
cooling of N0 non-interacting three-level ions by quantum trajectories, for an ensemble of jobs in
one launch.  Every method calls the C ABI of include/mdlc.h (libmdqt.so, gfx950 kernels); there is
no CPU fallback.  Method names follow the reference's functions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import MdlcParams, check, dptr, lib
from ._sweep import sweep_points


def default_params(**over) -> MdlcParams:
    """LC3:54-88, :393 defaults, with overrides."""
    p = MdlcParams()
    lib().mdlc_default_params(C.byref(p))
    for k, v in over.items():
        if k == "saveDirectory":
            v = v.encode() if isinstance(v, str) else v
        if not hasattr(p, k):
            raise AttributeError(f"mdlc_params has no field {k}")
        setattr(p, k, v)
    return p


def sample_velocities(seed: int, N0: int, temperature: float) -> np.ndarray:
    """init()'s velocity draws (:119-124) of one job: V [3][N0].  Runs without a GPU."""
    V = np.zeros((3, int(N0)))
    check(lib().mdlc_sample_velocities(int(seed), int(N0), float(temperature), dptr(V)), "mdlc_sample_velocities")
    return V


def format_directory(params: MdlcParams | None = None, job: int | None = None, **over) -> str:
    """main()'s directory of one job (:371-380).  Runs without a GPU."""
    p = params if params is not None else default_params(**over)
    buf = C.create_string_buffer(1024)
    check(lib().mdlc_format_directory(C.byref(p), int(p.job if job is None else job), buf, len(buf)),
          "mdlc_format_directory")
    return buf.value.decode()


SWEEP_FIELDS = ("detuning", "Om", "temperature")


def sweep_params(points, k: int) -> MdlcParams:
    """member k's parameters of a scan over `points` (a sequence of MdlcParams, each with njobs = R replicas) as a
    single job: point k // R, replica k % R (job + r, njobs = 1), after the checks mdlc_create_sweep makes of
    the points.  Runs without a GPU."""
    arr = (MdlcParams * len(points))(*points) if len(points) else (MdlcParams * 1)()
    out = MdlcParams()
    check(lib().mdlc_sweep_params(arr, len(points), int(k), C.byref(out)), "mdlc_sweep_params")
    return out


class LaserCooling:
    """An ensemble of LC3 jobs resident on a GPU (vx, psi and tPart in HBM).  Arrays are
    job-major: V (njobs, 3, N0), psi (njobs, N0, 3) complex, tPart (njobs, N0).

    ``sweep={"detuning": [-0.5, -1.0], "Om": [0.5, 1.0]}`` makes it a parameter scan (mdlc_create_sweep): the
    points are the product of the lists (the first name slowest) — or, given as a list of dicts, those points —
    each with ``njobs`` replicas.  ``members`` = ``npoints`` x ``njobs`` and the arrays are member-major (member
    k: point k // njobs, replica k % njobs); ``points`` lists the swept values, ``member_params(k)`` is member k
    as a single job.  The points share seed and job: replica r of every point sees the same random numbers."""

    def __init__(self, params: MdlcParams | None = None, sweep=None, **over):
        self.p = params if params is not None else default_params(**over)
        h = C.c_void_p()
        if sweep is None:
            self.points, self._points = [{}], (MdlcParams * 1)(self.p)
            check(lib().mdlc_create(C.byref(self.p), C.byref(h)), "mdlc_create")
        else:
            self.points, self._points = sweep_points(self.p, sweep, SWEEP_FIELDS)
            check(lib().mdlc_create_sweep(self._points, len(self._points), C.byref(h)), "mdlc_create_sweep")
        self._h = h
        self.N0 = int(self.p.N0)
        self.njobs = int(self.p.njobs)
        self.npoints = len(self._points)
        self.members = self.npoints * self.njobs

    def member_params(self, k: int) -> MdlcParams:
        """member k as a single job: its point's parameters, job + k % njobs, njobs = 1"""
        if not 0 <= int(k) < self.members:
            raise IndexError(f"member index {k} outside [0, {self.members})")
        out = MdlcParams()
        C.memmove(C.byref(out), C.byref(self._points[int(k) // self.njobs]), C.sizeof(MdlcParams))
        out.job += int(k) % self.njobs
        out.njobs = 1
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib().mdlc_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def const(self, name: str) -> float:
        return lib().mdlc_get_const(self._h, name.encode())

    # ---- the program's functions ----
    def init(self):                                   # init() :115-131
        check(lib().mdlc_init(self._h), "mdlc_init")
        return self

    def qsteps(self, n: int):                         # qstep() x n :140-293
        check(lib().mdlc_qsteps(self._h, int(n)), "mdlc_qsteps")

    def get_state(self) -> dict:
        J, N = self.members, self.N0
        V = np.zeros((J, 3, N)); a = np.zeros((J, N, 3, 2)); tp = np.zeros((J, N))
        q = C.c_uint64(0)
        check(lib().mdlc_get_state(self._h, dptr(V), dptr(a), dptr(tp), C.byref(q)), "mdlc_get_state")
        return {"V": V, "psi": a[..., 0] + 1j * a[..., 1], "tPart": tp, "q": int(q.value)}

    def set_state(self, V=None, psi=None, tPart=None, q=None):
        J, N = self.members, self.N0

        def arr(x, shape, what):
            if x is None:
                return None
            x = np.ascontiguousarray(x, dtype=np.float64)
            if x.shape != shape:
                raise ValueError(f"{what} must have shape {shape}, not {x.shape}")
            return x
        V = arr(V, (J, 3, N), "V")
        tPart = arr(tPart, (J, N), "tPart")
        if psi is not None:
            psi = np.asarray(psi, dtype=complex)
            psi = arr(np.stack([psi.real, psi.imag], -1), (J, N, 3, 2), "psi")
        qq = None if q is None else C.byref(C.c_uint64(int(q)))
        check(lib().mdlc_set_state(self._h, dptr(V), dptr(psi), dptr(tPart), qq), "mdlc_set_state")

    def ekin_x(self) -> np.ndarray:                   # output()'s EkinX :309-316, per job
        out = np.zeros(self.members)
        check(lib().mdlc_ekin_x(self._h, dptr(out)), "mdlc_ekin_x")
        return out

    def save_directory(self, k: int = 0) -> str:
        d = lib().mdlc_save_directory(self._h, int(k))
        if d is None:
            raise IndexError(f"job index {k} outside [0, {self.members})")
        return d.decode()

    def setup_directories(self) -> list:              # main() :364-380
        check(lib().mdlc_setup_directories(self._h), "mdlc_setup_directories")
        return [self.save_directory(k) for k in range(self.members)]

    def run(self, verbose: bool = False):             # main() :356-408
        check(lib().mdlc_run(self._h, int(bool(verbose))), "mdlc_run")

    def time_qsteps(self, nsteps: int, warmup: int, launches: int) -> np.ndarray:
        """ms of each of `launches` launches of nsteps qsteps (the kernels' own timestamps), after
        `warmup` untimed ones; the state advances (tools/mdlc_rate.py)."""
        ms = np.zeros(int(launches))
        check(lib().mdlc_time_qsteps(self._h, int(nsteps), int(warmup), int(launches), dptr(ms)), "mdlc_time_qsteps")
        return ms
