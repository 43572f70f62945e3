"""CPU checks of the ensemble's pooled output() seam (include/mdqt.h "Pooled output()"; no GPU needed): the header's
prototypes, the library's exports and the ctypes bindings agree and the Python methods exist; mdqt_pool_rows bit for
bit against plain float arithmetic in the stated order; mdqt_ensemble_pool_directory beside the members' directories;
the command line's --pool / --member_files refusals."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mdqt.h")

NEW = {
    "mdqt_pool_rows": ("int", ["const double* out7", "int R", "double* mean7", "double* sem6"]),
    "mdqt_ensemble_pool_directory": ("int", ["const mdqt_params* points", "int npoints", "int njobs", "int point", "char* buf",
                                             "size_t cap"]),
    "mdqt_ensemble_pool_observables": ("int", ["mdqt_ensemble* e", "double* mean7", "double* sem6", "double* Pvel",
                                               "long long* count", "double* spd"]),
}


@pytest.fixture(scope="module")
def L():
    from mdqtplasmasims_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.CLI_PATH):
        from mdqtplasmasims_amd.build import build
        build(quiet=True)
    return _lib.lib()


def header_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*([A-Za-z_][A-Za-z_ ]*?)\s+(mdqt_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        out[name] = (" ".join(ret.split()), [" ".join(a.split()) for a in args.split(",")])
    return out


# ---- the seam ----
def test_header_exports_and_bindings_agree(L):
    from mdqtplasmasims_amd._lib import SIGNATURES, MdqtParams
    protos = header_prototypes()
    bound = {s[0]: s for s in SIGNATURES}
    dp = C.POINTER(C.c_double)
    ctype = {"const double*": dp, "double*": dp, "int": C.c_int, "mdqt_ensemble*": C.c_void_p, "char*": C.c_char_p,
             "size_t": C.c_size_t, "long long*": C.POINTER(C.c_longlong), "const mdqt_params*": C.POINTER(MdqtParams)}
    for name, (ret, args) in NEW.items():
        assert protos.get(name) == (ret, args), name
        assert hasattr(L, name), name
        _, res, argtypes = bound[name]
        assert res is C.c_int, name
        assert list(argtypes) == [ctype[a.rsplit(" ", 1)[0]] for a in args], name
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == list(argtypes), name
    text = open(HEADER).read()
    for word in ('"pool"', '"member_files"', "pool_job<first>to<last>", "energies_sem.dat", "populations.dat",
                 "statePopulationsVsV_time%06d.dat", "rint(vx * 100.0)"):
        assert word in text, word


def test_python_methods():
    from mdqtplasmasims_amd import ensemble
    for m in ("pool_observables", "pool_directory", "output_kernel_times"):
        assert callable(getattr(ensemble.Ensemble, m)), m
    assert callable(ensemble.pool_directory) and ensemble.POOL_SLOTS == 1002


def test_null_arguments_are_refused_without_a_gpu(L):
    z7, z6 = (C.c_double * 7)(), (C.c_double * 6)()
    assert L.mdqt_pool_rows(None, 1, z7, z6) != 0 and b"NULL argument" in L.mdqt_last_error()
    assert L.mdqt_pool_rows(z7, 0, z7, z6) != 0 and b"R = 0" in L.mdqt_last_error()
    assert L.mdqt_ensemble_pool_observables(None, z7, z6, None, None, None) != 0 and b"NULL ensemble" in L.mdqt_last_error()
    assert L.mdqt_ensemble_pool_directory(None, 1, 1, 0, None, 0) != 0 and b"NULL argument" in L.mdqt_last_error()


# ---- mdqt_pool_rows: mean7[0] = the first row's t; [c] = (sum_r onto 0.0) / R; sem = sqrt(sum_r d^2 / (R (R - 1))) ----
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


def pool_rows(L, rows):
    from mdqtplasmasims_amd._lib import dptr
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    mean, sem = np.full(7, np.nan), np.full(6, np.nan)
    assert L.mdqt_pool_rows(dptr(rows), len(rows), dptr(mean), dptr(sem)) == 0, L.mdqt_last_error()
    return mean, sem


@pytest.mark.parametrize("R", [1, 2, 3, 64])
def test_pool_rows_bit_for_bit(L, R):
    rng = np.random.default_rng(100 + R)
    rows = rng.standard_normal((R, 7)) * np.array([1., 1e-3, 1e-3, 1e-3, 5., 1e-6, 1e-4])
    rows[:, 0] = 0.1234 + np.arange(R)           # only the first row's t is read
    rows[:, 3] = 0.40625                         # a column constant across the replicas (13 / 32: R x c is exact)
    mean, sem = pool_rows(L, rows)
    want_mean, want_sem = restate_rows(rows)
    assert np.array_equal(mean, want_mean) and np.array_equal(sem, want_sem)
    assert mean[0] == rows[0, 0]
    assert mean[3] == 0.40625 and sem[2] == 0.0
    if R == 1:
        assert np.array_equal(sem, np.zeros(6)) and np.array_equal(mean, rows[0])


def test_pool_rows_cancelling_and_constant_columns(L):
    x = 0.37
    rows = np.zeros((2, 7))
    rows[:, 0] = 2.5
    rows[0, 1], rows[1, 1] = x, -x               # mean exactly 0, sem = sqrt(2 x^2 / 2) = x
    rows[:, 2] = 4.25                            # constant, exactly representable: sem exactly 0
    rows[0, 4], rows[1, 4] = -0.0, -0.0          # sums start from +0.0
    mean, sem = pool_rows(L, rows)
    want_mean, want_sem = restate_rows(rows)
    assert np.array_equal(mean, want_mean) and np.array_equal(sem, want_sem)
    assert mean[1] == 0.0 and sem[0] == math.sqrt((x * x + x * x) / 2.0)
    assert mean[2] == 4.25 and sem[1] == 0.0
    assert mean[4] == 0.0 and not np.signbit(mean[4])
    rows64 = np.tile([[2.5, 0.375, 4.25, -1.0, 0.0, 3.0, -0.015625]], (64, 1))   # 64 equal dyadic rows: every sum exact
    mean, sem = pool_rows(L, rows64)
    assert np.array_equal(sem, np.zeros(6)) and np.array_equal(mean, rows64[0])


# ---- mdqt_ensemble_pool_directory ----
def run_name(p):
    """mdqt_setup_directories' name of a run (SpeedUp:1145-1160): the fields x their scales, truncated"""
    return ("Ge%dDensity%dE+11Sig0%dTe%dSigFrac%dDetSP%dDetDP%dOmSP%dOmDP%dNumIons%d" %
            (int(100 * p.Ge), int(p.density * 1000), int(10 * p.sig0), int(p.Te), int(p.fracOfSig * 100), int(p.detuning * 100),
             int(p.detuningDP * 100), int(p.Om * 100), int(p.OmDP * 100), p.N0))


def member_directory(p):
    return "%s%s/job%d/" % (p.saveDirectory.decode(), run_name(p), p.job)


def test_pool_directory_of_an_ordinary_ensemble(L):
    from mdqtplasmasims_amd.engine import default_params
    from mdqtplasmasims_amd.ensemble import job_params, pool_directory
    base = default_params(N0=62, job=3, seed=9, rng_mode=1, saveDirectory="out/")
    members = [member_directory(job_params(base, k)) for k in range(4)]
    assert members[0] == "out/Ge10Density2000E+11Sig040Te19SigFrac0DetSP-100DetDP100OmSP100OmDP100NumIons62/job3/"
    parents = {os.path.dirname(m.rstrip("/")) for m in members}
    assert len(parents) == 1
    assert pool_directory(base, 4) == parents.pop() + "/pool_job3to6/"
    assert pool_directory(base, 1) == os.path.dirname(members[0].rstrip("/")) + "/pool_job3to3/"


def test_pool_directory_of_a_scan_and_its_refusals(L):
    from mdqtplasmasims_amd import MdqtError
    from mdqtplasmasims_amd._sweep import sweep_points
    from mdqtplasmasims_amd.engine import default_params
    from mdqtplasmasims_amd.ensemble import SWEEP_FIELDS, pool_directory, sweep_params
    base = default_params(N0=300, job=1, seed=501, rng_mode=1, saveDirectory="scan/")
    sweep = {"detuningDP": [0.0, 1.0]}
    _, arr = sweep_points(base, sweep, SWEEP_FIELDS)
    seen = set()
    for q in range(2):
        members = [member_directory(sweep_params(base, sweep, 3, 3 * q + r)) for r in range(3)]
        parents = {os.path.dirname(m.rstrip("/")) for m in members}
        assert len(parents) == 1
        d = pool_directory(arr, 3, q)
        assert d == parents.pop() + "/pool_job1to3/"
        assert "DetDP%d" % (100 * q) in d
        seen.add(d)
    assert len(seen) == 2
    for bad in (2, -1, 7):
        with pytest.raises(MdqtError, match=r"point index %d outside \[0, 2\)" % bad):
            pool_directory(arr, 3, bad)
    buf = C.create_string_buffer(16)
    assert L.mdqt_ensemble_pool_directory(arr, 2, 3, 0, buf, len(buf)) != 0 and b"bytes" in L.mdqt_last_error()


# ---- the command line ----
def cli(*args):
    from mdqtplasmasims_amd._lib import CLI_PATH
    return subprocess.run([CLI_PATH, *args], capture_output=True, text=True, timeout=60)


REFUSED = {
    "pool 1 with an explicit output_batch 0": ["--njobs=2", "--pool=1", "--output_batch=0"],
    "output_batch 0 after pool 1": ["--njobs=2", "--output_batch=0", "--pool=1"],
    "pool without njobs": ["--pool=1"],
    "pool 0 without njobs": ["--pool=0"],
    "member_files without njobs": ["--member_files=1"],
    "pool with a pump program": ["--pump_program=1", "--pump_jobs=2", "--pool=1"],
    "member_files with a pump program": ["--pump_program=1", "--pump_jobs=2", "--member_files=1"],
    "member_files 0 without pool": ["--njobs=2", "--member_files=0"],
    "member_files 0 with pool 0": ["--njobs=2", "--pool=0", "--member_files=0"],
    "pool 2": ["--njobs=2", "--pool=2"],
    "pool -1": ["--njobs=2", "--pool=-1"],
    "pool empty": ["--njobs=2", "--pool="],
    "pool 1x": ["--njobs=2", "--pool=1x"],
    "pool 01": ["--njobs=2", "--pool=01"],
    "member_files 2": ["--njobs=2", "--pool=1", "--member_files=2"],
    "member_files x": ["--njobs=2", "--pool=1", "--member_files=x"],
    "member_files empty": ["--njobs=2", "--pool=1", "--member_files="],
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_cli_refusals(L, case, tmp_path):
    r = cli("1", *REFUSED[case], "--N0=62", "--tmax=0.01", f"--saveDirectory={tmp_path}/")
    assert r.returncode == 2, (case, r.stderr[-500:])
    assert "usage: mdqt" in r.stderr and "--pool" in r.stderr and "--member_files" in r.stderr
    assert r.stdout == ""
    assert os.listdir(tmp_path) == []
