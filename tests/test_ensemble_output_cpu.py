"""CPU checks of the ensemble's batched output() seam (include/mdqt.h "ensembles"; no GPU needed): the header's new
prototypes, the library's exports and the ctypes bindings agree; the Python methods exist; the command line's
--output_batch argument checks."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mdqt.h")

NEW = {
    "mdqt_ensemble_output": ("int", ["mdqt_ensemble* e"]),
    "mdqt_ensemble_observables": ("int", ["mdqt_ensemble* e", "double* out7", "double* Pvel", "double* pops"]),
    "mdqt_ensemble_epotential": ("int", ["mdqt_ensemble* e", "double* Epot"]),
    "mdqt_ensemble_output_launches": ("unsigned long long", ["const mdqt_ensemble* e"]),
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
    for ret, name, args in re.findall(r"^\s*([A-Za-z_][A-Za-z_ ]*?)\s+(mdqt_ensemble_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        out[name] = (" ".join(ret.split()), [" ".join(a.split()) for a in args.split(",")])
    return out


def test_header_exports_and_bindings_agree(L):
    from mdqtplasmasims_amd._lib import SIGNATURES
    protos = header_prototypes()
    bound = {s[0]: s for s in SIGNATURES}
    ctype = {"int": C.c_int, "unsigned long long": C.c_ulonglong}
    for name, (ret, args) in NEW.items():
        assert protos.get(name) == (ret, args), name
        assert hasattr(L, name), name
        _, res, argtypes = bound[name]
        assert res is ctype[ret], name
        assert len(argtypes) == len(args), name
        assert argtypes[0] is C.c_void_p and all(a is C.POINTER(C.c_double) for a in argtypes[1:]), name
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == list(argtypes), name
    assert "SpeedUp:917-1032" in open(HEADER).read() and ":244-281" in open(HEADER).read()


def test_null_ensemble_is_refused_without_a_gpu(L):
    assert L.mdqt_ensemble_output(None) != 0 and b"NULL ensemble" in L.mdqt_last_error()
    assert L.mdqt_ensemble_observables(None, None, None, None) != 0 and b"NULL ensemble" in L.mdqt_last_error()
    assert L.mdqt_ensemble_epotential(None, None) != 0 and b"NULL ensemble" in L.mdqt_last_error()
    assert L.mdqt_ensemble_output_launches(None) == 0


def test_python_methods():
    from mdqtplasmasims_amd.ensemble import Ensemble
    for m in ("output", "observables", "epotential", "output_kernel_times"):
        assert callable(getattr(Ensemble, m)), m
    assert isinstance(Ensemble.output_launches, property)


def cli(*args):
    from mdqtplasmasims_amd._lib import CLI_PATH
    return subprocess.run([CLI_PATH, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["2", "-1", "x", "", "1x"])
def test_cli_rejects_bad_output_batch(L, value):
    r = cli("1", "--njobs=2", f"--output_batch={value}", "--N0=62", "--tmax=0.01")
    assert r.returncode == 2
    assert "usage: mdqt" in r.stderr and "--output_batch" in r.stderr
    assert r.stdout == ""


def test_cli_rejects_output_batch_without_njobs(L):
    r = cli("1", "--output_batch=1", "--N0=62", "--tmax=0.01")
    assert r.returncode == 2 and "usage: mdqt" in r.stderr and r.stdout == ""
