"""CPU checks of the ensemble seam (include/mdqt.h "ensembles"; no GPU needed): job k's parameters, the
Python export, the command line's --njobs argument checks, and the header / binding pair."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mdqt.h")


@pytest.fixture(scope="module")
def L():
    from mdqtplasmasims_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.CLI_PATH):
        from mdqtplasmasims_amd.build import build
        build(quiet=True)
    return _lib.lib()


def test_job_params_shift_job_and_seed_only(L):
    from mdqtplasmasims_amd import default_params, job_params
    from mdqtplasmasims_amd._lib import MdqtParams
    base = default_params(N0=62, seed=501, job=7, tmax=0.25, density=0.5, saveDirectory="somewhere/")
    for k in (0, 1, 5, 1023):
        p = job_params(base, k)
        assert (p.job, p.seed) == (7 + k, 501 + k)
        for name, _ in MdqtParams._fields_:
            if name not in ("job", "seed"):
                assert getattr(p, name) == getattr(base, name), name
    wrap = job_params(default_params(seed=2**32 - 1, job=2**32 - 1), 2)     # uint32, as time(NULL) + job
    assert (wrap.job, wrap.seed) == (1, 1)


@pytest.mark.parametrize("k", [-1, 1024, 10**6])
def test_job_params_index_out_of_range(L, k):
    from mdqtplasmasims_amd import MdqtError, default_params, job_params
    with pytest.raises(MdqtError, match="job index"):
        job_params(default_params(), k)


def test_job_params_null_arguments(L):
    from mdqtplasmasims_amd._lib import MdqtParams
    p = MdqtParams()
    assert L.mdqt_ensemble_job_params(None, 0, C.byref(p)) != 0
    assert L.mdqt_ensemble_job_params(C.byref(p), 0, None) != 0
    assert b"NULL" in L.mdqt_last_error()


def test_ensemble_is_exported():
    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd.ensemble import Ensemble
    assert M.Ensemble is Ensemble and "Ensemble" in M.__all__
    for m in ("init", "forces", "substeps", "md_steps", "run", "synchronize", "close", "kernel_times",
              "__enter__", "__exit__", "N"):
        assert hasattr(Ensemble, m), m


def cli(*args):
    from mdqtplasmasims_amd._lib import CLI_PATH
    return subprocess.run([CLI_PATH, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["0", "-1", "-64", "x", "", "3x", "1025"])
def test_cli_rejects_bad_njobs(L, value):
    r = cli("1", f"--njobs={value}", "--N0=62", "--tmax=0.01")
    assert r.returncode == 2
    assert "usage: mdqt" in r.stderr and "--njobs" in r.stderr
    assert r.stdout == ""


@pytest.mark.parametrize("order", [("--njobs=2", "--pump_program=1"), ("--pump_program=3", "--njobs=2")])
def test_cli_rejects_njobs_with_pump_program(L, order):
    r = cli("1", *order)
    assert r.returncode == 2
    assert "usage: mdqt" in r.stderr


def header_ensemble_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mdqt_ensemble_[A-Za-z0-9_]+)\s*\(", src)))


def test_header_declares_what_the_binding_binds(L):
    from mdqtplasmasims_amd._lib import SIGNATURES
    bound = sorted(s[0] for s in SIGNATURES if s[0].startswith("mdqt_ensemble_"))
    assert bound == header_ensemble_symbols()
    for s in ("mdqt_ensemble_job_params", "mdqt_ensemble_create", "mdqt_ensemble_destroy", "mdqt_ensemble_size",
              "mdqt_ensemble_job", "mdqt_ensemble_init", "mdqt_ensemble_forces", "mdqt_ensemble_substeps",
              "mdqt_ensemble_md_steps", "mdqt_ensemble_run", "mdqt_ensemble_synchronize",
              "mdqt_ensemble_enable_timing", "mdqt_ensemble_kernel_times"):
        assert s in bound, s
        assert hasattr(L, s), s
