"""CPU checks of the MC + MD ensemble seam (include/mdmc.h "ensembles"; no GPU needed): job k's parameters,
the Python export, the command line's --njobs argument checks, and the header / binding pair."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mdmc.h")


@pytest.fixture(scope="module")
def L():
    from mdqtplasmasims_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.MDMC_CLI_PATH):
        from mdqtplasmasims_amd.build import build
        build(quiet=True)
    return _lib.lib()


def test_job_params_shift_job_and_seed_only(L):
    from mdqtplasmasims_amd import mdmc_job_params
    from mdqtplasmasims_amd._lib import MdmcParams
    from mdqtplasmasims_amd.mdmc import default_params
    base = default_params(qt_model=2, N=729, seed=501, job=7, Gamma=2.5, monteCarloSteps=123, saveDirectory="somewhere/")
    for k in (0, 1, 5, 1023):
        p = mdmc_job_params(base, k)
        assert (p.job, p.seed) == (7 + k, 501 + k)
        for name, _ in MdmcParams._fields_:
            if name not in ("job", "seed"):
                assert getattr(p, name) == getattr(base, name), name
    wrap = mdmc_job_params(default_params(seed=2**32 - 1, job=2**32 - 1), 2)     # uint32, as time(NULL) + job
    assert (wrap.job, wrap.seed) == (1, 1)


@pytest.mark.parametrize("k", [-1, 1024])
def test_job_params_index_out_of_range(L, k):
    from mdqtplasmasims_amd import MdqtError, mdmc_job_params
    from mdqtplasmasims_amd.mdmc import default_params
    with pytest.raises(MdqtError, match="job index"):
        mdmc_job_params(default_params(), k)


def test_job_params_null_arguments(L):
    from mdqtplasmasims_amd._lib import MdmcParams
    p = MdmcParams()
    assert L.mdmc_ensemble_job_params(None, 0, C.byref(p)) != 0
    assert L.mdmc_ensemble_job_params(C.byref(p), 0, None) != 0
    assert b"NULL" in L.mdqt_last_error()


def test_ensemble_is_exported():
    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd.mdmc_ensemble import MonteCarloEnsemble, mdmc_job_params
    assert M.MonteCarloEnsemble is MonteCarloEnsemble and "MonteCarloEnsemble" in M.__all__
    assert M.mdmc_job_params is mdmc_job_params and "mdmc_job_params" in M.__all__
    for m in ("init", "monte_carlo", "md_steps", "run", "kernel_times", "close", "__enter__", "__exit__"):
        assert callable(getattr(MonteCarloEnsemble, m, None)), m


def cli(*args):
    from mdqtplasmasims_amd._lib import MDMC_CLI_PATH
    return subprocess.run([MDMC_CLI_PATH, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["0", "-1", "x", "", "3x", "1025"])
def test_cli_rejects_bad_njobs(L, value):
    r = cli("1", f"--njobs={value}", "--N=512", "--monteCarloSteps=10")
    assert r.returncode == 2
    assert "usage: mdmc" in r.stderr and "--njobs" in r.stderr
    assert r.stdout == ""


def header_ensemble_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mdmc_ensemble_[A-Za-z0-9_]+)\s*\(", src)))


def test_header_declares_what_the_binding_binds(L):
    from mdqtplasmasims_amd._lib import MDMC_SIGNATURES, SIGNATURES
    bound = sorted(s[0] for s in SIGNATURES + MDMC_SIGNATURES if s[0].startswith("mdmc_ensemble_"))
    assert bound == header_ensemble_symbols()
    for s in ("mdmc_ensemble_job_params", "mdmc_ensemble_create", "mdmc_ensemble_destroy", "mdmc_ensemble_size",
              "mdmc_ensemble_job", "mdmc_ensemble_init", "mdmc_ensemble_monte_carlo", "mdmc_ensemble_md_steps",
              "mdmc_ensemble_run", "mdmc_ensemble_enable_timing", "mdmc_ensemble_kernel_times"):
        assert s in bound, s
        assert hasattr(L, s), s
