"""CPU checks of the MC + MD ensemble's md_batch switch (include/mdmc.h "ensembles"; no GPU needed, argument
parsing comes first): the command line's --md_batch argument, the NULL-ensemble refusal of the C ABI, and the
Python export."""
import ctypes as C
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def L():
    from mdqtplasmasims_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.MDMC_CLI_PATH):
        from mdqtplasmasims_amd.build import build
        build(quiet=True)
    return _lib.lib()


def cli(*args):
    from mdqtplasmasims_amd._lib import MDMC_CLI_PATH
    return subprocess.run([MDMC_CLI_PATH, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["2", "-1", "", "x", "01", "1x"])
def test_cli_rejects_md_batch_values_other_than_0_and_1(L, value):
    r = cli("1", "--njobs=2", f"--md_batch={value}", "--N=512", "--monteCarloSteps=10")
    assert r.returncode == 2
    assert "usage: mdmc" in r.stderr and "--md_batch" in r.stderr
    assert r.stdout == ""


@pytest.mark.parametrize("value", ["0", "1"])
def test_cli_rejects_md_batch_without_njobs(L, value):
    r = cli("1", f"--md_batch={value}", "--N=512", "--monteCarloSteps=10")
    assert r.returncode == 2
    assert "usage: mdmc" in r.stderr and "--md_batch" in r.stderr
    assert r.stdout == ""


def test_null_ensemble_is_an_error(L):
    assert L.mdmc_ensemble_set_md_batch(None, 1) != 0
    assert b"mdmc_ensemble_set_md_batch" in L.mdqt_last_error() and b"NULL" in L.mdqt_last_error()
    assert L.mdmc_ensemble_md_batch(None) < 0
    n = C.c_ulonglong(7)
    assert L.mdmc_ensemble_md_launches(None, C.byref(n)) != 0
    assert n.value == 7


def test_python_exports_the_switch():
    from mdqtplasmasims_amd.mdmc_ensemble import MonteCarloEnsemble
    assert isinstance(MonteCarloEnsemble.md_batch, property) and MonteCarloEnsemble.md_batch.fset is not None
    assert callable(MonteCarloEnsemble.md_launches)
