"""CPU checks of the pump ensemble's seam (include/mdqt.h "ensembles of the optical-pumping programs"; no GPU
needed): the header / binding pair, the Python export and the command line's --pump_jobs argument checks."""
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


def header_pump_ensemble_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mdqt_pump_ensemble_[A-Za-z0-9_]+)\s*\(", src)))


def test_header_declares_what_the_binding_binds(L):
    from mdqtplasmasims_amd._lib import SIGNATURES
    bound = sorted(s[0] for s in SIGNATURES if s[0].startswith("mdqt_pump_ensemble_"))
    assert bound == header_pump_ensemble_symbols()
    for s in ("create", "destroy", "size", "job", "set_option", "init", "md_steps", "qsteps", "tag_spin_up", "output",
              "run", "synchronize", "launches", "enable_timing", "kernel_times"):
        assert "mdqt_pump_ensemble_" + s in bound, s
        assert hasattr(L, "mdqt_pump_ensemble_" + s), s
    assert "mdqt_pump_md_steps" in {s[0] for s in SIGNATURES} and hasattr(L, "mdqt_pump_md_steps")


def test_pump_ensemble_is_exported():
    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd.pump_ensemble import PumpEnsemble
    assert M.PumpEnsemble is PumpEnsemble and "PumpEnsemble" in M.__all__
    for m in ("init", "md_steps", "qsteps", "tag_spin_up", "output", "run", "synchronize", "launches", "kernel_times",
              "close", "__enter__", "__exit__", "N"):
        assert hasattr(PumpEnsemble, m), m
    assert hasattr(M.Simulation, "pump_md_steps")


def cli(*args):
    from mdqtplasmasims_amd._lib import CLI_PATH
    return subprocess.run([CLI_PATH, *args], capture_output=True, text=True, timeout=60)


def refused(r):
    assert r.returncode == 2
    assert "usage: mdqt" in r.stderr and "--pump_jobs" in r.stderr
    assert r.stdout == ""


def test_cli_rejects_pump_jobs_without_pump_program(L):
    refused(cli("1", "--pump_jobs=2", "--N0=62", "--tmax=0.01"))


@pytest.mark.parametrize("order", [("--pump_program=1", "--pump_jobs=2", "--njobs=2"),
                                   ("--njobs=2", "--pump_jobs=2", "--pump_program=2")])
def test_cli_rejects_pump_jobs_with_njobs(L, order):
    refused(cli("1", *order))


@pytest.mark.parametrize("value", ["0", "-1", "x", "", "3x", "1025"])
def test_cli_rejects_bad_pump_jobs(L, value):
    refused(cli("1", "--pump_program=1", f"--pump_jobs={value}", "--N0=62", "--tmax=0.01"))


def test_cli_still_rejects_njobs_with_pump_program(L):
    refused(cli("1", "--njobs=2", "--pump_program=1"))
