"""CPU checks of the batched QT seam of the MC + MD ensemble (include/mdmc.h, "ensembles of the QT tagging
variants"; no GPU needed): every mdmc_ensemble_* function the header declares is exported by the library and bound
in _lib.py with the arity the header gives it, and MonteCarloEnsemble has the methods."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mdmc.h")
NEW = {"mdmc_ensemble_qsteps": 2, "mdmc_ensemble_tag_qt": 3, "mdmc_ensemble_tagged_moments_qt": 3,
       "mdmc_ensemble_qt_launches": 2}


@pytest.fixture(scope="module")
def L():
    from mdqtplasmasims_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mdqtplasmasims_amd.build import build
        build(quiet=True)
    return _lib.lib()


def header_ensemble_functions():
    """{name: number of parameters} of the header's mdmc_ensemble_* declarations"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(","))
            for m in re.finditer(r"\b(mdmc_ensemble_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_header_declares_what_the_binding_binds(L):
    from mdqtplasmasims_amd._lib import MDMC_SIGNATURES
    declared = header_ensemble_functions()
    bound = {s[0]: len(s[2]) for s in MDMC_SIGNATURES if s[0].startswith("mdmc_ensemble_")}
    assert bound == declared
    for name, nargs in NEW.items():
        assert declared.get(name) == nargs, name
        assert hasattr(L, name), name


def test_the_ensemble_class_has_the_qt_methods():
    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd.mdmc_ensemble import MonteCarloEnsemble
    assert M.MonteCarloEnsemble is MonteCarloEnsemble
    for m in ("qsteps", "tag_qt", "tagged_moments_qt", "qt_launches", "md_launches", "md_steps", "run", "kernel_times"):
        assert callable(getattr(MonteCarloEnsemble, m, None)), m
    doc = __import__("mdqtplasmasims_amd.mdmc_ensemble", fromlist=["x"]).__doc__
    for name in NEW:
        assert name in doc, name
