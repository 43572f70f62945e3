"""What the ensemble GPU tests share: an ensemble's members against the same jobs on contexts of their own, bit
for bit and byte for byte (test_gpu_jobs_ensemble, test_gpu_pump_ensemble, test_gpu_ensemble_output,
test_gpu_mdmc_ensemble, _md, _qt).  No fixtures here: a plain module, imported as `from tests import
ensemble_helpers`."""
import os

import numpy as np


def snapshot(sim):
    """a context's state and counters"""
    st = sim.get_state()
    c = sim.counters()
    return dict(st, qstep=sim.qstep_index, c0=c["c0"], counter=c["counter"], Epot=c["Epot"], Epot0=c["Epot0"],
                N=sim.N)


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), f"{what}: {k} differs"


def member_params(params, k):
    """job k of an ensemble of `params` (mdqt_ensemble_job_params: seed + k, job + k)"""
    return dict(params, seed=params["seed"] + k, job=params["job"] + k)


def tree(root):
    """every file below root: relative path -> bytes"""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def assert_same_trees(a, b):
    ta, tb = tree(a), tree(b)
    assert sorted(ta) == sorted(tb), (sorted(ta), sorted(tb))
    assert ta, "no files written"
    for f in ta:
        assert ta[f] == tb[f], f"{f} differs"
