"""mdqt_set_option, option by option (mdqt_options.cpp: one table row per option).

For every option: the values just outside its range are rejected with an error that names it, both ends of
the range are accepted, and where mdqt_get_const reports the same name the value reads back.  Then, with
every option back at its default, two MD steps leave a state bit-identical to a fresh Simulation's of the
same seed: setting and restoring options leaves no residue (pending partials, measured tail sums, buffers
and tables sized by the old value — what each row's settle / reset / ensure_aux guards)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (option, lo, hi, default)
OPTIONS = [
    ("force_scheme", 0, 3, 0),          # value 2 needs world_size 1
    ("expt_force_sig", 0, 1, 0),
    ("potential_n3", 0, 1, 1),
    ("force_n3b_pairs", 0, 1, 1),
    ("potential_plan", 0, 1, 1),
    ("qt_im01", 0, 1, None),            # 1 only with purely imaginary static slots; default: what create chose
    ("fused_step", 0, 1, 0),
    ("overlap", 0, 1, 0),
    ("force_ufar_exp", 0, 300, 13),
    ("force_vfar_exp", 0, 300, 13),
    ("force_mid_exp", 0, 300, 13),
    ("force_far_exp", 0, 300, 13),
    ("force_tail_exp", 0, 300, 12),
    ("force_form_mode", 0, 2, 2),
    ("force_tail_mode", 0, 1, 1),
    ("force_balance", 0, 1, 1),
    ("force_tile_split", 0, 2, 1),
    ("force_split_cus", 0, 65536, 0),
    ("force_reduce_mask", 0, 1, 1),
    ("force_ax1", 0, 1, 1),
    ("force_sort", 0, 2, 1),
    ("qt_enabled", 0, 1, 1),
    ("qt_math", 0, 2, 2),               # a non-zero qt_model needs 2
    ("force_kernel", 0, 1, 1),
    ("init_threads", 0, 256, 0),
    ("substep_kernel", 0, 2, 0),
]
SEED = 4242


def _gpu():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


def _reads_back(s, name, value):
    """mdqt_get_const of the option's own name, where it has one (NaN: it has none)"""
    got = s.const(name)
    if math.isnan(got):
        return
    want = value
    if name == "force_scheme" and value == 0:
        want = 1                        # the constant is the scheme in effect: auto takes the rows below 128 ions
    assert got == want, (name, value, got)


def test_every_option_range_readback_and_no_residue():
    M = _gpu()
    s = M.Simulation(N0=100, seed=SEED, job=1).init()
    assert 64 < s.N < 128               # more than one tile, the rows scheme by default
    defaults = {name: (s.const(name) if d is None else d) for name, _, _, d in OPTIONS}
    for name, lo, hi, _ in OPTIONS:
        if name != "force_sort":
            _reads_back(s, name, defaults[name])        # the defaults written above are the engine's
        for bad in (lo - 1, hi + 1):
            with pytest.raises(M.MdqtError, match=name):
                s.set_option(name, bad)
        if name == "force_sort":
            s.set_option("force_scheme", 3)             # the constant reports the order of the block scheme only
        for value in (lo, hi):
            if name == "qt_im01" and value == 1:
                try:
                    s.set_option(name, value)
                except M.MdqtError as e:
                    assert "not purely imaginary" in str(e)
                    continue
            else:
                s.set_option(name, value)
            _reads_back(s, name, value)
        s.set_option(name, int(defaults[name]))
        if name == "force_sort":
            s.set_option("force_scheme", 0)
    with pytest.raises(M.MdqtError, match="unknown option"):
        s.set_option("no_such_option", 0)
    for name, _, _, _ in OPTIONS:
        if name != "force_sort":
            _reads_back(s, name, defaults[name])
    fresh = M.Simulation(N0=100, seed=SEED, job=1).init()
    s.md_steps(2)
    fresh.md_steps(2)
    a, b = s.get_state(), fresh.get_state()
    for key in ("R", "V", "F", "psi", "tPart"):
        assert np.array_equal(a[key], b[key]), key
    assert a["t"] == b["t"] and s.qstep_index == fresh.qstep_index
    s.close()
    fresh.close()


def test_ensemble_forwards_options_and_keeps_qt_waves():
    M = _gpu()
    e = M.Ensemble(njobs=2, N0=100, seed=SEED, job=1).init()
    e.forces()
    fast = [j.get_state()["F"] for j in e.jobs]
    e.set_option("force_kernel", 0)                      # not the ensemble's own: every member's
    e.forces()
    for k, j in enumerate(e.jobs):
        alone = M.Simulation(N0=100, seed=SEED + k, job=1 + k).init()
        alone.set_option("force_kernel", 0)
        alone.forces()
        exact = alone.get_state()["F"]
        alone.close()
        got = j.get_state()["F"]
        assert np.array_equal(got, exact), k             # the member ran the exact pair form
        assert not np.array_equal(got, fast[k]), k       # ... which is not the fast one's bits
    with pytest.raises(M.MdqtError, match="unknown option"):
        e.set_option("no_such_option", 0)
    for value in (0, 3):
        e.set_option("qt_waves", value)
    for bad in (-1, 1, 2, 4):
        with pytest.raises(M.MdqtError, match="qt_waves"):
            e.set_option("qt_waves", bad)
    e.close()
