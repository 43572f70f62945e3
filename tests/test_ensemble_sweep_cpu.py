"""CPU checks of the parameter-sweep seam (include/mdqt.h "Parameter sweeps"; no GPU needed): member k's
parameters, every refusal mdqt_ensemble_create_sweep makes before it touches the device, the command line's
--sweep argument checks, and the header / binding / Python export."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mdqt.h")
SWEPT = ("detuning", "detuningDP", "Om", "OmDP", "fracOfSig")
NEW = ("mdqt_ensemble_create_sweep", "mdqt_ensemble_sweep_params", "mdqt_ensemble_points")


@pytest.fixture(scope="module")
def L():
    from mdqtplasmasims_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.CLI_PATH):
        from mdqtplasmasims_amd.build import build
        build(quiet=True)
    return _lib.lib()


def base_params(**kw):
    from mdqtplasmasims_amd import default_params
    return default_params(**dict(dict(N0=62, seed=501, job=7, tmax=0.25, density=0.5, saveDirectory="somewhere/"), **kw))


def points_of(*dicts, **base):
    """a C array of points: the base with each dict's fields"""
    from mdqtplasmasims_amd._lib import MdqtParams
    arr = (MdqtParams * len(dicts))()
    for q, d in enumerate(dicts):
        arr[q] = base_params(**dict(base, **d))
    return arr


def refused(L, arr, npoints, njobs, k=0):
    """the message of mdqt_ensemble_sweep_params' and of mdqt_ensemble_create_sweep's refusal (the same checks; the
    create entry makes them before any context or HIP call, so it fails the same way without a device)"""
    from mdqtplasmasims_amd._lib import MdqtParams
    out = MdqtParams()
    assert L.mdqt_ensemble_sweep_params(arr, npoints, njobs, k, C.byref(out)) != 0
    msg = L.mdqt_last_error().decode()
    h = C.c_void_p()
    assert L.mdqt_ensemble_create_sweep(arr, npoints, njobs, C.byref(h)) != 0 and not h.value
    created = L.mdqt_last_error().decode()
    assert created.replace("mdqt_ensemble_create_sweep", "mdqt_ensemble_sweep_params") == msg, (created, msg)
    return msg


# ---- member k's parameters ----
def test_sweep_params_point_major(L):
    from mdqtplasmasims_amd import sweep_params
    from mdqtplasmasims_amd._lib import MdqtParams
    base = base_params(Om=0.75)
    sweep = {"detuningDP": [0.0, 1.0], "Om": [0.5, 0.0, 1.0]}           # first-named axis slowest
    want = [(d, o) for d in (0.0, 1.0) for o in (0.5, 0.0, 1.0)]
    njobs = 3
    for k in range(len(want) * njobs):
        p = sweep_params(base, sweep, njobs, k)
        q, r = divmod(k, njobs)
        assert (p.detuningDP, p.Om) == want[q], k
        assert (p.job, p.seed) == (7 + r, 501 + r), k                  # per replica only: the points share job and seed
        for name, _ in MdqtParams._fields_:
            if name not in ("job", "seed", "detuningDP", "Om"):
                assert getattr(p, name) == getattr(base, name), name
    wrap = sweep_params(base_params(seed=2**32 - 1, job=2**32 - 1), {"Om": [0.5, 1.0]}, 3, 5)
    assert (wrap.job, wrap.seed, wrap.Om) == (1, 1, 1.0)


def test_sweep_params_one_point_is_job_params(L):
    from mdqtplasmasims_amd import job_params, sweep_params
    from mdqtplasmasims_amd._lib import MdqtParams
    base = base_params()
    for k in (0, 3):
        a, b = sweep_params(base, {"Om": [1.0]}, 4, k), job_params(base, k)
        for name, _ in MdqtParams._fields_:
            assert getattr(a, name) == getattr(b, name), name


@pytest.mark.parametrize("k", [-1, 4, 10**6])
def test_sweep_params_index_out_of_range(L, k):
    from mdqtplasmasims_amd import MdqtError, sweep_params
    with pytest.raises(MdqtError, match="job index"):
        sweep_params(base_params(), {"Om": [0.5, 1.0]}, 2, k)


def test_python_refuses_other_names_and_empty_lists(L):
    from mdqtplasmasims_amd import sweep_params
    with pytest.raises(ValueError, match="density"):
        sweep_params(base_params(), {"density": [1.0, 2.0]}, 2, 0)
    with pytest.raises(ValueError, match="Om"):
        sweep_params(base_params(), {"Om": []}, 2, 0)


# ---- refusals: point index and field ----
FIXED = [("Ge", 0.2), ("tmax", 0.5), ("density", 1.0), ("sig0", 3.0), ("Te", 25.0), ("N0", 63), ("newRun", 0), ("c0", 3),
         ("sampleFreq", 20), ("reNormalizewvFns", 1), ("qt_enabled", 0), ("seed", 502), ("job", 8), ("device", 1),
         ("rank", 1), ("force_segments", 2), ("saveDirectory", "elsewhere/"), ("tpumpreal", 1e-7), ("tstartV0", 3.0)]


@pytest.mark.parametrize("field, value", FIXED)
def test_refuses_a_fixed_field_that_differs(L, field, value):
    arr = points_of({"Om": 0.5}, {"Om": 0.75}, {"Om": 1.0, field: value})
    msg = refused(L, arr, 3, 2)
    assert "point 2 differs from point 0" in msg and re.search(rf"\bin {field}\b", msg), msg


def test_every_field_is_swept_or_fixed(L):
    """no field of mdqt_params is in neither list: a second point that differs from point 0 in one field alone is
    accepted where the field is swept and refused by that field's name where it is not"""
    from mdqtplasmasims_amd._lib import MdqtParams
    from mdqtplasmasims_amd.ensemble import SWEEP_FIELDS
    assert SWEEP_FIELDS == SWEPT
    swept = fixed = 0
    for name, ctype in MdqtParams._fields_:
        arr = points_of({}, {}, fracOfSig=1.0)                         # (non-zero: fracOfSig + 0.5 stays on its side of 0)
        old = getattr(arr[0], name)
        setattr(arr[1], name, b"elsewhere/" if isinstance(old, bytes) else old + (0.5 if ctype is C.c_double else 1))
        if name in SWEEP_FIELDS:                                       # + 0.5: x 100 another integer
            out = MdqtParams()
            assert L.mdqt_ensemble_sweep_params(arr, 2, 1, 1, C.byref(out)) == 0, (name, L.mdqt_last_error())
            assert getattr(out, name) == old + 0.5
            swept += 1
        else:
            msg = refused(L, arr, 2, 1)
            assert re.search(rf"point 1 differs from point 0 in {name}\b", msg), (name, msg)
            fixed += 1
    assert (fixed, swept) == (22, 5) and fixed + swept == len(MdqtParams._fields_)


def test_sweep_params_three_axes_against_itertools(L):
    import itertools
    from mdqtplasmasims_amd import sweep_params
    sweep = {"detuningDP": [0.0, 1.0], "Om": [0.5, 0.75, 1.0], "detuning": [-1.0, -2.0]}   # lengths 2, 3, 2
    want = list(itertools.product(*sweep.values()))
    assert len(want) == 12
    for k in range(24):
        p = sweep_params(base_params(), sweep, 2, k)
        assert (p.detuningDP, p.Om, p.detuning) == want[k // 2] and p.job == 7 + k % 2, k


def test_parse_sweep_args():
    from mdqtplasmasims_amd._sweep import parse_sweep_args
    assert parse_sweep_args([]) == {}
    got = parse_sweep_args(["Om:0.5,1", "detuning:-1"])
    assert got == {"Om": [0.5, 1.0], "detuning": [-1.0]} and list(got) == ["Om", "detuning"]   # the order given
    for bad in (["Om:0.5", "Om:1"], ["Om:"], ["Om"]):                  # a NAME twice, an empty list, no list
        with pytest.raises(ValueError, match="each NAME once"):
            parse_sweep_args(bad)
    with pytest.raises(ValueError):
        parse_sweep_args(["Om:1,x"])


@pytest.mark.parametrize("field, value, word", [("world_size", 2, "world_size"), ("rng_mode", 0, "rng_mode"),
                                                 ("qt_model", 1, "qt_model")])
def test_refuses_what_the_ensemble_refuses(L, field, value, word):
    from mdqtplasmasims_amd._lib import MdqtParams
    arr = points_of({"Om": 0.5}, {"Om": 1.0}, **{field: value})        # on every point: mdqt_ensemble_create's message
    msg = refused(L, arr, 2, 2)
    h = C.c_void_p()
    one = MdqtParams()
    C.memmove(C.byref(one), C.byref(arr[0]), C.sizeof(MdqtParams))
    assert L.mdqt_ensemble_create(C.byref(one), 2, C.byref(h)) != 0
    plain = L.mdqt_last_error().decode()
    assert word in msg and msg.split(": ", 1)[1] == plain.split(": ", 1)[1]
    arr = points_of({"Om": 0.5}, {"Om": 1.0, field: value})            # on one point only: the field, by point
    msg = refused(L, arr, 2, 2)
    assert "point 1 differs from point 0" in msg and word in msg


@pytest.mark.parametrize("fracs, q", [((0.0, 0.5), 1), ((0.5, 1.0, 0.0), 2), ((0.0, 0.0, 1.0), 2)])
def test_refuses_mixed_frac_of_sig(L, fracs, q):
    arr = points_of(*({"fracOfSig": f, "Om": 0.5 + 0.1 * i} for i, f in enumerate(fracs)))
    msg = refused(L, arr, len(fracs), 2)
    assert f"point {q} has fracOfSig" in msg and "instance" in msg and "not supported" in msg, msg


def test_accepts_frac_of_sig_all_nonzero_or_all_zero(L):
    from mdqtplasmasims_amd._lib import MdqtParams
    out = MdqtParams()
    for fr in ((0.5, 1.0), (0.0, 0.0)):
        arr = points_of({"fracOfSig": fr[0], "Om": 0.5}, {"fracOfSig": fr[1], "Om": 1.0})
        assert L.mdqt_ensemble_sweep_params(arr, 2, 2, 3, C.byref(out)) == 0, L.mdqt_last_error()
        assert (out.fracOfSig, out.Om, out.job, out.seed) == (fr[1], 1.0, 8, 502)


@pytest.mark.parametrize("field, a, b", [("detuning", -1.001, -1.002), ("detuningDP", 0.001, 0.002), ("Om", 1.0, 1.004),
                                         ("OmDP", 0.5, 0.509), ("fracOfSig", 0.5, 0.501)])
def test_refuses_a_directory_collision(L, field, a, b):
    arr = points_of({"Om": 0.25}, {field: a}, {field: b}, fracOfSig=1.0)   # (point 0: another directory)
    msg = refused(L, arr, 3, 1)
    assert "point 2 and point 1 give the same run directory name" in msg and field in msg, msg


def test_refuses_identical_points(L):
    arr = points_of({"Om": 0.5}, {"Om": 1.0}, {"Om": 0.5})
    msg = refused(L, arr, 3, 2)
    assert "point 2 is identical to point 0" in msg
    for f in SWEPT:
        assert f in msg


@pytest.mark.parametrize("npoints, njobs, word", [(0, 2, "npoints"), (-1, 2, "npoints"), (2, 0, "njobs"), (2, -5, "njobs"),
                                                  (2, 513, "1024"), (1, 1025, "1024")])
def test_refuses_sizes(L, npoints, njobs, word):
    arr = points_of({"Om": 0.5}, {"Om": 1.0})
    assert word in refused(L, arr, npoints, njobs)


def test_the_largest_sweep_passes_validation(L):
    from mdqtplasmasims_amd._lib import MdqtParams
    oms = [0.01 * i + 0.005 for i in range(512)]                       # x 100: i + 0.5, no two alike as integers
    arr = points_of(*({"Om": om} for om in oms))
    out = MdqtParams()
    assert L.mdqt_ensemble_sweep_params(arr, 512, 2, 1023, C.byref(out)) == 0, L.mdqt_last_error()
    assert (out.Om, out.job) == (oms[511], 8)


def test_null_arguments(L):
    from mdqtplasmasims_amd._lib import MdqtParams
    p, h = MdqtParams(), C.c_void_p()
    arr = points_of({"Om": 0.5})
    assert L.mdqt_ensemble_sweep_params(None, 1, 1, 0, C.byref(p)) != 0 and b"NULL" in L.mdqt_last_error()
    assert L.mdqt_ensemble_sweep_params(arr, 1, 1, 0, None) != 0 and b"NULL" in L.mdqt_last_error()
    assert L.mdqt_ensemble_create_sweep(None, 1, 1, C.byref(h)) != 0 and b"NULL" in L.mdqt_last_error()
    assert L.mdqt_ensemble_create_sweep(arr, 1, 1, None) != 0 and b"NULL" in L.mdqt_last_error()
    assert L.mdqt_ensemble_points(None) == -1


# ---- the command line ----
def cli(*args):
    from mdqtplasmasims_amd._lib import CLI_PATH
    return subprocess.run([CLI_PATH, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args", [
    ("--sweep=detuningDP:0,1",),                                        # without --njobs
    ("--sweep=detuningDP:0,1", "--njobs=2", "--pump_program=1"),
    ("--pump_program=2", "--pump_jobs=2", "--sweep=Om:0.5,1"),
    ("--njobs=2", "--sweep=density:1,2"),                               # not sweepable
    ("--njobs=2", "--sweep=nothing:1,2"),
    ("--njobs=2", "--sweep=Omx:1,2"),
    ("--njobs=2", "--sweep=Om"),
    ("--njobs=2", "--sweep=Om:"),                                       # empty list
    ("--njobs=2", "--sweep=Om:1,,2"),
    ("--njobs=2", "--sweep=Om:1,2,"),
    ("--njobs=2", "--sweep=Om:1,x"),                                    # not a number
    ("--njobs=2", "--sweep=Om:1e"),
    ("--njobs=2", "--sweep=Om:0.5,1", "--sweep=Om:2,3"),                # a NAME twice
    ("--njobs=2", "--sweep=Om:" + ",".join(str(0.01 * i) for i in range(513))),          # 1026 members
    ("--njobs=256", "--sweep=Om:0.5,1,2", "--sweep=detuningDP:0,1"),                     # 1536 members
])
def test_cli_rejects_bad_sweeps(L, args):
    r = cli("1", *args, "--N0=62", "--tmax=0.01")
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "usage: mdqt" in r.stderr and "--sweep=NAME:v1,v2" in r.stderr
    assert r.stdout == ""


# ---- header, binding, export ----
def test_header_binding_and_export(L):
    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd._lib import SIGNATURES
    from mdqtplasmasims_amd.ensemble import Ensemble, sweep_params
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    bound = {s[0] for s in SIGNATURES}
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in bound and hasattr(L, name), name
    assert M.sweep_params is sweep_params and "sweep_params" in M.__all__
    for m in ("member", "set_option", "init", "run"):
        assert hasattr(Ensemble, m), m
    assert "sweep" in Ensemble.__init__.__code__.co_varnames
    assert "points" in Ensemble.__init__.__code__.co_names               # set in __init__: Ensemble(...).points
