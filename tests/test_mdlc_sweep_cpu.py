"""CPU checks of the three-level laser-cooling program's parameter scan (mdlc_create_sweep, include/mdlc.h; no
GPU needed): the header / library / binding triple, the member order of mdlc_sweep_params, every refusal's
wording (the point and the field), and the command line's --sweep with --print-directory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mdlc.h")
NEW = ("mdlc_create_sweep", "mdlc_sweep_params")


@pytest.fixture(scope="module")
def L():
    from mdqtplasmasims_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mdqtplasmasims_amd.build import build
        build(quiet=True)
    return _lib.lib()


def points(values, **over):
    """one point per dict of `values`, every other field from the defaults with `over`"""
    from mdqtplasmasims_amd.mdlc import default_params
    return [default_params(**{**over, **v}) for v in values]


def refusal(pts, k=0):
    from mdqtplasmasims_amd import MdqtError
    from mdqtplasmasims_amd.mdlc import sweep_params
    with pytest.raises(MdqtError) as e:
        sweep_params(pts, k)
    return str(e.value)


# ---- 1. header, library and binding ----
def test_header_library_and_binding(L):
    from mdqtplasmasims_amd._lib import LIB_PATH, MDLC_SIGNATURES
    import ctypes as C
    from mdqtplasmasims_amd._lib import MdlcParams
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+mdlc_create_sweep\s*\(\s*const\s+mdlc_params\s*\*\s*points\s*,\s*int\s+npoints\s*,\s*"
                     r"mdlc_ctx\s*\*\*\s*out\s*\)\s*;", src)
    assert re.search(r"\bint\s+mdlc_sweep_params\s*\(\s*const\s+mdlc_params\s*\*\s*points\s*,\s*int\s+npoints\s*,\s*"
                     r"int\s+k\s*,\s*mdlc_params\s*\*\s*out\s*\)\s*;", src)
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (mdlc_[A-Za-z0-9_]+)$", nm, flags=re.M))
    assert set(NEW) <= exported
    sig = {s[0]: s[1:] for s in MDLC_SIGNATURES}
    pp = C.POINTER(MdlcParams)
    assert sig["mdlc_create_sweep"] == (C.c_int, [pp, C.c_int, C.POINTER(C.c_void_p)])
    assert sig["mdlc_sweep_params"] == (C.c_int, [pp, C.c_int, C.c_int, pp])
    for name in NEW:
        assert getattr(L, name).restype is C.c_int and list(getattr(L, name).argtypes) == sig[name][1]


def test_python_surface(L):
    import mdqtplasmasims_amd as M
    from mdqtplasmasims_amd.mdlc import SWEEP_FIELDS, sweep_params
    assert SWEEP_FIELDS == ("detuning", "Om", "temperature")
    assert M.mdlc_sweep_params is sweep_params and "mdlc_sweep_params" in M.__all__


# ---- 2. member order ----
def test_sweep_params_member_order(L):
    from mdqtplasmasims_amd.mdlc import default_params, format_directory, sweep_params
    vals = [dict(detuning=-0.5, Om=0.5), dict(detuning=-1.25, Om=1.5), dict(detuning=0.5, Om=0.5, temperature=0.0025)]
    pts = points(vals, njobs=2, job=7, seed=99, N0=70, saveDirectory="out/")
    base = default_params(njobs=2, job=7, seed=99, N0=70, saveDirectory="out/")
    for k in range(6):
        q, r = divmod(k, 2)                               # point-major
        p = sweep_params(pts, k)
        assert (p.detuning, p.Om) == (vals[q]["detuning"], vals[q]["Om"])
        assert p.temperature == vals[q].get("temperature", 0.01)
        assert p.job == 7 + r and p.njobs == 1 and p.seed == 99
        for f in ("N0", "tmax", "applyForce", "sampleFreq", "vKick", "dt", "device", "saveDirectory"):
            assert getattr(p, f) == getattr(base, f), f
        assert format_directory(p) == (f"out/Om{int(vals[q]['Om'] * 100)}/Det{int(vals[q]['detuning'] * 100)}NumIons70"
                                       f"InitialTemp{2500 if q == 2 else 10000}uK/job{7 + r}/")


# ---- 3. refusals: each names the point and the field ----
def test_refuses_a_fixed_field_that_differs(L):
    pts = points([dict(detuning=-0.5), dict(detuning=-1.0)], njobs=2)
    pts[1].N0 = 999
    msg = refusal(pts)
    assert "point 1 differs from point 0 in N0" in msg and "only detuning, Om and temperature may differ" in msg
    pts = points([dict(detuning=-0.5), dict(detuning=-1.0), dict(detuning=-1.5)], njobs=2)
    pts[2].vKick = 0.002
    msg = refusal(pts)
    assert "point 2 differs from point 0 in vKick" in msg and "no level for vKick" in msg


def test_every_field_is_swept_or_fixed(L):
    """no field of mdlc_params is in neither list: a second point that differs from point 0 in one field alone is
    accepted where the field is swept and refused by that field's name where it is not"""
    import ctypes as C
    from mdqtplasmasims_amd._lib import MdlcParams
    from mdqtplasmasims_amd.mdlc import SWEEP_FIELDS, sweep_params
    swept = fixed = 0
    for name, ctype in MdlcParams._fields_:
        pts = points([{}, {}], njobs=2)
        old = getattr(pts[0], name)
        setattr(pts[1], name, b"elsewhere/" if isinstance(old, bytes) else old + (0.5 if ctype is C.c_double else 1))
        if name in SWEEP_FIELDS:                              # + 0.5: x 100 (x 1000000) another integer
            assert getattr(sweep_params(pts, 2), name) == old + 0.5, name
            swept += 1
        else:
            assert re.search(rf"point 1 differs from point 0 in {name}\b", refusal(pts)), name
            fixed += 1
    assert (fixed, swept) == (11, 3) and fixed + swept == len(MdlcParams._fields_)


def test_refuses_identical_points(L):
    pts = points([dict(detuning=-0.5), dict(detuning=-1.0), dict(detuning=-0.5)])
    msg = refusal(pts)
    assert "point 2 is identical to point 0" in msg and "detuning, Om and temperature all equal" in msg


def test_refuses_colliding_directory_names(L):
    from mdqtplasmasims_amd.mdlc import format_directory
    pts = points([dict(detuning=-0.501), dict(detuning=-0.502)])
    assert format_directory(pts[0]) == format_directory(pts[1])           # why: (unsigned)(-50.1) = (unsigned)(-50.2)
    msg = refusal(pts)
    assert "point 1 and point 0 give the same run directory name" in msg
    assert "detuning -0.502 and -0.501" in msg
    # temperature's level is uK: 0.01 and 0.0100004 K print alike, 0.01 and 0.010002 K do not
    assert "temperature" in refusal(points([dict(temperature=0.01), dict(temperature=0.0100004)]))
    from mdqtplasmasims_amd.mdlc import sweep_params
    assert sweep_params(points([dict(temperature=0.01), dict(temperature=0.010002)]), 1).temperature == 0.010002


def test_refuses_no_points_and_a_member_out_of_range(L):
    assert "npoints must be >= 1" in refusal([])
    pts = points([dict(Om=0.5), dict(Om=1.0)], njobs=3)
    assert "member index 6 outside [0, 6)" in refusal(pts, 6)
    assert "member index -1 outside [0, 6)" in refusal(pts, -1)


def test_refuses_what_create_refuses_in_its_own_words(L):
    msg = refusal(points([dict(temperature=0.01), dict(temperature=-0.01)]))
    assert "point 1: temperature must be >= 0" in msg
    assert "point 0: njobs must be >= 1" in refusal(points([dict(Om=0.5), dict(Om=1.0)], njobs=0))


def test_refuses_a_grid_past_the_launch_limit(L):
    # 2^31 - 1 workgroups at the most: 4 workgroups per job x 2^28 replicas x 2 points
    pts = points([dict(Om=0.5), dict(Om=1.0)], N0=1024, njobs=2 ** 28)
    assert "too large for one launch grid" in refusal(pts)


def test_python_refuses_a_field_that_is_not_swept(L):
    from mdqtplasmasims_amd import LaserCooling
    with pytest.raises(ValueError, match="'vKick' is not one of detuning, Om, temperature"):
        LaserCooling(sweep={"vKick": [1, 2]})
    with pytest.raises(ValueError, match="no values for 'Om'"):
        LaserCooling(sweep={"Om": []})


def test_create_sweep_refuses_before_any_gpu_call(L):
    """the refusal is the points', not the missing device's"""
    from mdqtplasmasims_amd import LaserCooling, MdqtError
    with pytest.raises(MdqtError, match="point 1 and point 0 give the same run directory name"):
        LaserCooling(sweep={"detuning": [-0.501, -0.502]})


# ---- 4. the command line ----
def test_cli_print_directory_of_a_scan(L):
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    from mdqtplasmasims_amd.mdlc import format_directory, sweep_params
    r = subprocess.run([MDLC_CLI_PATH, "3", "--print-directory=1", "--njobs=2", "--sweep=detuning:-0.5,-1",
                        "--sweep=Om:0.5,1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    pts = points([dict(detuning=d, Om=o) for d in (-0.5, -1) for o in (0.5, 1)], njobs=2, job=3)   # first name slowest
    want = [format_directory(sweep_params(pts, k)) for k in range(8)]
    assert got == want
    assert len(set(got)) == 8
    assert got[0] == "dataLaserCoolTestDoppShift/Om50/Det-50NumIons1000InitialTemp10000uK/job3/"
    assert got[3] == "dataLaserCoolTestDoppShift/Om100/Det-50NumIons1000InitialTemp10000uK/job4/"
    assert got[4] == "dataLaserCoolTestDoppShift/Om50/Det-100NumIons1000InitialTemp10000uK/job3/"


def test_cli_print_directory_of_three_axes(L):
    """axis lengths 2, 3 and 2: the command line's product against Python's, the first-given NAME slowest"""
    import itertools
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    from mdqtplasmasims_amd.mdlc import format_directory, sweep_params
    axes = {"Om": (0.5, 1), "temperature": (0.01, 0.02, 0.03), "detuning": (-0.5, -1)}
    r = subprocess.run([MDLC_CLI_PATH, "3", "--print-directory=1", "--njobs=2",
                        *(f"--sweep={n}:{','.join(map(str, v))}" for n, v in axes.items())], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    pts = points([dict(zip(axes, v)) for v in itertools.product(*axes.values())], njobs=2, job=3)
    assert got == [format_directory(sweep_params(pts, k)) for k in range(24)]
    assert len(set(got)) == 24
    assert got[2] == "dataLaserCoolTestDoppShift/Om50/Det-100NumIons1000InitialTemp10000uK/job3/"   # last NAME fastest
    assert got[4] == "dataLaserCoolTestDoppShift/Om50/Det-50NumIons1000InitialTemp20000uK/job3/"
    assert got[12] == "dataLaserCoolTestDoppShift/Om100/Det-50NumIons1000InitialTemp10000uK/job3/"


@pytest.mark.parametrize("arg", [
    "--sweep=vKick:1,2", "--sweep=Om:", "--sweep=Om", "--sweep=Om:0.5,x",
    "--sweep=nothing:1,2", "--sweep=Omx:1,2",                          # unknown NAME, a NAME and more
    "--sweep=Om:1,,2", "--sweep=Om:1,2,", "--sweep=Om:1e",
    pytest.param(("--sweep=Om:0.5,1", "--sweep=Om:2,3"), id="a-NAME-twice"),
    pytest.param("--sweep=Om:" + ",".join(str(0.01 * i) for i in range(1025)), id="1025-values"),
])
def test_cli_bad_axis_is_usage(L, arg):
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    args = (arg,) if isinstance(arg, str) else arg
    r = subprocess.run([MDLC_CLI_PATH, "1", "--print-directory=1", *args], capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.startswith("usage: mdlc <job>") and "--sweep=NAME:v1,v2" in r.stderr
    assert r.stdout == ""


def test_cli_axis_given_twice_is_usage(L):
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    r = subprocess.run([MDLC_CLI_PATH, "1", "--sweep=Om:0.5,1", "--sweep=Om:2"], capture_output=True, text=True)
    assert r.returncode == 2


@pytest.mark.parametrize("print_dir", [1, 0])
def test_cli_refusal_is_the_librarys(L, print_dir):
    """(without --print-directory the run itself is refused: before any GPU call, so here too)"""
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    r = subprocess.run([MDLC_CLI_PATH, "1", f"--print-directory={print_dir}", "--sweep=detuning:-0.501,-0.502"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith("mdlc: mdlc_")
    assert "point 1 and point 0 give the same run directory name: detuning -0.502 and -0.501 print alike" in r.stderr
