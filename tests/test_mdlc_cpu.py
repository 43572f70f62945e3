"""CPU checks of the three-level laser-cooling program's engine (include/mdlc.h; no GPU needed):
the numpy checker against itself and against the physics, main()'s loop counts, the header /
library / binding triple, init()'s velocity draws bit for bit against the standard library, and
the reference's directory names."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dense_three_state as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "include", "mdlc.h")


@pytest.fixture(scope="module")
def L():
    from mdqtplasmasims_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mdqtplasmasims_amd.build import build
        build(quiet=True)
    return _lib.lib()


def random_states(rng, n):
    a = rng.normal(size=(n, 3)) + 1j * rng.normal(size=(n, 3))
    return a / np.sqrt((np.abs(a) ** 2).sum(1))[:, None]


# ---- 1. the vectorised checker against the literal one ----
@pytest.mark.parametrize("branch", ["nojump", "jump"])
def test_batch_matches_literal(branch):
    rng = np.random.default_rng(2024)
    n = 50
    psi = random_states(rng, n)
    vx = rng.normal(0, 0.105, n)
    tPart = rng.uniform(0, 3, n)
    rand = np.full(n, 0.5 if branch == "nojump" else 0.0)     # dp <= dt = 0.01 > 0: 0.5 never jumps, 0 always does
    randDir = rng.uniform(size=n)
    bp, bv, bt, bj, _ = D.qstep_batch(psi, vx, tPart, rand, randDir)
    assert bj.all() == (branch == "jump") and bj.any() == (branch == "jump")
    for i in range(n):
        p, v, t, j = D.qstep_ion(psi[i], vx[i], tPart[i], rand[i], randDir[i])
        assert j == bj[i]
        assert np.abs(p - bp[i]).max() <= 1e-14
        assert abs(v - bv[i]) <= 1e-14 and abs(t - bt[i]) <= 1e-14
    if branch == "jump":
        assert (bp == np.array([1, 0, 0])).all() and (bt == 0).all()
        assert ((bv == vx + 0.0012076) | (bv == vx - 0.0012076)).all()
        assert ((bv > vx) == (randDir < 0.5)).all()


# ---- 2. physics pin: the force cools (a sign error in the detunings or the kick heats) ----
@pytest.mark.parametrize("v0", [0.2, -0.2])
def test_checker_force_opposes_velocity(v0):
    n, steps = 1024, 5000
    rng = np.random.default_rng(7)
    psi = np.zeros((n, 3), complex)
    psi[:, 0] = 1
    vx = np.full(n, v0)
    tPart = np.zeros(n)
    for _ in range(steps):
        psi, vx, tPart, _, _ = D.qstep_batch(psi, vx, tPart, rng.uniform(size=n), rng.uniform(size=n))
    dv = vx - v0
    z = dv.mean() / (dv.std(ddof=1) / np.sqrt(n))
    print(f"v0 = {v0:+.1f}: mean dv = {dv.mean():.3e}, z = {z:.1f}")
    assert np.sign(dv.mean()) == -np.sign(v0)
    assert abs(z) >= 5


# ---- 3. main()'s loop ----
def test_main_loop_counts_defaults():
    outs, iterations = D.main_loop()
    assert iterations == 4_500_000
    assert len(outs) == 4500
    assert outs[0][0] == 999


def test_main_loop_counts_short():
    outs, iterations = D.main_loop(0.35, 10, 0.01)
    assert iterations == 35
    assert [c for c, _ in outs] == [9, 19, 29]
    assert [D.lg(t) for _, t in outs] == ["0.1", "0.2", "0.3"]


# ---- 4. header, library and binding ----
def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mdlc_[A-Za-z0-9_]+)\s*\(", src)))


def test_header_library_and_binding_agree(L):
    from mdqtplasmasims_amd._lib import LIB_PATH, MDLC_SIGNATURES
    syms = set(header_symbols())
    assert {"mdlc_default_params", "mdlc_create", "mdlc_destroy", "mdlc_get_const", "mdlc_sample_velocities",
            "mdlc_init", "mdlc_qsteps", "mdlc_get_state", "mdlc_set_state", "mdlc_ekin_x",
            "mdlc_setup_directories", "mdlc_save_directory", "mdlc_run"} <= syms
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (mdlc_[A-Za-z0-9_]+)$", nm, flags=re.M))
    assert exported == syms
    assert {s[0] for s in MDLC_SIGNATURES} == syms


def test_params_layout_and_reference_defaults(L):
    from mdqtplasmasims_amd import mdlc_default_params
    from mdqtplasmasims_amd._lib import MdlcParams
    from mdqtplasmasims_amd.mdlc import default_params
    assert mdlc_default_params is default_params
    src = open(HEADER).read()
    body = src[src.index("typedef struct mdlc_params {"):src.index("} mdlc_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b(?:double|int|uint32_t|char)\s+(\w+)", body)
    assert names == [f[0] for f in MdlcParams._fields_]
    ctype = {"double": ctypes.c_double, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32}
    for (typ, name), (fname, ftype) in zip(re.findall(r"\b(double|int|uint32_t)\s+(\w+);", body), MdlcParams._fields_):
        assert name == fname and ctype[typ] is ftype, name
    p = default_params()
    # LC3:59-68, :82, :88, :393, :54
    assert (p.N0, p.detuning, p.Om, p.tmax, p.applyForce) == (1000, -0.5, 0.5, 45000, 1)
    assert (p.sampleFreq, p.temperature, p.vKick, p.dt) == (1000, 0.01, 0.0012076, 0.01)
    assert p.saveDirectory == b"dataLaserCoolTestDoppShift/"
    assert p.njobs == 1
    assert default_params(njobs=8, Om=1.25).njobs == 8
    with pytest.raises(AttributeError):
        default_params(bogus=1)


def test_cli_usage(L):
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    r = subprocess.run([MDLC_CLI_PATH], capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.startswith("usage: mdlc <job>")
    r = subprocess.run([MDLC_CLI_PATH, "1", "--bogus=3"], capture_output=True, text=True)
    assert r.returncode == 2


def test_create_fails_loudly_without_gpu(L):
    from mdqtplasmasims_amd import LaserCooling, MdqtError, device_count
    if device_count() > 0:
        with pytest.raises(MdqtError, match="njobs must be"):
            LaserCooling(njobs=0)
        return
    with pytest.raises(MdqtError, match="no HIP device"):
        LaserCooling(N0=70)


# ---- 5. init()'s draws, bit for bit against the standard library ----
@pytest.fixture(scope="module")
def init_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mdlc") / "mdlc_init_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(HERE, "native", "mdlc_init_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("seed", [12346, 4000000007])
def test_sample_velocities_bit_for_bit(L, init_check, seed):
    from mdqtplasmasims_amd.mdlc import sample_velocities
    N0 = 1000
    r = subprocess.run([init_check, str(seed), str(N0), "0.01"], capture_output=True, text=True, check=True)
    ref = np.array([[float.fromhex(x) for x in line.split()] for line in r.stdout.splitlines()])   # [N0][3]
    assert ref.shape == (N0, 3)
    V = sample_velocities(seed, N0, 0.01)
    assert V.shape == (3, N0)
    assert (np.ascontiguousarray(V.T).view(np.uint64) == np.ascontiguousarray(ref).view(np.uint64)).all()
    assert 0.09 < V.std() < 0.12                          # 1.0508 sqrt(0.01) = 0.105


# ---- 6. directory names (main() :371-380), computed without a GPU ----
def test_directory_names(L):
    from mdqtplasmasims_amd._lib import MDLC_CLI_PATH
    from mdqtplasmasims_amd.mdlc import format_directory
    assert format_directory() == "dataLaserCoolTestDoppShift/Om50/Det-50NumIons1000InitialTemp10000uK/job1/"
    # (unsigned)(1.25 * 100) = 125, (unsigned)(0.5 * 100) = 50
    assert format_directory(Om=1.25, detuning=0.5, job=7, saveDirectory="out/") == \
        "out/Om125/Det50NumIons1000InitialTemp10000uK/job7/"
    r = subprocess.run([MDLC_CLI_PATH, "3", "--njobs=2", "--print-directory=1"], capture_output=True, text=True)
    assert r.returncode == 0
    assert r.stdout.splitlines() == [
        "dataLaserCoolTestDoppShift/Om50/Det-50NumIons1000InitialTemp10000uK/job3/",
        "dataLaserCoolTestDoppShift/Om50/Det-50NumIons1000InitialTemp10000uK/job4/"]
