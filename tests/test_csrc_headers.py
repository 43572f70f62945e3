"""The include graph of mdqtplasmasims_amd/csrc and the Makefile's header dependencies.  CPU only: hipcc parses and
lists, nothing runs.

The headers are cut by what they serve: mdqt_internal.hpp is the MDQT kernels' interface, and the
block scheme, the ensembles, the MC + MD program, the three-level cooling program, the device math and the error
plumbing each have a header of their own, so that an engine sees its own interface and not the others'.  Three
properties keep it that way:
  * every header compiles alone (it includes what it uses);
  * the translation units of EDGES include what the table requires and nothing it excludes, by the compiler's own
    list of the headers they reach (-MM) - a later include that re-couples two engines fails here by name;
  * the Makefile takes an object's header prerequisites from the compiler (the .d beside it), not from a list.
"""
import glob
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "mdqtplasmasims_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the Makefile's -I flags and language modes
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I/opt/rocm/include"]
AS_HIP = ["-x", "hip", "--offload-arch=gfx950", "-std=c++17"]
AS_CPP = ["-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17"]

HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp")))


def test_the_glob_finds_the_headers():
    assert len(HEADERS) >= 20 and "mdqt_internal.hpp" in HEADERS, HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header):
    r = subprocess.run([HIPCC, *AS_HIP, "-fsyntax-only", "-Wno-pragma-once-outside-header", *INCLUDES,
                        os.path.join(CSRC, header)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def reached(unit):
    """the project's headers (csrc/*.hpp, include/*.h) the unit reaches, by base name"""
    mode = AS_CPP if unit.endswith(".cpp") or unit in HOST_HEADERS else AS_HIP + ["--cuda-host-only"]
    r = subprocess.run([HIPCC, *mode, "-Wno-pragma-once-outside-header", *INCLUDES, "-MM", os.path.join(CSRC, unit)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    names = {os.path.basename(t) for t in re.findall(r"[^\s\\:]+\.(?:hpp|h)\b", r.stdout)}
    return names - {unit}


# headers that only host sources include: listed as C++, as the Makefile compiles their users
HOST_HEADERS = {"mdmc_ctx.hpp", "mdqt_sweep.hpp", "mdqt_ctx.hpp", "mdqt_ensemble.hpp"}

MDQT_ALL = ["mdqt_ctx.hpp", "mdqt_internal.hpp", "mdqt_main_loops.hpp", "mdqt_writer.hpp"]
OTHER_ENGINES = ["mdqt_n3b_args.hpp", "mdmc_kernels.hpp", "mdqt_ens_args.hpp"]
NO_ENSEMBLE = ["mdqt_ensemble.hpp", "mdqt_ens_args.hpp"]

# translation unit (or header, listed alone): (must reach, must not reach)
EDGES = {
    # the three-level cooling program sees its own interface and the shared host tools, nothing of MDQT
    "mdlc_engine.cpp": (["mdlc_kernels.hpp", "mdqt_error.hpp", "mdqt_devbuf.hpp", "mdqt_batch.hpp", "mdlc.h"],
                        MDQT_ALL + OTHER_ENGINES),
    # its device side reaches mdqt_internal.hpp through mdqt_device.hpp (Philox takes a QTConst), no other engine
    "mdlc_kernels.hip": (["mdlc_kernels.hpp", "mdqt_device.hpp", "mdqt_internal.hpp"], OTHER_ENGINES),
    "mdlc_sweep_kernels.hip": (["mdlc_kernels.hpp", "mdqt_device.hpp", "mdqt_internal.hpp"], OTHER_ENGINES),
    "mdlc_device.hpp": (["mdlc_kernels.hpp", "mdqt_device.hpp", "mdqt_internal.hpp"], OTHER_ENGINES),
    # the MC + MD program shares QTConst, FastTab, N3Args and SubstepArgs with MDQT, not its context
    "mdmc_ctx.hpp": (["mdqt_internal.hpp", "mdmc_kernels.hpp", "mdqt_error.hpp", "mdqt_batch.hpp", "mdqt_devbuf.hpp",
                      "mdqt_mt32.hpp", "mdmc.h"], ["mdqt_ctx.hpp", "mdqt_ensemble.hpp"]),
    "mdmc_engine.cpp": (["mdmc_ctx.hpp"], ["mdqt_ctx.hpp", "mdqt_ensemble.hpp"]),
    "mdmc_ensemble.cpp": (["mdmc_ctx.hpp", "mdqt.h"], ["mdqt_ctx.hpp", "mdqt_ensemble.hpp"]),
    "mdmc_device.hpp": (["mdmc_kernels.hpp"], ["mdqt_n3b_args.hpp", "mdqt_ens_args.hpp", "mdlc_kernels.hpp"]),
    "mdmc_kernels.hip": (["mdmc_kernels.hpp", "mdqt_internal.hpp"],
                         ["mdqt_n3b_args.hpp", "mdqt_ens_args.hpp", "mdlc_kernels.hpp"]),
    # the shared host tools need the error plumbing only
    "mdqt_batch.cpp": (["mdqt_error.hpp", "mdqt_batch.hpp"], ["mdqt_ctx.hpp", "mdqt_internal.hpp"]),
    "mdqt_sweep.hpp": (["mdqt_error.hpp"], ["mdqt_ctx.hpp", "mdqt_internal.hpp"]),
    # the block scheme's interface and the device math, where they are used
    "mdqt_n3b.hpp": (["mdqt_n3b_args.hpp", "mdqt_math.hpp"], ["mdqt_ens_args.hpp", "mdmc_kernels.hpp", "mdlc_kernels.hpp"]),
    "mdqt_sort.hip": (["mdqt_n3b_args.hpp"], ["mdqt_internal.hpp", "mdqt_ens_args.hpp", "mdmc_kernels.hpp"]),
    "mdqt_force_plan.cpp": (["mdqt_math.hpp", "mdqt_ctx.hpp"], NO_ENSEMBLE),
    # one context does not see the ensembles ...
    "mdqt_ctx.hpp": (["mdqt_internal.hpp", "mdqt_n3b_args.hpp", "mdqt_error.hpp"],
                     NO_ENSEMBLE + ["mdmc_kernels.hpp", "mdlc_kernels.hpp"]),
    "mdqt_engine.cpp": (["mdqt_ctx.hpp"], NO_ENSEMBLE),
    "mdqt_step.cpp": (["mdqt_ctx.hpp"], NO_ENSEMBLE),
    "mdqt_observables.cpp": (["mdqt_ctx.hpp"], NO_ENSEMBLE),
    "mdqt_options.cpp": (["mdqt_ctx.hpp"], NO_ENSEMBLE),
    "mdqt_comm.cpp": (["mdqt_ctx.hpp"], NO_ENSEMBLE),
    # ... and the ensembles' sources see both
    "mdqt_ensemble.hpp": (["mdqt_ctx.hpp", "mdqt_ens_args.hpp"], ["mdmc_kernels.hpp", "mdlc_kernels.hpp"]),
    "mdqt_ensemble.cpp": (["mdqt_ensemble.hpp"], []),
    "mdqt_ensemble_output.cpp": (["mdqt_ensemble.hpp"], []),
    "mdqt_pump_ensemble.cpp": (["mdqt_ensemble.hpp"], []),
    "mdqt_ensemble_forces.hip": (["mdqt_ens_args.hpp"], ["mdmc_kernels.hpp", "mdlc_kernels.hpp"]),
    "mdqt_ensemble_qt.hip": (["mdqt_ens_args.hpp"], ["mdmc_kernels.hpp", "mdlc_kernels.hpp"]),
    "mdqt_ensemble_sweep_qt.hip": (["mdqt_ens_args.hpp"], ["mdmc_kernels.hpp", "mdlc_kernels.hpp"]),
    "mdqt_ensemble_obs.hip": (["mdqt_ens_args.hpp"], ["mdmc_kernels.hpp", "mdlc_kernels.hpp"]),
    "mdqt_pump_ensemble_kernels.hip": (["mdqt_ens_args.hpp"], ["mdmc_kernels.hpp", "mdlc_kernels.hpp"]),
}


@pytest.mark.parametrize("unit", sorted(EDGES))
def test_include_edges(unit):
    must, must_not = EDGES[unit]
    got = reached(unit)
    print(unit, "reaches", sorted(got))
    assert not [h for h in must if h not in got], (unit, "does not reach", [h for h in must if h not in got])
    assert not [h for h in must_not if h in got], (unit, "reaches", [h for h in must_not if h in got])


@pytest.mark.parametrize("unit", ["mdlc_kernels.hip", "mdlc_sweep_kernels.hip", "mdlc_device.hpp"])
def test_mdlc_device_side_names_mdqt_internal_only_through_mdqt_device(unit):
    text = open(os.path.join(CSRC, unit)).read()
    assert '#include "mdqt_internal.hpp"' not in text


def test_no_umbrella_header():
    """no header re-includes the parts: none names more than two of the six interface headers (two: a context
    holds the block scheme's arguments and checks errors, the block kernels' header takes arguments and math)"""
    parts = ["mdqt_math.hpp", "mdqt_n3b_args.hpp", "mdqt_ens_args.hpp", "mdmc_kernels.hpp", "mdlc_kernels.hpp",
             "mdqt_error.hpp"]
    for h in HEADERS:
        text = open(os.path.join(CSRC, h)).read()
        n = sum('#include "%s"' % p in text for p in parts)
        assert n <= 2, (h, n)


def make(*args):
    return subprocess.run(["make", "-C", CSRC, *args], capture_output=True, text=True, timeout=600)


def test_makefile_takes_header_dependencies_from_the_compiler(tmp_path):
    """One object into an OBJDIR of its own: a newer header that the object's .d names puts it out of date, one that
    the .d does not name leaves it up to date.  The newer header is make's --what-if (-W), which treats the file as
    just modified without touching the source tree."""
    lines = [ln for ln in open(os.path.join(CSRC, "Makefile")) if not ln.lstrip().startswith("#")]
    assert not [ln for ln in lines if ".hpp" in ln], "a header is named in a rule"
    objdir = str(tmp_path / "obj")
    obj = os.path.join(objdir, "mdlc_kernels.o")
    r = make("OBJDIR=" + objdir, obj)
    assert r.returncode == 0, r.stderr[-4000:]
    deps = set(re.findall(r"[^\s\\:]+", open(os.path.join(objdir, "mdlc_kernels.d")).read()))
    named = os.path.join(CSRC, "mdlc_kernels.hpp")
    other = os.path.join(CSRC, "mdmc_kernels.hpp")
    assert named in deps and os.path.join(CSRC, "mdqt_internal.hpp") in deps, sorted(deps)
    assert other not in deps and os.path.exists(other)
    assert make("OBJDIR=" + objdir, "-q", obj).returncode == 0, "not up to date right after it was built"
    assert make("OBJDIR=" + objdir, "-q", "-W", named, obj).returncode == 1, "a named header does not rebuild it"
    assert make("OBJDIR=" + objdir, "-q", "-W", other, obj).returncode == 0, "an unrelated header rebuilds it"
    # the listing has a dependency file of its own
    lst = os.path.join(objdir, "mdlc_kernels.s")
    assert make("OBJDIR=" + objdir, lst).returncode == 0
    assert os.path.exists(os.path.join(objdir, "mdlc_kernels.s.d"))
    assert make("OBJDIR=" + objdir, "-q", "-W", named, lst).returncode == 1
    assert make("OBJDIR=" + objdir, "-q", "-W", other, lst).returncode == 0
