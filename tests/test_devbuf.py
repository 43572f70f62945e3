"""The owner of the engines' device and pinned memory (mdqtplasmasims_amd/csrc/mdqt_devbuf.hpp): Buf<T, Space>.
CPU only: tests/native/devbuf_check.cpp (compiled with g++ here, against the HIP API header alone) runs the buffer
over a Space of its own that counts calls and live bytes and fails an allocation on request, and prints one line
per check.  The program is built twice: plain, and with -fsanitize=address,undefined, where a block released twice
or never (its blocks are malloc'ed) ends the run with a report.  Stand-alone both times: nothing is preloaded."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mdqtplasmasims_amd", "csrc")

# what the program must report, each exactly once and "ok"
CHECKS = [
    "reserve0_empty",                      # reserve(0) on an empty buffer allocates nothing
    "reserve_first",
    "reserve_within_capacity_no_call",     # reserve(n <= capacity): no allocator call
    "grow_frees_then_allocates",           # a grow frees before it allocates; capacity() == n afterwards
    "alloc_exact",
    "reads_like_a_pointer",
    "reset",
    "reset_twice_one_release",
    "balanced_after_scope",
    "fail_setup",
    "failed_reserve_empty",                # a failed reserve: pointer null, capacity 0
    "reserve_after_failure_allocates",     # ... and the next reserve calls the allocator again and succeeds
    "failed_alloc_empty",
    "reserve_after_failed_alloc",
    "flags_reach_the_space",
    "balanced_after_failures",
    "move_setup",
    "move_construct_empties_source",       # a move leaves the source empty
    "swap_pointer_and_capacity",           # std::swap exchanges both
    "move_assign",
    "self_move_keeps",
    "vector_setup",
    "vector_growth_moves",
    "balanced_after_moves",
    "early_return_releases_first_local",   # the early return of a function holding two local buffers
    "normal_return_releases_both",
    "live_bytes_zero_at_exit",             # every block released exactly once, live bytes 0
]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def report(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devbuf") / ("devbuf_check_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC,
                        os.path.join(HERE, "native", "devbuf_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))


def test_every_check_passes(report):
    assert report.returncode == 0, report.stdout + report.stderr
    assert report.stderr == "", report.stderr          # no sanitizer report
    lines = report.stdout.splitlines()
    assert lines == ["ok " + c for c in CHECKS], [ln for ln in lines if not ln.startswith("ok ")]
