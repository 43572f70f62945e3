"""The file writer's cap on submitted-but-unwritten files (mdqtplasmasims_amd/csrc/mdqt_writer.hpp), which the QT
tagging programs' recorded stage sets: 2,000 files of 4,001 rows through a writer of 4 threads and a cap of 8 keep
at most cap + threads snapshots alive, every file's bytes are fprintf("%lg\\t%lg\\n")'s (a NaN row included), and an
unwritable path comes back from flush() with its name.  CPU only: the header is compiled with g++ into a
stand-alone driver (tests/native/writer_bound_check.cpp), once plainly and once under the thread sanitizer where
g++ links it."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mdqtplasmasims_amd", "csrc")
SRC = os.path.join(HERE, "native", "writer_bound_check.cpp")


def compile_driver(exe, *flags):
    return subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", *flags, "-I", CSRC, SRC, "-o", exe],
                          capture_output=True, text=True)


def run_driver(exe, out):
    os.makedirs(out)
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    m = re.fullmatch(r"max_live=(\d+) cap=(\d+) threads=(\d+)\n", r.stdout)
    assert m, r.stdout
    live, cap, threads = map(int, m.groups())
    assert (cap, threads) == (8, 4)
    assert 1 <= live <= cap + threads
    assert os.listdir(out) == []                     # every file compared and removed


def test_capped_writer_bounds_its_snapshots_and_writes_fprintf_bytes(tmp_path):
    exe = str(tmp_path / "writer_bound_check")
    r = compile_driver(exe)
    assert r.returncode == 0, r.stderr
    run_driver(exe, tmp_path / "out")


def test_capped_writer_under_the_thread_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++", "-fsanitize=thread", str(probe), "-o", str(tmp_path / "probe")], capture_output=True,
                       text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ does not link -fsanitize=thread here")
    exe = str(tmp_path / "writer_bound_check_tsan")
    r = compile_driver(exe, "-g", "-fsanitize=thread")
    assert r.returncode == 0, r.stderr
    run_driver(exe, tmp_path / "out")
