"""A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run (GPU): K timed steps, the
headline alone (nothing of --full), and DIR/<name>.npy = the state those W + K MD steps leave — the
same bits as the same steps through the package (the engine's operation order is fixed, so equal
inputs give equal outputs, run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 2


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    d = str(tmp_path_factory.mktemp("bench") / "out")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--dump-outputs", d], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), d


def test_plain_run_prints_the_headline_alone(plain_run):
    h, _ = plain_run
    assert h["steps"] == STEPS and h["warmup"] == WARMUP and h["n_gpus"] == 1
    assert h["unit"] == "particle-qsteps/s" and h["higher_is_better"] is True and h["dtype"] == "f64"
    N, ratio = h["config"]["N"], h["config"]["qsteps_per_md_step"]
    assert h["ms_per_step"] > 0
    assert h["value"] == pytest.approx(N * ratio / (h["ms_per_step"] * 1e-3), rel=1e-9)
    assert h["timed_region_s"] == pytest.approx(STEPS * h["ms_per_step"] * 1e-3, rel=1e-9)
    assert h["cpu_baseline"] is None and h["lines"] == {} and "secondary_errors" not in h
    assert h["roofline"]["frac"] > 0


def test_dumped_outputs_are_the_state_after_the_timed_steps(plain_run):
    import mdqtplasmasims_amd as M
    h, d = plain_run
    assert sorted(os.listdir(d)) == ["F.npy", "R.npy", "V.npy", "psi.npy", "t.npy", "tPart.npy"]
    s = M.Simulation(device=0, seed=12346, job=1, qt_enabled=1, N0=3500).init()   # bench.py's C2, rank 0
    s.set_option("qt_math", 2)
    s.set_option("overlap", 0)
    s.md_steps(WARMUP)
    s.md_steps(STEPS)
    st = s.get_state()
    s.close()
    assert h["config"]["N"] == st["R"].shape[1]
    for k in ("R", "V", "F", "psi", "tPart"):
        a = np.load(os.path.join(d, k + ".npy"))
        assert a.dtype == np.float64 and a.shape == st[k].shape, k
        assert np.all(np.isfinite(a)), k
        assert np.array_equal(a, st[k]), k
    assert np.load(os.path.join(d, "t.npy"))[0] == st["t"]
