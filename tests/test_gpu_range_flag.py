"""The position-range flag (a position outside [-L/8, 9L/8]: an ion moved more than L/8 in half a
substep, a broken run) lives in host-pinned memory the substep kernels store to: mdqt_md_steps polls it
with a host load before every MD step and issues no stream synchronisation on a healthy run;
mdqt_synchronize and the state read-backs drain the stream and then check, so a broken run is reported
no later than the next host synchronisation (include/mdqt.h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(N0=60, seed=7, rng_mode=1)


@pytest.fixture(scope="module")
def eng():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


def equal_states(a, b):
    for k in ("R", "V", "F", "psi", "tPart"):
        assert np.array_equal(a[k], b[k]), k
    assert a["t"] == b["t"]


def test_healthy_run_across_the_old_check_period(eng):
    """md_steps(130) (the loop used to drain the stream before steps 64 and 128) == 130 single MD steps
    with a synchronisation after each, bit for bit"""
    a = eng.Simulation(**KW).init()
    b = eng.Simulation(**KW).init()
    a.md_steps(130)
    for _ in range(130):
        b.md_steps(1)
        b.synchronize()
    a.synchronize()
    assert a.const("range_guard") == 0 and b.const("range_guard") == 0
    assert a.qstep_index == b.qstep_index
    equal_states(a.get_state(), b.get_state())
    a.close(); b.close()


def test_broken_run_is_reported_by_the_next_synchronisation(eng):
    """one ion moving 3 L per half substep: md_steps(3); synchronize() raises the "positions left"
    error from one of the two calls; afterwards the context runs with the range guard on, and a second
    context on the same device is unaffected"""
    ref = eng.Simulation(**KW).init()
    ref.md_steps(3)
    ref.synchronize()
    healthy = ref.get_state()
    ref.close()

    s = eng.Simulation(**KW).init()
    other = eng.Simulation(**KW).init()
    st = s.get_state()
    V = st["V"].copy()
    V[0, 5] = 6. * s.const("L") / s.const("quantumTimestep")
    s.set_state(st["R"], V, st["psi"], st["tPart"], st["t"])
    assert s.const("range_guard") == 0
    with pytest.raises(eng.MdqtError, match=r"positions left \[-L/8, 9L/8\]"):
        s.md_steps(3)
        s.synchronize()
    assert s.const("range_guard") == 1
    s.md_steps(1)                                   # runs, range-checking every pair; reported once
    s.synchronize()
    assert s.const("range_guard") == 1

    other.md_steps(3)
    other.synchronize()
    assert other.const("range_guard") == 0
    equal_states(other.get_state(), healthy)
    s.close(); other.close()
