"""The QT substep kernels, per ion, against the extended-precision truth of n x (step(); qstep()).

Every case of tests/qt_cases.py runs one substep kernel instance — asserted through the "qt_kernel"
constant (mdqt_internal.hpp QTKernel), the code a reading of launch_substeps_r / launch_substeps predicts
for the case's options, time and parameters — from a state set with set_state and forces set with
set_forces (no force kernel is involved), and every ion's psi (12 x 2 components), vx, vy / vz and R must
be within the bound B of tests/qt_truth.py, which is derived there by counting roundings and is 3 to 4
orders below the 1e-12 / 1e-9 gates of the tests against the double oracle.  tPart is bit-equal to the
double accumulation (which also fixes the jumped set and the substep of every jump), an ion that jumps in
the last substep holds its target's basis state exactly, and any other wrong target is an O(1) error in
psi.  The decision margins (>= 2^-30, positions >= 2^-30 L, no ion excluded) are asserted again here.

The three-level program (mdlc_kernels.hip) runs through LaserCooling.qsteps against the same truth module.

Measured err / B on an MI355X: docs/QT_KERNEL.md ("The QT kernels' per-ion gate")."""
import numpy as np
import pytest

from tests import qt_cases as qc
from tests import qt_truth as qt

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not qt.extended_ok(), reason=qt.SKIP_MESSAGE)]

LD = np.longdouble


@pytest.fixture(scope="module")
def eng():
    import mdqtplasmasims_amd as M
    if M.device_count() < 1:
        pytest.fail("no GPU visible to the gpu-marked tests")
    return M


def run_engine(eng, c, seed, st):
    """the case on the GPU: (final state, qt_kernel code, qt_kernel_nseg)"""
    kw = dict(N0=c["N"], seed=seed, job=qc.PHILOX_JOB, rng_mode=1, **c["params"])
    if c["model"] != 0:
        kw["qt_model"] = c["model"]
    s = eng.Simulation(**kw)
    try:
        for k, v in c["options"].items():
            s.set_option(k, v)
        assert s.const("L") == st["L"]
        s.set_state(st["R"], st["V"], st["psi"], st["tPart"], c["t0"])
        s.set_forces(st["F"])
        s.qstep_index = qc.PHILOX_Q0
        if c["stepwise"]:
            for _ in range(c["nsub"]):
                s.step()
                s.qstep()
        else:
            s.substeps(c["nsub"])
        g = s.get_state()
        assert s.qstep_index == qc.PHILOX_Q0 + c["nsub"]
        return g, int(s.const("qt_kernel")), int(s.const("qt_kernel_nseg"))
    finally:
        s.close()


def run_three_level(c, seed, st):
    from mdqtplasmasims_amd import LaserCooling
    N = c["N"]
    with LaserCooling(N0=N, seed=seed, job=qc.PHILOX_JOB, device=0) as s:
        psi = (st["psi"][:, :3, 0] + 1j * st["psi"][:, :3, 1])[None]
        V = st["V"][None].copy()
        s.set_state(V=V, psi=psi, tPart=st["tPart"][None], q=qc.PHILOX_Q0)
        s.qsteps(c["nsub"])
        g = s.get_state()
    assert g["q"] == qc.PHILOX_Q0 + c["nsub"]
    p12 = np.zeros((N, 12, 2))
    p12[:, :3, 0], p12[:, :3, 1] = g["psi"][0].real, g["psi"][0].imag
    assert np.array_equal(g["V"][0, 1:], st["V"][1:])                    # vy, vz are carried, never touched
    return dict(psi=p12, V=g["V"][0], R=None, tPart=g["tPart"][0])


@pytest.mark.parametrize("name", [c["name"] for c in qc.CASES])
def test_substep_kernel_within_bound(eng, orc, name):
    c = qc.BY_NAME[name]
    seed, st, U, tr = qc.build(c, orc)
    d, p = qt.min_margins(tr)
    assert d >= qc.MARGIN and (c["model"] == "lc3" or p >= qc.MARGIN * st["L"])
    if c["model"] == "lc3":
        g = run_three_level(c, seed, st)
    else:
        g, kernel, nseg = run_engine(eng, c, seed, st)
        assert kernel == c["kernel"], (name, kernel)
        assert nseg == 1                                # F came from set_forces: nothing to sum
    s = c["nsub"] - 1
    # tPart: the double accumulation, bit for bit — the jumped set and the substep of every jump with it
    assert np.array_equal(g["tPart"], tr["tPart_double"][s])
    last = tr["jumped"][s]
    for i in np.nonzero(last)[0]:
        e = np.zeros((12, 2))
        e[tr["target"][s][i], 0] = 1.0
        if c["params"].get("reNormalizewvFns"):
            assert np.abs(g["psi"][i] - e).max() <= 2 * qt.U53, (i, "jump target")
        else:
            assert np.array_equal(g["psi"][i], e), (i, "jump target")
    nst = tr["psi_re"][s].shape[1]
    assert np.all(g["psi"][:, nst:] == 0)
    ep = qt.psi_error(tr, s, g["psi"])
    Bp = np.where(last, 4 * qt.U53, tr["Bpsi"][s])       # (a renormalised basis state: rsq3 and a product)
    rp = ep / Bp
    ev = np.abs(g["V"].astype(LD) - tr["V"][s]).astype(np.float64)
    rv = ev[0] / tr["Bvx"][s]
    i = int(np.argmax(rp))
    msg = (f"{name}: qt_kernel {c['kernel']}, seed {seed}, {int(np.array(tr['jumped']).sum())} jumps; err/B psi {rp.max():.3g} "
           f"(ion {i}: err {ep[i]:.3e}, B {Bp[i]:.3e}, K {tr['K'][s][i]:.1f}, c {tr['c'][s][i]:.0f}), vx {rv.max():.3g} (ion {int(np.argmax(rv))})")
    worst = max(rp.max(), rv.max())
    if g["R"] is not None:
        ryz = ev[1:].max(axis=0) / tr["Bv"][s]
        rr = np.abs(g["R"].astype(LD) - tr["R"][s]).astype(np.float64).max(axis=0) / tr["BR"][s]
        msg += f", vy/vz {ryz.max():.3g}, R {rr.max():.3g} (ion {int(np.argmax(rr))})"
        worst = max(worst, ryz.max(), rr.max())
    print(msg)
    assert worst <= 1.0, msg
