"""Literal dense-matrix numpy transcription of laserCoolNoPlasmaThreeState.cpp ("LC3": qstep()
:140-293, cs/gs in main :384-387, main()'s loop :392-407) — test infrastructure only, the checker
of the mdlc engine (include/mdlc.h).

qstep_ion follows the reference statement by statement with complex matrices: the cs/gs
operators, the full Hamiltonian built every step, the 3/8-rule propagator with its per-stage
1/sqrt(1 - dp) prefactor.  qstep_batch is the same step vectorised over ions for the longer
comparisons.  The uniform draws (rand, randDir) are passed in.
"""
import numpy as np

# LC3:59-68, :82, :88, :393
DEFAULTS = dict(detuning=-0.5, Om=0.5, dt=0.01, vKick=0.0012076, applyForce=True)


def operators():
    ident = np.eye(3)
    w = [ident[:, k].reshape(3, 1).astype(complex) for k in range(3)]      # wvFn1, wvFn2, wvFn3 (:94-96)
    H = lambda a: a.conj().T
    cs = [w[0] @ H(w[1]), w[0] @ H(w[2])]                                    # :384-385
    gs = [1., 1.]                                                            # :386-387
    return ident, w, cs, gs


def qstep_ion(psi, vx, tPart, rand, randDir, detuning=-0.5, Om=0.5, dt=0.01, vKick=0.0012076, applyForce=True):
    """One ion through qstep() (:167-291).  Returns (psi', vx', tPart', jumped)."""
    ident, (wvFn1, wvFn2, wvFn3), cs, gs = operators()
    H = lambda a: a.conj().T
    I = 1j
    wvFn = np.asarray(psi, complex).reshape(3, 1)
    velQuant = vx                                                            # :170
    tPart = tPart + dt                                                       # :171

    def dp_of(y):                                                            # :172-180
        dpmat = np.zeros((1, 1), complex)
        for j in range(2):
            dpmat = dpmat + (dt * H(y) @ H(cs[j]) @ cs[j] @ y) * gs[j]
        return dpmat[0, 0].real

    dp = dp_of(wvFn)
    if rand > dp:                                                            # :182
        densMatrix = wvFn @ H(wvFn)
        p13 = H(wvFn1) @ densMatrix @ wvFn3
        p12 = H(wvFn1) @ densMatrix @ wvFn2
        kick = 1 * vKick * Om * (p13[0, 0].imag * np.sqrt(gs[0]) - p12[0, 0].imag * np.sqrt(gs[1])) * dt   # :189
        totalDetRight = -detuning - velQuant                                 # :192
        totalDetLeft = -detuning + velQuant                                  # :193
        hamCouplingTerm = -Om / 2 * wvFn1 @ H(wvFn3) * np.sqrt(gs[0]) - Om / 2 * wvFn1 @ H(wvFn2) * np.sqrt(gs[1])
        hamEnergyTerm = totalDetRight * (wvFn3 @ H(wvFn3)) + totalDetLeft * (wvFn2 @ H(wvFn2))
        hamWithoutDecay = hamEnergyTerm + hamCouplingTerm + H(hamCouplingTerm)
        hamDecayTerm = np.zeros((3, 3), complex)
        for j in range(2):
            hamDecayTerm = hamDecayTerm - 1. / 2 * I * (gs[j] * H(cs[j]) @ cs[j])
        hamil = hamWithoutDecay + hamDecayTerm                               # :208
        dtHalf = dt / 2

        def slope(y):                                                        # :221-225
            prefactor = 1 / np.sqrt(1 - dp_of(y))
            matPrefactor = ident - I * dt * hamil
            wvFnStepped = prefactor * matPrefactor @ y
            return 1. / dt * (wvFnStepped - y)

        k1 = slope(wvFn)
        wvFnk1 = wvFn + dtHalf * k1
        k2 = slope(wvFnk1)
        wvFnk2 = wvFn + dtHalf * k2
        k3 = slope(wvFnk2)
        wvFnk3 = wvFn + dt * k3
        k4 = slope(wvFnk3)
        wvFn = wvFn + (k1 + 3 * k2 + 3 * k3 + k4) / 8 * dt                   # :271
        jumped = False
    else:                                                                    # :273-285
        tPart = 0.
        wvFn = np.zeros((3, 1), complex)
        wvFn[0, 0] = 1.
        kick = vKick if randDir < 0.5 else -vKick
        jumped = True
    if applyForce:
        vx = vx + kick                                                       # :288
    return wvFn.reshape(3), vx, tPart, jumped


def qstep_batch(psi, vx, tPart, rand, randDir, detuning=-0.5, Om=0.5, dt=0.01, vKick=0.0012076, applyForce=True):
    """qstep() for n ions at once: psi (n, 3) complex, vx, tPart, rand, randDir (n,).
    Returns (psi', vx', tPart', jumped (n,) bool, dp (n,))."""
    psi = np.asarray(psi, complex)
    vx = np.asarray(vx, float)
    n = psi.shape[0]
    tPart = np.asarray(tPart, float) + dt

    def dp_of(y):
        return dt * (y[:, 1] * y[:, 1].conj()).real * 1. + dt * (y[:, 2] * y[:, 2].conj()).real * 1.

    dp = dp_of(psi)
    nojump = np.asarray(rand) > dp
    kick_opt = 1 * vKick * Om * ((psi[:, 0] * psi[:, 2].conj()).imag - (psi[:, 0] * psi[:, 1].conj()).imag) * dt
    hamil = np.zeros((n, 3, 3), complex)
    hamil[:, 2, 2] = (-detuning - vx) - 0.5j
    hamil[:, 1, 1] = (-detuning + vx) - 0.5j
    hamil[:, 0, 1] = hamil[:, 1, 0] = hamil[:, 0, 2] = hamil[:, 2, 0] = -Om / 2
    matPrefactor = np.eye(3)[None] - 1j * dt * hamil

    def slope(y):
        prefactor = 1 / np.sqrt(1 - dp_of(y))
        stepped = prefactor[:, None] * np.einsum("nij,nj->ni", matPrefactor, y)
        return 1. / dt * (stepped - y)

    k1 = slope(psi)
    k2 = slope(psi + dt / 2 * k1)
    k3 = slope(psi + dt / 2 * k2)
    k4 = slope(psi + dt * k3)
    evolved = psi + (k1 + 3 * k2 + 3 * k3 + k4) / 8 * dt
    ground = np.zeros_like(psi)
    ground[:, 0] = 1.
    psi_new = np.where(nojump[:, None], evolved, ground)
    tPart = np.where(nojump, tPart, 0.)
    kick = np.where(nojump, kick_opt, np.where(np.asarray(randDir) < 0.5, vKick, -vKick))
    if applyForce:
        vx = vx + kick
    return psi_new, vx, tPart, ~nojump, dp


def main_loop(tmax=45000, sampleFreq=1000, dt=0.01):
    """main()'s loop (:392-407): ([(c0, t) of every output()], number of iterations).  output() at
    (c0, t) sees the state after c0 qsteps."""
    t = 0.
    c0 = 0
    outs = []
    while t <= tmax:
        t += dt
        if (c0 + 1) % sampleFreq == 0:
            outs.append((c0, t))
        c0 += 1
    return outs, c0


def lg(x):
    """printf("%lg")"""
    return "%g" % x
