"""The cases of the QT substep kernels' per-ion gate, shared by tests/test_qt_truth.py (CPU: the truth
against mpmath, the oracle inside B, the perturbed oracle outside it, the decision margins) and
tests/test_gpu_qt_accuracy.py (the HIP kernels inside B).  Inputs and their extended-precision truth are
built once per process and never modified.

Shapes: N = 3 (less than one row of a wave), 17 (one lane workgroup of 16 ions plus one: idle groups shadow
the last ion), 70, 300 (more than one 256-thread block of the thread kernel); nsub 1, 2, 16, 17, 25, 32 in
one launch (17 and 25 take the odd tail of the two-substep loop; the Philox staging uses lanes k and k + 16);
density 0.5 at N = 70 (ratio 50: launches of 32 + 18).  Seeds are picked from the truth alone: every decision
margin >= 2^-30 and every position margin >= 2^-30 L, no ion excluded."""
import numpy as np

from tests import qt_truth as qt

# substep kernel instances (mdqt_internal.hpp QTKernel)
QTK_LANES_IM_EDZ, QTK_LANES_IM, QTK_LANES_R_FAST, QTK_LANES_R = 1, 2, 3, 4
QTK_LANES_R_PUMP_FAST, QTK_LANES_R_PUMP, QTK_LANES_IM_EDZ_RN = 5, 6, 7
QTK_THREAD_R, QTK_EXACT_LANES, QTK_EXACT_THREAD = 10, 30, 40

PUMP = {1: dict(Om=0.7, detuning=-2.5), 2: dict(Om=2.0, detuning=0.0), 3: dict(Om=1.3, detuning=-1.0)}
MARGIN = 2.0 ** -30


def case(name, N, nsub, kernel, model=0, params=None, options=None, t0=0.3, stepwise=False, state="mixed", seed0=100):
    return dict(name=name, N=N, nsub=nsub, kernel=kernel, model=model, params=dict(params or {}),
                options=dict(options or {}), t0=t0, stepwise=stepwise, state=state, seed0=seed0)


HEAVY = dict(Om=3.0, OmDP=2.0)
CASES = [
    # the production instance over the shapes
    case("prod_N3_s1", 3, 1, QTK_LANES_IM_EDZ),
    case("prod_N17_s2", 17, 2, QTK_LANES_IM_EDZ),
    case("prod_N3_s16", 3, 16, QTK_LANES_IM_EDZ),
    case("prod_N17_s17", 17, 17, QTK_LANES_IM_EDZ),
    case("prod_N70_s25", 70, 25, QTK_LANES_IM_EDZ),
    case("prod_N300_s32", 300, 32, QTK_LANES_IM_EDZ),
    case("prod_density0.5_N70_s50", 70, 50, QTK_LANES_IM_EDZ, params=dict(density=0.5)),
    # parameters beyond the defaults
    case("heavy_jump_N70_s25", 70, 25, QTK_LANES_IM_EDZ, params=HEAVY, state="random"),
    case("detuning-0.5_N17_s25", 17, 25, QTK_LANES_IM_EDZ, params=dict(detuning=-0.5, detuningDP=-0.5)),
    case("phase_ladder_N70_s25", 70, 25, QTK_LANES_IM_EDZ, state="ladder"),
    case("phase_ladder_heavy_N70_s17", 70, 17, QTK_LANES_IM_EDZ, params=HEAVY, state="ladder"),
    # the other lane instances
    case("fracOfSig0.4_N70_s25", 70, 25, QTK_LANES_IM, params=dict(fracOfSig=0.4, Te=5.0, sig0=2.0)),
    case("fracOfSig0.4_ladder_N17_s17", 17, 17, QTK_LANES_IM, params=dict(fracOfSig=0.4, Te=5.0, sig0=2.0), state="ladder"),
    case("renorm_N70_s25", 70, 25, QTK_LANES_IM_EDZ_RN, params=dict(reNormalizewvFns=1)),
    case("renorm_heavy_N17_s32", 17, 32, QTK_LANES_IM_EDZ_RN, params=dict(reNormalizewvFns=1, **HEAVY), state="random"),
    case("general_fast_N70_s25", 70, 25, QTK_LANES_R_FAST, options=dict(qt_im01=0)),
    case("general_t0_N70_s2", 70, 2, QTK_LANES_R, t0=0.0),
    case("general_t0_N17_s17", 17, 17, QTK_LANES_R, t0=0.0, params=HEAVY, state="random"),
    case("general_stepwise_N17_s3", 17, 3, QTK_LANES_R, t0=0.0, stepwise=True),
    # thread per ion
    case("thread_N300_s25", 300, 25, QTK_THREAD_R, options=dict(substep_kernel=1)),
    case("thread_heavy_ladder_N70_s17", 70, 17, QTK_THREAD_R, options=dict(substep_kernel=1), params=HEAVY, state="ladder"),
    # the exact modes in both layouts
    case("exact_lanes_math0_N70_s25", 70, 25, QTK_EXACT_LANES + 0, options=dict(qt_math=0, substep_kernel=2)),
    case("exact_lanes_math1_N70_s25", 70, 25, QTK_EXACT_LANES + 1, options=dict(qt_math=1, substep_kernel=2), params=HEAVY, state="ladder"),
    case("exact_thread_math0_N300_s17", 300, 17, QTK_EXACT_THREAD + 0, options=dict(qt_math=0, substep_kernel=1), params=HEAVY, state="random"),
    case("exact_thread_math1_N70_s25", 70, 25, QTK_EXACT_THREAD + 1, options=dict(qt_math=1, substep_kernel=1), state="ladder"),
]
for _m in (1, 2, 3):
    CASES += [
        case(f"pump{_m}_lanes_N70_s25", 70, 25, QTK_LANES_R_PUMP_FAST, model=_m, params=PUMP[_m], state="random"),
        case(f"pump{_m}_lanes_t0_N17_s17", 17, 17, QTK_LANES_R_PUMP, model=_m, params=PUMP[_m], t0=0.0, state="random"),
        case(f"pump{_m}_thread_N300_s2", 300, 2, QTK_THREAD_R + _m, model=_m, params=PUMP[_m], options=dict(substep_kernel=1), state="random"),
    ]
CASES.append(case("three_level_N70_s32", 70, 32, None, model="lc3", state="random"))
CASES.append(case("three_level_N300_s17", 300, 17, None, model="lc3", state="random"))
BY_NAME = {c["name"]: c for c in CASES}

# model 0 defaults (SpeedUp:60-74; tests/test_capi.py holds the engine's and the oracle's to the same values)
DEFAULT0 = dict(Om=1.0, OmDP=1.0, detuning=-1.0, detuningDP=1.0, density=2.0, fracOfSig=0.0, Te=19.0, sig0=4.0,
                reNormalizewvFns=0)


def program(c, B=qt.LDB, gamToE_rel=0.0):
    if c["model"] == "lc3":
        return qt.program_three_level(B)
    if c["model"] == 0:
        p = dict(DEFAULT0, **c["params"])
        return qt.program_model0(B, p["Om"], p["OmDP"], p["detuning"], p["detuningDP"], p["density"], p["fracOfSig"],
                                 p["Te"], p["sig0"], gamToE_rel=gamToE_rel)
    return qt.program_pump(B, c["model"], c["params"]["Om"], c["params"]["detuning"])


def box(N0):
    return float(np.power(N0 * 4. * np.pi / 3., 0.333333333))           # SpeedUp:297


def make_state(c, seed):
    """the inputs of a case for one seed: R, V, F [3][N], psi [N][12][2], tPart [N]"""
    N, nst = c["N"], {0: 12, 1: 7, 2: 7, 3: 5, "lc3": 3}[c["model"]]
    rng = np.random.default_rng(seed)
    L = box(N)
    z = rng.normal(size=(N, nst)) + 1j * rng.normal(size=(N, nst))
    if c["state"] != "random" and c["model"] == 0:
        i = np.arange(N)
        z[i % 5 == 0, 2:] *= 0.05                                       # mostly S (the cooled ions)
        z[i % 5 == 1, :6] *= 0.02                                       # psi concentrated in the D levels
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    if c["model"] == 0 and not dict(DEFAULT0, **c["params"])["reNormalizewvFns"] and c["state"] != "random":
        z[np.arange(N) % 5 == 2] *= np.sqrt(0.5)                        # norm^2 0.5, renormalisation off
    psi = np.zeros((N, 12, 2))
    psi[:, :nst, 0], psi[:, :nst, 1] = z.real, z.imag
    R = rng.uniform(0.02 * L, 0.98 * L, (3, N))
    V = rng.normal(0, 1.0, (3, N))
    V[0] = rng.uniform(-3.0, 3.0, N)                                    # |vx| up to 3
    if c["model"] == "lc3":
        V[0] = rng.normal(0, 0.105, N)
    edge = np.arange(N) % 7 == 3                                        # wraps through 0 and L
    R[0, edge] = np.where(V[0, edge] < 0, rng.uniform(0, 2e-4, edge.sum()), L - rng.uniform(0, 2e-4, edge.sum()))
    F = rng.normal(0, 1.0, (3, N))
    tPart = rng.uniform(0, 0.5, N)
    if c["state"] == "ladder":
        # |phi| = |vx pv2q cphi tPart| in every octave from 2^8 to 2^19 and a few beyond 2^20 (the library
        # fallback), on the first ions; the rest keep small phases, so whole waves run the phase_small loop
        P = program(c)
        scale = float(P.pv2q * P.cphi)
        k = 0
        for i in range(min(N, 40)):
            if i % 4 == 3 and i > 16:
                continue
            octv = 8 + (k % 13)                                         # 8 .. 19, and 20: beyond 2^20
            k += 1
            vx = np.sign(V[0, i]) * (rng.uniform(0.8, 2.5) if octv < 18 else rng.uniform(2.0, 2.5))
            V[0, i] = vx
            tPart[i] = 2.0 ** (octv + rng.uniform(0.05, 0.9)) / (abs(vx) * scale)
    return dict(R=R, V=V, F=F, psi=psi, tPart=tPart, L=L)


PHILOX_JOB, PHILOX_Q0 = 1, 1000


def uniforms(c, orc, seed):
    return qt.philox_tape(orc, seed, PHILOX_JOB, c["N"], PHILOX_Q0, c["nsub"])


def run_truth(c, st, U, B=qt.LDB, gamToE_rel=0.0, nsub=None, bound=True):
    P = program(c, B, gamToE_rel)
    renorm = bool(c["params"].get("reNormalizewvFns", 0))
    return qt.trajectory(P, st["psi"], st["V"][0], st["tPart"], c["t0"], U, nsub or c["nsub"], R=st["R"], V=st["V"],
                         F=st["F"], L=st["L"], renorm=renorm, B=B, bound=bound)


def requirements(c, tr):
    """what a case's seed must provide besides the margins"""
    jumps = np.array(tr["jumped"])
    if c["name"].startswith("heavy_jump"):
        # two ions of one wave (4 ions per wave of the lane kernel) jumping in the same substep
        same_wave = any(np.bincount(np.nonzero(j)[0] // 4).max(initial=0) >= 2 for j in jumps)
        return same_wave and jumps.sum() >= 8
    if "heavy" in c["name"] or c["model"] != 0:
        return jumps.sum() >= 1
    return True


_CACHE = {}


def build(c, orc):
    """(seed, inputs, uniforms, truth) of a case: the first seed from seed0 whose truth has every decision
    margin >= 2^-30, every position margin >= 2^-30 L and the case's requirements; cached"""
    if c["name"] in _CACHE:
        return _CACHE[c["name"]]
    for seed in range(c["seed0"], c["seed0"] + 40):
        st = make_state(c, seed)
        U = uniforms(c, orc, seed)
        tr = run_truth(c, st, U)
        d, p = qt.min_margins(tr)
        if d >= MARGIN and (c["model"] == "lc3" or p >= MARGIN * st["L"]) and requirements(c, tr):
            _CACHE[c["name"]] = (seed, st, U, tr)
            return _CACHE[c["name"]]
    raise AssertionError(f"{c['name']}: no seed in 40 with the margins and requirements")
