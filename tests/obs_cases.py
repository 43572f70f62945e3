"""The cases of the observables' per-element gate, shared by tests/test_obs_truth.py (CPU: the truth against
mpmath, the double restatements inside B, the one-defect models outside it) and tests/test_gpu_obs_accuracy.py
(the HIP kernels inside B).  Inputs and truths are built once per process and never modified.

Velocities (every part in every case with N >= 64, scaled down below): a cold core normal(0, 0.02); a spread
uniform(-5.3, 5.3) reaching beyond the last bin; ions at vel[j] +- (0.0773 + {-1.2e-3, -1e-4, -1 ulp, 0, +1 ulp,
+1e-4}) with j at both ends of a wave's 64 bins and at the first and last bin (0.0773 is the kernels' skip
radius; at 0.0761 a term is of order 1e-314, visible per bin only); v = +-0.0 and 5.0 exactly; vx shifted by
+0.37 so that <vx> matters.  Each axis places its parts at ion indices of its own.

Sizes: where observables_w1's shapes change (docs/OBSERVABLES.md lists them).  Seeds are picked from the truth
alone: at N = 65, 255, 256 and 257 a wave-edge bin of the y or z distribution must hold nothing but the terms of
order 1e-314 (lone_edge_terms)."""
import numpy as np

from tests import obs_truth as ot

LD = ot.LD
SKIP = 0.0773
OFFSETS = (-1.2e-3, -1e-4, "-ulp", 0.0, "+ulp", 1e-4)
# vel index: the first and last bin, then wave ends 64 k + 63 and wave starts 64 k — of waves apart, so that the ions
# beyond one wave's end do not fill the bins next to another's start (an ion beyond the end of a wave, at 0.0761
# from its last bin, is what a smaller skip radius would drop there)
EDGE_J = (0, 2000, 63, 128, 1023, 1088, 1983, 1920)
EDGE_J_TAGGED = (-2000, 2000, -1937, -1872, 47, 112, 1967, 1904)         # (index j + 2000 = 64 k + 63, 64 k)
WAVE_EDGE_BINS = (63, 128, 1023, 1088, 1983, 1920)
SIZES = (3, 31, 33, 63, 65, 255, 256, 257, 1023, 1024, 1025, 1089, 2049, 16385)
BIG = 132_000
QUIET_SIZES = (65, 255, 256, 257)


def special_values(edge_j):
    out = []
    for j in edge_j:
        for s in (1.0, -1.0):
            for o in OFFSETS:
                r = np.nextafter(SKIP, 0.0) if o == "-ulp" else np.nextafter(SKIP, 1.0) if o == "+ulp" else SKIP + o
                out.append(j * ot.DV + s * r)
    out = np.array(out)
    np.random.default_rng(7).shuffle(out)
    return np.concatenate([[0.0, -0.0, 5.0], out])


def velocities(N, seed, shift=0.37, edge_j=EDGE_J, drift=False):
    rng = np.random.default_rng(seed)
    if drift:                                    # a drifting plasma: cancellation in (vx - <vx>)^2
        V = rng.normal(0, 0.05, (3, N))
        V[0] += 3.0
        return V
    sp = special_values(edge_j)
    nsp = min(sp.size, N // 2) if N >= 64 else max(1, N // 3)
    ncold = (N - nsp) // 2
    V = np.empty((3, N))
    for c in range(3):
        v = np.concatenate([sp[:nsp] if N >= 64 else rng.permutation(sp[3:])[:nsp], rng.normal(0, 0.02, ncold),
                            rng.uniform(-5.3, 5.3, N - nsp - ncold)])
        V[c] = v[rng.permutation(N)]
    V[0] += shift
    return V


def big_velocities(seed=1):
    """N = 132,000: 512 chunks of 258 ions, so ions 256 and 257 of every chunk take kde_chunk's second staging
    pass.  Those (1,022) and about 3,000 others lie inside the bin range; the rest at 5.2 <= |v| <= 6, where
    every term is below the floor, which keeps the truth sparse."""
    N = BIG
    rng = np.random.default_rng(seed)
    V = rng.uniform(5.2, 6.0, (3, N)) * rng.choice([-1.0, 1.0], (3, N))
    chunk = -(-N // 512)
    assert chunk == 258
    second = np.array([z * chunk + k for z in range(512) for k in (256, 257) if z * chunk + k < min(N, (z + 1) * chunk)])
    assert second.size == 1022
    small = velocities(3000, seed + 1, shift=0.0)
    for c in range(3):
        V[c, second] = rng.uniform(-4.9, 4.9, second.size)
        others = rng.choice(np.setdiff1d(np.arange(N), second), 3000, replace=False)
        V[c, others] = small[c]
    V[0] += 0.37
    return V


def positions(N, L, seed=11):
    return np.random.default_rng(seed).uniform(0, L, (3, N))


def random_psi(N, model, seed=5):
    """random complex amplitudes, a third of the ions unnormalised; for model 3 states 5..11 are non-zero in the
    input (the populations ignore them)"""
    rng = np.random.default_rng(seed + model)
    z = rng.normal(size=(N, 12)) + 1j * rng.normal(size=(N, 12))
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    z[::3] *= rng.uniform(0.1, 3.0, (len(z[::3]), 1))
    return np.ascontiguousarray(np.stack([z.real, z.imag], -1))


def lone_edge_terms(tr):
    """the wave-edge bins of y and z that hold nothing but the terms of order 1e-314 of the ions at 0.0761"""
    return [(c, j) for c in (1, 2) for j in WAVE_EDGE_BINS if LD(1e-316) < tr.P[c, j] < LD(1e-311)]


def quiet_bins(tr):
    """(axis, bin) of the y and z bins whose value is a non-zero subnormal"""
    P = tr.P[1:]
    c, j = np.nonzero((P > 0) & (P < LD(2.0) ** -1022))
    return list(zip((c + 1).tolist(), j.tolist()))


_V, _T = {}, {}


def case_velocities(name):
    """name: "N<size>", "drift257", "big" -> V[3][N] (read-only, cached)"""
    if name not in _V:
        if name == "big":
            V = big_velocities()
        elif name == "drift257":
            V = velocities(257, 3, drift=True)
        else:
            N = int(name[1:])
            seed = 100
            V = velocities(N, seed)
            while N in QUIET_SIZES and not lone_edge_terms(ot.observables(V)):
                seed += 1
                V = velocities(N, seed)
        V.setflags(write=False)
        _V[name] = V
    return _V[name]


def kinetic_truth(name):
    """the truth of a case without the potential rows (<vx>, the kinetic sums, P): cached"""
    if name not in _T:
        _T[name] = ot.observables(case_velocities(name))
    return _T[name]


def with_potential(name, Urow, t=0.0, Epot0=0.0):
    """the cached truth completed with the engine's potential rows (sum U_i is the exact sum of these)"""
    k = kinetic_truth(name)
    V = case_velocities(name)
    r = ot.Truth()
    r.__dict__.update(k.__dict__)
    r.sums, r.B_sums, r.T_sums = ot.energy_sums(V, k.avg, k.B_avg, Urow)
    r.out7, r.B_out7 = ot.finish(r.sums, r.B_sums, k.avg, k.B_avg, V.shape[1], t, Epot0)
    return r


NAMES = tuple(f"N{n}" for n in SIZES) + ("drift257", "big")

# ---- the tagged distribution ----
TAG_SIZES = (255, 256, 257, 513)
TAG_PATTERNS = ("all", "first", "last", "middle_off", "alternate", "none")


def tag_pattern(N, pattern):
    t = np.zeros(N, dtype=np.int32)
    if pattern == "all":
        t[:] = 1
    elif pattern == "first":
        t[0] = 1
    elif pattern == "last":                      # the last ion of the (ragged) last chunk of 256
        t[N - 1] = 1
    elif pattern == "middle_off":                # a whole chunk untagged (N = 513: ions 256..511), else the middle third
        t[:] = 1
        if N > 512:
            t[256:512] = 0
        else:
            t[N // 3:2 * N // 3] = 0
    elif pattern == "alternate":
        t[::2] = 1
    return t


def tag_psi(tags):
    """an ion wholly in state 0 is always tagged, one wholly in state 1 never (tag_spin_up_ion)"""
    z = np.zeros((tags.size, 12), complex)
    z[np.arange(tags.size), np.where(tags != 0, 0, 1)] = 1.0
    return z


def tagged_velocities(N):
    name = f"tag{N}"
    if name not in _V:
        V = velocities(N, 40 + N, shift=0.0, edge_j=EDGE_J_TAGGED)
        V.setflags(write=False)
        _V[name] = V
    return _V[name]


def tagged_truth(N, pattern):
    key = (N, pattern)
    if key not in _T:
        _T[key] = ot.tagged(tagged_velocities(N), tag_pattern(N, pattern))
    return _T[key]
