"""The cadence of the programs' main() time loops (mdqtplasmasims_amd/csrc/mdqt_main_loops.hpp), which the four
run entry points share: which calls happen in which order, how many substeps a launch fuses, which half drifts
ride along with a kick launch.  CPU only: tests/native/main_loops_check.cpp (compiled with g++ here) runs each
loop with a driver that records its calls; this file holds the reference's loops one iteration at a time
(SpeedUp:1248, :1365, :1369, :1376; randomFrozenStartTag408Linear.cpp:1050-1080) and compares.

Doubles travel as hex floats, and both sides advance t by separate t += dtQ, so the final t is compared bit for
bit."""
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mdqtplasmasims_amd", "csrc")
MAXSUB = 32                       # mdqt_internal.hpp
TIMESTEP = 0.002


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loops") / "main_loops_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC,
                        os.path.join(HERE, "native", "main_loops_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_cases(driver, lines):
    """the recorded calls, the loop's result, the final t and c0 of every case"""
    r = subprocess.run([driver], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    res = []
    for ln in out:
        calls, tail = ln.split("|")
        w = tail.split()
        assert w[0::2] == ["rc", "t", "c0"]
        res.append((calls.split(), int(w[1]), float.fromhex(w[3]), int(w[5])))
    return res


def start_of(c0):
    """(t, c0, recorded): a new run, or a resume at c0"""
    return (0.0, 0, 0) if c0 is None else ((c0 - 9) * 0.002 + 0.02, c0, 1)


def hx(*xs):
    return " ".join(float(x).hex() for x in xs)


# ---- the SpeedUp program ----
def speedup_unfused(ratio, sf, dtQ, tend, t, c0):
    seq = []
    tsc = ratio                                             # :1235
    while t <= tend:                                        # :1248
        if (c0 + 1) % sf == 0 and tsc == 1:                 # :1365
            seq.append("O")
        if tsc == ratio:                                    # :1369
            seq.append("F")
            c0 += 1
            tsc = 0
        seq.append("s")                                     # :1376-1377 step(); qstep()
        t += dtQ
        tsc += 1
    return "".join(seq), t, c0


SPEEDUP_RATIOS = (25, 35, 50, 21)
SPEEDUP_STARTS = (None, 20, 39)
SPEEDUP_REST = list(itertools.product((1, 2, 40, 100000), (0.2, 0.05, 0.0115, 0.0), (0, 1)))   # sampleFreq, tmax, fuse


@pytest.mark.parametrize("start", SPEEDUP_STARTS)
@pytest.mark.parametrize("ratio", SPEEDUP_RATIOS)
def test_speedup_loop(driver, ratio, start):
    dtQ = TIMESTEP / ratio
    t0, c0, _ = start_of(start)
    lines = [f"S {ratio} {sf} {MAXSUB} {hx(dtQ, tmax + 0.0009, t0)} {c0} {fuse}" for sf, tmax, fuse in SPEEDUP_REST]
    fused_intervals = 0
    for (sf, tmax, fuse), (calls, rc, t, c) in zip(SPEEDUP_REST, run_cases(driver, lines)):
        what = f"ratio {ratio} sampleFreq {sf} tmax {tmax} start {start} fuse {fuse}"
        assert rc == 0, what
        seq = []
        for w in calls:
            if w[0] == "S":
                assert 1 <= int(w[1:]) <= MAXSUB, what
                seq.append("s" * int(w[1:]))
            elif w == "W":                                  # one launch: forces() and the interval's substeps
                assert fuse and ratio <= MAXSUB, what
                fused_intervals += 1
                seq.append("F" + "s" * ratio)
            else:
                assert w in ("O", "F"), what
                seq.append(w)
        want, wt, wc = speedup_unfused(ratio, sf, dtQ, tmax + 0.0009, t0, c0)
        assert "".join(seq) == want, what
        assert t.hex() == wt.hex() and c == wc, what
    assert (fused_intervals > 0) == (ratio <= MAXSUB), "the fused branch did not run"


# ---- the optical-pumping programs ----
def pump_unfused(ratio, sf, dtQ, tend, tstartV0, tendV0, t, c0, recorded):
    seq = []
    tsc = ratio                                             # :1033
    while t <= tend:                                        # :1050
        if recorded == 0 and t >= tendV0:                   # :1052-1058
            seq.append("TO0")                               # measureSpinUps, output, Zfunc(0), printVAF
            recorded = 1
        if (c0 + 1) % sf == 0 and tsc == 1 and recorded == 1:   # :1062-1069
            seq.append("O1")
        if tsc == ratio:                                    # :1070-1074
            seq.append("M")
            c0 += 1
            tsc = 0
        if tendV0 > t > tstartV0:                           # :1075-1077
            seq.append("q")
            t += dtQ
        else:                                               # :1078-1080
            seq.append("i")
            t += dtQ
        tsc += 1
    return "".join(seq), t, c0


PUMP_RATIOS = (25, 35, 50, 21, 22)
PUMP_STARTS = (None, 20, 49)
PUMP_REST = list(itertools.product((1, 10, 40, 100000), (0.3, 0.05, 0.011), (0.1, 0.0, 0.02, 1.0),
                                   (0.12, 0.0371, 0.001, 5.0)))      # sampleFreq, tmax, tstartV0, pump length


def check_folds(calls, what):
    """md_step(lead, fold): the leading drifts are each done once, and a drift is folded exactly when it may be"""
    steps = [(i, w) for i, w in enumerate(calls) if w[0] == "M"]
    prev_fold = False
    for n, (i, w) in enumerate(steps):
        lead, fold, t = w[1] == "1", w[2] == "1", float.fromhex(w[4:])
        assert lead == (not prev_fold), what
        if t == 0:
            assert lead, what
        nxt = next((x for x in calls[i + 1:] if x[0] not in "IQ"), None)
        assert fold == (nxt is not None and nxt[0] == "M" and float.fromhex(nxt[4:]) > 0), f"{what}: step {n} at t {t}"
        prev_fold = fold
    assert not prev_fold, what
    return sum(w[1] == "1" for _, w in steps), sum(w[2] == "1" for _, w in steps)


@pytest.mark.parametrize("start", PUMP_STARTS)
@pytest.mark.parametrize("ratio", PUMP_RATIOS)
def test_pump_loop(driver, ratio, start):
    dtQ = TIMESTEP / ratio
    t0, c0, recorded = start_of(start)
    lines = [f"P {ratio} {sf} {MAXSUB} {hx(dtQ, tmax + 0.0009, ts, ts + length, t0)} {c0} {recorded}"
             for sf, tmax, ts, length in PUMP_REST]
    folded = 0
    for (sf, tmax, ts, length), (calls, rc, t, c) in zip(PUMP_REST, run_cases(driver, lines)):
        what = f"ratio {ratio} sampleFreq {sf} tmax {tmax} tstartV0 {ts} pump {length} start {start}"
        assert rc == 0, what                                # neither the t == tv check nor an unused fold
        seq = []
        for w in calls:
            if w[0] in "QI":
                if w[0] == "Q":
                    assert 1 <= int(w[1:]) <= MAXSUB, what
                seq.append(w[0].lower() * int(w[1:]))
            elif w[0] == "M":
                seq.append("M")
            else:
                assert w in ("T", "O0", "O1"), what
                seq.append(w)
        want, wt, wc = pump_unfused(ratio, sf, dtQ, tmax + 0.0009, ts, ts + length, t0, c0, recorded)
        assert "".join(seq) == want, what
        assert t.hex() == wt.hex() and c == wc, what
        folded += check_folds(calls, what)[1]
    assert folded > 0
