// The programs' main() time loops, written once: SpeedUp's (laserCoolingPlusExpansionMDQTSpeedUp.cpp:1248-1383)
// and the optical-pumping programs' (randomFrozenStartTag408Linear.cpp:1050-1080).  A loop decides WHEN things
// happen: the outputs, the MD intervals, how many substeps one launch fuses, which half drifts ride along with a
// kick launch.  Its driver says WHAT one operation is: a lone context's call (mdqt_run, mdqt_run_pump) or one
// batched call over an ensemble's members in lockstep (mdqt_ensemble_run, mdqt_pump_ensemble_run).  A driver's
// operations return nonzero after they have set the error; t() and c0() are the context's, or member 0's.
// Host only, no HIP (MAXSUB is the schedule's maxsub): tests/test_main_loops.py runs the cadence on the CPU.
#pragma once

namespace mdqt {

struct SpeedUpSchedule { double dtQ, tend; int sampleFreq, ratio, maxsub; };      // tend = tmax + 0.0009

// main()'s loop, looking ahead from t with MD step counter c0 and ts substeps of the interval done: how
// many of the following iterations are pure step(); qstep() (App. C-9), i.e. can run as one launch — up to
// maxsub, the end of the run, the next output (:1365) or the end of the interval, whichever comes first
inline int fusable_substeps(double t, double dtQ, double tend, long c0, int ts, int sampleFreq, int ratio, int maxsub) {
    int n = 0;
    do {
        n++; ts++; t += dtQ;
    } while (n < maxsub && t <= tend && !((c0 + 1) % sampleFreq == 0 && ts == 1) && ts != ratio);
    return n;
}

// Driver: t(), c0(), output(), may_fuse_interval(), start_interval(whole), substeps(n).  start_interval(false)
// is forces() and c0++; start_interval(true) is the whole interval (forces(), c0++, `ratio` substeps) as one
// launch, asked for only when may_fuse_interval() says that the driver has such a launch now and the look-ahead
// finds no output and no end of the run inside the interval.
template <class Driver>
int speedup_loop(const SpeedUpSchedule& k, Driver& d) {
    int tsc = k.ratio;                                                                  // :1235
    while (d.t() <= k.tend) {                                                           // :1248
        if ((d.c0() + 1) % k.sampleFreq == 0 && tsc == 1)                               // :1365
            if (d.output()) return -1;
        if (tsc == k.ratio) {                                                           // :1369
            const bool whole = d.may_fuse_interval() &&
                               fusable_substeps(d.t(), k.dtQ, k.tend, (long)d.c0() + 1, 0, k.sampleFreq, k.ratio, k.maxsub) == k.ratio;
            if (d.start_interval(whole)) return -1;
            if (whole) continue;                        // tsc stays = ratio
            tsc = 0;
        }
        const int n = fusable_substeps(d.t(), k.dtQ, k.tend, d.c0(), tsc, k.sampleFreq, k.ratio, k.maxsub);
        if (d.substeps(n)) return -1;                                                   // :1376-1377
        tsc += n;
    }
    return 0;
}

// qstep() runs while tstartV0 < t < tendV0 (:1075), the tagging at the first t >= tendV0 (:1052)
struct PumpSchedule { double dtQ, tend, tstartV0, tendV0; int sampleFreq, ratio, maxsub; };

// After the MD step at hand (c0n: c0 with that step counted): does the loop reach the next MD step, at a t > 0,
// before anything reads R, V or F — the measurement, an output, the end of the run?  The loop's own conditions,
// run ahead on copies (both branches of the loop's tail advance t by the same t += dtQ).
inline bool pump_step_folds(const PumpSchedule& k, double t, int c0n, int recorded) {
    for (int ts = 0;;) {
        t += k.dtQ; ts++;
        if (!(t <= k.tend)) return false;
        if (recorded == 0 && t >= k.tendV0) return false;
        if ((c0n + 1) % k.sampleFreq == 0 && ts == 1 && recorded == 1) return false;
        if (ts == k.ratio) return t > 0;
    }
}

// Driver: t(), c0(), qsteps(n), measure() (measureSpinUps and its file), output(vaf) (output(), Zfunc(vaf),
// printVAF), md_step(lead, fold) (step() and c0++), idle() (the t += dtQ of an iteration without a qstep) and
// fail(what), which sets the error "<entry point>: <what>" and returns nonzero.  lead: the step's leading half
// drift is still to be done; fold: the next step's may go with this step's kick launch (a driver whose step does
// both of its own half drifts ignores the two).  recorded: recordedSpinUps (:81), 1 on a resumed run.  qsteps
// are queued and run as one fused launch of at most maxsub: the loop's t (tv) runs ahead of the driver's by
// `pending` qsteps and must equal it, bit for bit, after every flush.
template <class Driver>
int pump_loop(const PumpSchedule& k, int recorded, Driver& d) {
    int tsc = k.ratio, pending = 0;                              // :1033
    double tv = d.t();
    bool lead_done = false;                                      // the next step's leading drift went with the last launch
    auto flush = [&]() -> int {
        if (pending > 0) {
            if (d.qsteps(pending)) return -1;                    // qstep() x pending :396-598
            pending = 0;
            if (d.t() != tv) return d.fail("time bookkeeping mismatch");
        }
        return 0;
    };
    while (tv <= k.tend) {                                       // :1050
        if (recorded == 0 && tv >= k.tendV0) {                   // :1052-1058
            if (flush() || d.measure()) return -1;
            recorded = 1;
            if (d.output(0)) return -1;
        }
        if ((d.c0() + 1) % k.sampleFreq == 0 && tsc == 1 && recorded == 1)   // :1062-1069
            if (flush() || d.output(1)) return -1;
        if (tsc == k.ratio) {                                    // :1070-1074
            if (flush()) return -1;
            const bool fold = pump_step_folds(k, tv, d.c0() + 1, recorded);
            if (d.md_step(!lead_done, fold)) return -1;
            lead_done = fold;
            tsc = 0;
        }
        if (tv < k.tendV0 && tv > k.tstartV0) {                  // :1075-1077 qstep()
            pending++;
            tv += k.dtQ;                                         // qstep's t += dtQuant :597
            if (pending == k.maxsub && flush()) return -1;
        } else {                                                 // :1078-1080
            if (flush() || d.idle()) return -1;
            tv = d.t();
        }
        tsc++;
    }
    if (flush()) return -1;
    return lead_done ? d.fail("a folded drift without its step") : 0;
}

}  // namespace mdqt
