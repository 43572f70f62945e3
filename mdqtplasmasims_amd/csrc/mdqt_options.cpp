// mdqt_get_const and mdqt_set_option, the stream entry points, and the timing events of the hot kernels.

#include <math.h>
#include <stdlib.h>

#include "mdqt_ctx.hpp"

using namespace mdqt;

// mdqt_get_const's pair-form tiers: the names of a tier's radius and force bound, its exponent option and its
// level (far_err)
struct TierConst { const char *radius, *bound; int mdqt_ctx::*exp; int level; };
static const TierConst kTierConsts[] = {
    {"force_far_radius", "force_far_bound", &mdqt_ctx::far_exp, 1},
    {"force_mid_radius", "force_mid_bound", &mdqt_ctx::mid_exp, 5},
    {"force_vfar_radius", "force_vfar_bound", &mdqt_ctx::vfar_exp, 2},
    {"force_ufar_radius", "force_ufar_bound", &mdqt_ctx::ufar_exp, 3},
};
// a tier's radius and force bound as the force call takes them (L/2 and 0: off): the tiers apply to the
// Newton-3 blocks in spatial order with the fast pair form and no range guard; the mid form needs its table
static double tier_const(const mdqt_ctx* s, int k, int level, double* bound) {
    *bound = 0.;
    const bool on = s->use_n3b && s->sort_mode != 0 && s->force_variant == 1 && !s->guard;
    return on ? tier_radius(s, k, level, bound) : s->L / 2.;
}

extern "C" double mdqt_get_const(const mdqt_ctx* s, const char* n) {
    if (!strcmp(n, "gamToEinsteinFreq")) return s->gamToE;
    if (!strcmp(n, "quantumTimestep")) return s->dtQ;
    if (!strcmp(n, "plasmaToQuantumTimestepRatio")) return s->ratio;
    if (!strcmp(n, "plasVelToQuantVel")) return s->pv2q;
    if (!strcmp(n, "vKick")) return s->vKick;
    if (!strcmp(n, "vKickDP")) return s->vKickDP;
    if (!strcmp(n, "lDeb")) return s->lDeb;
    if (!strcmp(n, "L")) return s->L;
    if (!strcmp(n, "range_guard")) return s->guard ? 1 : 0;   // the pair kernels range-check (see poll_flags)
    if (!strcmp(n, "decayRatioD5Halves")) return s->r;
    if (!strcmp(n, "kRat")) return s->kRat;
    if (!strcmp(n, "force_segments")) return s->nseg;
    if (!strcmp(n, "force_scheme")) return s->use_n3b ? 3 : s->use_n3 ? 2 : 1;
    if (!strcmp(n, "force_sort")) return s->use_n3b ? s->sort_mode : 0;
    if (!strcmp(n, "force_ax1")) return s->ax1_mode;
    if (!strcmp(n, "force_reduce_mask")) return s->tmask_mode;
    if (!strcmp(n, "force_tile_split")) return s->split_opt;
    if (!strcmp(n, "force_split_cus")) return s->split_cus;
    if (!strcmp(n, "force_tile_split_pairs")) return s->nsplit;
    if (!strcmp(n, "device_cus")) {                    // compute units of the context's device
        int ncu = 0;
        return hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->dev) == hipSuccess ? ncu : -1;
    }
    if (!strcmp(n, "force_balance")) return s->balance_opt;
    if (!strcmp(n, "force_balance_ratio")) return s->balance_ratio;           // max / mean rank work (NaN: not sharded yet)
    if (!strcmp(n, "force_balance_ratio_equal")) return s->balance_ratio_eq;  // the same for equal block counts
    if (!strcmp(n, "n3b_block_lo")) return s->use_n3b ? s->n3b.Plo : 0;
    if (!strcmp(n, "n3b_block_hi")) return s->use_n3b ? s->n3b.Phi : 0;
    if (!strcmp(n, "force_skip_radius") || !strcmp(n, "force_tail_bound")) {   // the tile-pair skip radius
        double bound;                                  // and its force bound (0: exact, r = L/2)
        const double r = (s->use_n3b && s->sort_mode == 1) ? skip_radius(s, &bound) : (bound = 0., s->L / 2.);
        if (n[6] == 's') return r;
        N3BArgs ea{};                                  // (what the call's sums hold: error_eps > 0)
        ea.Rcut = s->L / 2.; ea.Rskip = r;
        if (s->use_n3b) tier_radii(s, ea);
        if (s->use_n3b && (tail_measured(s) || form_measured(s)) && error_eps(s, ea) > 0.) {
            // mode 1: the running maximum of the per-tile sums each call met after the exact pass
            // (1e-12 relative: the device sum's rounding); NaN until a force call has measured.  With
            // force_form_mode 1 the sums hold the error-bounded forms' terms too: the bound on every
            // ion's total deviation from the exact sum to L/2 (held to force_error_eps)
            unsigned long long h[8];
            if (!s->dTailSt || hipStreamSynchronize(s->stream) != hipSuccess ||
                hipMemcpy(h, s->dTailSt, sizeof h, hipMemcpyDeviceToHost) != hipSuccess || h[4] == 0) return NAN;
            return u64_as_double(h[0]) * (1. + 1e-12);
        }
        return bound;
    }
    // mode 1 diagnostics: the largest per-tile sum the skip radius alone left (before the exact
    // pass), the tiles that exceeded eps so far, the measured force calls, the model scale
    if (!strcmp(n, "force_tail_raw_bound") || !strcmp(n, "force_tail_fixed_tiles") ||
        !strcmp(n, "force_tail_calls")) {
        unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (s->dTailSt && (hipStreamSynchronize(s->stream) != hipSuccess ||
                           hipMemcpy(h, s->dTailSt, sizeof h, hipMemcpyDeviceToHost) != hipSuccess)) return NAN;
        if (n[11] == 'r') return u64_as_double(h[1]) * (1. + 1e-12);
        return (double)(n[11] == 'f' ? h[2] : h[4]);
    }
    if (!strcmp(n, "force_tail_scale")) return s->tail_scale;
    if (!strcmp(n, "force_tail_model_bound")) {       // mode 1: the model bound r_t was chosen by
        double bound;
        const double r = (s->use_n3b && tail_measured(s)) ? tail_radius_sum(s, &bound) : (bound = 0., 0.);
        (void)r;
        return bound;
    }
    if (!strcmp(n, "force_tail_mode")) return s->tail_mode;
    if (!strcmp(n, "force_form_mode")) return s->form_mode;
    if (!strcmp(n, "force_form_measured")) return form_measured(s) ? 1. : 0.;
    if (!strcmp(n, "force_error_eps")) {               // the eps the measured sums are held to (0: none)
        if (!(s->use_n3b && (tail_measured(s) || form_measured(s)))) return 0.;
        N3BArgs a{};
        double b;
        a.Rcut = s->L / 2.;
        a.Rskip = skip_radius(s, &b);
        tier_radii(s, a);
        return error_eps(s, a);
    }
    for (const TierConst& tc : kTierConsts) {          // the error-bounded pair forms' radii and force bounds
        const bool radius = !strcmp(n, tc.radius);
        if (!radius && strcmp(n, tc.bound)) continue;
        double bound;
        double r = tier_const(s, s->*tc.exp, tc.level, &bound);
        if (tc.level == 3) {                           // ultra far: never beyond f32's normal range (tier_radii)
            if (r < s->L / 2. && s->L / 2. > 80. * s->lDeb) { r = s->L / 2.; bound = 0.; }
            double b32 = 0.;                           // + the f32 shell beyond force_ufar32_radius
            if (r < s->L / 2.) tier_radius(s, s->ufar_exp, 4, &b32);
            bound += b32;
        }
        return radius ? r : bound;
    }
    if (!strcmp(n, "force_ufar32_radius")) {          // the f32 ultra-far form's radius (L/2: off)
        double bound;
        const double r3 = mdqt_get_const(s, "force_ufar_radius");
        return r3 < s->L / 2. ? tier_radius(s, s->ufar_exp, 4, &bound) : s->L / 2.;
    }
    if (!strcmp(n, "fused_step")) return s->fused_opt;
    if (!strcmp(n, "qt_im01")) return s->qc.im01;
    if (!strcmp(n, "potential_n3")) return s->n3_potential;
    if (!strcmp(n, "potential_plan")) return s->pot_plan;
    if (!strcmp(n, "force_n3b_pairs")) return s->n3b_pairs;
    if (!strcmp(n, "md_step_fused")) return s->last_fused;     // 1: the last MD step was one k_md_step launch
    if (!strcmp(n, "qt_kernel")) return s->last_qt_kernel;     // instance of the last substep launch (QTKernel)
    if (!strcmp(n, "qt_kernel_nseg")) return s->last_qt_nseg;  // force partials its prologue summed
    if (!strcmp(n, "force_slots")) return s->nslots;           // Newton-3 tile slots (0: other schemes)
    if (!strcmp(n, "n3b_blocks")) return s->use_n3b ? s->n3b.Phi - s->n3b.Plo : 0;   // this rank's blocks
    if (!strcmp(n, "n3b_block_count")) return s->use_n3b ? s->n3b.NB : 0;             // all blocks
    if (!strcmp(n, "slab_S")) return s->S;
    if (!strncmp(n, "gs", 2)) return s->gs[atoi(n + 2)];
    return NAN;
}

// mdqt_set_option: one row per option.  A value outside [lo, hi] gives range_error.  Then a row with a
// handler (the options with logic of their own) leaves the rest to it; every other row stores the value in
// its field, after completing what the old value left behind and before rebuilding what the new one sizes:
enum Invalidates {
    NOTHING,        // read at the next launch
    SETTLE,         // pending force partials were formed under the old value: settle_forces
    SETTLE_RESET,   // ... and, where the value differs (and reset_when holds), the measured tail sums: tail_reset
    SETTLE_AUX,     // ... and the buffers and tables sized by it: ensure_aux
};
struct Option {
    const char* name;
    int lo, hi;
    const char* range_error;
    Invalidates inv;
    int mdqt_ctx::*field;                   // nullptr: the handler stores the value
    int (*handler)(mdqt_ctx*, int) = nullptr;
    bool (*reset_when)(const mdqt_ctx*) = nullptr;
};

static int set_force_scheme(mdqt_ctx* s, int value) {
    if (value == 2 && s->p.world_size != 1) return set_error("force_scheme 2 needs world_size 1");
    if (settle_forces(s)) return -1;
    s->scheme_opt = value;
    choose_segments(s);
    return ensure_aux(s);
}
static int set_expt_force_sig(mdqt_ctx* s, int value) {
    if (value && arrive_setup(s)) return -1;
    s->force_arrive = value ? s->dArrive : nullptr;
    return 0;
}
static int set_qt_im01(mdqt_ctx* s, int value) {
    if (value) {                                   // only where the table allows it
        int ok = 1;
        for (int k = 0; k < 16; ++k)
            if (s->ftab.cre[0][k] != 0. || s->ftab.cre[1][k] != 0.) ok = 0;
        if (!ok) return set_error("qt_im01: the static coupling slots are not purely imaginary");
    }
    s->qc.im01 = value;
    return 0;
}
static int set_force_balance(mdqt_ctx* s, int value) {
    if (value != s->balance_opt) {
        if (settle_forces(s)) return -1;
        s->balance_opt = value;
        if (s->use_n3b) {                           // back to the equal ranges; weighted again at the next call
            const int W = s->p.world_size;
            n3b_set_range(s->n3b, (int)((long)s->p.rank * s->n3b.NB / W), (int)((long)(s->p.rank + 1) * s->n3b.NB / W));
            s->balanced = false;
            if (ensure_aux(s)) return -1;
        }
    }
    return 0;
}
static int set_qt_enabled(mdqt_ctx* s, int value) { s->p.qt_enabled = value; return 0; }
static int set_qt_math(mdqt_ctx* s, int value) {
    if (value != 2 && s->p.qt_model != 0) return set_error("the optical-pumping qt_models need qt_math 2");
    s->qt_math = value;
    return 0;
}

static const Option kOptions[] = {
    {"force_scheme", 0, 3, "force_scheme must be 0 (auto), 1 (rows), 2 (Newton-3 tiles) or 3 (Newton-3 blocks)",
     NOTHING, nullptr, set_force_scheme},
    // diagnostic: unfused force launches with the fused step's signalling
    {"expt_force_sig", 0, 1, "expt_force_sig must be 0 or 1", NOTHING, nullptr, set_expt_force_sig},
    // Epotential on the Newton-3 tiles (1) or the rows (0)
    {"potential_n3", 0, 1, "potential_n3 must be 0 or 1", NOTHING, &mdqt_ctx::n3_potential},
    // Newton-3 blocks: 4 waves on two I tiles each (1) or 8 waves (0)
    {"force_n3b_pairs", 0, 1, "force_n3b_pairs must be 0 (8 waves, one I tile each) or 1 (4 waves, two each)",
     SETTLE, &mdqt_ctx::n3b_pairs},
    // Epotential on the blocks: the force call's plan (1) or exact (0)
    {"potential_plan", 0, 1, "potential_plan must be 0 (every pair to L/2) or 1 (the plan)", NOTHING, &mdqt_ctx::pot_plan},
    // 0: the general FAST lane instance (tests)
    {"qt_im01", 0, 1, "qt_im01 must be 0 or 1", NOTHING, nullptr, set_qt_im01},
    // one k_md_step launch per MD step (mdqt_md_steps)
    {"fused_step", 0, 1, "fused_step must be 0 or 1", NOTHING, &mdqt_ctx::fused_opt},
    // force || QT launches of an MD step (mdqt_md_steps)
    {"overlap", 0, 1, "overlap must be 0 or 1", NOTHING, &mdqt_ctx::overlap_opt},
    // the error-bounded pair forms: eps = 10^-value (0: off).  force_form_mode >= 1: the measured sums hold
    // their terms — forget what earlier calls measured
    {"force_ufar_exp", 0, 300, "force_ufar_exp must be 0 (off) .. 300", SETTLE_RESET, &mdqt_ctx::ufar_exp, nullptr, form_measured},
    {"force_vfar_exp", 0, 300, "force_vfar_exp must be 0 (off) .. 300", SETTLE_RESET, &mdqt_ctx::vfar_exp, nullptr, form_measured},
    {"force_mid_exp", 0, 300, "force_mid_exp must be 0 (off) .. 300", SETTLE_RESET, &mdqt_ctx::mid_exp, nullptr, form_measured},
    {"force_far_exp", 0, 300, "force_far_exp must be 0 (off) .. 300", SETTLE_RESET, &mdqt_ctx::far_exp, nullptr, form_measured},
    // error-bounded tail: eps = 10^-value (0: exact)
    {"force_tail_exp", 0, 300, "force_tail_exp must be 0 (exact) .. 300", SETTLE_RESET, &mdqt_ctx::tail_exp},
    // the tiers' radii: 0 a priori, 1 measured and enforced, 2 as 1 with an exact tail's eps shared
    {"force_form_mode", 0, 2, "force_form_mode must be 0 (a priori), 1 (measured) or 2 (measured, sharing an exact tail's eps)",
     SETTLE_RESET, &mdqt_ctx::form_mode},
    // 0: a-priori bound, 1: measured and enforced
    {"force_tail_mode", 0, 1, "force_tail_mode must be 0 (a priori) or 1 (measured)", SETTLE_RESET, &mdqt_ctx::tail_mode},
    // sharded Newton-3 blocks: ranges by work (1) or by count (0)
    {"force_balance", 0, 1, "force_balance must be 0 (equal block counts) or 1 (by work)", NOTHING, nullptr, set_force_balance},
    // Newton-3 tiles: the last round's whole tile pairs as halves
    {"force_tile_split", 0, 2, "force_tile_split must be 0 (off), 1 (halves) or 2 (quarters)", SETTLE_AUX, &mdqt_ctx::split_opt},
    // the CU count the split table is cut for (0: the device's)
    {"force_split_cus", 0, 65536, "force_split_cus must be 0 (the device's CU count) or a CU count",
     SETTLE_AUX, &mdqt_ctx::split_cus},
    // Newton-3 blocks: the reduction reads only written j-slots
    {"force_reduce_mask", 0, 1, "force_reduce_mask must be 0 (every j-slot) or 1 (the written ones)",
     SETTLE, &mdqt_ctx::tmask_mode},
    // Newton-3 blocks: the one-axis per-pair image instance
    {"force_ax1", 0, 1, "force_ax1 must be 0 (off) or 1 (where the skip radius reaches L/2)", SETTLE, &mdqt_ctx::ax1_mode},
    // Newton-3 blocks: Hilbert order + tile-pair skipping
    {"force_sort", 0, 2, "force_sort must be 0 (off), 1 (on) or 2 (sorted, no skipping)", SETTLE_AUX, &mdqt_ctx::sort_mode},
    // pump window of the tagging programs
    {"qt_enabled", 0, 1, "qt_enabled must be 0 or 1", NOTHING, nullptr, set_qt_enabled},
    {"qt_math", 0, 2, "qt_math must be 0 (exact), 1 (FMA-contracted) or 2 (reassociated)", NOTHING, nullptr, set_qt_math},
    // (tail_measured changes with it)
    {"force_kernel", 0, 1, "force_kernel must be 0 (exact) or 1 (fast)", SETTLE_RESET, &mdqt_ctx::force_variant},
    // init() sampling: 0 auto, 1 sequential, k threads
    {"init_threads", 0, 256, "init_threads must be in [0, 256]", NOTHING, &mdqt_ctx::init_threads},
    {"substep_kernel", 0, 2, "substep_kernel must be 0 (auto), 1 (thread/ion) or 2 (lanes/ion)", NOTHING, &mdqt_ctx::substep_mode},
};

extern "C" int mdqt_set_option(mdqt_ctx* s, const char* name, int value) {
    if (!s || !name) return set_error("mdqt_set_option: NULL argument");
    for (const Option& o : kOptions) {
        if (strcmp(name, o.name)) continue;
        if (value < o.lo || value > o.hi) return set_error("%s", o.range_error);
        if (o.handler) return o.handler(s, value);
        if (o.inv == SETTLE_RESET) {
            if (value != s->*o.field && (!o.reset_when || o.reset_when(s)) && (settle_forces(s) || tail_reset(s))) return -1;
        } else if (o.inv != NOTHING && settle_forces(s)) {
            return -1;
        }
        s->*o.field = value;
        return o.inv == SETTLE_AUX ? ensure_aux(s) : 0;
    }
    return set_error("unknown option %s", name);
}

extern "C" int mdqt_set_stream(mdqt_ctx* s, void* st) {
    s->stream = st ? (hipStream_t)st : s->own;
    return 0;
}
extern "C" void* mdqt_get_stream(mdqt_ctx* s) { return (void*)s->stream; }
extern "C" int mdqt_synchronize(mdqt_ctx* s) {
    HIPCHK(hipSetDevice(s->dev));
    HIPCHK(hipStreamSynchronize(s->stream));
    return check_range_flag(s);
}
extern "C" int mdqt_positions_device(mdqt_ctx* s, void** dptr, int* S) {
    if (dptr) *dptr = (void*)s->dR;
    if (S) *S = s->S;
    return 0;
}

// record the next timing event of kind k (start/stop alternate)
int mdqt::mark(mdqt_ctx* s, int k) {
    hipEvent_t e = nullptr;
    if (s->timers[k].next(&e)) return -1;
    HIPCHK(hipEventRecord(e, s->stream));
    return 0;
}

// force-call breakdown (timing kind bit 3): one event recorded now on the context stream, from the free list
hipEvent_t mdqt::bd_event(mdqt_ctx* s) {
    hipEvent_t e = nullptr;
    if (!s->bdfree.empty()) { e = s->bdfree.back(); s->bdfree.pop_back(); }
    else if (hipEventCreateWithFlags(&e, kTimingEventFlags) != hipSuccess) return nullptr;
    if (hipEventRecord(e, s->stream) != hipSuccess) { s->bdfree.push_back(e); return nullptr; }
    return e;
}
// will the next force call be timed (its tcount not yet advanced)?
bool mdqt::force_timed_next(const mdqt_ctx* s) {
    return s->timing && (s->tkinds & 1u) && (s->tkinds & 8u) && (s->tcount[0] % s->tperiod == s->toffset);
}

extern "C" int mdqt_enable_timing_at(mdqt_ctx* s, int on, int kinds, int offset) {
    if (!s) return set_error("NULL context");
    if (kinds < 1 || kinds > 15) return set_error("mdqt_enable_timing_at: kinds must be 1 .. 15 (bits: force, substeps, potential block kernel, force breakdown)");
    if (on > 0 && (offset < 0 || offset >= on)) return set_error("mdqt_enable_timing_at: offset must be in [0, period)");
    s->timing = on > 0;
    s->tperiod = on > 0 ? (unsigned)on : 1u;
    s->toffset = on > 0 ? (unsigned)offset : 0u;
    s->tkinds = (unsigned)kinds;
    s->tcount[0] = s->tcount[1] = 0;
    for (LaunchTimer& t : s->timers) t.reset();
    for (auto& c : s->bdcalls) {                    // (the breakdown restarts with the timing)
        for (hipEvent_t e : c.m) if (e) s->bdfree.push_back(e);
        if (c.ag0) s->bdfree.push_back(c.ag0);
        if (c.ag1) s->bdfree.push_back(c.ag1);
    }
    s->bdcalls.clear();
    return 0;
}
extern "C" int mdqt_enable_timing_kinds(mdqt_ctx* s, int on, int kinds) {
    return mdqt_enable_timing_at(s, on, kinds, on > 0 ? on / 2 : 0);
}
extern "C" int mdqt_enable_timing(mdqt_ctx* s, int on) { return mdqt_enable_timing_kinds(s, on, 3); }

extern "C" int mdqt_kernel_times(mdqt_ctx* s, double* out, int n) {
    if (!s || !out) return set_error("mdqt_kernel_times: NULL argument");
    if (n < 6) return set_error("mdqt_kernel_times: need 6 doubles");
    HIPCHK(hipSetDevice(s->dev));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (int k = 0; k < 4; ++k) {
        if (2 * k + 1 >= n) { s->timers[k].reset(); continue; }
        double v[5];
        if (s->timers[k].stats(v)) return -1;
        out[2 * k] = v[0];
        out[2 * k + 1] = v[1];
    }
    return 0;
}

extern "C" int mdqt_kernel_time_totals(mdqt_ctx* s, double* force_ms, int* nforce, double* sub_ms, int* nsub) {
    if (!s) return set_error("NULL context");
    double t[6];
    if (mdqt_kernel_times(s, t, 6)) return -1;
    if (force_ms) *force_ms = t[0];
    if (nforce) *nforce = (int)t[1];
    if (sub_ms) *sub_ms = t[2];
    if (nsub) *nsub = (int)t[3];
    return 0;
}

// the force-call breakdown (timing kind bit 3) since the last call: average ms per timed block-scheme force
// call of out[0] the preceding position all-gather (0 at world 1), [1] sort and boxes (with the first sharded
// call's balance census), [2] plan, [3] block kernel (launch to end, incl. its dispatch gap), [4] slot reduction,
// [5] tail pass (all-reduce of the per-sub-tile sums, list, exact fix), [6] reduce-scatter, [7] forces() start to
// end (= [1] + ... + [6]), out[8] the calls; resets
extern "C" int mdqt_force_breakdown(mdqt_ctx* s, double* out, int n) {
    if (!s || !out) return set_error("mdqt_force_breakdown: NULL argument");
    if (n < 9) return set_error("mdqt_force_breakdown: need 9 doubles");
    HIPCHK(hipSetDevice(s->dev));
    HIPCHK(hipStreamSynchronize(s->stream));
    double acc[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    auto ms = [](hipEvent_t a, hipEvent_t b) -> double {
        float t = 0.f;
        return (a && b && hipEventElapsedTime(&t, a, b) == hipSuccess) ? (double)t : 0.;
    };
    for (auto& c : s->bdcalls) {
        acc[0] += ms(c.ag0, c.ag1);
        for (int k = 0; k < 6; ++k) acc[1 + k] += ms(c.m[k], c.m[k + 1]);
        acc[7] += ms(c.m[0], c.m[6]);
        for (hipEvent_t e : c.m) if (e) s->bdfree.push_back(e);
        if (c.ag0) s->bdfree.push_back(c.ag0);
        if (c.ag1) s->bdfree.push_back(c.ag1);
    }
    const double nc = (double)s->bdcalls.size();
    for (int k = 0; k < 8; ++k) out[k] = nc > 0 ? acc[k] / nc : 0.;
    out[8] = nc;
    s->bdcalls.clear();
    return 0;
}
