// The host model of the Newton-3 block scheme (mdqt_n3b.hip k_pairs_n3b; its plan: mdqt_n3b_plan.hip): the
// error-bounded tail and tier radii, their measurement and enforcement, the block kernel's arguments, the ranks' block
// ranges by work, and the census queries.  Host arithmetic only; the launches are mdqt_step.cpp's.

#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "mdqt_ctx.hpp"
#include "mdqt_math.hpp"   // the pair forms' error constants

using namespace mdqt;

// force_tail_mode 1: forget what earlier calls measured (a new size or tail option).  keep_scale (new
// positions of the same system, e.g. a driver that uploads R every MD step): the statistics restart
// but the widened r_t stays — a clustered configuration does not rerun the exact pass, and warn, at
// every upload.  Callers settle pending forces first (they were measured with the old
// options: their enforcement must complete before the sums are cleared).
int mdqt::tail_reset(mdqt_ctx* s, bool keep_scale) {
    if (!keep_scale) s->tail_scale = 1.;
    s->tail_seen = 0;
    s->tail_pending = false;
    if (s->dTailSt) HIPCHK(hipMemsetAsync(s->dTailSt, 0, 16 * sizeof(unsigned long long), s->stream));
    return 0;
}

// smallest d with fl(d / L) >= 0.5 in IEEE double (the device's division is IEEE too), so that
// round(dx/L) == (dx >= T) - (dx <= -T) for |dx| < 1.25 L: the minimum image without a division
static double mic_threshold(double L) {
    double d = 0.5 * L;
    while (d > 0 && d / L >= 0.5) d = nextafter(d, 0.);
    while (d / L < 0.5) d = nextafter(d, INFINITY);
    return d;
}

void mdqt::fill_pair_consts(ForceArgs& a, double L, double lDeb, int variant) {
    a.L = L; a.lDeb = lDeb; a.Rcut = L / 2.;               // :196
    a.invlDeb = 1. / lDeb;                                  // :224
    a.micT = mic_threshold(L);
    a.micGuard = 1.25 * L;
    a.variant = variant;
}

// The error-bounded tail radius: the smallest r in (0, L/2] with (N - 1) g(r) <= eps, where
// g(r) = (1/r + 1/lDeb) exp(-r/lDeb) / r is |F| of one pair at distance r (SpeedUp:224 times r),
// decreasing in r.  A skipped tile pair's boxes are >= r_t apart, so each of its pairs is, and the
// pairs an ion loses number at most N - 1: |dF_i| <= (N - 1) g(r_t) <= eps (rigorous; the actual
// tail is far smaller — its terms have random directions).  L/2 (exact: nothing extra skipped)
// when eps = 0 or (N - 1) g(L/2) > eps.  bound = (N - 1) g(r_t) (0 when exact).
static double tail_g(double r, double lDeb) { return (1. / r + 1. / lDeb) * exp(-r / lDeb) / r; }
static double tail_radius(int N, double L, double lDeb, int k, double* bound) {
    const double Rcut = L / 2.;
    *bound = 0.;
    if (k <= 0 || N < 2) return Rcut;
    const double eps = pow(10., -k);
    const double n1 = (double)(N - 1);
    if (n1 * tail_g(Rcut, lDeb) > eps) return Rcut;
    double lo = 0., hi = Rcut;                      // n1 g(hi) <= eps < n1 g(lo)
    for (int it = 0; it < 200 && hi - lo > 1e-12 * Rcut; ++it) {
        const double m = 0.5 * (lo + hi);
        if (m > 0 && n1 * tail_g(m, lDeb) <= eps) hi = m; else lo = m;
    }
    *bound = n1 * tail_g(hi, lDeb);
    return hi;
}
// force_tail_mode 1: r_t from a model of the bound the device measures, per 16-ion sub-tile a sum over
// the dropped sub-blocks (a, b) of n_b g(sub-box gap): at density rho = N / L^3 the sub-tiles with box
// gap in [x, x + dx] hold about rho 4 pi (x + delta)^2 dx ions, delta = two sub-tile widths
// (16 / rho)^(1/3) bounding the box extents, so B(r) = rho int_r^(L/2) 4 pi (x + delta)^2 g(x) dx
// (beyond L/2 only pairs beyond the cutoff); r_t the smallest r with m s B(r) <= eps (m = kTailMargin, a
// margin for the model, s = tail_scale: 1, raised by tail_check when a configuration's measured
// sums exceeded eps), never beyond the a-priori radius (rigorous for any configuration).  The
// model only picks r_t: the kernel measures every tile's sum and k_tail_fix enforces eps.
// Memoised per context.
static double tail_model(double r, int N, double L, double lDeb) {
    const double rho = N / (L * L * L), delta = 2. * cbrt(16. / rho), hi = L / 2.;
    if (r >= hi) return 0.;
    const int n = 2000;                             // Simpson on [r, L/2]
    const double h = (hi - r) / n;
    auto f = [&](double x) { return 4. * M_PI * (x + delta) * (x + delta) * tail_g(x, lDeb); };
    double acc = f(r) + f(hi);
    for (int i = 1; i < n; ++i) acc += (i & 1 ? 4. : 2.) * f(r + i * h);
    return rho * acc * h / 3.;
}
// the model's margin: the measured per-sub-tile sums stayed at ~0.7 of the model at N = 1e6 (C4 and
// C2's parameters, uniform init()), and the exact pass enforces eps whenever a configuration exceeds
// it, so the margin only sets how rarely that pass runs
constexpr double kTailMargin = 1.25;
double mdqt::tail_radius_sum(const mdqt_ctx* s, double* bound) {
    const int N = s->N, k = s->tail_exp;
    const double L = s->L, lDeb = s->lDeb, Rcut = L / 2.;
    *bound = 0.;
    if (k <= 0 || N < 2) return Rcut;
    const double sc = s->tail_scale;
    if (s->tail_key[0] == N && s->tail_key[1] == L && s->tail_key[2] == lDeb && s->tail_key[3] == k &&
        s->tail_key[4] == sc) {
        *bound = s->tail_val[1];
        return s->tail_val[0];
    }
    const double eps = pow(10., -k);
    double r = Rcut, b = 0.;
    // only where the a-priori radius is below L/2 (N ~ 1e6): elsewhere the model would skip a sliver
    // just inside L/2 for nothing, and those sizes keep the exact cutoff
    double b0;
    const double ra = tail_radius(N, L, lDeb, k, &b0);
    if (ra < Rcut) {
        double lo = 0., hi = Rcut;
        for (int it = 0; it < 60 && hi - lo > 1e-9 * Rcut; ++it) {
            const double m = 0.5 * (lo + hi);
            if (m > 0 && kTailMargin * sc * tail_model(m, N, L, lDeb) <= eps) hi = m; else lo = m;
        }
        r = hi;
        b = tail_model(hi, N, L, lDeb);
        if (r > ra) { r = ra; b = b0; }              // the a-priori radius bounds any configuration
    }
    s->tail_key[0] = N; s->tail_key[1] = L; s->tail_key[2] = lDeb; s->tail_key[3] = k; s->tail_key[4] = sc;
    s->tail_val[0] = r; s->tail_val[1] = b;
    *bound = b;
    return r;
}
// the context's skip radius: mode 1 (measured and enforced) in spatial order at every world size
// (the per-tile sums are all-reduced, so 1 and W ranks run the same algorithm), else a priori
// — for the fast pair form only: k_tail_fix recomputes the listed tiles in that form (pair_ft<1>, the
// cutoff on dr < Rcut), so the other variants keep the a-priori radius
bool mdqt::tail_measured(const mdqt_ctx* s) { return s->tail_mode == 1 && s->sort_mode == 1 && s->force_variant == 1; }
double mdqt::skip_radius(const mdqt_ctx* s, double* bound) {
    return tail_measured(s) ? tail_radius_sum(s, bound) : tail_radius(s->N, s->L, s->lDeb, s->tail_exp, bound);
}
// force_tail_mode 1 at a host synchronisation point: if tiles exceeded eps since the last check
// (k_tail_fix summed their skipped tile pairs exactly, so those calls met eps anyway), the density
// model underestimated this configuration's tail by u = (largest measured sum) / (the model's at
// r_t): the next calls take r_t for tail_scale = max(2 tail_scale, 2^ceil(log2 u)) — capped at the
// a-priori radius — and stderr says so.  Every rank sees the same all-reduced sums, so ranks
// widen alike.
static double model_total(const mdqt_ctx* s);
int mdqt::tail_check(mdqt_ctx* s) {
    if (!s->dTailSt || !s->use_n3b || !(tail_measured(s) || form_measured(s))) return 0;
    unsigned long long h[8];
    HIPCHK(hipMemcpyAsync(h, s->dTailSt, sizeof h, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (h[2] <= s->tail_seen) return 0;
    double b0, b1;
    const double r0 = tail_radius_sum(s, &b0);
    const double raw = u64_as_double(h[1]);
    b0 = model_total(s);                            // (the tail's model bound + the tiers', force_form_mode 1)
    const double u = b0 > 0. ? raw / b0 : INFINITY;
    // a power of two: the sums' last bits (atomic order, the ranks' partial sums) cannot move it
    s->tail_scale = std::max(2. * s->tail_scale, std::isfinite(u) && u < 1e300 ? exp2(ceil(log2(u))) : 1e300);
    const double r1 = tail_radius_sum(s, &b1);
    if (s->tail_warned++ < 8)                       // (rate-limited: a few lines per context)
        fprintf(stderr, "mdqt: force error bound exceeded on %llu tile(s) so far (largest per-tile sum %.3e; the model's "
                "%.3e at r_t = %.4f): corrected by the exact pass; r_t widened to %.4f (the tiers' radii likewise)\n",
                (unsigned long long)h[2], raw, b0, r0, r1);
    s->tail_seen = h[2];
    return 0;
}

// the enforcement after a force call's tail sums are complete: list the tiles over eps, add their
// skipped pairs exactly (k_tail_fix) to `out` (F, or this rank's dense partial)
int mdqt::tail_enforce(mdqt_ctx* s, const N3BArgs& a, double* out) {
    const double eps = error_eps(s, a);
    HIPCHK(launch_tail_max(a.tailb, a.T, eps, s->dTailSt, s->dTailList, s->stream));
    HIPCHK(launch_tail_fix(a, s->dTailSt, s->dTailList, out, s->stream));
    return 0;
}

// the far radii: the smallest r with (N - 1) g(r) err(r) <= 10^-k, err the relative error of a term
// at distance r in the form (far: kFarRelErr; very far: (r/lDeb + 3) kRsqRawErr + kExp5RelErr) —
// L/2 (= never) and bound 0 when k = 0 or that r is >= L/2; bound = (N - 1) g(r) err(r)
static double far_err(double r, double lDeb, int level) {
    if (level == 5) return (r / lDeb + 3.) * (kRsq1RelErr + 0x1p-52) + kTab4RelErr;   // the mid form
    if (level == 4) return (r / lDeb) * kUfar32A + kUfar32B;   // the f32 ultra-far form
    if (level == 3) return (r / lDeb) * (kRsqRawErr + 0x1p-24) + 3. * kRsqRawErr + kExp2fRelErr;
    return level == 2 ? (r / lDeb + 3.) * kRsqRawErr + kExp5RelErr : kFarRelErr;
}
static double far_radius_l(int N, double L, double lDeb, int k, int level, double* bound, bool cutterm = true) {
    const double Rcut = L / 2.;
    *bound = 0.;
    if (k <= 0 || N < 2) return Rcut;
    const double eps = pow(10., -k), n1 = (double)(N - 1);
    // level 4 (f32) decides the cutoff on its f32 r^2 (relative error <= 6 2^-24): pairs within
    // 3 2^-24 Rcut of L/2 may land on either side, each at most g(Rcut (1 - 2^-20)) — a constant term
    // (not with force_form_mode 1, cutterm false: the plan keeps the f32 form off the cutoff)
    const double cut = level == 4 && cutterm ? n1 * tail_g(Rcut * (1. - 0x1p-20), lDeb) : 0.;
    auto b = [&](double r) { return n1 * tail_g(r, lDeb) * far_err(r, lDeb, level) + cut; };
    if (b(Rcut) > eps) return Rcut;
    double lo = 0., hi = Rcut;
    for (int it = 0; it < 200 && hi - lo > 1e-12 * Rcut; ++it) {
        const double m = 0.5 * (lo + hi);
        if (m > 0 && b(m) <= eps) hi = m; else lo = m;
    }
    *bound = b(hi);
    return hi;
}

// force_form_mode 1 (round 6): the tiers' radii from a density model of the per-sub-tile form sums the
// plan measures (k_n3b_plan), as tail_model for the tail: at density rho the sub-tiles with box gap in
// [x, x + dx] hold about rho 4 pi (x + delta)^2 dx ions, so a sub-tile's sum over a tier's sub-blocks (gap
// >= r) is about F(r) = rho int_r^hi 4 pi (x + delta)^2 g(x) err(x) dx, hi = r_t (nothing beyond it is
// evaluated).  The radius is the smallest r with m s F(r) <= 10^-k (m = kTailMargin, s = tail_scale:
// raised with r_t's when a call's sums exceeded its eps), never beyond the a-priori radius (rigorous for
// any configuration; level 4 without the cutoff term).  The model only picks the radii: the plan measures
// every tile's sum and k_tail_fix enforces the call's eps (error_eps).
// (force_sort 1 and 2 alike: 2 runs the same plan without skipping, and must give the same forms)
bool mdqt::form_measured(const mdqt_ctx* s) {
    return s->form_mode >= 1 && s->use_n3b && s->tail_mode == 1 && s->sort_mode >= 1 && s->force_variant == 1 &&
           !s->guard;
}
// a tier's eps (k > 0): 10^-k, + (force_form_mode 2, where the tail skips nothing: r_t = L/2) an equal
// share of the tail's 10^-tail_exp among the tiers with k > 0 — the per-ion total stays 10^-tail_exp + sum
// 10^-k, as where the tail is active
static double tier_eps(const mdqt_ctx* s, int k) {
    if (k <= 0) return 0.;
    double e = pow(10., -k);
    double tb;
    if (s->form_mode == 2 && form_measured(s) && s->tail_exp > 0 && tail_radius_sum(s, &tb) >= s->L / 2.) {
        const int n = (s->mid_exp > 0) + (s->far_exp > 0) + (s->vfar_exp > 0) + (s->ufar_exp > 0) * 2;
        e += pow(10., -s->tail_exp) / n;
    }
    return e;
}
static double form_model(double r, double hi, int N, double L, double lDeb, int level) {
    const double rho = N / (L * L * L), delta = 2. * cbrt(16. / rho);
    if (r >= hi) return 0.;
    const int n = 2000;                             // Simpson on [r, hi]
    const double h = (hi - r) / n;
    auto f = [&](double x) { return 4. * M_PI * (x + delta) * (x + delta) * tail_g(x, lDeb) * far_err(x, lDeb, level); };
    double acc = f(r) + f(hi);
    for (int i = 1; i < n; ++i) acc += (i & 1 ? 4. : 2.) * f(r + i * h);
    return rho * acc * h / 3.;
}
// the model radius of a tier (context-free; mdqt_tier_radius_model exports it for the CPU tests): the
// smallest r with m s F(r) <= eps (10^-k, or tier_eps) on [0, hi], hi = r_t, capped by the a-priori
// radius of 10^-k (its bound <= 10^-k <= eps); L/2 = off
static double model_tier_radius(int N, double L, double lDeb, int k, double eps, int level, double hi, double sc,
                                double* bound) {
    const double Rcut = L / 2.;
    *bound = 0.;
    if (k <= 0 || N < 2) return Rcut;
    double ba;
    const double ra = far_radius_l(N, L, lDeb, k, level, &ba, false);
    double lo = 0., up = hi;
    for (int it = 0; it < 60 && up - lo > 1e-9 * Rcut; ++it) {
        const double m = 0.5 * (lo + up);
        if (m > 0 && kTailMargin * sc * form_model(m, hi, N, L, lDeb, level) <= eps) up = m; else lo = m;
    }
    double r = up, b = form_model(up, hi, N, L, lDeb, level);
    if (r >= ra) { r = ra; b = ba; }                // the a-priori radius bounds any configuration
    if (r >= hi) { r = Rcut; b = 0.; }              // (nothing evaluated that far: the tier is off)
    *bound = b;
    return r;
}
// a tier's radius (L/2: off) and bound: a priori (force_form_mode 0) or the model's (1; memoised per context)
double mdqt::tier_radius(const mdqt_ctx* s, int k, int level, double* bound) {
    if (!form_measured(s)) return far_radius_l(s->N, s->L, s->lDeb, k, level, bound);
    *bound = 0.;
    if (k <= 0 || s->N < 2) return s->L / 2.;
    const double sc = s->tail_scale, eps = tier_eps(s, k);
    double* key = s->form_key[level];
    if (key[0] == s->N && key[1] == s->L && key[2] == s->lDeb && key[3] == eps && key[4] == s->tail_exp &&
        key[5] == sc) {
        *bound = s->form_val[level][1];
        return s->form_val[level][0];
    }
    double tb;
    const double hi = tail_radius_sum(s, &tb);      // r_t (L/2 where the tail is exact)
    double b;
    const double r = model_tier_radius(s->N, s->L, s->lDeb, k, eps, level, hi, sc, &b);
    key[0] = s->N; key[1] = s->L; key[2] = s->lDeb; key[3] = eps; key[4] = s->tail_exp; key[5] = sc;
    s->form_val[level][0] = r; s->form_val[level][1] = b;
    *bound = b;
    return r;
}
// C ABI for the CPU tests (no device needed): a tier's model radius and bound for given parameters,
// level as far_err (1 far, 2 very far, 3 ultra far, 4 ultra far in f32, 5 mid); hi = the skip radius
// the integral ends at (L/2 without a tail); apriori 1: force_form_mode 0's a-priori radius instead, 2: the
// a-priori radius without the f32 tier's cutoff term (the cap the model radius takes)
extern "C" int mdqt_tier_radius_model(int N, double L, double lDeb, int k, int level, double hi, double scale,
                                      int apriori, double* radius, double* bound) {
    if (!radius || !bound || N < 1 || !(L > 0.) || !(lDeb > 0.) || level < 1 || level > 5 || !(hi > 0.) ||
        !(scale > 0.) || apriori < 0 || apriori > 2)
        return -1;
    *radius = apriori ? far_radius_l(N, L, lDeb, k, level, bound, apriori == 1)
                      : model_tier_radius(N, L, lDeb, k, pow(10., -k), level, std::min(hi, L / 2.), scale, bound);
    return 0;
}
// the model's per-sub-tile sum at the current radii — the tail's where r_t < L/2, + the tiers' evaluated
// inside r_t (force_form_mode 1) — that tail_check compares the measured sums with
static double model_total(const mdqt_ctx* s) {
    double b = 0., t;
    const double rt = tail_radius_sum(s, &t);
    if (rt < s->L / 2.) b += t;
    if (form_measured(s)) {
        if (tier_radius(s, s->mid_exp, 5, &t) < rt) b += t;
        if (tier_radius(s, s->far_exp, 1, &t) < rt) b += t;
        if (tier_radius(s, s->vfar_exp, 2, &t) < rt) b += t;
        if (tier_radius(s, s->ufar_exp, 3, &t) < rt) b += t;
        if (tier_radius(s, s->ufar_exp, 4, &t) < rt) b += t;
    }
    return b;
}
// the eps a force call's per-sub-tile sums are held to (k_tail_max): the tail's where r_t < L/2, plus
// (force_form_mode >= 1) the eps of every tier evaluated inside r_t (tier_eps)
double mdqt::error_eps(const mdqt_ctx* s, const N3BArgs& a) {
    double e = a.Rskip < a.Rcut ? pow(10., -s->tail_exp) : 0.;
    if (a.formm) {
        if (a.Rmid < a.Rskip) e += tier_eps(s, s->mid_exp);
        if (a.Rfar < a.Rskip) e += tier_eps(s, s->far_exp);
        if (a.Rvfar < a.Rskip) e += tier_eps(s, s->vfar_exp);
        if (a.Rufar < a.Rskip) e += tier_eps(s, s->ufar_exp);
        if (a.Rufar32 < a.Rskip) e += tier_eps(s, s->ufar_exp);
    }
    return e;
}

// the tiers' radii of a force call (a.Rcut set): a priori or from the model (force_form_mode 1)
void mdqt::tier_radii(const mdqt_ctx* s, N3BArgs& a) {
    double bound;
    a.Rmid = tier_radius(s, s->mid_exp, 5, &bound);
    a.Rfar = tier_radius(s, s->far_exp, 1, &bound);
    a.Rvfar = tier_radius(s, s->vfar_exp, 2, &bound);
    a.Rufar = tier_radius(s, s->ufar_exp, 3, &bound);
    a.Rufar32 = tier_radius(s, s->ufar_exp, 4, &bound);
    a.formm = form_measured(s) ? 1 : 0;
    a.u32lim2 = (a.Rcut * (1. - 0x1p-20)) * (a.Rcut * (1. - 0x1p-20));
    // f32's normal range: 2^t for t >= -126 (r <= 126 lDeb ln2 = 87 lDeb); never beyond it
    if (a.Rufar < a.Rcut && a.Rcut > 80. * s->lDeb) a.Rufar = a.Rcut;
    if (a.Rufar >= a.Rcut) a.Rufar32 = a.Rcut;
}

// the block-pair kernels' arguments for the current positions: with force_sort, the Hilbert order,
// the sorted copy and the tile boxes are recomputed here (mdqt_sort.hip)
int mdqt::n3b_args(mdqt_ctx* s, N3BArgs& a) {
    a = s->n3b;
    ForceArgs c = force_args(s, nullptr);
    a.Rall = s->dR; a.slots = s->dSlots; a.S = s->S;
    a.L = c.L; a.lDeb = c.lDeb; a.Rcut = c.Rcut; a.invlDeb = c.invlDeb; a.micT = c.micT;
    a.micGuard = c.micGuard; a.guard = c.guard;
    a.use_sort = 0; a.Rs = nullptr; a.perm = nullptr; a.boxes = nullptr; a.subboxes = nullptr; a.plan = nullptr;
    a.tmask = nullptr; a.tmw = 0;
    a.ax1 = s->ax1_mode;
    a.pairs = s->n3b_pairs;
    double bound;
    a.Rskip = skip_radius(s, &bound);
    a.tailb = nullptr;
    tier_radii(s, a);
    a.rc2 = a.Rcut * a.Rcut;
    if (s->sort_mode) {                            // Hilbert order + tile boxes (mdqt_sort.hip)
        SortArgs o;
        o.Rall = s->dR; o.N = s->N; o.S = s->S; o.Npad = a.Npad; o.L = s->L;
        o.keys = s->dKeys; o.keys2 = s->dKeys + s->N; o.ion = s->dIon; o.perm = s->dIon + s->N;
        o.tmp = s->dSortTmp; o.tmp_bytes = s->dSortTmp.capacity(); o.Rs = s->dRs; o.boxes = s->dBoxes;
        o.subboxes = s->dSubBoxes;
        HIPCHK(launch_spatial_order(o, s->stream));
        a.use_sort = s->sort_mode; a.Rs = s->dRs; a.perm = o.perm; a.boxes = s->dBoxes; a.subboxes = s->dSubBoxes;
        // the per-sub-tile sums: where the tail skips pairs, or (force_form_mode 1) a tier is evaluated
        const bool tiers = a.formm && (a.Rmid < a.Rskip || a.Rfar < a.Rskip || a.Rvfar < a.Rskip || a.Rufar < a.Rskip);
        if ((tail_measured(s) && a.Rskip < a.Rcut) || tiers) a.tailb = s->dTail;
        // the plan (k_n3b_plan): kN3BBlock^2 tile-pair words per (P, db), then one J-step mask per (P, db)
        // and the per-J-tile masks of the block distances whose j-slots the block kernel writes (k_n3b_reduce
        // reads only those): T x ceil(nd / 64) words
        const size_t nplan = (size_t)std::max(a.Phi - a.Plo, 0) * a.nd * (kN3BBlock * kN3BBlock + 1);
        const int tmw = (a.nd + 63) / 64;
        const size_t need = nplan + (size_t)a.T * tmw;
        HIPCHK(s->dPlan.reserve(need));
        a.plan = s->dPlan;
        // (no masks for a rank without blocks: nothing would clear or fill them — ADVICE r05)
        const bool masks = s->tmask_mode && a.Phi > a.Plo;
        a.tmw = masks ? tmw : 0;
        a.tmask = masks ? (unsigned long long*)(s->dPlan + nplan) : nullptr;
    }
    return 0;
}

ForceArgs mdqt::force_args(mdqt_ctx* s, double* out) {
    ForceArgs a;
    a.Rall = s->dR;
    a.Fpart = out;
    a.N = s->N; a.S = s->S;
    a.row_lo = s->lo; a.nrows = s->nloc;
    a.nseg = s->nseg; a.seglen = s->seglen;
    fill_pair_consts(a, s->L, s->lDeb, s->force_variant);
    a.guard = s->guard ? 1 : 0;
    return a;
}

// fold pending force partials into F (consumers other than the substep kernels)
int mdqt::settle_forces(mdqt_ctx* s) {
    if (local_reduce(s)) return -1;
    if (!s->f_pending) return 0;
    HIPCHK(launch_reduce_segments(s->dFpart, s->dF, s->pend_nseg, s->nloc, s->S, 3, s->stream));
    s->f_pending = false;
    return 0;
}

// k_n3b_census for the current positions (it runs the spatial order itself), over this rank's blocks or all of
// them: its 2 kCensus class counters (extra 0), or behind them `extra` words of per-block sums (per_block) or of
// the J-step balance; h takes the class counters, or the extra words
static int run_census(mdqt_ctx* s, size_t extra, bool per_block, unsigned long long* h, const char* what,
                      bool all_blocks = false) {
    HIPCHK(hipSetDevice(s->dev));
    N3BArgs a;
    if (n3b_args(s, a)) return -1;
    if (all_blocks) { a.Plo = 0; a.Phi = a.NB; }
    DevBuf<unsigned long long> d;
    HIPCHK(d.alloc(2 * kCensus + extra));
    unsigned long long* x = extra ? d + 2 * kCensus : nullptr;
    hipError_t e = launch_n3b_census(a, d, s->stream, per_block ? x : nullptr, per_block ? nullptr : x);
    if (e == hipSuccess) e = hipMemcpyAsync(h, extra ? x : d, (extra ? extra : 2 * kCensus) * sizeof(unsigned long long),
                                            hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) return set_error("%s: %s", what, hipGetErrorString(e));
    return 0;
}

// the block kernel's work by tile-pair class for the current positions (k_n3b_census): out[0, 12)
// lane-steps, out[12, 24) distinct ion pairs — this rank's block pairs (diagnostic, outside any
// timed region: it runs the spatial order itself)
extern "C" int mdqt_force_census(mdqt_ctx* s, double* out, int n) {
    if (!s || !out) return set_error("mdqt_force_census: NULL argument");
    if (n < 2 * kCensus) return set_error("mdqt_force_census: need %d doubles", 2 * kCensus);
    if (!s->use_n3b || !s->sort_mode) return set_error("mdqt_force_census: Newton-3 blocks in spatial order only");
    unsigned long long h[2 * kCensus];
    if (run_census(s, 0, false, h, "mdqt_force_census")) return -1;
    for (int k = 0; k < 2 * kCensus; ++k) out[k] = (double)h[k];
    return 0;
}

// the lock-step J loop's balance over a workgroup's 8 waves for the current positions (k_n3b_census, bal):
// out[0] the estimated VALU instructions of all tile pairs, out[1] the sum over J steps of 8 x the busiest
// wave's, out[2] the J steps with work — out[1] / out[0] is the excess of max over mean (diagnostic)
extern "C" int mdqt_force_jstep_balance(mdqt_ctx* s, double* out, int n) {
    if (!s || !out) return set_error("mdqt_force_jstep_balance: NULL argument");
    if (n < 3) return set_error("mdqt_force_jstep_balance: need 3 doubles");
    // (out[3..5] when n >= 6: 8 x the J-step pairs' best two-sub-step schedule, 8 x the same pairs in
    // lock-step, 8 x the per-(P, db) busiest wave's 8-step sum — see k_n3b_census)
    if (!s->use_n3b || !s->sort_mode) return set_error("mdqt_force_jstep_balance: Newton-3 blocks in spatial order only");
    unsigned long long h[11];
    if (run_census(s, 11, false, h, "mdqt_force_jstep_balance")) return -1;
    out[0] = (double)h[0]; out[1] = 8. * (double)h[1]; out[2] = (double)h[2];
    if (n >= 6) { out[3] = 8. * (double)h[3]; out[4] = 8. * (double)h[4]; out[5] = 8. * (double)h[5]; }
    // (out[6..8] when n >= 9: 4 waves on two I tiles each — heavy-light pairing, (q, 7 - q), (q, q + 4) —
    // 4 x the sum over J steps of the busiest wave's pair)
    if (n >= 9) { out[6] = 4. * (double)h[6]; out[7] = 4. * (double)h[7]; out[8] = 4. * (double)h[8]; }
    if (n >= 10) out[9] = 4. * (double)h[9];       // each J step paired heavy-light on its own
    if (n >= 11) out[10] = 4. * (double)h[10];     // the best of the 105 pairings per (P, db)
    return 0;
}

// the block kernel's evaluated lane-steps per block of this rank for the current positions (k_n3b_census's
// per-block sums): out[P - Plo], P = Plo .. Phi - 1 (*nblocks = Phi - Plo) — what each block's workgroups
// do; at world 1 every block, so the work of any rank partition follows
extern "C" int mdqt_force_block_work(mdqt_ctx* s, double* out, int n, int* nblocks) {
    if (!s || !out || !nblocks) return set_error("mdqt_force_block_work: NULL argument");
    if (!s->use_n3b || !s->sort_mode) return set_error("mdqt_force_block_work: Newton-3 blocks in spatial order only");
    const int nb = std::max(s->n3b.Phi - s->n3b.Plo, 0);
    *nblocks = nb;
    if (n < nb) return set_error("mdqt_force_block_work: need %d doubles", nb);
    if (nb == 0) return 0;
    std::vector<unsigned long long> h((size_t)nb);
    if (run_census(s, (size_t)nb, true, h.data(), "mdqt_force_block_work")) return -1;
    for (int k = 0; k < nb; ++k) out[k] = (double)h[k];
    return 0;
}

// Sharded Newton-3 blocks: the ranks' block ranges by work.  The blocks' evaluated
// lane-steps vary several-fold along the Hilbert order (N = 1M: 0.49 .. 1.52 of the mean), and equal
// block counts left world 8 at 1.13 x the mean work on its busiest rank (world 2 and 4: 1.002;
// profiles/r05a_load_balance.json).  Once per size, at the first sharded force call (positions
// gathered): the census of EVERY block (k_n3b_census; integer counts, so every rank computes the same
// numbers from the same positions), then rank r takes the blocks [c_r, c_r+1) whose prefix work is
// nearest r / W of the total.  Any partition covers every block pair exactly once (the ownership is by
// P alone; tests/test_n3b_protocol.py); only the partial sums' order changes with it.
int mdqt::n3b_balance(mdqt_ctx* s) {
    const int W = s->p.world_size;
    if (s->balanced || W == 1 || !s->use_n3b || !s->sort_mode) return 0;
    s->balanced = true;
    N3BArgs& b = s->n3b;
    const int NB = b.NB;
    if (NB < W) return 0;
    std::vector<unsigned long long> w((size_t)NB);  // (with the spatial order and boxes of these positions)
    if (run_census(s, (size_t)NB, true, w.data(), "force balance census", true)) return -1;
    std::vector<double> pre((size_t)NB + 1, 0.);
    for (int k = 0; k < NB; ++k) pre[k + 1] = pre[k] + (double)w[k];
    const double tot = pre[NB];
    std::vector<int> cut((size_t)W + 1, 0);
    cut[W] = NB;
    for (int r = 1; r < W; ++r) {
        const double t = tot * r / W;
        int k = (int)(std::lower_bound(pre.begin(), pre.end(), t) - pre.begin());   // pre[k] >= t
        if (k > 0 && t - pre[k - 1] < pre[k] - t) --k;                             // the nearer boundary
        cut[r] = std::min(std::max(k, cut[r - 1] + 1), NB - (W - r));               // >= 1 block per rank
    }
    auto ratio = [&](const std::vector<int>& c) {
        double mx = 0.;
        for (int r = 0; r < W; ++r) mx = std::max(mx, pre[c[r + 1]] - pre[c[r]]);
        return tot > 0. ? mx / (tot / W) : 1.;
    };
    std::vector<int> eq((size_t)W + 1);
    for (int r = 0; r <= W; ++r) eq[r] = (int)((long)r * NB / W);
    s->balance_ratio_eq = ratio(eq);
    if (s->balance_opt) {
        s->balance_ratio = ratio(cut);
        n3b_set_range(b, cut[s->p.rank], cut[s->p.rank + 1]);
        if (ensure_aux(s)) return -1;               // (the runs, hence the i-slots, follow the range)
    } else {
        s->balance_ratio = s->balance_ratio_eq;
    }
    return 0;
}
