// Host engine of the MI355X MDQT path: the C ABI of include/mdqt.h.
//
// The engine owns the device-resident state of one simulation (or one rank's slab of it), builds the
// reference's derived constants and QT operators, drives the gfx950 kernels of
// mdqt_kernels.hip on one HIP stream, and reproduces the reference program's control flow
// (main() time loop), initial conditions and text files.  Every function cites the lines of
// laserCoolingPlusExpansionMDQTSpeedUp.cpp ("SpeedUp") it stands in for.
//
// This file: parameters, constants and QT tables, sizing and allocation, create / destroy, state transfer
// and init().  The rest of the engine by file: DESIGN.md §1; the context itself: mdqt_ctx.hpp.

#include <math.h>
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <thread>

#include "mdqt_ctx.hpp"
#include "mdqt_init_sample.hpp"

using namespace mdqt;

namespace {

thread_local std::string g_err;

struct cx { double re, im; };
inline cx cx_make(double r, double i) { return {r, i}; }
inline cx cx_mul(cx a, cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline cx cx_add(cx a, cx b) { return {a.re + b.re, a.im + b.im}; }
inline cx cx_sub(cx a, cx b) { return {a.re - b.re, a.im - b.im}; }
inline cx cx_conj(cx a) { return {a.re, -a.im}; }

// glibc drand48 (SpeedUp:303-333, srand48 :1219): mdqt_init_sample.hpp

}  // namespace

// ---------------------------------------------------------------------------------------------
// parameters and constants
// ---------------------------------------------------------------------------------------------

extern "C" void mdqt_default_params(mdqt_params* p) {
    memset(p, 0, sizeof(*p));
    p->Ge = 0.1; p->tmax = 30; p->density = 2; p->sig0 = 4.0; p->Te = 19.0; p->fracOfSig = 0;   // :60-68
    p->detuning = -1; p->detuningDP = 1; p->Om = 1; p->OmDP = 1;                               // :70-73
    p->N0 = 3500; p->newRun = 1; p->c0 = 0; p->sampleFreq = 40; p->reNormalizewvFns = 0;       // :61-78
    p->qt_enabled = 1; p->rng_mode = 1; p->seed = 12345; p->job = 1;
    p->device = -1; p->world_size = 1; p->rank = 0; p->force_segments = 0; p->qt_model = 0;
    strcpy(p->saveDirectory, "dataLaserCool/");                                              // :56
    p->tpumpreal = 0.0000002; p->tstartV0 = 15;           // randomFrozenStartTag408Linear.cpp:58, :78
}

// The optical-pumping programs' compile-time globals (randomFrozenStartTag408Linear.cpp:52-80,
// randomFrozenStartTag408Quad.cpp:55-81, randomFrozenStartTag422Linear.cpp:52-78): N0 3500,
// Ge 0.1, density 2, sampleFreq 40, tmax 25, tstartV0 15 in all three; per program the pump
// detuning, Rabi frequency, pump time and directory.
extern "C" void mdqt_default_params_pump(mdqt_params* p, int qt_model) {
    mdqt_default_params(p);
    p->qt_model = qt_model;
    p->tmax = 25; p->Ge = 0.1; p->density = 2; p->N0 = 3500; p->sampleFreq = 40; p->tstartV0 = 15;
    if (qt_model == 2) {
        p->detuning = 0; p->Om = 2; p->tpumpreal = 0.0000001; strcpy(p->saveDirectory, "data/");
    } else if (qt_model == 3) {
        p->detuning = -1; p->Om = 1.3; p->tpumpreal = 0.0000001; strcpy(p->saveDirectory, "data422/");
    } else {
        p->detuning = -2.5; p->Om = 0.7; p->tpumpreal = 0.0000002; strcpy(p->saveDirectory, "data408/");
    }
}

extern "C" const char* mdqt_last_error(void) { return g_err.c_str(); }

extern "C" long long mdqt_live_bytes(int space) {
    return space == 0 ? DeviceSpace::live.load() : space == 1 ? PinnedSpace::live.load() : -1;
}

namespace mdqt {
int set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}
}  // namespace mdqt
extern "C" const char* mdqt_version(void) { return "mdqt-mi355x 0.1 (gfx950)"; }

extern "C" int mdqt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// FastTab of the optical-pumping models (qt_model 1..3).  Decay channels cs[j] = |a><b| with
// weights gs[j] (randomFrozenStartTag408Linear.cpp main :1000-1019; ...422Linear.cpp main):
// decayMatrix_bb = sum_j gs[j] over the channels leaving b, hamDecayTerm = -i/2 decayMatrix;
// H = detunings on the P levels (-det -/+ v_q, :439) + S-P couplings -Om/2 sqrt(gs[x]) |a><b|
// + h.c. (:438); M = I - i h H.  No optical kick, no time-dependent coupling.
static void build_pump_tables(const mdqt_params* p, QTConst& q, FastTab& f) {
    const double r = q.r, h = q.h;                             // decayRatio (408: 0.0617 :118; 422: 0.0754 :116)
    // channel j = |a_j><b_j|: 408 a = {0,0,0,1,1,1,6,6,6,6}, 422 a = {1,1,0,0,4,4}; only b enters D
    static const int B408[10] = {2, 3, 4, 3, 4, 5, 2, 3, 4, 5};
    const double G408[10] = {1, 2. / 3, 1. / 3, 1. / 3, 2. / 3, 1, r, r, r, r};
    static const int B422[6] = {2, 3, 3, 2, 2, 3};
    const double G422[6] = {2. / 3, 1. / 3, 2. / 3, 1. / 3, r, r};
    const int m = p->qt_model;
    const int nch = m == 3 ? 6 : 10;
    double D[NS] = {0.};
    for (int j = 0; j < nch; ++j) {
        const int b = m == 3 ? B422[j] : B408[j];
        D[b] += m == 3 ? G422[j] : G408[j];
    }
    // couplings (row, col, sqrt(gs) factor): |a><b| and its conjugate
    struct Cp { int a, b; double g; };
    Cp cp[4];
    int ncp = 0;
    if (m == 1) { cp[0] = {1, 3, G408[3]}; cp[1] = {1, 5, G408[5]}; cp[2] = {0, 2, G408[0]}; cp[3] = {0, 4, G408[2]}; ncp = 4; }
    if (m == 2) { cp[0] = {1, 5, G408[5]}; cp[1] = {0, 4, G408[2]}; ncp = 2; }
    if (m == 3) { cp[0] = {1, 2, G422[0]}; cp[1] = {0, 3, G422[2]}; ncp = 2; }
    memset(&f, 0, sizeof f);
    for (int k = 0; k < 16; ++k)
        for (int j = 0; j < 3; ++j) f.col[j][k] = k < NS ? kFastColM[m][k][j] : k;
    const int nst = kModelStates[m];
    const int nP = m == 3 ? 2 : 4;
    for (int k = 0; k < nst; ++k) {
        f.mre[k] = 1. + h * (-0.5 * D[k]);
        f.hdp[k] = h * D[k];
        double e1 = 0.;
        if (k >= 2 && k < 2 + nP) e1 = (k < 2 + nP / 2) ? -1. : 1.;   // right (-v) / left (+v) P levels
        const double e0 = (k >= 2 && k < 2 + nP) ? -p->detuning : 0.;
        f.mi0[k] = -(h * e0);
        f.mi1[k] = -(h * e1);
    }
    for (int c = 0; c < ncp; ++c) {
        const double v = (-p->Om / 2) * sqrt(cp[c].g);      // H_ab = H_ba = v; M = -i h v
        const int rc[2][2] = {{cp[c].a, cp[c].b}, {cp[c].b, cp[c].a}};
        for (const auto& e : rc)
            for (int j = 0; j < 3; ++j)
                if (kFastColM[m][e[0]][j] == e[1]) { f.cre[j][e[0]] = 0.; f.cim[j][e[0]] = -(h * v); }
    }
    f.cphi = 0.;
    q.kickS = q.kickD = 0.;
    q.vKick = q.vKickDP = 0.;
}

static void build_constants(mdqt_ctx* s) {
    const mdqt_params* p = &s->p;
    // SpeedUp :79-85, :146; the pumping programs' own constants: 408 nm
    // (randomFrozenStartTag408Linear.cpp:67-75, :118; 408Quad :69-77, :121: round, not ceil) and
    // 422 nm (randomFrozenStartTag422Linear.cpp:66-74, :116: gamma ratio .894, velocity .967, D/S 0.0754)
    const int m = p->qt_model;
    s->gamToE = m == 3 ? 174.07 * .894 / sqrt(p->density) : 174.07 / sqrt(p->density);
    s->ratio = m == 0   ? (int)ceil(34.81 / sqrt(p->density))
               : m == 3 ? (int)round(34.81 * .894 / sqrt(p->density))
                        : (int)round(34.81 / sqrt(p->density));
    s->dtQ = TIMESTEP / s->ratio;
    s->pv2q = m == 3 ? 1.1821 * pow(p->density, 1. / 6) * .967 : 1.1821 * pow(p->density, 1. / 6);
    s->r = m == 3 ? 0.0754 : 0.0617;
    s->kRat = 0.395;                                            // :147
    s->vKick = 0.001208 / s->pv2q;                              // :148
    s->vKickDP = s->vKick * s->kRat;                            // :149
    s->lDeb = 1. / sqrt(3. * p->Ge);                            // :295
    s->L = pow(p->N0 * 4. * M_PI / 3., 0.333333333);            // :297
    const double r = s->r;
    double* gs = s->gs;                                         // :1181-1198
    gs[0] = sqrt(1.); gs[1] = sqrt(2. / 3); gs[2] = sqrt(1. / 3); gs[3] = sqrt(2. / 3);
    gs[4] = sqrt(1. / 3); gs[5] = sqrt(1.);
    gs[6] = sqrt(r * 2. / 3); gs[7] = sqrt(r * 4. / 15); gs[8] = sqrt(r * 1. / 15);
    gs[9] = sqrt(r * 2. / 5); gs[10] = sqrt(r * 2. / 5); gs[11] = sqrt(r * 1. / 5);
    gs[12] = sqrt(r * 1. / 5); gs[13] = sqrt(r * 2. / 5); gs[14] = sqrt(r * 2. / 5);
    gs[15] = sqrt(r * 1. / 15); gs[16] = sqrt(r * 4. / 15); gs[17] = sqrt(r * 2. / 3);
    // cs[k] = |a><b| (0-based), :1163-1180
    static const int A[18] = {1, 1, 0, 0, 1, 0, 6, 7, 8, 7, 8, 9, 8, 9, 10, 9, 10, 11};
    static const int B[18] = {2, 3, 3, 4, 4, 5, 5, 5, 5, 4, 4, 4, 3, 3, 3, 2, 2, 2};
    cx decay[NS][NS], hamDecay[NS][NS], ham[NS][NS];
    memset(decay, 0, sizeof decay); memset(hamDecay, 0, sizeof hamDecay); memset(ham, 0, sizeof ham);
    for (int j = 0; j < 18; ++j) {                              // :1201-1204
        const int b = B[j];
        const double g2 = gs[j] * gs[j];
        hamDecay[b][b] = cx_sub(hamDecay[b][b], cx_make(0., 0.5 * g2));
        decay[b][b] = cx_add(decay[b][b], cx_make(g2, 0.));
    }
    for (int k = 0; k < 6; ++k)                                 // :1206-1210
        if (k != 1 && k != 3) {
            const double v = ((-1. * gs[k]) * p->Om) / 2;
            ham[B[k]][A[k]] = cx_add(ham[B[k]][A[k]], cx_make(v, 0.));
        }
    for (int k = 6; k < 18; ++k)                                // :1211-1215
        if (k != 8 && k != 11 && k != 7 && k != 10 && k != 13 && k != 16) {
            const double v = (((-1. * gs[k]) * p->OmDP) / 2) / sqrt(r);
            ham[B[k]][A[k]] = cx_add(ham[B[k]][A[k]], cx_make(v, 0.));
        }
    QTConst& q = s->qc;
    memset(&q, 0, sizeof q);
    q.dtQ = s->dtQ; q.gamToE = s->gamToE;
    q.h = s->dtQ * s->gamToE;                                   // :526, :530
    q.dtHalf = s->dtQ * s->gamToE / 2;                          // :525
    q.invh = 1. / (s->dtQ * s->gamToE);                         // :532
    q.pv2q = s->pv2q; q.kRat = s->kRat; q.r = r;
    q.det = p->detuning; q.detDP = p->detuningDP;
    q.kickS = 1 * s->vKick * p->Om;                             // :503
    q.kickD = s->vKickDP * (p->OmDP / r);
    q.vKick = s->vKick; q.vKickDP = s->vKickDP;
    q.pD = r / (r + 1);                                         // :589
    for (int k = 0; k < 4; ++k) {
        q.dP[k] = decay[2 + k][2 + k].re;
        q.hdP[k] = hamDecay[2 + k][2 + k].im;
    }
    q.a8 = ((p->OmDP / 2) * gs[8]) / sqrt(r);                   // :508
    q.a11 = ((p->OmDP / 2) * gs[11]) / sqrt(r);
    // static off-diagonal M = I - i h H entries, built exactly as the dense algebra does
    const cx sI = cx_make(0., s->dtQ * s->gamToE);
    for (int e = 0; e < NSTATIC; ++e) {
        const int a = kStaticRC[e][0], b = kStaticRC[e][1];
        cx h = cx_add(cx_add(cx_make(0., 0.), ham[a][b]), cx_conj(ham[b][a]));
        cx hamil = cx_add(h, hamDecay[a][b]);
        cx M = cx_sub(cx_make(0., 0.), cx_mul(sI, hamil));
        q.Mre[e] = M.re; q.Mim[e] = M.im;
    }
    q.thS3 = gs[2] * gs[2];                                     // :637-643
    q.thS4 = gs[4] * gs[4];                                     // :652-658
    q.thD[0][0] = gs[17] * gs[17] / r; q.thD[0][1] = gs[17] * gs[17] / r + gs[16] * gs[16] / r;   // :612-632
    q.thD[1][0] = gs[14] * gs[14] / r; q.thD[1][1] = gs[14] * gs[14] / r + gs[13] * gs[13] / r;   // :644-650
    q.thD[2][0] = gs[11] * gs[11] / r; q.thD[2][1] = gs[11] * gs[11] / r + gs[10] * gs[10] / r;   // :659-665
    q.thD[3][0] = gs[8] * gs[8] / r;   q.thD[3][1] = gs[8] * gs[8] / r + gs[7] * gs[7] / r;       // :675-697
    for (int k = 0; k < 18; ++k) q.gs[k] = gs[k];
    q.renorm = p->reNormalizewvFns;
    q.model = p->qt_model;
    q.seed = p->seed; q.job = p->job;
    for (int i = 0; i < NBINS; ++i) s->vel[i] = (double)i * 0.0025;   // :340-344
    // lane tables of the lane-per-state kernel: row k of M, slots A < B < C by column
    LaneTab& t = s->tab;
    memset(&t, 0, sizeof t);
    static const int cols[NS][3] = {{3, 5, -1}, {2, 4, -1}, {1, 9, 11}, {0, 8, 10}, {1, 7, 9}, {0, 6, 8},
                                    {5, -1, -1}, {4, -1, -1}, {3, 5, -1}, {2, 4, -1}, {3, -1, -1}, {2, -1, -1}};
    static const int order[NS] = {0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 2, 2};
    auto static_idx = [](int r, int c) {
        for (int e = 0; e < NSTATIC; ++e)
            if (kStaticRC[e][0] == r && kStaticRC[e][1] == c) return e;
        return -1;
    };
    for (int k = 0; k < 16; ++k) {
        t.colA[k] = t.colB[k] = t.colC[k] = 0;
        t.order[k] = 2;
    }
    for (int k = 0; k < NS; ++k) {
        t.order[k] = order[k];
        int* slot[3] = {&t.colA[k], &t.colB[k], &t.colC[k]};
        double* cre[3] = {&t.cAre[k], &t.cBre[k], &t.cCre[k]};
        double* cim[3] = {&t.cAim[k], &t.cBim[k], &t.cCim[k]};
        for (int j = 0; j < 3; ++j) {
            const int c = cols[k][j];
            if (c < 0) continue;
            *slot[j] = c;
            const int e = static_idx(k, c);
            if (e >= 0) { *cre[j] = q.Mre[e]; *cim[j] = q.Mim[e]; }
        }
        t.hasB[k] = cols[k][1] >= 0;
        t.hasC[k] = cols[k][2] >= 0;
        if (k >= 2 && k < 6) { t.dP[k] = q.dP[k - 2]; t.hd[k] = q.hdP[k - 2]; }
    }
    t.dynC[4] = 1; t.dynScale[4] = q.a11;      // M49
    t.dynC[5] = 1; t.dynScale[5] = q.a8;       // M58
    t.dynB[8] = 1; t.dynScale[8] = q.a8;       // M85
    t.dynB[9] = 1; t.dynScale[9] = q.a11;      // M94
    // kick weights: lane k multiplies rho_im(w_k, w_colA) by gA, rho_im(w_k, w_colB) by gB (:503)
    t.gA[1] = gs[0]; t.gA[0] = gs[2]; t.gB[1] = gs[4]; t.gB[0] = gs[5];
    t.gB[8] = gs[8]; t.gB[9] = gs[11]; t.gA[10] = gs[14]; t.gA[11] = gs[17];
    t.gA[6] = gs[6]; t.gA[7] = gs[9]; t.gA[8] = gs[12]; t.gA[9] = gs[15];
    // qt_math 2 tables (mdqt_qtfast.hip): slots of kFastCol, constants folded
    FastTab& f = s->ftab;
    memset(&f, 0, sizeof f);
    const double h = q.h;
    for (int k = 0; k < 16; ++k)
        for (int j = 0; j < 3; ++j) f.col[j][k] = k < NS ? kFastCol[k][j] : k;
    for (int k = 0; k < NS; ++k) {
        for (int j = 0; j < 3; ++j) {
            const int c = kFastCol[k][j];
            if (c == k || c >= NS) continue;       // unused slot
            const int e = static_idx(k, c);
            if (e >= 0) { f.cre[j][k] = q.Mre[e]; f.cim[j][k] = q.Mim[e]; }
        }
        const bool P = k >= 2 && k < 6;
        f.mre[k] = P ? 1. + h * q.hdP[k - 2] : 1.;
        f.hdp[k] = P ? h * q.dP[k - 2] : 0.;
        // E_k = e0 + e1 u (:506-510); Im M_kk = -h E_k
        double e0 = 0., e1 = 0.;
        if (k >= 2) e0 = (k < 6) ? -q.det : -q.det + q.detDP;
        if (k == 2 || k == 3) e1 = -1.;
        else if (k == 4 || k == 5) e1 = 1.;
        else if (k == 6 || k == 7) e1 = 1. - q.kRat;
        else if (k == 8 || k == 9) e1 = -(1. + q.kRat);
        else if (k >= 10) e1 = q.kRat - 1.;
        f.mi0[k] = -(h * e0);
        f.mi1[k] = -(h * e1);
    }
    // time-dependent slot 2: M85, M94 = h a {-sin, cos}; M58, M49 = h a {sin, cos} (:508)
    f.dms[8] = -(h * q.a8);  f.dmc[8] = h * q.a8;
    f.dms[9] = -(h * q.a11); f.dmc[9] = h * q.a11;
    f.dms[5] = h * q.a8;     f.dmc[5] = h * q.a8;
    f.dms[4] = h * q.a11;    f.dmc[4] = h * q.a11;
    // kick weights of Im(w_k conj(w_c)) (:503), scale kickS/kickD * dtQ * gamToE folded in
    const double kS = q.kickS * q.dtQ * q.gamToE, kD = q.kickD * q.dtQ * q.gamToE;
    struct KW { int row, col, g; double sgn, scale; };
    const KW kws[12] = {{1, 2, 0, 1., kS},  {0, 3, 2, 1., kS},  {1, 4, 4, -1., kS}, {0, 5, 5, -1., kS},
                        {8, 5, 8, 1., kD},  {9, 4, 11, 1., kD}, {10, 3, 14, 1., kD}, {11, 2, 17, 1., kD},
                        {6, 5, 6, -1., kD}, {7, 4, 9, -1., kD}, {8, 3, 12, -1., kD}, {9, 2, 15, -1., kD}};
    // Every coupling edge has exactly one P endpoint (S-P and P-D edges; each P level has three),
    // so each term sits on its P state's lane: Im(w_a conj(w_P)) = -Im(w_P conj(w_a)).  The kick
    // is then the sum over the four P lanes — the same broadcast pattern as dp, not a 16-lane tree.
    for (const KW& w : kws)
        for (int j = 0; j < 3; ++j)
            if (kFastCol[w.col][j] == w.row) f.kw[j][w.col] = -(w.sgn * (w.scale * gs[w.g]));
    f.cphi = 2. * (1. + q.kRat) * q.gamToE;
    if (p->qt_model != 0) build_pump_tables(p, q, f);
    f.dt2 = (0.5 * q.dtQ) * (0.5 * q.dtQ);
    for (int k = 0; k < 4; ++k) q.hdPh[k] = f.hdp[2 + k];
    // the lane-indexed copy: model 0 moves state kStateOfLane0[l] to lane l (its slots are DPP
    // moves, col unused: self); the pumping models keep lane = state
    FastTab& fl = s->ftabL;
    fl = f;
    // one substep's kick is the recoil (vKick or vKickDP) or the optical kick sum_j kw_j Im(w conj(w_j))
    // over the P lanes, |w| |w_j| <= 16 taken generously
    {
        double kw = 0.;
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 16; ++k) kw += fabs(f.kw[j][k]);
        q.kickmax = fmax(fabs(q.vKick), fabs(q.vKickDP)) + 16. * kw;
    }
    q.im01 = 1;                                        // slots 0 and 1 purely imaginary (checked)
    for (int k = 0; k < 16; ++k)
        if (f.cre[0][k] != 0. || f.cre[1][k] != 0.) q.im01 = 0;
    if (p->qt_model == 0) {
        memset(&fl, 0, sizeof fl);
        fl.cphi = f.cphi; fl.dt2 = f.dt2;
        for (int l = 0; l < 16; ++l) {
            for (int j = 0; j < 3; ++j) fl.col[j][l] = l;
            const int k = state_of_lane0(l);
            if (k >= NS) continue;
            for (int j = 0; j < 3; ++j) {
                fl.cre[j][l] = f.cre[j][k]; fl.cim[j][l] = f.cim[j][k]; fl.kw[j][l] = f.kw[j][k];
            }
            fl.dms[l] = f.dms[k]; fl.dmc[l] = f.dmc[k]; fl.mre[l] = f.mre[k];
            fl.mi0[l] = f.mi0[k]; fl.mi1[l] = f.mi1[k]; fl.hdp[l] = f.hdp[k];
        }
    }
}

// QT constants and FastTab of a pumping model driven by another engine (the MC + MD tagging
// programs, include/mdmc.h): the model's couplings, decay and jump rule (build_pump_tables)
// with the caller's quantum time step, gamma and velocity conversion
namespace mdqt {
void build_pump_program(int model, double detuning, double Om, double dtQ, double gamToE, double pv2q,
                        double decayRatio, uint32_t seed, uint32_t job, QTConst& q, FastTab& f) {
    memset(&q, 0, sizeof q);
    q.dtQ = dtQ; q.gamToE = gamToE;
    q.h = dtQ * gamToE;
    q.dtHalf = dtQ * gamToE / 2;
    q.invh = 1. / (dtQ * gamToE);
    q.pv2q = pv2q; q.r = decayRatio;
    q.pD = decayRatio / (decayRatio + 1);
    q.det = detuning;
    q.model = model; q.seed = seed; q.job = job; q.renorm = 0;
    mdqt_params p;
    memset(&p, 0, sizeof p);
    p.qt_model = model; p.detuning = detuning; p.Om = Om;
    build_pump_tables(&p, q, f);
    f.dt2 = (0.5 * dtQ) * (0.5 * dtQ);
    for (int k = 0; k < 4; ++k) q.hdPh[k] = f.hdp[2 + k];
}
}  // namespace mdqt

// ---------------------------------------------------------------------------------------------
// sizing and allocation
// ---------------------------------------------------------------------------------------------

extern "C" int mdqt_slab(int N, int world, int rank, int* lo, int* hi, int* S) {
    if (N < 0 || world < 1 || rank < 0 || rank >= world) return set_error("mdqt_slab: bad arguments");
    int s = (N + world - 1) / world;
    s = ((s + 63) / 64) * 64;
    if (s == 0) s = 64;
    int l = rank * s; if (l > N) l = N;
    int h = (rank + 1) * s; if (h > N) h = N;
    if (lo) *lo = l;
    if (hi) *hi = h;
    if (S) *S = s;
    return 0;
}

// this rank's blocks [lo, hi) of the Newton-3 block kernel and its runs: up to 65,536 workgroups per rank
// (runs of one or a few block distances, dispatched run-major: a short last round; A/B with 8-tile
// blocks: N = 1M -1.2 % vs 16,384, C3 and C5 flat)
void mdqt::n3b_set_range(N3BArgs& b, int lo, int hi) {
    b.Plo = lo;
    b.Phi = hi;
    const int nblk = std::max(b.Phi - b.Plo, 1);
    constexpr int wg_target = 65536;                // workgroups per rank
    int R = std::min(b.nd, (wg_target + nblk - 1) / nblk);
    b.runlen = (b.nd + R - 1) / R;
    b.R = (b.nd + b.runlen - 1) / b.runlen;
}

// j segmentation of the force sum: a function of N only (partition invariance across world
// sizes); enough (row x segment) threads to fill 256 CUs at small N, segments >= 64 ions.
void mdqt::choose_segments(mdqt_ctx* s) {
    const int N = s->N;
    int nseg = s->p.force_segments;
    if (nseg <= 0) {
        const long target = 1L << 20;
        long a = (target + N - 1) / (N > 0 ? N : 1);
        long b = N / 64;
        nseg = (int)(a < b ? a : b);
        if (nseg < 1) nseg = 1;
    }
    if (nseg > N && N > 0) nseg = N;
    if (nseg < 1) nseg = 1;
    s->seglen = N > 0 ? (N + nseg - 1) / nseg : 1;
    s->nseg = N > 0 ? (N + s->seglen - 1) / s->seglen : 1;
    // Newton-3 tile pairs (one GPU, ntiles slots of 3 x S) up to 64k ions; above that Newton-3
    // block pairs (O(N^2/1024) slots, one GPU or sharded with a reduce-scatter); owner-computes
    // rows for small sharded systems (bit-identical across world sizes)
    const int W = s->p.world_size;
    int sch = s->scheme_opt;
    if (sch == 0) {
        if (W == 1) sch = N > 65536 ? 3 : (N >= 128 ? 2 : 1);
        else sch = N > 65536 ? 3 : 1;
    }
    s->use_n3 = sch == 2 && W == 1 && N >= 1;
    s->use_n3b = sch == 3 && N >= 1;
    const int nt = (N + 63) / 64;
    s->nslots = s->use_n3 ? nt : 0;
    s->npairs = s->use_n3 ? nt * (nt + 1) / 2 : 0;
    N3BArgs& b = s->n3b;
    memset(&b, 0, sizeof b);
    if (s->use_n3b) {
        b.N = N; b.T = nt; b.Npad = nt * 64;
        b.NB = (nt + kN3BBlock - 1) / kN3BBlock;
        b.nd = b.NB / 2 + 1;
        n3b_set_range(b, (int)((long)s->p.rank * b.NB / W), (int)((long)(s->p.rank + 1) * b.NB / W));
        s->balanced = false;
    }
}

// partial-sum buffer (row segments or Newton-3 slots) and the tile-pair table
// The tile kernel's last round of workgroups (C2: 1,596 on 256 CUs, 6 per CU and 60 more) decides
// its end: the 56 diagonal tile pairs (half the steps) go last already (the table below), and the
// split table also runs the 4 full tile pairs that remain in that round as two half workgroups each
// (the first / second 8 of every wave's 16 rotation steps) — 64 half-work workgroups in the last
// round instead of 56 + 4 whole ones, so no CU runs 7 whole tile pairs.  The second halves write
// their rows into one extra slot (ntiles; the split pairs have disjoint tiles, (0, 1), (2, 3), ...,
// and every other row of that slot stays 0), so F = the sum of ntiles + 1 slots.  The overlapped and
// fused MD steps (tile arrival counts) keep the plain table.
// Option 2 (quarters) runs those tile pairs in four parts and every diagonal tile in two: the last
// round is then 4 k + 2 nt quarter-size workgroups (C2: 128), so its CUs carry 6.25 tile pairs of work
// instead of 6.5 (measured: the same launch time as halves, profiles/r05n_tile_split_quarters_ab.txt).
// Extra slots: halves ntiles; quarters ntiles + 0 .. 2 (parts 1-3) and ntiles + 3 (diagonal halves).
int mdqt::split_slots(const mdqt_ctx* s) { return s->nsplit > 0 ? (s->split_opt == 2 ? 4 : 1) : 0; }
static int tile_split_count(const mdqt_ctx* s, int nt) {
    if (!s->split_opt || nt < 2) return 0;
    // the table (hence the summation order of the split tiles' forces, F's last bits) follows the CU count:
    // force_split_cus fixes it, so that devices with different counts give the same bits
    int ncu = s->split_cus;
    if (ncu <= 0 && (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->dev) != hipSuccess || ncu <= 0))
        return 0;
    const long w0 = (long)nt * (nt + 1) / 2;
    if (w0 <= ncu || w0 > 8L * ncu) return 0;    // one round (nothing to balance) / many (dispatched as CUs free up)
    const int k = (int)(w0 % ncu) - nt;          // whole tile pairs in the last round
    const int last = s->split_opt == 2 ? 4 * k + 2 * nt : 2 * k + nt;   // workgroups of the last round
    return (k > 0 && last <= ncu && 2 * k <= nt) ? k : 0;
}

int mdqt::ensure_aux(mdqt_ctx* s) {
    const int nt_split = (s->N + 63) / 64;
    s->nsplit = s->use_n3 && s->npairs > 0 ? tile_split_count(s, nt_split) : 0;
    const int need = std::max(std::max(s->nseg, s->nslots + split_slots(s)), 2);
    HIPCHK(s->dFpart.reserve((size_t)s->capS * 3 * need));
    if (s->use_n3b) {
        HIPCHK(s->dSlots.reserve((size_t)(s->n3b.nd + s->n3b.R) * 3 * s->n3b.Npad));
        if (s->p.world_size > 1 && !s->dFr) HIPCHK(s->dFr.alloc((size_t)s->capS * 3 * s->p.world_size));
        if (s->sort_mode && s->N > s->capSortN) {
            const int Nc = s->N;
            const int Tc = (Nc + 63) / 64;
            s->capSortN = 0;                         // until every buffer of the new size is there
            HIPCHK(s->dKeys.alloc((size_t)2 * Nc));
            HIPCHK(s->dIon.alloc((size_t)2 * Nc));
            const size_t tmp_bytes = spatial_order_tmp_bytes(Nc);
            if (!tmp_bytes) return set_error("radix sort scratch size query failed");
            HIPCHK(s->dSortTmp.alloc(tmp_bytes));
            HIPCHK(s->dRs.alloc((size_t)3 * Tc * 64));
            HIPCHK(s->dBoxes.alloc((size_t)12 * Tc));
            HIPCHK(s->dSubBoxes.alloc((size_t)6 * 4 * Tc));
            HIPCHK(s->dTail.alloc((size_t)4 * Tc));
            HIPCHK(hipMemset(s->dTail, 0, (size_t)4 * Tc * sizeof(double)));
            HIPCHK(s->dTailList.alloc((size_t)Tc));
            if (!s->dTailSt) {                       // [0, 8) the force calls', [8, 16) the potential calls'
                HIPCHK(s->dTailSt.alloc(16));
                HIPCHK(hipMemset(s->dTailSt, 0, 16 * sizeof(unsigned long long)));
            }
            s->capSortN = Nc;
            if (tail_reset(s)) return -1;                // a new size: nothing measured yet
        }
    }
    if (s->use_n3 && s->npairs > 0) {
        const int tot = s->npairs + (s->nsplit > 0 ? s->npairs + 3 * s->nsplit + s->npairs : 0);   // (bound)
        HIPCHK(s->dPairs.reserve((size_t)tot));
        const int nt = (s->N + 63) / 64;
        std::vector<int2> h;
        h.reserve(s->npairs);
        // the diagonal tile pairs (half the rotation steps) last: they land in the dispatcher's
        // last round of workgroups, where the 7th workgroup of a CU goes (C2: 1,596 workgroups on
        // 256 CUs), so those CUs finish sooner (force launch 17.8 -> 17.3 us).  The slots a tile
        // pair writes do not depend on its position in the list: the same results.
        for (int I = 0; I < nt; ++I)
            for (int J = I + 1; J < nt; ++J) h.push_back(make_int2(I, J));
        for (int I = 0; I < nt; ++I) h.push_back(make_int2(I, I));
        if ((int)h.size() != s->npairs) return set_error("tile-pair table size mismatch");
        if (s->nsplit > 0) {                         // the split table (tile_split_count)
            const int k = s->nsplit;
            auto split = [&](int I, int J) { return J == I + 1 && (I & 1) == 0 && I < 2 * k; };
            auto part = [](int I, int pl, int p) { return (int)(((unsigned)pl << 30) | ((unsigned)p << 28) | (unsigned)I); };
            for (int I = 0; I < nt; ++I)
                for (int J = I + 1; J < nt; ++J)
                    if (!split(I, J)) h.push_back(make_int2(I, J));
            if (s->split_opt == 2) {                 // quarters of the split pairs, halves of the diagonal tiles
                for (int p = 0; p < 4; ++p)
                    for (int m = 0; m < k; ++m) h.push_back(make_int2(part(2 * m, 2, p), 2 * m + 1));
                for (int p = 0; p < 2; ++p)
                    for (int I = 0; I < nt; ++I) h.push_back(make_int2(part(I, 1, p), I));
            } else {                                 // halves of the split pairs around the diagonal tiles
                for (int m = 0; m < k; ++m) h.push_back(make_int2(part(2 * m, 1, 0), 2 * m + 1));
                for (int I = 0; I < nt; ++I) h.push_back(make_int2(I, I));
                for (int m = 0; m < k; ++m) h.push_back(make_int2(part(2 * m, 1, 1), 2 * m + 1));
            }
            s->nsplit_wg = (int)h.size() - s->npairs;
            if (s->nsplit_wg != s->npairs + (s->split_opt == 2 ? 3 * k + nt : k)) return set_error("split tile-pair table size mismatch");
            // the extra slots: only later parts of split tile pairs write them (their rows), every other row 0
            HIPCHK(hipMemsetAsync(s->dFpart + (size_t)nt * 3 * s->S, 0, (size_t)split_slots(s) * 3 * s->S * sizeof(double),
                                  s->stream));
        }
        HIPCHK(hipMemcpyAsync(s->dPairs, h.data(), h.size() * sizeof(int2), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    return 0;
}

// a new slab size S: what ensure_aux and the later calls size by it (or by N) starts over
static void drop_sized(mdqt_ctx* s) {
    s->dFpart.reset(); s->dUpart.reset(); s->dPairs.reset(); s->dSlots.reset(); s->dFr.reset(); s->dPlan.reset();
    s->dKeys.reset(); s->dIon.reset(); s->dSortTmp.reset(); s->dRs.reset(); s->dBoxes.reset(); s->dSubBoxes.reset();
    s->dTail.reset(); s->dTailList.reset(); s->dTailSt.reset(); s->dPeerParts.reset();
    s->capSortN = 0;
    s->capS = 0; s->kdeChunks = 0;
}

// (re)size everything for N ions; device contents are NOT preserved (callers upload after)
int mdqt::resize(mdqt_ctx* s, int N) {
    if (N < 0) return set_error("negative N");
    int lo, hi, S;
    if (mdqt_slab(N, s->p.world_size, s->p.rank, &lo, &hi, &S)) return -1;
    s->N = N; s->lo = lo; s->hi = hi; s->nloc = hi - lo;
    choose_segments(s);
    const int W = s->p.world_size;
    if (S != s->capS) {
        drop_sized(s);
        HIPCHK(hipSetDevice(s->dev));
        const size_t sz = (size_t)S * sizeof(double);
        HIPCHK(s->dR.alloc((size_t)S * 3 * W));
        HIPCHK(s->dV.alloc((size_t)S * 3));
        HIPCHK(s->dF.alloc((size_t)S * 3));
        HIPCHK(s->dPsi.alloc((size_t)S * 24));
        HIPCHK(s->dTp.alloc((size_t)S));
        HIPCHK(s->dUrow.alloc((size_t)S));
        if (s->p.rng_mode == 0) HIPCHK(s->dU.alloc((size_t)S * 5));
        HIPCHK(s->dScr.alloc(64 + 3 * NBINS));
        s->kdeChunks = 512;                            // chunks of >= 32 ions (the bins near v = 0 hold
        HIPCHK(s->dKde.alloc((size_t)s->kdeChunks * 3 * NBINS));   // the work)
        HIPCHK(s->dPack.alloc((size_t)S * 4));
        s->capS = S;
        HIPCHK(hipMemsetAsync(s->dR, 0, sz * 3 * W, s->stream));
        HIPCHK(hipMemsetAsync(s->dV, 0, sz * 3, s->stream));
        HIPCHK(hipMemsetAsync(s->dF, 0, sz * 3, s->stream));
        HIPCHK(hipMemsetAsync(s->dPsi, 0, sz * 24, s->stream));
        HIPCHK(hipMemsetAsync(s->dTp, 0, sz, s->stream));
    }
    s->S = S;
    if (ensure_aux(s)) return -1;
    s->Vholder.assign((size_t)NINTERVALV * 3 * (N > 0 ? N : 1), 0.);
    return 0;
}

extern "C" int mdqt_create(const mdqt_params* p, mdqt_ctx** out) {
    if (!p || !out) return set_error("mdqt_create: NULL argument");
    *out = nullptr;
    if (p->rng_mode != 0 && p->rng_mode != 1)
        return set_error("rng_mode must be 0 (drand48, reference order) or 1 (Philox)");
    if (p->rng_mode == 0 && p->world_size != 1)
        return set_error("rng_mode 0 (one sequential drand48 stream) needs world_size 1");
    if (p->world_size < 1 || p->rank < 0 || p->rank >= p->world_size) return set_error("bad world_size/rank");
    if (p->N0 < 1) return set_error("N0 must be >= 1");
    if (p->sampleFreq < 1) return set_error("sampleFreq must be >= 1");
    if (p->qt_model < 0 || p->qt_model >= NMODELS) return set_error("qt_model must be 0..%d", NMODELS - 1);
    if (p->qt_model != 0 && p->rng_mode != 1)
        return set_error("the optical-pumping qt_models run on the Philox stream (rng_mode 1)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) return set_error("no HIP device available (%s)", hipGetErrorString(e));
    std::unique_ptr<mdqt_ctx, void (*)(mdqt_ctx*)> guard(new mdqt_ctx(), mdqt_destroy);
    mdqt_ctx* s = guard.get();
    s->p = *p;
    s->p.saveDirectory[sizeof(s->p.saveDirectory) - 1] = 0;
    if (p->device >= 0) {
        if (p->device >= ndev) return set_error("device %d >= device count %d", p->device, ndev);
        s->dev = p->device;
    } else {
        (void)hipGetDevice(&s->dev);
    }
    if (hipSetDevice(s->dev) != hipSuccess || hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking) != hipSuccess)
        return set_error("cannot create HIP stream on device %d", p->device);
    s->stream = s->own;
    if (s->dTab.alloc(1) != hipSuccess || s->dFTab.alloc(2) != hipSuccess) return set_error("hipMalloc lane tables");
    {
        void* d = nullptr;
        if (s->hFlags.alloc(2, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess)
            return set_error("hipHostMalloc flags");
        s->hFlags[0] = s->hFlags[1] = 0;
        if (hipHostGetDevicePointer(&d, (void*)s->hFlags.get(), 0) != hipSuccess) return set_error("hipHostGetDevicePointer flags");
        s->dFlags = (int*)d;
        s->dSpinErr = s->dFlags + 1;
    }
    build_constants(s);
    if (s->p.rng_mode == 0) {
        unsigned long long h[97];
        h[0] = srand48_state(s->p.seed);
        unsigned long long A = 0x5DEECE66Dull, Cc = 0xBull;
        for (int b = 0; b < 48; ++b) {            // 2^b steps of X' = A X + C (mod 2^48)
            h[1 + b] = A; h[49 + b] = Cc;
            Cc = (A * Cc + Cc) & 0xFFFFFFFFFFFFull;
            A = (A * A) & 0xFFFFFFFFFFFFull;
        }
        if (s->dX48.alloc(97) != hipSuccess || hipMemcpy(s->dX48, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess)
            return set_error("drand48 state upload failed");
    }
    if (hipMemcpy(s->dTab, &s->tab, sizeof(LaneTab), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(s->dFTab, &s->ftab, sizeof(FastTab), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(s->dFTab + 1, &s->ftabL, sizeof(FastTab), hipMemcpyHostToDevice) != hipSuccess)
        return set_error("upload of the lane table failed");
    s->t = 0.; s->qidx = 0; s->c0 = p->c0; s->counter = 0;
    s->x48 = srand48_state(p->seed);
    strncpy(s->saveDirectory, s->p.saveDirectory, sizeof(s->saveDirectory) - 1);
    s->saveDirectory[sizeof(s->saveDirectory) - 1] = 0;
    if (resize(s, 0)) return -1;
    *out = guard.release();
    return 0;
}

extern "C" void mdqt_destroy(mdqt_ctx* s) {
    if (!s) return;
    s->writer.reset();                                   // joins the file writers
    (void)hipSetDevice(s->dev);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->evQ) (void)hipEventDestroy(s->evQ);
    if (s->evS) (void)hipEventDestroy(s->evS);
    if (s->qs) (void)hipStreamDestroy(s->qs);
    comm_destroy(s);
    for (auto& c : s->bdcalls) {
        for (hipEvent_t ev : c.m) if (ev) (void)hipEventDestroy(ev);
        if (c.ag0) (void)hipEventDestroy(c.ag0);
        if (c.ag1) (void)hipEventDestroy(c.ag1);
    }
    for (hipEvent_t ev : s->bdfree) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : s->bd_ag) if (ev) (void)hipEventDestroy(ev);
    if (s->own) (void)hipStreamDestroy(s->own);
    delete s;
}

// ---------------------------------------------------------------------------------------------
// state transfer (host <-> HBM); psi: host [N][12][2] interleaved <-> device [24][S]
// ---------------------------------------------------------------------------------------------

int mdqt::upload(mdqt_ctx* s, const double* R, const double* V, size_t ld, const double* psi,
                  const double* tPart) {
    const int N = s->N, S = s->S, W = s->p.world_size;
    HIPCHK(hipSetDevice(s->dev));
    if (R) {
        std::vector<double> h((size_t)3 * S * W, 0.);
        for (int g = 0; g < N; ++g) {
            const int w = g / S, l = g - w * S;
            for (int c = 0; c < 3; ++c) h[(size_t)w * 3 * S + (size_t)c * S + l] = R[(size_t)c * ld + g];
        }
        HIPCHK(hipMemcpyAsync(s->dR, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
        int oor = 0;                                     // positions outside [-L/8, 9L/8]?
        const double plo = -0.125 * s->L, phi = 1.125 * s->L;
        for (size_t k = 0; k < (size_t)3 * N && !oor; ++k) {
            const double x = R[(k / N) * ld + k % N];
            if (!(x >= plo && x <= phi)) oor = 1;
        }
        s->guard = oor != 0;
        HIPCHK(hipStreamSynchronize(s->stream));         // no earlier launch can raise the flag any more
        s->hFlags[0] = 0;
    }
    const int lo = s->lo, n = s->nloc;
    if (V) {
        std::vector<double> h((size_t)3 * S, 0.);
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < n; ++i) h[(size_t)c * S + i] = V[(size_t)c * ld + lo + i];
        HIPCHK(hipMemcpyAsync(s->dV, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    if (psi) {
        std::vector<double> h((size_t)24 * S, 0.);
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 24; ++k) h[(size_t)k * S + i] = psi[(size_t)(lo + i) * 24 + k];
        HIPCHK(hipMemcpyAsync(s->dPsi, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    if (tPart) {
        std::vector<double> h((size_t)S, 0.);
        for (int i = 0; i < n; ++i) h[i] = tPart[lo + i];
        HIPCHK(hipMemcpyAsync(s->dTp, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    return 0;
}

extern "C" int mdqt_set_state(mdqt_ctx* s, int N, const double* R, const double* V, size_t ld,
                              const double* psi, const double* tPart, double t) {
    if (!s) return set_error("NULL context");
    if (settle_forces(s)) return -1;                   // pending partials of the previous positions
    const bool sameN = N == s->N;
    if (!sameN && resize(s, N)) return -1;
    if (ld < (size_t)N) return set_error("ld < N");
    if (upload(s, R, V, ld, psi, tPart)) return -1;
    if (R && tail_reset(s, sameN)) return -1;          // new positions: the tail statistics restart
    s->t = t;
    return 0;
}

extern "C" int mdqt_set_forces(mdqt_ctx* s, const double* F, size_t ld) {
    s->f_pending = false;
    s->rs_pending = false;
    const int S = s->S, lo = s->lo, n = s->nloc;
    std::vector<double> h((size_t)3 * S, 0.);
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < n; ++i) h[(size_t)c * S + i] = F[(size_t)c * ld + lo + i];
    HIPCHK(hipSetDevice(s->dev));
    HIPCHK(hipMemcpyAsync(s->dF, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int mdqt_get_state(mdqt_ctx* s, double* R, double* V, double* F, size_t ld, double* psi,
                              double* tPart, double* t) {
    if (!s) return set_error("NULL context");
    const int N = s->N, S = s->S, W = s->p.world_size, lo = s->lo, n = s->nloc;
    if (ld < (size_t)N) return set_error("ld < N");
    HIPCHK(hipSetDevice(s->dev));
    if (check_range_flag(s)) return -1;
    if (F && settle_forces(s)) return -1;
    if (R) {
        std::vector<double> h((size_t)3 * S * W);
        HIPCHK(hipMemcpyAsync(h.data(), s->dR, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        for (int g = 0; g < N; ++g) {
            const int w = g / S, l = g - w * S;
            for (int c = 0; c < 3; ++c) R[(size_t)c * ld + g] = h[(size_t)w * 3 * S + (size_t)c * S + l];
        }
    }
    auto get3 = [&](const double* d, double* out) -> int {
        std::vector<double> h((size_t)3 * S);
        HIPCHK(hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < n; ++i) out[(size_t)c * ld + lo + i] = h[(size_t)c * S + i];
        return 0;
    };
    if (V && get3(s->dV, V)) return -1;
    if (F && get3(s->dF, F)) return -1;
    if (psi) {
        std::vector<double> h((size_t)24 * S);
        HIPCHK(hipMemcpyAsync(h.data(), s->dPsi, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 24; ++k) psi[(size_t)(lo + i) * 24 + k] = h[(size_t)k * S + i];
    }
    if (tPart) {
        std::vector<double> h((size_t)S);
        HIPCHK(hipMemcpyAsync(h.data(), s->dTp, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        for (int i = 0; i < n; ++i) tPart[lo + i] = h[i];
    }
    if (t) *t = s->t;
    return 0;
}

extern "C" int mdqt_get_N(const mdqt_ctx* s) { return s ? s->N : -1; }
extern "C" double mdqt_get_time(const mdqt_ctx* s) { return s->t; }
extern "C" int mdqt_set_time(mdqt_ctx* s, double t) { s->t = t; return 0; }
extern "C" uint64_t mdqt_get_qstep_index(const mdqt_ctx* s) { return s->qidx; }
extern "C" int mdqt_set_qstep_index(mdqt_ctx* s, uint64_t q) { s->qidx = q; return 0; }
extern "C" int mdqt_get_counters(const mdqt_ctx* s, int* c0, unsigned* counter, double* Epot, double* Epot0) {
    if (c0) *c0 = s->c0;
    if (counter) *counter = s->counter;
    if (Epot) *Epot = s->Epot;
    if (Epot0) *Epot0 = s->Epot0;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// init() (SpeedUp:289-348): rejection sampling of N9L candidate triples from ONE drand48 stream;
// a kept triple consumes 4 more draws for its wavefunction.
//
// Sequentially that is 3 N9L + 4 N draws (2.2e9 at N0 = 1M: ~13 s on one core).  In parallel,
// with the same stream and the same result bit for bit: a candidate starting at draw index p is
// kept iff ok(u_p) && ok(u_p+1) && ok(u_p+2), independently of the walk, so (1) threads scan
// disjoint ranges of draw indices (LCG jump-ahead to each range start) and list every p that
// WOULD be kept (rate 1/729); (2) one pass walks the candidates: from p the walk visits p, p+3,
// ... until the first listed p' in the same residue class mod 3, takes it and continues at
// p' + 7 (so the class shifts by one per kept ion), counting candidates up to N9L; (3) the kept
// ions' 7 draws are regenerated by jump-ahead, in parallel.  If the walk runs past the scanned
// range (more ions than the bound allows) it finishes sequentially from there.
// ---------------------------------------------------------------------------------------------

extern "C" int mdqt_init(mdqt_ctx* s) {
    if (!s) return set_error("NULL context");
    const double L = s->L;
    const double N9L = (unsigned)(9. * 9. * 9. * (L * L * L) * 3. / (4. * M_PI));   // :299
    int threads = s->init_threads;
    if (threads <= 0) {
        const unsigned hc = std::thread::hardware_concurrency();
        threads = (int)std::min(16u, hc ? hc : 1u);
    }
    const long Nbound = (long)s->p.N0 + 1000 + (long)(20. * sqrt((double)s->p.N0 + 1.));
    uint64_t xend = 0;
    const std::vector<InitIon> ions =
        init_sample(srand48_state(s->p.seed), L, (long)N9L, Nbound, threads, &xend);   // :1219, :303-335
    s->x48 = xend;
    std::vector<double> X, Y, Z, psi((size_t)24 * ions.size(), 0.);
    for (size_t k = 0; k < ions.size(); ++k) {
        X.push_back(ions[k].x); Y.push_back(ions[k].y); Z.push_back(ions[k].z);
        psi[24 * k] = ions[k].w0; psi[24 * k + 2] = ions[k].w2; psi[24 * k + 3] = ions[k].w3;
    }
    const int N = (int)X.size();
    std::vector<double> R((size_t)3 * N), V((size_t)3 * N, 0.), tp((size_t)N, 0.);
    for (int i = 0; i < N; ++i) { R[i] = X[i]; R[(size_t)N + i] = Y[i]; R[(size_t)2 * N + i] = Z[i]; }
    if (resize(s, N)) return -1;
    if (upload(s, R.data(), V.data(), N, psi.data(), tp.data())) return -1;
    if (tail_reset(s)) return -1;
    if (s->dX48) {                                   // the qstep draws continue this stream
        unsigned long long x = s->x48;
        HIPCHK(hipMemcpy(s->dX48, &x, sizeof x, hipMemcpyHostToDevice));
    }
    double e;
    if (mdqt_epotential(s, &e)) return -1;                                           // :345-347
    s->Epot0 = s->Epot;
    s->c0 = -1;
    s->t = 0.;
    s->qidx = 0;
    return 0;
}

extern "C" int mdqt_slab_bounds(const mdqt_ctx* s, int* lo, int* hi) {
    if (lo) *lo = s->lo;
    if (hi) *hi = s->hi;
    return 0;
}

extern "C" int mdqt_set_counters(mdqt_ctx* s, int c0, unsigned counter, double Epot, double Epot0) {
    s->c0 = c0; s->counter = counter; s->Epot = Epot; s->Epot0 = Epot0;
    return 0;
}

extern "C" int mdqt_get_drand48_state(mdqt_ctx* s, uint64_t* x) {
    if (!s || !x) return set_error("mdqt_get_drand48_state: bad arguments");
    if (!s->dX48) { *x = s->x48; return 0; }
    unsigned long long h = 0;
    HIPCHK(hipSetDevice(s->dev));
    HIPCHK(hipMemcpyAsync(&h, s->dX48, sizeof h, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    *x = h;
    return 0;
}
