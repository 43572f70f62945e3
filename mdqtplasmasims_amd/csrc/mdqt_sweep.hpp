// The host rules of a parameter scan ("sweep"): npoints parameter points x R replicas as the members of one
// ensemble, point-major.  Shared by the engines that have one (mdqt_ensemble_create_sweep, mdqt_ensemble.cpp;
// mdlc_create_sweep, mdlc_engine.cpp), each of which describes its params struct P by a table of the fields that
// may differ between the points and by a function naming the first of the other fields in which two points differ
// (fixed_field_differs: the list of the struct's other fields).  Host arithmetic only; every refusal is a
// set_error.  What stays with an engine: its size limits, the rules of its own fields, what a replica changes in
// the parameters, and each message's closing explanation.
#pragma once
#include <stdio.h>
#include <string.h>

#include <string>

#include "mdqt_error.hpp"   // set_error, ref_udcast

namespace mdqt {

// a field that may differ between the points; the run directory's name holds ref_udcast(value * scale)
template <class P>
struct SweepField {
    const char* name;
    double P::*field;
    double scale;
};

// "a, b and c" of the table's names; scales: "a x 100, b x 100 and c x 1000000"
template <class P, size_t N>
std::string sweep_names(const SweepField<P> (&tab)[N], bool scales = false) {
    std::string s;
    for (size_t f = 0; f < N; ++f) {
        char b[96];
        if (scales) snprintf(b, sizeof b, "%s x %.0f", tab[f].name, tab[f].scale);
        else snprintf(b, sizeof b, "%s", tab[f].name);
        s += (f == 0 ? "" : f + 1 == N ? " and " : ", ");
        s += b;
    }
    return s;
}

// Point q against point 0: `fixed` = the engine's fixed_field_differs(pts[0], pts[q]), `why` = what the fixed
// fields fix.  (One point per call: the engines place their own rules of a point before or after it.)
template <class P, size_t N>
int sweep_refuse_fixed(const SweepField<P> (&tab)[N], int q, const char* fixed, const char* why, const char* what) {
    if (!fixed) return 0;
    return set_error("%s: point %d differs from point 0 in %s: only %s may differ between the points (%s)", what, q, fixed,
                     sweep_names(tab).c_str(), why);
}

// Every pair of points: two identical points, or two whose run directories have the same name, would write the
// same files
template <class P, size_t N>
int sweep_refuse_same(const SweepField<P> (&tab)[N], const P* pts, int npoints, const char* what) {
    for (int q = 1; q < npoints; ++q)
        for (int o = 0; o < q; ++o) {
            size_t same = 0, collide = 0, first = N;
            for (size_t f = 0; f < N; ++f) {
                const double a = pts[o].*tab[f].field, b = pts[q].*tab[f].field;
                const bool eq = !memcmp(&a, &b, sizeof a) || a == b;
                same += eq;
                collide += ref_udcast(a * tab[f].scale) == ref_udcast(b * tab[f].scale);
                if (first == N && !eq) first = f;
            }
            if (same == N)
                return set_error("%s: point %d is identical to point %d (%s all equal): both would write the same run "
                                 "directories", what, q, o, sweep_names(tab).c_str());
            if (collide == N)
                return set_error("%s: point %d and point %d give the same run directory name: %s %.17g and %.17g print alike "
                                 "(the name holds %s as integers)", what, q, o, tab[first].name, pts[q].*tab[first].field,
                                 pts[o].*tab[first].field, sweep_names(tab, true).c_str());
        }
    return 0;
}

// member k of npoints x R: point k / R, replica k % R; `word`: what the engine calls k ("job", "member")
inline int sweep_member(int npoints, int R, int k, const char* word, const char* what, int* point, int* replica) {
    const long long members = (long long)npoints * R;
    if (k < 0 || k >= members) return set_error("%s: %s index %d outside [0, %lld)", what, word, k, members);
    *point = k / R;
    *replica = k % R;
    return 0;
}

}  // namespace mdqt
