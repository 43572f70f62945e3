// What the command lines (mdqt_cli.cpp, mdmc_cli.cpp, mdlc_cli.cpp) parse alike: an argument "--key=value", a 0 | 1
// switch, and the axes of a parameter scan, --sweep=NAME:v1,v2,... once per NAME, with the points they span.  Nothing here
// prints or exits: a false result is the caller's usage() and exit 2.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <vector>

// "--key=value" -> key (at most cap - 1 characters) and value
inline bool cli_key_value(const char* a, char* key, size_t cap, const char** value) {
    const char* eq = strchr(a, '=');
    if (strncmp(a, "--", 2) != 0 || !eq) return false;
    const size_t kl = (size_t)(eq - a - 2);
    if (kl >= cap) return false;
    memcpy(key, a + 2, kl);
    key[kl] = 0;
    *value = eq + 1;
    return true;
}

// a 0 | 1 switch's value: false for anything else (empty, signs, trailing text)
inline bool cli_switch(const char* v, long* out) {
    if ((v[0] != '0' && v[0] != '1') || v[1]) return false;
    *out = v[0] - '0';
    return true;
}

enum { kSweepMax = 1024 };   // values of one axis (and mdqt's members in all)

// one axis of the scan: the index of its NAME in the program's table and its values
struct SweepAxis {
    int field;
    std::vector<double> v;
};

// the axes in the order given
struct SweepAxes {
    std::vector<SweepAxis> axes;

    bool empty() const { return axes.empty(); }

    // "NAME:v1,v2,..." as one more axis: NAME one of `names` and not given before, a non-empty list of at most
    // kSweepMax numbers
    template <size_t N>
    bool add(const char* text, const char* const (&names)[N]) {
        const char* colon = strchr(text, ':');
        if (!colon) return false;
        SweepAxis ax;
        ax.field = -1;
        for (size_t f = 0; f < N; ++f)
            if (strlen(names[f]) == (size_t)(colon - text) && !strncmp(text, names[f], (size_t)(colon - text))) ax.field = (int)f;
        if (ax.field < 0) return false;
        for (const SweepAxis& o : axes)
            if (o.field == ax.field) return false;
        for (const char* s = colon + 1;;) {
            char* end = NULL;
            const double x = strtod(s, &end);
            if (end == s || (*end != ',' && *end != 0) || ax.v.size() >= kSweepMax) return false;
            ax.v.push_back(x);
            if (!*end) break;
            s = end + 1;
        }
        axes.push_back(ax);
        return true;
    }

    // The points: the product of the axes, the first-given axis slowest, every other field from `base`;
    // fields[f] is the member of NAME f.  max_points > 0: false where there are more (the size is otherwise
    // the library's to refuse).
    template <class P>
    bool points(const P& base, double P::*const* fields, long max_points, std::vector<P>* out) const {
        long n = 1;
        for (const SweepAxis& ax : axes) {
            n *= (long)ax.v.size();
            if (max_points > 0 && n > max_points) return false;
        }
        out->assign((size_t)n, base);
        for (long q = 0; q < n; ++q) {
            long rest = q;
            for (size_t o = axes.size(); o-- > 0;) {
                const long len = (long)axes[o].v.size();
                (*out)[(size_t)q].*fields[axes[o].field] = axes[o].v[(size_t)(rest % len)];
                rest /= len;
            }
        }
        return true;
    }
};
