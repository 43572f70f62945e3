// "%lg" text of the reference programs' output files, without the background writers (mdqt_writer.hpp, which
// formats through it): std::to_chars(general, precision 6) is specified to produce exactly printf("%.6g") in the
// C locale (= "%lg") — same bytes, several times faster; non-finite values go through snprintf so "inf"/"-nan"
// spellings stay glibc's.  On its own for the engine that writes on its own thread (mdlc_engine.cpp).
#pragma once

#include <charconv>
#include <cmath>
#include <cstdio>
#include <string>

namespace mdqt {

// "%lg" text into a growing buffer, spilled to the FILE every ~1 MB (bounded memory at N = 1M)
class LgText {
  public:
    explicit LgText(FILE* f = nullptr) : f_(f) { s_.reserve(kSpill + 4096); }
    ~LgText() { spill(); }
    void num(double x) {
        char b[40];
        if (std::isfinite(x)) {
            auto r = std::to_chars(b, b + sizeof b, x, std::chars_format::general, 6);
            s_.append(b, r.ptr - b);
        } else {
            int n = snprintf(b, sizeof b, "%lg", x);
            s_.append(b, n);
        }
        if (s_.size() >= kSpill) spill();
    }
    void integer(long long v) {
        char b[24];
        auto r = std::to_chars(b, b + sizeof b, v);
        s_.append(b, r.ptr - b);
    }
    void ch(char c) { s_.push_back(c); }
    void str(const char* p) { s_.append(p); }
    const std::string& text() const { return s_; }   // (no FILE: the whole text, for tests)
    bool ok() const { return ok_; }
    void spill() {
        if (!f_ || s_.empty()) return;
        if (fwrite(s_.data(), 1, s_.size(), f_) != s_.size()) ok_ = false;
        s_.clear();
    }

  private:
    static constexpr size_t kSpill = 1 << 20;
    FILE* f_;
    std::string s_;
    bool ok_ = true;
};

}  // namespace mdqt
