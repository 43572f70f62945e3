// std::mt19937 ([rand.predef]) with the state in plain view, shared by the host engines that keep
// a reference program's std::mt19937 stream (mdmc_engine.cpp, mdlc_engine.cpp): the same sequence
// as the reference's engine (so uniform_real_distribution / normal_distribution draw the same
// values from it), a discard that skips the tempering, and the device MC kernel's [624 words,
// position] layout without a text round trip.
#pragma once

#include <stdint.h>

#include <algorithm>

namespace mdqt {

struct Mt32 {
    using result_type = uint32_t;
    static constexpr result_type min() { return 0u; }
    static constexpr result_type max() { return 0xffffffffu; }
    uint32_t x[625];   // x[624] = position
    void seed(uint32_t s) {
        x[0] = s;
        for (uint32_t i = 1; i < 624; ++i) x[i] = 1812433253u * (x[i - 1] ^ (x[i - 1] >> 30)) + i;
        x[624] = 624;
    }
    void twist() {
        uint32_t* v = x;
        auto f = [](uint32_t a, uint32_t b, uint32_t m) {
            const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
            return m ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        };
        for (int k = 0; k < 227; ++k) v[k] = f(v[k], v[k + 1], v[k + 397]);
        for (int k = 227; k < 623; ++k) v[k] = f(v[k], v[k + 1], v[k - 227]);
        v[623] = f(v[623], v[0], v[396]);
        x[624] = 0;
    }
    result_type operator()() {
        if (x[624] >= 624) twist();
        uint32_t z = x[x[624]++];
        z ^= z >> 11;
        z ^= (z << 7) & 0x9d2c5680u;
        z ^= (z << 15) & 0xefc60000u;
        z ^= z >> 18;
        return z;
    }
    void discard(unsigned long long n) {
        while (n) {
            if (x[624] >= 624) twist();
            const unsigned long long k = std::min<unsigned long long>(n, 624 - x[624]);
            x[624] += (uint32_t)k;
            n -= k;
        }
    }
};

}  // namespace mdqt
