// init()'s velocity draws of laserCoolNoPlasmaThreeState.cpp (:45-48, :83, :119-124) with the
// standard library's own std::mt19937 and std::normal_distribution, seeded with argv[1] instead of
// std::random_device: prints V[0][i], V[1][i], V[2][i] per ion as hexadecimal floats (exact).
// tests/test_mdlc_cpu.py compares mdlc_sample_velocities with it bit for bit.
//   mdlc_init_check <seed> <N0> <temperature>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: mdlc_init_check <seed> <N0> <temperature>\n");
        return 2;
    }
    const unsigned seed = (unsigned)strtoul(argv[1], nullptr, 10);
    const int N0 = atoi(argv[2]);
    const double temperature = atof(argv[3]);
    std::mt19937 rng(seed);                                            // :46
    std::uniform_real_distribution<double> uni(0, 1);                  // :47
    auto random_double = uni(rng);                                     // :48
    (void)random_double;
    std::normal_distribution<double> velocityDistribution(0, 1.0508 * sqrt(temperature));   // :83
    for (int i = 0; i < N0; ++i) {                                     // :119-124
        const double vx = velocityDistribution(rng);
        const double vy = velocityDistribution(rng);
        const double vz = velocityDistribution(rng);
        printf("%a %a %a\n", vx, vy, vz);
    }
    return 0;
}
