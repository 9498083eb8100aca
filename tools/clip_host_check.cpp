/*
 * clip_host_check.cpp -- the clipping-aware stage's map (declip_value, lfbm5d_amd/csrc/lfbm5d_clip_values.h) compiled for the host alone:
 * for every sigma of a grid from 1/100 of a grey level to 40 times the range, and the ranges 0..255 and 16..235, walks the ramp lo - 50
 * .. hi + 50 in steps of 1/64 through the code the kernel runs and checks, per value, the residual |E(y) - d| of the Newton result
 * against a bisection's and that the float results do not decrease.  Prints one line per case and the worst figures; exit status 1 when a
 * result decreases or a residual exceeds 1e-9.  tests/test_clip_host.py builds and runs it; it also serves as the program for a host
 * sanitizer build (g++ -fsanitize=address,undefined).
 *   clip_host_check
 */
#include "../lfbm5d_amd/csrc/lfbm5d_clip_values.h"

#include <cstdio>

using namespace lfbm5d_clip;

static double bisect(const Map& m, double d) {
    if (d <= m.e_lo) return m.lo;
    if (d >= m.e_hi) return m.hi;
    double a = m.lo, b = m.hi;
    for (int i = 0; i < 100; i++) {
        const double mid = 0.5 * (a + b);
        double E, dE;
        mean_slope(m, mid, E, dE);
        if (E < d) a = mid; else b = mid;
    }
    return 0.5 * (a + b);
}

int main() {
    const double sigmas[] = {0.01, 0.1, 1.0, 5.0, 25.0, 50.0, 100.0, 300.0, 1000.0, 10000.0};
    const double ranges[][2] = {{0.0, 255.0}, {16.0, 235.0}};
    double worst_res = 0.0, worst_dif = 0.0;
    int bad = 0;
    for (const auto& r : ranges)
        for (const double sigma : sigmas) {
            Map m;
            if (!make_map(r[0], r[1], sigma, m)) { std::printf("range %g..%g sigma %g: rejected\n", r[0], r[1], sigma); return 1; }
            double res = 0.0, dif = 0.0;
            float prev = (float)r[0];
            int down = 0;
            const int n = (int)((r[1] - r[0] + 100.0) * 64.0);
            for (int i = 0; i <= n; i++) {
                const float d = (float)(r[0] - 50.0 + (double)i / 64.0);
                const double y = declip_value(m, (double)d);
                const float yf = (float)y;
                if (yf < prev) down++;
                prev = yf;
                if ((double)d > m.e_lo && (double)d < m.e_hi) {
                    double E, dE;
                    mean_slope(m, y, E, dE);
                    res = std::max(res, std::fabs(E - (double)d));
                }
                dif = std::max(dif, std::fabs(y - bisect(m, (double)d)));
            }
            std::printf("range %g..%g sigma %g: E(lo) = %.6f, max |E(y) - d| = %.3g, max |y - bisection| = %.3g, decreases %d\n", r[0], r[1],
                        sigma, m.e_lo, res, dif, down);
            worst_res = std::max(worst_res, res); worst_dif = std::max(worst_dif, dif);
            bad += down;
        }
    std::printf("worst: |E(y) - d| = %.3g, |y - bisection| = %.3g, decreases %d\n", worst_res, worst_dif, bad);
    return bad || worst_res > 1e-9 ? 1 : 0;
}
