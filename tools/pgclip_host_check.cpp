/*
 * pgclip_host_check.cpp -- the clipped Poisson-Gaussian stage's curves and look-up (lfbm5d_amd/csrc/lfbm5d_pgclip_values.h) compiled for
 * the host alone.  For the five models of tests/test_pgclip.py it builds the curves and checks them against a brute-force quadrature
 * (the trapezoid rule over n = -12..12 in 120001 points, 16 times finer than the stage's own and wider, of the integrand itself):
 *   moments   the closed forms of the clipped mean and deviation at 33 values of y against the quadrature of clip(y + sigma n) and of
 *             its square about y                                                                       (allowed: 1e-6)
 *   G         G at the same y against the quadrature of F(clip(y + sigma n))                            (allowed: 1e-3, in units of F)
 *   look-up   the ramp lo - 50 .. hi + 50 in steps of 1/64 through curve_value, the code the kernel runs per value: the forward
 *             results never decrease and stay within 2e-3 of F in double inside lo..hi; the inverse results of the forward results
 *             stay in lo..hi and never decrease; inverse(G by quadrature) returns y within 1e-3.
 * Prints one line per case and the worst figures; exit status 1 when a bound is missed.  tests/test_pgclip_host.py builds and runs it;
 * it also serves as the program for a host sanitizer build (g++ -fsanitize=address,undefined).
 *   pgclip_host_check
 */
#include "../lfbm5d_amd/csrc/lfbm5d_pgclip_values.h"

#include <cstdio>

using namespace lfbm5d_pgclip;

namespace {

constexpr int kFine = 120001;
constexpr double kFineR = 12.0;

/* E[f(clip(y + sg n, lo, hi))] by the fine trapezoid rule, normalised */
template <class F>
double expect(double y, double sg, double lo, double hi, F f) {
    double acc = 0.0, wsum = 0.0;
    for (int j = 0; j < kFine; j++) {
        const double n = -kFineR + j * (2.0 * kFineR / (kFine - 1));
        const double w = std::exp(-0.5 * n * n) * (j == 0 || j == kFine - 1 ? 0.5 : 1.0);
        const double z = y + sg * n;
        acc += w * f(z < lo ? lo : z > hi ? hi : z);
        wsum += w;
    }
    return acc / wsum;
}

} /* namespace */

int main() {
    const double cases[][4] = {{0.0, 625.0, 0.0, 255.0}, {0.0, 2500.0, 0.0, 255.0}, {2.0, 25.0, 0.0, 255.0}, {1.0, 100.0, 0.0, 255.0},
                               {0.0, 625.0, 16.0, 235.0}};
    double worst_m = 0.0, worst_g = 0.0, worst_f = 0.0, worst_i = 0.0;
    int bad = 0;
    for (const auto& k : cases) {
        const double a = k[0], b = k[1], lo = k[2], hi = k[3];
        Curves c;
        const int rc = make_curves(a, b, lo, hi, true, c);
        if (rc) { std::printf("case (%g, %g, %g, %g): refused (%d)\n", a, b, lo, hi, rc); return 1; }
        std::vector<float> fwd(kKnots), inv(kKnots);
        for (int i = 0; i < kKnots; i++) { fwd[i] = (float)c.fwd[i]; inv[i] = (float)c.inv[i]; }
        const float fx0 = (float)c.fwd_x0, fidx = (float)(1.0 / c.fwd_dx), ix0 = (float)c.inv_x0, iidx = (float)(1.0 / c.inv_dx);
        double em = 0.0, eg = 0.0, ef = 0.0, ei = 0.0;
        for (int q = 0; q <= 32; q++) {
            const int i = q * (kSegs / 32);
            const double y = c.y[i], sg = sigma_of(y, a, b, lo);
            const double m = expect(y, sg, lo, hi, [](double z) { return z; });
            const double v = expect(y, sg, lo, hi, [&](double z) { return (z - y) * (z - y); }) - (m - y) * (m - y);
            em = std::max(em, std::max(std::fabs(m - c.mean[i]), std::fabs(std::sqrt(v) - c.dev[i])));
            const double g = expect(y, sg, lo, hi, [&](double z) { return c.F_of(z); });
            eg = std::max(eg, std::fabs(g - c.G[i]));
            const float back = curve_value<true>(inv.data(), ix0, iidx, (float)g);
            ei = std::max(ei, std::fabs((double)back - y));
        }
        int down = 0, out = 0;
        float prev_f = -INFINITY, prev_i = (float)lo;
        const int n = (int)((hi - lo + 100.0) * 64.0);
        for (int i = 0; i <= n; i++) {
            const float x = (float)(lo - 50.0 + (double)i / 64.0);
            const float f = curve_value<false>(fwd.data(), fx0, fidx, x);
            if (f < prev_f) down++;
            prev_f = f;
            if ((double)x >= lo && (double)x <= hi) ef = std::max(ef, std::fabs((double)f - c.F_of((double)x)));
            const float y = curve_value<true>(inv.data(), ix0, iidx, f);
            if (y < prev_i) down++;
            prev_i = y;
            if (!((double)y >= lo && (double)y <= hi)) out++;
        }
        std::printf("case (%g, %g, %g, %g): s = %.6f, moments %.3g, G %.3g, forward table %.3g, inverse of G %.3g, decreases %d, "
                    "outside the range %d\n", a, b, lo, hi, c.s, em, eg, ef, ei, down, out);
        worst_m = std::max(worst_m, em); worst_g = std::max(worst_g, eg); worst_f = std::max(worst_f, ef); worst_i = std::max(worst_i, ei);
        bad += down + out;
    }
    std::printf("worst: moments %.3g, G %.3g, forward table %.3g, inverse of G %.3g, bad %d\n", worst_m, worst_g, worst_f, worst_i, bad);
    return bad || worst_m > 1e-6 || worst_g > 1e-3 || worst_f > 2e-3 || worst_i > 1e-3 ? 1 : 0;
}
