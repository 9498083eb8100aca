/*
 * lfbm5d_pgclip_values.h -- the host-and-device maths of the clipped Poisson-Gaussian stage (lfbm5d_pgclip.hip;
 * include/lfbm5d_pgclip.h has the definitions): the censored line fit on the clipped stage's statistics, the curves of a model
 * (clipped moments, stabiliser, exact unbiased inverse, both as 4097-knot tables) and the table look-up of one value.  Free of HIP
 * headers: tools/pgclip_host_check.cpp compiles it for the host alone (tests/test_pgclip_host.py).  Internal.
 */
#ifndef LFBM5D_PGCLIP_VALUES_H
#define LFBM5D_PGCLIP_VALUES_H

#include "lfbm5d_clip_values.h"

#include <vector>

namespace lfbm5d_pgclip {

constexpr int kKnots = 4097, kSegs = kKnots - 1;
constexpr int kQuad = 3201;                       /* points of the trapezoid rule over n = -kQuadR..kQuadR */
constexpr double kQuadR = 8.0;
constexpr double kVMin = 1.0 / 12.0;              /* the variance of rounding to whole numbers: the floor of sigma^2 */
constexpr double kMaxRatio = 0.5, kMaxA = 5.0;     /* the accepted domain: a^2 <= kMaxRatio b and a <= kMaxA (DESIGN 3o has the table) */

/* ---- the look-up ---- */

/* one finite value through a table T[4097]: float32, every operation on its own (the file is compiled without FMA contraction) */
template <bool INVERSE>
LFBM5D_HD float curve_value(const float* T, float x0, float inv_dx, float x) {
    const float t = (x - x0) * inv_dx;
    const int i = (int)fminf(fmaxf(floorf(t), 0.0f), (float)(kSegs - 1));
    float r = t - (float)i;
    if (INVERSE) r = fminf(fmaxf(r, 0.0f), 1.0f);
    const float t0 = T[i], t1 = T[i + 1];
    return t0 + r * (t1 - t0);
}

/* ---- the fit ---- */

struct Line { double a, b, f_max; unsigned levels; };

/* one histogram [64][322] with sum [64], cens [64] and `whole` (lfbm5d_clip::fit_one's arguments): the level variances of the clipped
 * stage, down its ladder until four levels count, then lfbm5d_pg_fit's constrained weighted line over those levels; a and b come back
 * in the data's own units.  false when even f_max = 1 leaves fewer than four levels. */
inline bool fit_one(const unsigned long long* hist, const unsigned long long* sum, const unsigned long long* cens, unsigned long long whole,
                    double s, Line& out) {
    using namespace lfbm5d_clip;
    unsigned long long total = 0;
    for (size_t i = 0; i < (size_t)kLevels * kKeys; i++) total += hist[i];
    const double delta = total && whole == total ? 0.5 * s : 0.0;
    LevelVar lv[kLevels];
    level_variances(hist, delta, lv);
    for (int r = 0; r < kLadder; r++) {
        double Sw = 0.0, Swx = 0.0, Swv = 0.0, Swxx = 0.0, Swxv = 0.0;
        unsigned used = 0;
        for (int l = 0; l < kLevels; l++) {
            if (!lv[l].ok || (double)cens[l] > kFMax[r] * (double)lv[l].n) continue;
            const double v = lv[l].v, x = (double)sum[l] / (256.0 * (double)lv[l].n);
            const double w = (double)lv[l].n / (v * v);
            Sw += w; Swx += w * x; Swv += w * v; Swxx += w * x * x; Swxv += w * x * v;
            used++;
        }
        if (used < kMinLevels) continue;
        const double det = Sw * Swxx - Swx * Swx;
        double a, b;
        if (!(det > 1e-12 * Sw * Swxx)) { a = 0.0; b = Swv / Sw; }
        else {
            a = (Sw * Swxv - Swx * Swv) / det;
            b = (Swxx * Swv - Swx * Swxv) / det;
            if (a < 0.0) { a = 0.0; b = Swv / Sw; }
            else if (b < 0.0) { b = 0.0; a = Swxv / Swxx; }
        }
        out.a = a / s; out.b = b / (s * s); out.f_max = kFMax[r]; out.levels = used;
        return true;
    }
    return false;
}

/* ---- the curves ---- */

inline bool valid_model(double a, double b, double lo, double hi) {
    return std::isfinite(a) && std::isfinite(b) && std::isfinite(lo) && std::isfinite(hi) && a >= 0.0 && b >= 0.0 && a + b > 0.0 && lo < hi &&
           std::isfinite(hi - lo);
}
inline bool in_domain(double a, double b) { return a * a <= kMaxRatio * b && a <= kMaxA; }

inline double sigma_of(double y, double a, double b, double lo) { return std::sqrt(std::max(a * (y - lo) + b, kVMin)); }

/* the mean and the deviation (about the mean) of clip(y + sigma n, lo, hi): both tails from erfc of the tail's own side, the second
 * moment taken about y so that nothing large cancels */
inline void clipped_moments(double y, double sg, double lo, double hi, double& mean, double& dev) {
    using lfbm5d_clip::kInvSqrt2; using lfbm5d_clip::kInvSqrt2Pi;
    const double al = (lo - y) / sg, be = (hi - y) / sg;
    const double ta = 0.5 * std::erfc(-al * kInvSqrt2), tb = 0.5 * std::erfc(be * kInvSqrt2);
    const double pa = kInvSqrt2Pi * std::exp(-0.5 * al * al), pb = kInvSqrt2Pi * std::exp(-0.5 * be * be);
    const double mid = 1.0 - ta - tb;
    mean = lo * ta + hi * tb + y * mid + sg * (pa - pb);
    const double var = (lo - y) * (lo - y) * ta + (hi - y) * (hi - y) * tb + sg * sg * (mid + al * pa - be * pb) - (mean - y) * (mean - y);
    dev = std::sqrt(var);
}

/* piecewise linear through (xk, fk)[n], xk strictly increasing, extended with slopes s0 below xk[0] and s1 above xk[n - 1] */
inline double pl_value(const double* xk, const double* fk, int n, double s0, double s1, double x) {
    if (x < xk[0]) return fk[0] + (x - xk[0]) * s0;
    if (x > xk[n - 1]) return fk[n - 1] + (x - xk[n - 1]) * s1;
    int l = 0, h = n - 1;                               /* xk[l] <= x <= xk[h] */
    while (h - l > 1) {
        const int m = (l + h) / 2;
        if (xk[m] <= x) l = m; else h = m;
    }
    return fk[l] + (fk[h] - fk[l]) * (x - xk[l]) / (xk[h] - xk[l]);
}

struct Curves {
    double s, fwd_x0, fwd_dx, inv_x0, inv_dx;
    std::vector<double> y, mean, dev, F, G, fwd, inv;    /* the grid, the moments, F at `mean`, G at y; the tables in double */
    double s0, s1;                                       /* F's slopes beyond the ends */
    double F_of(double z) const { return pl_value(mean.data(), F.data(), kKnots, s0, s1, z); }
};

/* 0: built.  1: the model is invalid.  2: outside the accepted domain.  3: a moment is not finite or positive, the clipped mean or G
 * is not strictly increasing. */
inline int make_curves(double a, double b, double lo, double hi, bool domain, Curves& c) {
    if (!valid_model(a, b, lo, hi)) return 1;
    if (domain && !in_domain(a, b)) return 2;
    const int n = kSegs;
    c.y.resize(kKnots); c.mean.resize(kKnots); c.dev.resize(kKnots); c.F.resize(kKnots); c.G.resize(kKnots);
    c.fwd.resize(kKnots); c.inv.resize(kKnots);
    std::vector<double> sg(kKnots);
    const double step = (hi - lo) / n;
    for (int i = 0; i <= n; i++) {
        c.y[i] = lo + i * step;
        sg[i] = sigma_of(c.y[i], a, b, lo);
        clipped_moments(c.y[i], sg[i], lo, hi, c.mean[i], c.dev[i]);
        if (!std::isfinite(c.mean[i]) || !std::isfinite(c.dev[i]) || !(c.dev[i] > 0.0)) return 3;
        if (i && !(c.mean[i] > c.mean[i - 1])) return 3;
    }
    c.F[0] = 0.0;
    for (int i = 1; i <= n; i++) c.F[i] = c.F[i - 1] + 0.5 * (1.0 / c.dev[i - 1] + 1.0 / c.dev[i]) * (c.mean[i] - c.mean[i - 1]);
    c.s = 255.0 / c.F[n];
    if (!std::isfinite(c.s) || !(c.s > 0.0)) return 3;
    for (int i = 0; i <= n; i++) c.F[i] *= c.s;
    c.s0 = c.s / c.dev[0]; c.s1 = c.s / c.dev[n];
    for (int i = 0; i <= n; i++) c.fwd[i] = c.F_of(c.y[i]);
    std::vector<double> nq(kQuad), w(kQuad);
    double wsum = 0.0;
    for (int j = 0; j < kQuad; j++) {
        nq[j] = -kQuadR + j * (2.0 * kQuadR / (kQuad - 1));
        w[j] = lfbm5d_clip::kInvSqrt2Pi * std::exp(-0.5 * nq[j] * nq[j]) * (j == 0 || j == kQuad - 1 ? 0.5 : 1.0);
        wsum += w[j];
    }
    const double* xk = c.mean.data();
    const double* fk = c.F.data();
    for (int i = 0; i <= n; i++) {
        double g = 0.0;
        int l = 0;                                       /* z rises with j: the segment of F is walked, not searched (pl_value's own) */
        for (int j = 0; j < kQuad; j++) {
            double z = c.y[i] + sg[i] * nq[j];
            z = z < lo ? lo : z > hi ? hi : z;
            double f;
            if (z < xk[0]) f = fk[0] + (z - xk[0]) * c.s0;
            else if (z > xk[n]) f = fk[n] + (z - xk[n]) * c.s1;
            else {
                while (l + 1 < n && xk[l + 1] <= z) l++;
                f = fk[l] + (fk[l + 1] - fk[l]) * (z - xk[l]) / (xk[l + 1] - xk[l]);
            }
            g += w[j] * f;
        }
        c.G[i] = g / wsum;
        if (i && !(c.G[i] > c.G[i - 1])) return 3;
    }
    c.fwd_x0 = lo; c.fwd_dx = step;
    c.inv_x0 = c.G[0]; c.inv_dx = (c.G[n] - c.G[0]) / n;
    for (int i = 0; i <= n; i++) c.inv[i] = pl_value(c.G.data(), c.y.data(), kKnots, 0.0, 0.0, c.inv_x0 + i * c.inv_dx);
    c.inv[0] = lo; c.inv[n] = hi;
    return 0;
}

} /* namespace lfbm5d_pgclip */
#endif
