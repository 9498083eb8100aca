/*
 * lfbm5d_clip_values.h -- the host-and-device maths of the clipping-aware stage (lfbm5d_clip.hip; include/lfbm5d.h has the definitions):
 * the clipped mean E(y) of a value under Gaussian noise and a known range with its slope, its inverse by a fixed number of Newton steps,
 * and the fit of sigma to the block statistics with its ladder over the censored fraction.  Free of HIP headers:
 * tools/clip_host_check.cpp compiles it for the host alone (tests/test_clip_host.py).  Internal.
 */
#ifndef LFBM5D_CLIP_VALUES_H
#define LFBM5D_CLIP_VALUES_H

#include "lfbm5d_side_values.h"

#include <cstring>

namespace lfbm5d_clip {

constexpr int kLevels = 64;
constexpr int kEMin = -12, kEMax = 8;
constexpr int kKeys = (kEMax - kEMin) * 16 + 2;      /* 322: the keys of |d| of the Poisson-Gaussian statistics */
constexpr int kKeyBase = (kEMin + 127) << 4;
constexpr unsigned long long kMinBlocks = 256;       /* a level counts from this many blocks on */
constexpr unsigned kMinLevels = 4;                   /* the fit needs this many levels */
constexpr double kQuartile = 0.31863936396437514;    /* the 0.25 quantile of |N(0,1)| */
constexpr int kLadder = 5;
constexpr double kFMax[kLadder] = {0.05, 0.1, 0.2, 0.4, 1.0};
constexpr double kHeavy = 0.1;                       /* f_max above it: heavily clipped */
constexpr int kNewtonF = 4, kNewtonD = 2;            /* steps of the inverse in float, then in double: see declip_value */
constexpr double kFar = 9.0;                         /* beyond this many sigma from both bounds E is the identity in double */
constexpr double kInvSqrt2 = 0.7071067811865475244, kInvSqrt2Pi = 0.3989422804014326779;

/* the factor that takes lo..hi onto the 0..255 of the levels and keys, as the statistics kernel applies it */
inline float rescale(double lo, double hi) { return (float)(255.0 / (hi - lo)); }

/* ---- the map ---- */

struct Map { double lo, hi, sigma, inv_sigma, e_lo, e_hi; };

/* E(y) = lo Phi(a) + hi Phi(-b) + y (1 - Phi(a) - Phi(-b)) + sigma (phi(a) - phi(b)), a = (lo - y) / sigma, b = (hi - y) / sigma, and
 * its slope 1 - Phi(a) - Phi(-b), for lo <= y <= hi: both tails come from erfc of a non-negative argument, nothing cancels */
LFBM5D_HD void mean_slope(const Map& m, double y, double& E, double& dE) {
    const double a = (m.lo - y) * m.inv_sigma, b = (m.hi - y) * m.inv_sigma;
    const double ta = 0.5 * erfc(-a * kInvSqrt2), tb = 0.5 * erfc(b * kInvSqrt2);
    const double pa = kInvSqrt2Pi * exp(-0.5 * a * a), pb = kInvSqrt2Pi * exp(-0.5 * b * b);
    dE = 1.0 - ta - tb;
    E = m.lo * ta + m.hi * tb + y * dE + m.sigma * (pa - pb);
}

/* the same in float: what the first Newton steps run on */
LFBM5D_HD void mean_slope_f(const Map& m, float y, float& E, float& dE) {
    const float lo = (float)m.lo, hi = (float)m.hi, is = (float)m.inv_sigma;
    const float a = (lo - y) * is, b = (hi - y) * is;
    const float ta = 0.5f * erfcf(-a * (float)kInvSqrt2), tb = 0.5f * erfcf(b * (float)kInvSqrt2);
    const float pa = (float)kInvSqrt2Pi * expf(-0.5f * a * a), pb = (float)kInvSqrt2Pi * expf(-0.5f * b * b);
    dE = 1.0f - ta - tb;
    E = lo * ta + hi * tb + y * dE + (float)m.sigma * (pa - pb);
}

/* clamp(E^-1(d), lo, hi) of a finite d.  Newton from y = d: E(y) - y is positive and E convex below the middle of the range, negative
 * and concave above it, so the steps approach the root from d's side without passing it; with e the error in units of sigma,
 * e' <= phi(0) / (2 slope) e^2 and e_0 <= phi(0).  A Newton step forgets the error of the steps before it, so the first kNewtonF steps
 * run in float (down to float's own resolution of E) and only the last kNewtonD in double: those take the error from 1e-5 to below
 * double precision for every sigma from 1/100 grey level to many times the range (tools/clip_host_check.cpp walks the grid).  The
 * counts are fixed: no value decides how long a thread runs. */
LFBM5D_HD double declip_value(const Map& m, double d) {
    if (d <= m.e_lo) return m.lo;
    if (d >= m.e_hi) return m.hi;
    if (d - m.lo > kFar * m.sigma && m.hi - d > kFar * m.sigma) return d;
    const float df = (float)d, flo = (float)m.lo, fhi = (float)m.hi;
    float yf = df;
#ifdef __HIPCC__
#pragma unroll 1
#endif
    for (int k = 0; k < kNewtonF; k++) {
        float E, dE;
        mean_slope_f(m, yf, E, dE);
        yf -= (E - df) / dE;
        yf = yf >= flo ? (yf <= fhi ? yf : fhi) : flo;       /* a NaN (0 / 0 at a sigma beyond float's reach) goes to lo */
    }
    double y = (double)yf;
    y = y < m.lo ? m.lo : y > m.hi ? m.hi : y;
#ifdef __HIPCC__
#pragma unroll 1
#endif
    for (int k = 0; k < kNewtonD; k++) {
        double E, dE;
        mean_slope(m, y, E, dE);
        y -= (E - d) / dE;
        y = y < m.lo ? m.lo : y > m.hi ? m.hi : y;
    }
    return y;
}

/* false on a rejected range or sigma (lo < hi, both finite; sigma finite and positive, 1 / sigma finite) */
inline bool make_map(double lo, double hi, double sigma, Map& m) {
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !std::isfinite(hi - lo)) return false;
    if (!std::isfinite(sigma) || !(sigma > 0.0) || !std::isfinite(1.0 / sigma)) return false;
    m.lo = lo; m.hi = hi; m.sigma = sigma; m.inv_sigma = 1.0 / sigma;
    double dE;
    mean_slope(m, lo, m.e_lo, dE);
    mean_slope(m, hi, m.e_hi, dE);
    return true;
}

/* ---- the fit ---- */

/* lower edge of key k (1 <= k <= 321): the float whose bits are (k - 1 + 1840) << 19; key 0 starts at 0.  delta > 0: every d is a
 * multiple of delta and stands for the continuous values within delta / 2 of it, so the counts below the edge hold the mass below
 * (the first multiple of delta >= the edge) - delta / 2 */
inline double key_edge(int k, double delta) {
    if (k <= 0) return 0.0;
    const unsigned bits = (unsigned)(k - 1 + kKeyBase) << 19;
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    const double e = (double)f;
    return delta > 0.0 ? std::ceil(e / delta) * delta - 0.5 * delta : e;
}

struct LevelVar { unsigned long long n; double v; bool ok; };

/* n and the variance of every level of one histogram [64][322]: the 0.25 quantile of |d| as lfbm5d_pg_fit takes it, on the edges of
 * key_edge, less the rounding's own variance delta^2 / 3; ok = false under 256 blocks, on a quantile in an end key, or v <= 0 */
inline void level_variances(const unsigned long long* hist, double delta, LevelVar* lv) {
    for (int l = 0; l < kLevels; l++) {
        const unsigned long long* h = hist + (size_t)l * kKeys;
        unsigned long long n = 0;
        for (int k = 0; k < kKeys; k++) n += h[k];
        lv[l].n = n; lv[l].v = 0.0; lv[l].ok = false;
        if (n < kMinBlocks) continue;
        const double T = 0.25 * (double)n;
        unsigned long long cum = 0, before = 0;
        int ks = 0;
        for (; ks < kKeys; ks++) {
            before = cum;
            cum += h[ks];
            if ((double)cum >= T) break;
        }
        if (ks <= 0 || ks >= kKeys - 1) continue;
        const double e0 = key_edge(ks, delta), e1 = key_edge(ks + 1, delta);
        const double Qv = e0 + (e1 - e0) * (T - (double)before) / (double)h[ks];
        const double r = Qv / kQuartile, v = r * r - delta * delta / 3.0;
        if (!(v > 0.0)) continue;
        lv[l].v = v; lv[l].ok = true;
    }
}

struct Fit { double sigma, f_max; unsigned levels; };

/* one histogram [64][322] with cens [64] and `whole`, the blocks of whole-numbered pixels (all of them: the data are quantised, delta =
 * s / 2): down the ladder until four levels count; false when even f_max = 1 leaves fewer */
inline bool fit_one(const unsigned long long* hist, const unsigned long long* cens, unsigned long long whole, double s, Fit& out) {
    unsigned long long total = 0;
    for (size_t i = 0; i < (size_t)kLevels * kKeys; i++) total += hist[i];
    const double delta = total && whole == total ? 0.5 * s : 0.0;
    LevelVar lv[kLevels];
    level_variances(hist, delta, lv);
    for (int r = 0; r < kLadder; r++) {
        double Sw = 0.0, Swv = 0.0;
        unsigned used = 0;
        for (int l = 0; l < kLevels; l++) {
            if (!lv[l].ok || (double)cens[l] > kFMax[r] * (double)lv[l].n) continue;
            const double w = (double)lv[l].n / (lv[l].v * lv[l].v);
            Sw += w; Swv += w * lv[l].v;
            used++;
        }
        if (used >= kMinLevels) {
            out.sigma = std::sqrt(Swv / Sw) / s; out.f_max = kFMax[r]; out.levels = used;
            return true;
        }
    }
    return false;
}

} /* namespace lfbm5d_clip */
#endif
