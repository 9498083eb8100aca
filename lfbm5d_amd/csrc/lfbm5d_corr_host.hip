/*
 * lfbm5d_corr_host.hip -- spatially correlated noise (include/lfbm5d_corr.h), the part that needs neither a GPU nor a context: the
 * checks of an autocorrelation, the autocorrelation of filtered white noise, the variance table of a 2-D transform.  Plain C++ (no
 * kernel, no HIP call), so that a host compiler can build it alone, with sanitizers.
 */
#include "../../include/lfbm5d.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace {

thread_local std::string t_corr_error;
int host_fail(const std::string& m) { t_corr_error = m; return 1; }

constexpr int L = LFBM5D_CORR_LAGS, LH = LFBM5D_CORR_LAGS / 2;

/* one analysis level of bior1.5 on the first n1 of x (stride `step`), periodic extension, as the kernels run it: sample j of the
 * extension is x[(j - 4) mod n1]; low[j] = sum_t ext[t + 2 j] lpd[t] in front, high[j] behind */
void bior_level(double* x, unsigned n1, unsigned step) {
    static const double cn = 1.0 / (std::sqrt(2.0) * 128.0);
    static const double lpd[10] = {3 * cn, -3 * cn, -22 * cn, 22 * cn, 128 * cn, 128 * cn, 22 * cn, -22 * cn, -3 * cn, 3 * cn};
    const double r = 1.0 / std::sqrt(2.0);
    double out[32];
    const unsigned h = n1 / 2;
    for (unsigned j = 0; j < h; j++) {
        double lo = 0.0;
        for (unsigned t = 0; t < 10; t++) lo += lpd[t] * x[((t + 2 * j + 8 * n1 - 4) % n1) * step];
        out[j] = lo;
        out[h + j] = -r * x[((4 + 2 * j + 8 * n1 - 4) % n1) * step] + r * x[((5 + 2 * j + 8 * n1 - 4) % n1) * step];
    }
    for (unsigned j = 0; j < n1; j++) x[j * step] = out[j];
}

/* M [k2][k2]: row pq is the basis function of coefficient pq over the row-major patch */
void transform_matrix(unsigned tau2, unsigned k, std::vector<double>& M) {
    const unsigned k2 = k * k;
    M.assign((size_t)k2 * k2, 0.0);
    if (tau2 == LFBM5D_DCT) {
        std::vector<double> D((size_t)k * k);
        for (unsigned u = 0; u < k; u++)
            for (unsigned j = 0; j < k; j++)
                D[(size_t)u * k + j] = std::cos(3.14159265358979323846 * ((double)j + 0.5) * (double)u / (double)k) * std::sqrt(2.0 / (double)k) * (u == 0 ? 1.0 / std::sqrt(2.0) : 1.0);
        for (unsigned p = 0; p < k; p++)
            for (unsigned q = 0; q < k; q++)
                for (unsigned y = 0; y < k; y++)
                    for (unsigned x = 0; x < k; x++) M[(size_t)(p * k + q) * k2 + y * k + x] = D[(size_t)p * k + y] * D[(size_t)q * k + x];
        return;
    }
    /* bior1.5: the transform of every unit patch is a column of M */
    std::vector<double> patch(k2);
    for (unsigned i = 0; i < k2; i++) {
        std::fill(patch.begin(), patch.end(), 0.0);
        patch[i] = 1.0;
        for (unsigned n1 = k; n1 > 1; n1 /= 2) {
            for (unsigned y = 0; y < n1; y++) bior_level(&patch[(size_t)y * k], n1, 1);   /* rows of the leading block ... */
            for (unsigned x = 0; x < n1; x++) bior_level(&patch[x], n1, k);               /* ... then its columns */
        }
        for (unsigned pq = 0; pq < k2; pq++) M[(size_t)pq * k2 + i] = patch[pq];
    }
}

} /* namespace */

extern "C" {

const char* lfbm5d_corr_error(void) { return t_corr_error.c_str(); }

int lfbm5d_corr_check(const double* acf) {
    const std::string who = "lfbm5d_corr: ";
    if (!acf) return host_fail(who + "NULL pointer for the autocorrelation");
    for (int i = 0; i < L * L; i++)
        if (!std::isfinite(acf[i]) || std::fabs(acf[i]) > 1.0)
            return host_fail(who + "acf[" + std::to_string(i / L) + "][" + std::to_string(i % L) + "] = " + std::to_string(acf[i]) + " is not a finite value of magnitude at most 1");
    if (acf[LH * L + LH] != 1.0) return host_fail(who + "the autocorrelation must be 1 at lag 0 (acf[3][3] = " + std::to_string(acf[LH * L + LH]) + ")");
    for (int i = 0; i < L * L; i++)
        if (acf[i] != acf[L * L - 1 - i])
            return host_fail(who + "the autocorrelation must be point-symmetric (acf[" + std::to_string(i / L) + "][" + std::to_string(i % L) + "] differs from its mirror)");
    return 0;
}

int lfbm5d_corr_from_kernel(const double* g, unsigned gh, unsigned gw, double* acf_out) {
    const std::string who = "lfbm5d_corr_from_kernel: ";
    if (!g || !acf_out) return host_fail(who + "NULL pointer for a required buffer");
    if (gh < 1 || gh > (unsigned)L || gw < 1 || gw > (unsigned)L) return host_fail(who + "the taps must be 1..7 rows of 1..7 values");
    double e = 0.0;
    for (unsigned i = 0; i < gh * gw; i++) {
        if (!std::isfinite(g[i])) return host_fail(who + "tap " + std::to_string(i) + " is not finite");
        e += g[i] * g[i];
    }
    if (!(e > 0.0) || !std::isfinite(e)) return host_fail(who + "the taps are all zero (or their energy overflows)");
    for (int dy = 0; dy <= LH; dy++)
        for (int dx = (dy == 0 ? 0 : -LH); dx <= LH; dx++) {
            double s = 0.0;
            for (int y = 0; y < (int)gh; y++)
                for (int x = 0; x < (int)gw; x++) {
                    const int y2 = y + dy, x2 = x + dx;
                    if (y2 < (int)gh && x2 >= 0 && x2 < (int)gw) s += g[y * gw + x] * g[y2 * gw + x2];
                }
            double r = (dy == 0 && dx == 0) ? 1.0 : s / e;
            r = std::max(-1.0, std::min(1.0, r));   /* (Cauchy-Schwarz up to rounding) */
            acf_out[(LH + dy) * L + LH + dx] = r;
            acf_out[(LH - dy) * L + LH - dx] = r;
        }
    return 0;
}

int lfbm5d_corr_table(const double* acf, unsigned tau_2D, unsigned k, float* s_out, float* v_out, unsigned* clamped) {
#pragma clang fp contract(off)
    const std::string who = "lfbm5d_corr_table: ";
    if (lfbm5d_corr_check(acf)) return 1;
    if (tau_2D != LFBM5D_ID && tau_2D != LFBM5D_DCT && tau_2D != LFBM5D_BIOR) return host_fail(who + "tau_2D must be id, dct or bior");
    if (k < 2 || k > 32) return host_fail(who + "patch size k outside 2..32");
    if (tau_2D == LFBM5D_BIOR && (k & (k - 1))) return host_fail(who + "bior1.5 needs a power-of-two patch size");
    const unsigned k2 = k * k;
    unsigned n_clamped = 0;
    std::vector<double> M;
    if (tau_2D != LFBM5D_ID) transform_matrix(tau_2D, k, M);
    for (unsigned pq = 0; pq < k2; pq++) {
        double v = 1.0;                      /* id: R's diagonal */
        if (tau_2D != LFBM5D_ID) {
            const double* b = &M[(size_t)pq * k2];
            double num = 0.0, den = 0.0;
            for (int y = 0; y < (int)k; y++)
                for (int x = 0; x < (int)k; x++) {
                    double rb = 0.0;         /* (R b)[y][x], the lags in ascending order */
                    for (int dy = -LH; dy <= LH; dy++)
                        for (int dx = -LH; dx <= LH; dx++) {
                            const int y2 = y + dy, x2 = x + dx;
                            if (y2 >= 0 && y2 < (int)k && x2 >= 0 && x2 < (int)k) rb += acf[(LH + dy) * L + LH + dx] * b[y2 * k + x2];
                        }
                    num += b[y * k + x] * rb;
                    den += b[y * k + x] * b[y * k + x];
                }
            v = num / den;
        }
        if (!(v >= LFBM5D_CORR_FLOOR)) { v = LFBM5D_CORR_FLOOR; n_clamped++; }
        if (v_out) v_out[pq] = (float)v;
        if (s_out) s_out[pq] = (float)std::sqrt(v);
    }
    if (clamped) *clamped = n_clamped;
    return 0;
}

} /* extern "C" */

