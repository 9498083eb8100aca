// Stand-alone check of the host-only part of the correlated-noise feature (include/lfbm5d_corr.h), built by tests/test_corr.py from this
// file and lfbm5d_amd/csrc/lfbm5d_corr_host.hip with a host compiler and -fsanitize=address,undefined: no GPU, no HIP runtime.
// Exit status 0 and "ok" on stdout when every check holds.
#include "../include/lfbm5d.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

int main() {
    double white[49] = {0};
    white[24] = 1.0;
    CHECK(lfbm5d_corr_check(white) == 0);
    const unsigned taus[3] = {LFBM5D_ID, LFBM5D_DCT, LFBM5D_BIOR};
    for (unsigned tau : taus)
        for (unsigned k = 2; k <= 32; k++) {
            if (tau == LFBM5D_BIOR && (k & (k - 1))) { CHECK(lfbm5d_corr_table(white, tau, k, nullptr, nullptr, nullptr) == 1); continue; }
            std::vector<float> s(k * k, -1.0f), v(k * k, -1.0f);
            unsigned cl = 99;
            CHECK(lfbm5d_corr_table(white, tau, k, s.data(), v.data(), &cl) == 0);
            CHECK(cl == 0);
            for (unsigned i = 0; i < k * k; i++) CHECK(s[i] == 1.0f && v[i] == 1.0f);
        }
    // Gaussian taps of every size up to 7 x 7, several widths: a valid autocorrelation, a table above the floor
    for (unsigned gh = 1; gh <= 7; gh++)
        for (unsigned gw = 1; gw <= 7; gw++)
            for (double width : {0.3, 0.8, 1.2, 3.0}) {
                std::vector<double> g(gh * gw);
                for (unsigned y = 0; y < gh; y++)
                    for (unsigned x = 0; x < gw; x++) {
                        const double dy = y - 0.5 * (gh - 1), dx = x - 0.5 * (gw - 1);
                        g[y * gw + x] = std::exp(-0.5 * (dy * dy + dx * dx) / (width * width));
                    }
                double acf[49];
                CHECK(lfbm5d_corr_from_kernel(g.data(), gh, gw, acf) == 0);
                CHECK(lfbm5d_corr_check(acf) == 0);
                for (unsigned k : {2u, 8u, 11u, 16u}) {
                    std::vector<float> s(k * k), v(k * k);
                    unsigned cl = 0, low = 0;
                    CHECK(lfbm5d_corr_table(acf, LFBM5D_DCT, k, s.data(), v.data(), &cl) == 0);
                    for (unsigned i = 0; i < k * k; i++) { CHECK(v[i] >= 1.0f / 64.0f && std::isfinite(v[i])); low += v[i] == 1.0f / 64.0f; }
                    CHECK(low >= cl);
                }
                std::vector<float> v(16 * 16);
                CHECK(lfbm5d_corr_table(acf, LFBM5D_BIOR, 16, nullptr, v.data(), nullptr) == 0);
            }
    // a delta anywhere in the taps is white
    for (unsigned at = 0; at < 49; at++) {
        double g[49] = {0}, acf[49];
        g[at] = -2.5;
        CHECK(lfbm5d_corr_from_kernel(g, 7, 7, acf) == 0);
        CHECK(std::memcmp(acf, white, sizeof(white)) == 0);
    }
    // refusals leave a message
    double bad[49];
    std::memcpy(bad, white, sizeof(bad));
    bad[0] = 0.5;
    CHECK(lfbm5d_corr_check(bad) == 1 && std::strlen(lfbm5d_corr_error()) > 0);
    CHECK(lfbm5d_corr_table(bad, LFBM5D_DCT, 8, nullptr, nullptr, nullptr) == 1);
    CHECK(lfbm5d_corr_table(white, LFBM5D_DCT, 1, nullptr, nullptr, nullptr) == 1);
    CHECK(lfbm5d_corr_table(white, LFBM5D_DCT, 33, nullptr, nullptr, nullptr) == 1);
    CHECK(lfbm5d_corr_table(white, 6, 8, nullptr, nullptr, nullptr) == 1);
    CHECK(lfbm5d_corr_table(nullptr, LFBM5D_DCT, 8, nullptr, nullptr, nullptr) == 1);
    double zero[4] = {0, 0, 0, 0}, out[49];
    CHECK(lfbm5d_corr_from_kernel(zero, 2, 2, out) == 1);
    CHECK(lfbm5d_corr_from_kernel(zero, 0, 2, out) == 1);
    CHECK(lfbm5d_corr_from_kernel(zero, 8, 2, out) == 1);
    CHECK(lfbm5d_corr_from_kernel(nullptr, 2, 2, out) == 1);
    std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
