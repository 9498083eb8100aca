/*
 * dropin_refusals.cpp -- what the drop-in (lfbm5d_amd/csrc/run_bm5d.h, run_bm3d_lf.h) returns and prints when it is handed bad
 * arguments.  For each of its 30 functions that take a light field or a mask, three calls on 2 x 2 SAIs of 16 x 16 x 3, zero-filled:
 *   a  the mask one entry short                         (refused before a context exists: runs without a GPU)
 *   b  a correct count, one non-empty SAI one float short
 *   c  correct vectors with chnls = 2                   (the library refuses: the backend line)
 * A function without such an argument gets the nearest call (views_from_gains has no light field: b is a good call, c is chnls = 2,
 * which it accepts; the BM3D functions take a short SAI for an empty one and filter).  One JSON object per line: id = name/case,
 * rc = the return value, out = what the call wrote to std::cout.  `dropin_refusals a` runs the a cases, `dropin_refusals bc` the rest.
 * tests/test_dropin_refusals.py compares the lines with tests/golden/dropin_refusals.json.
 */
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/lfbm5d.h"
#include "../lfbm5d_amd/csrc/run_bm3d_lf.h"
#include "../lfbm5d_amd/csrc/run_bm5d.h"

namespace {

typedef std::vector<std::vector<float> > LF;
const unsigned AW = 2, AH = 2, AN = 1, W = 16, H = 16, ROW = LFBM5D_ROWMAJOR, CS = LFBM5D_OPP;
/* N, nSim, nDisp, k, p, useSD, tau_2D, tau_4D, tau_5D of the two steps; N, n, k, p of BM3D */
#define HARD 8u, 8u, 3u, 8u, 3u, false, (unsigned)LFBM5D_DCT, (unsigned)LFBM5D_SADCT, (unsigned)LFBM5D_HAAR
#define WIEN 8u, 8u, 3u, 8u, 3u, false, (unsigned)LFBM5D_DCT, (unsigned)LFBM5D_SADCT, (unsigned)LFBM5D_HAAR
#define BM3D 6u, 6u, 8u, 8u, 8u, 8u, 3u, 3u, false, false, (unsigned)LFBM5D_BIOR, (unsigned)LFBM5D_DCT, 2.7f, CS

struct Field {
    unsigned C;
    LF lf, basic, den;
    std::vector<unsigned> mask, none;
    std::vector<std::vector<unsigned char> > flags;
    explicit Field(char k)
        : C(k == 'c' ? 2u : 3u), lf(AW * AH, std::vector<float>(W * H * C, 0.0f)), mask(k == 'a' ? AW * AH - 1 : AW * AH, 1u), none(AW * AH, 0u),
          flags(AW * AH, std::vector<unsigned char>(W * H * C, 0)) {
        if (k == 'b') lf[1].pop_back();
    }
};

std::string which;

template <class F> void three(const char* name, F call) {
    for (char k : which) {
        Field f(k);
        std::ostringstream cap;
        std::streambuf* const old = std::cout.rdbuf(cap.rdbuf());
        const int rc = call(f);
        std::cout.rdbuf(old);
        std::string esc;
        for (char ch : cap.str()) {
            if (ch == '\n') esc += "\\n";
            else if (ch == '"' || ch == '\\') { esc += '\\'; esc += ch; }
            else esc += ch;
        }
        std::cout << "{\"id\": \"" << name << "/" << k << "\", \"rc\": " << rc << ", \"out\": \"" << esc << "\"}" << std::endl;
    }
}

} // namespace

int main(int argc, char** argv) {
    if (argc != 2 || (std::string(argv[1]) != "a" && std::string(argv[1]) != "bc")) { std::fprintf(stderr, "usage: dropin_refusals a|bc\n"); return 2; }
    which = argv[1];
    float s = 25.0f; double a = 1.0, b = 4.0, d = 0.0; unsigned u = 0, v = 0, w = 0, x = 0; int i = 0, j = 0; unsigned long long p = 0, q = 0;
    std::vector<double> table, gains(3 * AW * AH, 1.0), acf(49, 0.0);
    acf[24] = 1.0;
    std::vector<float> ws, v1, v2, v3; float f1, f2, f3, f4, f5, f6;
    std::vector<unsigned> state;
    double t3[3]; unsigned long long c6[6];

    three("run_bm5d_1st_step", [&](Field& f) { return run_bm5d_1st_step(s, 2.7f, f.lf, f.mask, f.basic, ROW, AW, AH, AN, W, H, f.C, HARD, CS, 1); });
    three("run_bm5d_2nd_step", [&](Field& f) { f.basic.assign(AW * AH, std::vector<float>(W * H * f.C, 0.0f));
                                               return run_bm5d_2nd_step(s, f.lf, f.mask, f.basic, f.den, ROW, AW, AH, AN, W, H, f.C, WIEN, CS, 1); });
    three("run_bm5d", [&](Field& f) { return run_bm5d(s, 2.7f, f.lf, f.mask, f.basic, f.den, ROW, AW, AH, AN, AN, W, H, f.C, HARD, WIEN, CS, 1); });
    three("noise_level_LF", [&](Field& f) { return noise_level_LF(f.lf, f.mask, W, H, f.C, s); });
    three("impulse_repair_LF", [&](Field& f) { return impulse_repair_LF(f.lf, f.mask, W, H, f.C, 8.0, p, q, t3); });
    three("pg_estimate_LF", [&](Field& f) { return pg_estimate_LF(f.lf, f.mask, W, H, f.C, a, b); });
    a = 1.0; b = 4.0;
    three("pg_forward_LF", [&](Field& f) { return pg_forward_LF(1.0, 4.0, f.lf, f.mask, W, H, f.C, s); });
    three("pg_inverse_LF", [&](Field& f) { return pg_inverse_LF(1.0, 4.0, f.lf, f.mask, W, H, f.C); });
    three("denoise_pg_LF", [&](Field& f) { a = 1.0; b = 4.0;
                                           return denoise_pg_LF(a, b, false, s, 2.7f, f.lf, f.mask, f.basic, f.den, ROW, AW, AH, AN, AN, W, H, f.C, HARD, WIEN, CS, 1); });
    three("noise_level_clipped_LF", [&](Field& f) { return noise_level_clipped_LF(f.lf, f.mask, W, H, f.C, 0.0, 255.0, s, u, d); });
    three("declip_LF", [&](Field& f) { return declip_LF(25.0, 0.0, 255.0, f.lf, f.mask, W, H, f.C); });
    three("denoise_clipped_LF", [&](Field& f) { s = 25.0f;
                                                return denoise_clipped_LF(s, 0.0, 255.0, 2.7f, f.lf, f.mask, f.basic, f.den, ROW, AW, AH, AN, AN, W, H, f.C, HARD, WIEN, CS, 1); });
    three("pgclip_estimate_LF", [&](Field& f) { return pgclip_estimate_LF(f.lf, f.mask, W, H, f.C, 0.0, 255.0, a, b, u, d); });
    three("pgclip_forward_LF", [&](Field& f) { return pgclip_forward_LF(0.5, 4.0, 0.0, 255.0, f.lf, f.mask, W, H, f.C, s); });
    three("pgclip_inverse_LF", [&](Field& f) { return pgclip_inverse_LF(0.5, 4.0, 0.0, 255.0, f.lf, f.mask, W, H, f.C); });
    three("denoise_pgclip_LF", [&](Field& f) { a = 0.5; b = 4.0;
                                               return denoise_pgclip_LF(a, b, 0.0, 255.0, false, s, u, d, 2.7f, f.lf, f.mask, f.basic, f.den, ROW, AW, AH, AN, AN, W, H,
                                                                        f.C, HARD, WIEN, CS, 1); });
    three("quality_LF", [&](Field& f) { f.basic.assign(AW * AH, std::vector<float>(W * H * f.C, 0.0f));
                                        return quality_LF(f.lf, f.basic, f.mask, W, H, f.C, v1, f1, f2, v2, f3, f4, v3, f5, f6); });
    three("inpaint_LF", [&](Field& f) { return inpaint_LF(f.lf, f.flags, f.mask, ROW, AW, AH, AN, W, H, f.C, 0, 0.0f, 0.0f, 0.0f, 2.7f, HARD, CS, p, q, u); });
    three("view_synth_LF", [&](Field& f) { return view_synth_LF(f.lf, f.mask, f.none, ROW, AW, AH, AN, W, H, f.C, -1, -1, -1, 0, 0.0f, 0.0f, 0.0f, 2.7f, HARD, CS,
                                                                u, v, i, j); });
    three("repair_LF", [&](Field& f) { return repair_LF(f.lf, f.flags, f.mask, f.none, ROW, AW, AH, AN, W, H, f.C, -1, -1, -1, -1, 0, 0.0f, 0.0f, 0.0f, 2.7f, HARD,
                                                        CS, c6, i, j); });
    three("consist_LF", [&](Field& f) { std::vector<std::vector<unsigned char> > out;
                                        return consist_LF(f.lf, f.mask, std::vector<unsigned>(), ROW, AW, AH, W, H, f.C, -1, -1, -1, -1, -1, -1.0, -1.0, -1.0, out,
                                                          state, p, q, u, v, w, t3); });
    three("equalise_LF", [&](Field& f) { return equalise_LF(f.lf, f.mask, f.basic, ROW, AW, AH, W, H, f.C, -1, -1, -1, -1, -1, -1, -1, -1.0, -1.0, -1.0, table,
                                                            state, u, v, w, x, d, a, b); });
    three("apply_gains_LF", [&](Field& f) { return apply_gains_LF(f.lf, f.mask, gains, false, AW, AH, W, H, f.C); });
    three("denoise_views_LF", [&](Field& f) { table.assign(AW * AH, 25.0);
                                              return denoise_views_LF(table, ws, 2.7f, f.lf, f.mask, f.basic, f.den, ROW, AW, AH, AN, AN, W, H, f.C, HARD, WIEN, CS, 1); });
    three("denoise_corr_LF", [&](Field& f) { return denoise_corr_LF(acf, 25.0f, 2.7f, f.lf, f.mask, f.basic, f.den, ROW, AW, AH, AN, AN, W, H, f.C, HARD, WIEN, CS, 1); });
    three("corr_measure_LF", [&](Field& f) { std::vector<double> m;
                                             return corr_measure_LF(f.lf, f.mask, W, H, f.C, 0, 0.0, m, d); });
    three("views_from_gains", [&](Field& f) { return views_from_gains(25.0, gains, f.C, f.mask, table); });
    three("bm3d_views_LF", [&](Field& f) { table.assign(AW * AH, 25.0);
                                           return bm3d_views_LF(table, f.lf, f.mask, f.basic, f.den, W, H, f.C, BM3D); });
    three("superres_LF", [&](Field& f) { return superres_LF(f.lf, f.mask, f.basic, ROW, AW, AH, AN, W, H, f.C, 2, LFBM5D_SR_BICUBIC, 0.0f, 1, 0.0f, 0.0f, 2.7f, HARD,
                                                            CS); });
    three("run_bm3d_LF", [&](Field& f) { return run_bm3d_LF(25.0f, f.lf, f.mask, f.basic, f.den, W, H, f.C, BM3D, 1, nullptr); });
    return 0;
}
