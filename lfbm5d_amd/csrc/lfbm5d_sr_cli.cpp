/*
 * lfbm5d_sr_cli.cpp -- `LFBM5Dsuperres`: light-field super-resolution on the GPU backend (superres_LF, run_bm5d.h: the scheme of
 * SR-LFBM5D with the operators of include/lfbm5d.h -- not the output of the reference's SR branch).
 *
 *   LFBM5Dsuperres LFLowDir SAIName sep awidth aheight sIdxStart tIdxStart aswSize row|col scale bicubic|gaussian blurSigma
 *       iterations sigmaStart sigmaEnd LFOutDir NHard nSimHard nDispHard kHard pHard id|dct|bior id|dct|sadct hw|haar|dct useSD
 *       rgb|yuv|ycbcr|opp [LFSourceDir resultsFile]
 *
 * Reads <LFLowDir>/<name><sep><ss><sep><tt>.png, writes SAIs of `scale` times the size to LFOutDir under the same names.  0 for
 * iterations / sigmaStart / sigmaEnd selects the library's defaults for the scale.  With LFSourceDir (the high-resolution ground
 * truth) it prints the PSNR of plain bicubic interpolation and of the result and appends both to resultsFile in the report format
 * of LFBM5Ddenoising.  Environment: LFBM5D_REPORT_SSIM=1 adds the average SSIM next to both average PSNRs and an SSIM block behind
 * each PSNR block of resultsFile (cli_quality.h: on the images as the files hold them); any other value is an error; unset, the
 * output is unchanged.
 */
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/lfbm5d.h"
#include "png_min.h"
#include "run_bm5d.h"
#include "cli_quality.h"

using namespace std;

namespace {

string sai_path(const char* dir, const char* name, const char* sep, unsigned s, unsigned t) {
    ostringstream o;
    o << dir << "/" << name << sep << setfill('0') << setw(2) << s << sep << setfill('0') << setw(2) << t << ".png";
    return o.str();
}

unsigned sai_index(unsigned ang_major, unsigned aw, unsigned ah, unsigned s, unsigned t) { return ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah; }

/* load_LF of LFBM5Ddenoising (utilities_LF.cpp:72-167), one SAI after the other */
int load_LF(const char* dir, const char* name, const char* sep, vector<vector<float> >& LF, vector<unsigned>& mask, unsigned ang_major,
            unsigned aw, unsigned ah, unsigned s0, unsigned t0, unsigned& W, unsigned& H, unsigned& C) {
    mask.assign(aw * ah, 0u);
    LF.assign(aw * ah, vector<float>());
    W = H = C = 0;
    for (unsigned s = 0; s < ah; s++)
        for (unsigned t = 0; t < aw; t++) {
            const string p = sai_path(dir, name, sep, s + s0, t + t0);
            vector<float> img;
            size_t w, h, c;
            if (!png_read_planar_f32(p, img, w, h, c)) { cout << "error :: " << p << " not found or not a correct png image." << endl; return EXIT_FAILURE; }
            if (c == 2) c = 1;
            if (c > 2) {
                size_t k = 0; float acc = 0.0f;
                while (k < w * h && img[k] == img[w * h + k] && img[k] == img[2 * w * h + k]) { acc += img[k] + img[w * h + k] + img[2 * w * h + k]; k++; }
                c = (k == w * h && acc > 0.0f) ? 1 : 3;
            }
            if (!W) { W = (unsigned)w; H = (unsigned)h; C = (unsigned)c; }
            if (w != W || h != H || c != C) { cout << "error :: SAIs of different sizes" << endl; return EXIT_FAILURE; }
            const unsigned st = sai_index(ang_major, aw, ah, s, t);
            LF[st].assign(img.begin(), img.begin() + w * h * c);
            for (float v : LF[st]) if (v) { mask[st] = 1; break; }
        }
    cout << " Light field size :" << endl << " - awidth         = " << aw << endl << " - aheight        = " << ah << endl
         << " - width          = " << W << endl << " - height         = " << H << endl << " - nb of channels = " << C << endl;
    return EXIT_SUCCESS;
}

int save_LF(const char* dir, const char* name, const char* sep, const vector<vector<float> >& LF, unsigned ang_major, unsigned aw, unsigned ah,
            unsigned s0, unsigned t0, unsigned W, unsigned H, unsigned C) {
    for (unsigned s = 0; s < ah; s++)
        for (unsigned t = 0; t < aw; t++) {
            const unsigned st = sai_index(ang_major, aw, ah, s, t);
            const string p = sai_path(dir, name, sep, s + s0, t + t0);
            vector<float> tmp((size_t)W * H * C, 0.0f);
            if (LF[st].size() == tmp.size())
                for (size_t k = 0; k < tmp.size(); k++) tmp[k] = LF[st][k] > 255.0f ? 255.0f : (LF[st][k] < 0.0f ? 0.0f : LF[st][k]);
            if (!png_write_planar_f32(p, tmp.data(), W, H, C)) { cout << "... failed to save png image " << p << endl; return EXIT_FAILURE; }
        }
    return EXIT_SUCCESS;
}

/* compute_psnr_LF (utilities_LF.cpp:639-692) */
void psnr_LF(const vector<vector<float> >& A, const vector<vector<float> >& B, const vector<unsigned>& mask, vector<float>& psnr, float& avg_p,
             float& std_p, vector<float>& rmse, float& avg_r, float& std_r) {
    const size_t n = mask.size();
    psnr.assign(n, 0.0f); rmse.assign(n, 0.0f);
    float cnt = 0, sp = 0, sr = 0;
    for (size_t st = 0; st < n; st++) {
        if (!mask[st]) continue;
        float tmp = 0.0f;
        for (size_t k = 0; k < A[st].size(); k++) tmp += (A[st][k] - B[st][k]) * (A[st][k] - B[st][k]);
        rmse[st] = sqrtf(tmp / (float)A[st].size());
        psnr[st] = 20.0f * log10f(255.0f / rmse[st]);
        cnt++; sp += psnr[st]; sr += rmse[st];
    }
    avg_p = sp / cnt; avg_r = sr / cnt;
    float vp = 0, vr = 0;
    for (size_t st = 0; st < n; st++) if (mask[st]) { vp += (psnr[st] - avg_p) * (psnr[st] - avg_p); vr += (rmse[st] - avg_r) * (rmse[st] - avg_r); }
    std_p = sqrtf(vp / cnt); std_r = sqrtf(vr / cnt);
}

/* write_psnr_LF (utilities_LF.cpp:782-869) */
void write_psnr(const char* file, const char* what, const vector<unsigned>& mask, unsigned ang_major, unsigned aw, unsigned ah,
                const vector<float>& psnr, float avg_p, float std_p, const vector<float>& rmse, float avg_r, float std_r) {
    ofstream f(file, ios::out | ios::app);
    if (!f) { cout << "Can't open " << file << endl; return; }
    f << endl << "******************************************" << endl;
    f << "-> Average PSNR " << what << " = " << avg_p << endl << "-> Standard deviation PSNR " << what << " = " << std_p << endl;
    f << "PSNR for all " << what << " SAIs:" << endl;
    for (unsigned s = 0; s < ah; s++) { for (unsigned t = 0; t < aw; t++) { const unsigned st = sai_index(ang_major, aw, ah, s, t); if (mask[st]) f << psnr[st] << " "; else f << "No SAI "; } f << endl; }
    f << endl << "-> Average RMSE " << what << " = " << avg_r << endl << "-> Standard deviation RMSE " << what << " = " << std_r << endl;
    f << "RMSE for all " << what << " SAIs:" << endl;
    for (unsigned s = 0; s < ah; s++) { for (unsigned t = 0; t < aw; t++) f << rmse[sai_index(ang_major, aw, ah, s, t)] << " "; f << endl; }
    f << "******************************************" << endl;
}

/* U of include/lfbm5d.h on the host (the library's own tap table), for the bicubic line of the report */
bool bicubic_LF(const vector<vector<float> >& low, const vector<unsigned>& mask, vector<vector<float> >& high, unsigned scale, unsigned w, unsigned h,
                unsigned C) {
    lfbm5d_sr_params sr;
    if (lfbm5d_sr_defaults(scale, &sr) != 0) return false;
    const unsigned W = w * scale, H = h * scale;
    unsigned T = 0;
    vector<int> fx(W), fy(H);
    vector<float> wx((size_t)W * 4), wy((size_t)H * 4);
    if (lfbm5d_sr_taps(LFBM5D_SR_UP, &sr, w, fx.data(), wx.data(), &T, (unsigned)wx.size()) != 0 || T != 4) return false;
    if (lfbm5d_sr_taps(LFBM5D_SR_UP, &sr, h, fy.data(), wy.data(), &T, (unsigned)wy.size()) != 0 || T != 4) return false;
    auto clampi = [](int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
    high.assign(low.size(), vector<float>());
    vector<float> tmp((size_t)h * W);
    for (size_t st = 0; st < low.size(); st++) {
        if (!mask[st]) continue;
        high[st].assign((size_t)C * W * H, 0.0f);
        for (unsigned c = 0; c < C; c++) {
            const float* in = &low[st][(size_t)c * w * h];
            float* out = &high[st][(size_t)c * W * H];
            for (unsigned y = 0; y < h; y++)
                for (unsigned X = 0; X < W; X++) {
                    float acc = 0.0f;
                    for (int t = 0; t < 4; t++) acc = fmaf(wx[(size_t)X * 4 + t], in[(size_t)y * w + clampi(fx[X] + t, (int)w)], acc);
                    tmp[(size_t)y * W + X] = acc;
                }
            for (unsigned Y = 0; Y < H; Y++)
                for (unsigned X = 0; X < W; X++) {
                    float acc = 0.0f;
                    for (int t = 0; t < 4; t++) acc = fmaf(wy[(size_t)Y * 4 + t], tmp[(size_t)clampi(fy[Y] + t, (int)h) * W + X], acc);
                    out[(size_t)Y * W + X] = acc;
                }
        }
    }
    return true;
}

int tau(const char* s, int which) {
    if (!strcmp(s, "id")) return LFBM5D_ID;
    if (!strcmp(s, "dct")) return LFBM5D_DCT;
    if (which == 2 && !strcmp(s, "bior")) return LFBM5D_BIOR;
    if (which == 4 && !strcmp(s, "sadct")) return LFBM5D_SADCT;
    if (which == 5 && !strcmp(s, "hw")) return LFBM5D_HADAMARD;
    if (which == 5 && !strcmp(s, "haar")) return LFBM5D_HAAR;
    return -1;
}

void usage(const char* a0) {
    cout << "usage: " << a0 << " LFLowDir SAIName sep awidth aheight sIdxStart tIdxStart aswSize row|col scale bicubic|gaussian blurSigma "
            "iterations sigmaStart sigmaEnd LFOutDir NHard nSimHard nDispHard kHard pHard id|dct|bior id|dct|sadct hw|haar|dct useSD "
            "rgb|yuv|ycbcr|opp [LFSourceDir resultsFile]" << endl;
}

} // namespace

int main(int argc, char** argv) {
    if (argc != 27 && argc != 29) { usage(argv[0]); cout << "Problem while reading parameters from command line !" << endl; return EXIT_FAILURE; }
    int a = 1;
    const char* d_low = argv[a++]; const char* name = argv[a++]; const char* sep_in = argv[a++];
    const char* sep = strcmp(sep_in, "none") ? sep_in : "";
    if (!strcmp(name, "none")) name = "";
    const unsigned aw = atoi(argv[a++]), ah = atoi(argv[a++]), s0 = atoi(argv[a++]), t0 = atoi(argv[a++]), an = atoi(argv[a++]);
    const char* maj = argv[a++];
    const unsigned ang_major = !strcmp(maj, "row") ? LFBM5D_ROWMAJOR : !strcmp(maj, "col") ? LFBM5D_COLMAJOR : 0;
    const unsigned scale = atoi(argv[a++]);
    const char* kn = argv[a++];
    const int kernel = !strcmp(kn, "bicubic") ? LFBM5D_SR_BICUBIC : !strcmp(kn, "gaussian") ? LFBM5D_SR_GAUSSIAN : -1;
    const float blur = (float)atof(argv[a++]);
    const unsigned iters = atoi(argv[a++]);
    const float sig0 = (float)atof(argv[a++]), sig1 = (float)atof(argv[a++]);
    const char* d_out = argv[a++];
    const unsigned N = atoi(argv[a++]), nSim = atoi(argv[a++]), nDisp = atoi(argv[a++]), k = atoi(argv[a++]), p = atoi(argv[a++]);
    const int t2 = tau(argv[a++], 2), t4 = tau(argv[a++], 4), t5 = tau(argv[a++], 5);
    const unsigned sd = atoi(argv[a++]);
    const char* csn = argv[a++];
    const int cs = !strcmp(csn, "rgb") ? LFBM5D_RGB : !strcmp(csn, "yuv") ? LFBM5D_YUV : !strcmp(csn, "ycbcr") ? LFBM5D_YCBCR : !strcmp(csn, "opp") ? LFBM5D_OPP : -1;
    const char* d_src = argc == 29 ? argv[a++] : nullptr;
    const char* results = argc == 29 ? argv[a++] : nullptr;
    if (!ang_major || cs < 0 || kernel < 0 || t2 < 0 || t4 < 0 || t5 < 0 || scale < 2 || scale > 4) {
        usage(argv[0]); cout << "Problem while reading parameters from command line !" << endl; return EXIT_FAILURE;
    }

    const int qmode = cli_quality::ssim_mode();
    if (qmode < 0) return EXIT_FAILURE;

    vector<vector<float> > LF_low, LF_high, LF_src, LF_bic;
    vector<unsigned> mask, mask_src;
    unsigned w = 0, h = 0, C = 0;
    if (load_LF(d_low, name, sep, LF_low, mask, ang_major, aw, ah, s0, t0, w, h, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    const unsigned W = w * scale, H = h * scale;
    if (d_src) {
        unsigned Ws = 0, Hs = 0, Cs = 0;
        if (load_LF(d_src, name, sep, LF_src, mask_src, ang_major, aw, ah, s0, t0, Ws, Hs, Cs) != EXIT_SUCCESS) return EXIT_FAILURE;
        if (Ws != W || Hs != H || Cs != C) { cout << "error :: the source light field is not scale times the low-resolution one" << endl; return EXIT_FAILURE; }
    }
    cout << endl << " ---> Running LFBM5D super-resolution (x" << scale << ") <--- " << endl << endl;
    if (superres_LF(LF_low, mask, LF_high, ang_major, aw, ah, an, w, h, C, scale, (unsigned)kernel, blur, iters, sig0, sig1, 2.7f, N, nSim, nDisp, k, p,
                    sd != 0, t2, t4, t5, cs) != EXIT_SUCCESS) return EXIT_FAILURE;
    if (d_src) {
        if (!bicubic_LF(LF_low, mask, LF_bic, scale, w, h, C)) { cout << "bicubic interpolation failed" << endl; return EXIT_FAILURE; }
        vector<float> ps, rm; float sp = 0, ar = 0, sr = 0;
        cli_quality::Avg ap_b, ap_s;
        cli_quality::Block qb;
        psnr_LF(LF_src, LF_bic, mask, ps, ap_b.psnr, sp, rm, ar, sr);
        write_psnr(results, "bicubic", mask, ang_major, aw, ah, ps, ap_b.psnr, sp, rm, ar, sr);
        if (qmode) { if (!cli_quality::compute(LF_src, LF_bic, mask, W, H, C, ap_b, qb)) return EXIT_FAILURE; cli_quality::write(results, "bicubic", mask, ang_major, aw, ah, qb); }
        psnr_LF(LF_src, LF_high, mask, ps, ap_s.psnr, sp, rm, ar, sr);
        write_psnr(results, "super-resolved", mask, ang_major, aw, ah, ps, ap_s.psnr, sp, rm, ar, sr);
        if (qmode) { if (!cli_quality::compute(LF_src, LF_high, mask, W, H, C, ap_s, qb)) return EXIT_FAILURE; cli_quality::write(results, "super-resolved", mask, ang_major, aw, ah, qb); }
        cout << endl << "Average PSNR:" << endl << "- Bicubic light field: " << ap_b << endl << "- Super-resolved light field: " << ap_s << endl << endl;
    }
    cout << "Save super-resolved light field..." << endl;
    if (save_LF(d_out, name, sep, LF_high, ang_major, aw, ah, s0, t0, W, H, C) != EXIT_SUCCESS) return EXIT_FAILURE;
    return EXIT_SUCCESS;
}
