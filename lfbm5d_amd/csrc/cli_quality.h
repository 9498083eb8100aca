/*
 * cli_quality.h -- LFBM5D_REPORT_SSIM of the command lines (LFBM5Ddenoising, LFBM3Ddenoising, LFBM5Dsuperres): the average SSIM next
 * to every average PSNR on stdout, and an SSIM block behind every PSNR block of the results file.  The values come from quality_LF
 * (run_bm5d.h: the GPU, double sums) on the light fields AS THE FILES HOLD THEM -- clipped to 0..255 and rounded to 8 bits like
 * save_LF / io_png write them -- so a reader of the PNG files measures the same SSIM; the PSNR beside it stays the reference's
 * float figure on the unrounded data.  Unset, the commands' output is what it was, byte for byte.
 */
#ifndef LFBM5D_CLI_QUALITY_H
#define LFBM5D_CLI_QUALITY_H

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "../../include/lfbm5d.h"
#include "run_bm5d.h"

namespace cli_quality {

/* LFBM5D_REPORT_SSIM: unset -> 0, "1" -> 1, anything else -> -1 (error, message printed); read by the drop-in (run_bm5d.h) */
inline int ssim_mode() { return report_ssim_mode(); }

/* an average PSNR as the commands print it, with the average SSIM behind it when it was computed */
struct Avg { float psnr = 0.0f, ssim = 0.0f; bool has_ssim = false; };
inline std::ostream& operator<<(std::ostream& o, const Avg& a) {
    o << a.psnr;
    if (a.has_ssim) o << " (SSIM " << a.ssim << ")";
    return o;
}

inline std::vector<std::vector<float> > as_written(const std::vector<std::vector<float> >& LF) {
    std::vector<std::vector<float> > q(LF);
    for (auto& img : q)
        for (float& v : img) { const float c = v > 255.0f ? 255.0f : (v < 0.0f ? 0.0f : v); v = (float)(unsigned char)(c + 0.5f); }
    return q;
}

/* the SSIM block of one light field: per SAI, average and standard deviation */
struct Block { std::vector<float> sai; float avg = 0.0f, sd = 0.0f; };

/* SSIM of B against A (quality_LF) into blk and avg.ssim; false = the GPU backend failed (message on stdout) */
inline bool compute(const std::vector<std::vector<float> >& A, const std::vector<std::vector<float> >& B, const std::vector<unsigned>& mask,
                    unsigned W, unsigned H, unsigned C, Avg& avg, Block& blk) {
    std::vector<float> ps, rm;
    float ap, sp, ar, sr;
    if (quality_LF(as_written(A), as_written(B), mask, W, H, C, ps, ap, sp, rm, ar, sr, blk.sai, blk.avg, blk.sd) != EXIT_SUCCESS) return false;
    avg.ssim = blk.avg; avg.has_ssim = true;
    return true;
}

/* the block, in the PSNR grid's layout, at the end of the results file (behind the PSNR block write_psnr has just appended) */
inline void write(const char* file, const char* what, const std::vector<unsigned>& mask, unsigned ang_major, unsigned aw, unsigned ah,
                  const Block& blk) {
    std::ofstream f(file, std::ios::out | std::ios::app);
    if (!f) { std::cout << "Can't open " << file << std::endl; return; }
    f << std::endl << "******************************************" << std::endl;
    f << "-> Average SSIM " << what << " = " << blk.avg << std::endl << "-> Standard deviation SSIM " << what << " = " << blk.sd << std::endl;
    f << "SSIM for all " << what << " SAIs:" << std::endl;
    for (unsigned s = 0; s < ah; s++) {
        for (unsigned t = 0; t < aw; t++) {
            const unsigned st = ang_major == LFBM5D_ROWMAJOR ? s * aw + t : s + t * ah;
            if (mask[st]) f << blk.sai[st] << " "; else f << "No SAI ";
        }
        f << std::endl;
    }
    f << "******************************************" << std::endl;
}

} /* namespace cli_quality */
#endif
