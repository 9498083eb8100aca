/*
 * lfbm5d_side_values.h -- what the side stages (impulse repair, inpainting, view synthesis, consistency check) share per value: the
 * 64 x 32 tile of a 256-thread workgroup, the plane's mirror, the bit tests, the 386-key histogram layout, the per-channel thresholds
 * (the key of a value stays with its two users: the impulse repair's min / max spelling and the consistency check's comparisons
 * compile to different instructions, and neither kernel is to change); and the sigma schedule of the refinement loop (lfbm5d_side.h).
 * Host-and-device, and free of HIP headers: tools/consist_host_check.cpp and tools/loop_schedule_check.cpp compile it for the host
 * alone.  Internal.
 */
#ifndef LFBM5D_SIDE_VALUES_H
#define LFBM5D_SIDE_VALUES_H

#include <algorithm>
#include <cmath>
#include <cstddef>

#ifdef __HIPCC__
#define LFBM5D_HD __host__ __device__ __forceinline__
#else
#define LFBM5D_HD inline
#endif

namespace lfbm5d_side {

constexpr int kTW = 64, kTH = 32, kThreads = 256;                 /* a workgroup's tile and its threads */
constexpr int kKeys = 386, kKeyBase = (-12 + 127) << 4;           /* 16 keys per octave of 2^-12 .. 2^12, two end keys (LFBM5D_IMPULSE_KEYS) */

struct Thresholds { float t[3]; };

LFBM5D_HD unsigned bits_of(float x) { return __builtin_bit_cast(unsigned, x); }
LFBM5D_HD bool finite_bits(float x) { return (bits_of(x) & 0x7f800000u) != 0x7f800000u; }

/* coordinate g of the mirrored plane (period 2 (n - 1), no edge repeated) -> 0..n-1; n >= 2; any g (a halo or a shift can exceed a
 * narrow plane) */
LFBM5D_HD int mirror(int g, int n) {
    if ((unsigned)g < (unsigned)n) return g;   /* inside the plane: every lane of an interior tile */
    const int P = 2 * (n - 1);
    g %= P;
    if (g < 0) g += P;
    return g < n ? g : P - g;
}

/* sigma of step k = 1..K of the refinement loop: geometric from sigma_start to sigma_end, never below sigma_noise */
inline float loop_sigma(unsigned k, unsigned K, float sigma_start, float sigma_end, float sigma_noise) {
    const double s0 = (double)sigma_start, s1 = (double)sigma_end;
    const double tau = K == 1 ? s0 : s0 * std::pow(s1 / s0, (double)(k - 1) / (double)(K - 1));
    return (float)std::max(tau, (double)sigma_noise);
}

} /* namespace lfbm5d_side */
#endif
