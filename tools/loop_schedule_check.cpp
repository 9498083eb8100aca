/*
 * loop_schedule_check.cpp -- the refinement loop's sigma schedule (loop_sigma, lfbm5d_amd/csrc/lfbm5d_side_values.h) compiled for the host
 * alone: prints the bits of sigma_k, k = 1..K, one hexadecimal word per line.  tests/test_loop_schedule.py builds and runs it.
 *   loop_schedule_check K sigma_start sigma_end sigma_noise      (the three sigmas as the hexadecimal bits of a float)
 */
#include "../lfbm5d_amd/csrc/lfbm5d_side_values.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static float from_bits(const char* s) {
    const unsigned b = (unsigned)std::strtoul(s, nullptr, 16);
    float f;
    std::memcpy(&f, &b, sizeof(f));
    return f;
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const unsigned K = (unsigned)std::strtoul(argv[1], nullptr, 10);
    for (unsigned k = 1; k <= K; k++) {
        const float s = lfbm5d_side::loop_sigma(k, K, from_bits(argv[2]), from_bits(argv[3]), from_bits(argv[4]));
        unsigned b;
        std::memcpy(&b, &s, sizeof(b));
        std::printf("%08x\n", b);
    }
    return 0;
}
