/*
 * photo_host_check.cpp -- the per-thread code of k_photo_stats and k_photo_apply (lfbm5d_amd/csrc/lfbm5d_photo_device.h) compiled for the
 * host and run as the kernels run it: a grid of (tiles, tested SAIs) workgroups of 256 threads, the workgroup's counters zeroed, every
 * thread's work, the counters flushed; and a grid of (blocks, planes) workgroups over the planes of the non-empty SAIs.  Built with the
 * address and undefined-behaviour sanitizers by tools/photo_host_check.py, which writes the case file from the numpy model and compares
 * what this program writes: a load or a store out of bounds stops it.
 *
 * Case file: int32 A, C, H, W, n_tested, n_planes, blocks; float32 lo, hi; float32 in[A*C*H*W], pred[A*C*H*W]; int32 table[n_tested*74];
 *            int32 planes[n_planes]; float32 factors[n_planes].
 * Result file: uint64 hist[A*C*1026], skipped[2]; float32 out[A*C*H*W] (apply into a buffer of 0), inplace[A*C*H*W] (apply on a copy),
 *              shifted[A*C*H*W] (apply into a buffer that starts 4 bytes off the input's alignment: every value goes single).
 */
#include "../lfbm5d_amd/csrc/lfbm5d_photo_device.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace lfbm5d_photo;

constexpr int kTabStride = 2 + 3 * 24;

struct Inc { void operator()(unsigned* p) const { ++*p; } };

template <class T>
static std::unique_ptr<T[]> read(FILE* f, size_t n) {   /* exact-size heap blocks: the sanitizer sees every overrun */
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    if (n && fread(p.get(), sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s case result\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    auto head = read<int>(f, 7);
    const int A = head[0], C = head[1], H = head[2], W = head[3], nt = head[4], np = head[5], blocks = head[6];
    auto par = read<float>(f, 2);
    const size_t plane = (size_t)W * H, values = (size_t)A * C * plane;
    auto in = read<float>(f, values);
    auto pred = read<float>(f, values);
    auto table = read<int>(f, (size_t)nt * kTabStride);
    auto planes = read<int>(f, np);
    auto factors = read<float>(f, np);
    fclose(f);

    const size_t n_hist = (size_t)A * C * kRatioKeys;
    std::unique_ptr<unsigned long long[]> hist(new unsigned long long[n_hist]());
    unsigned long long skipped[2] = {0, 0};
    const unsigned tx_n = (W + kTW - 1) / kTW, ty_n = (H + kTH - 1) / kTH;
    for (int by = 0; by < nt; by++)
        for (unsigned bx = 0; bx < tx_n * ty_n; bx++) {   /* k_photo_stats */
            const int m = table[(size_t)by * kTabStride];
            const unsigned ty = bx / tx_n, tx = bx - ty * tx_n;
            std::unique_ptr<unsigned[]> h(new unsigned[C * kRatioKeys]()), skip(new unsigned[2]());
            for (int tid = 0; tid < kThreads; tid++)
                stats_thread(in.get(), pred.get(), m, C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid, par[0], par[1], h.get(), skip.get(), Inc());
            for (int i = 0; i < C * kRatioKeys; i++) hist[(size_t)m * C * kRatioKeys + i] += h[i];
            skipped[0] += skip[0]; skipped[1] += skip[1];
        }

    std::unique_ptr<float[]> out(new float[values]()), inplace(new float[values]), shifted(new float[values + 1]());
    std::memcpy(inplace.get(), in.get(), values * sizeof(float));
    for (int by = 0; by < np; by++)
        for (int bx = 0; bx < blocks; bx++)
            for (int tid = 0; tid < kThreads; tid++) {   /* k_photo_apply */
                const size_t at = (size_t)planes[by] * plane, t = (size_t)bx * kThreads + tid, threads = (size_t)blocks * kThreads;
                apply_thread(in.get() + at, out.get() + at, plane, factors[by], t, threads);
                apply_thread(inplace.get() + at, inplace.get() + at, plane, factors[by], t, threads);
                apply_thread(in.get() + at, shifted.get() + 1 + at, plane, factors[by], t, threads);
            }

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(hist.get(), sizeof(unsigned long long), n_hist, f);
    fwrite(skipped, sizeof(unsigned long long), 2, f);
    fwrite(out.get(), sizeof(float), values, f);
    fwrite(inplace.get(), sizeof(float), values, f);
    fwrite(shifted.get() + 1, sizeof(float), values, f);
    fclose(f);
    return 0;
}
