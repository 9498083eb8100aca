/*
 * consist_host_check.cpp -- the per-thread code of k_consist_stats and k_consist_flag (lfbm5d_amd/csrc/lfbm5d_consist_device.h) compiled
 * for the host and run as the kernels run it: a grid of (tiles, tested SAIs) workgroups of 256 threads, the workgroup's counters zeroed,
 * every thread's work, the counters flushed.  Built with the address and undefined-behaviour sanitizers by tools/consist_host_check.py,
 * which writes the case file from the numpy model and compares what this program writes: a gather or a store out of bounds stops it.
 *
 * Case file: int32 A, C, H, W, n_tested; float32 thr[3], g; float32 in[A*C*H*W], pred[A*C*H*W]; int8 disp[A*H*W]; int32 table[n_tested*74].
 * Result file: uint64 hist[A*C*386], skipped; uint8 flags[A*C*H*W]; uint64 counts[A*6].
 */
#include "../lfbm5d_amd/csrc/lfbm5d_consist_device.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace lfbm5d_consist;

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
    auto head = read<int>(f, 5);
    const int A = head[0], C = head[1], H = head[2], W = head[3], nt = head[4];
    auto par = read<float>(f, 4);
    const size_t plane = (size_t)W * H, values = (size_t)A * C * plane;
    auto in = read<float>(f, values);
    auto pred = read<float>(f, values);
    auto disp = read<signed char>(f, (size_t)A * plane);
    auto table = read<int>(f, (size_t)nt * kTabStride);
    fclose(f);
    const Thresholds thr = {{par[0], par[1], par[2]}};
    const float g = par[3];

    const size_t n_hist = (size_t)A * C * kKeys;
    std::unique_ptr<unsigned long long[]> hist(new unsigned long long[n_hist]()), counts(new unsigned long long[(size_t)A * 6]());
    std::unique_ptr<unsigned char[]> flags(new unsigned char[values]());
    unsigned long long skipped = 0;
    const unsigned tx_n = (W + kTW - 1) / kTW, ty_n = (H + kTH - 1) / kTH;
    for (int by = 0; by < nt; by++)
        for (unsigned bx = 0; bx < tx_n * ty_n; bx++) {
            const int* tab = table.get() + (size_t)by * kTabStride;
            const unsigned ty = bx / tx_n, tx = bx - ty * tx_n;
            {   /* k_consist_stats */
                std::unique_ptr<unsigned[]> h(new unsigned[C * kKeys]());
                unsigned skip = 0;
                for (int tid = 0; tid < kThreads; tid++)
                    stats_thread(in.get(), pred.get(), tab[0], C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid, h.get(), &skip, Inc());
                for (int i = 0; i < C * kKeys; i++) hist[(size_t)tab[0] * C * kKeys + i] += h[i];
                skipped += skip;
            }
            {   /* k_consist_flag */
                std::unique_ptr<unsigned[]> cnt(new unsigned[6]());
                for (int tid = 0; tid < kThreads; tid++)
                    flag_thread(in.get(), pred.get(), disp.get(), flags.get(), tab, C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid, thr, g,
                                cnt.get(), Inc());
                for (int i = 0; i < 6; i++) counts[(size_t)tab[0] * 6 + i] += cnt[i];
            }
        }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(hist.get(), sizeof(unsigned long long), n_hist, f);
    fwrite(&skipped, sizeof(skipped), 1, f);
    fwrite(flags.get(), 1, values, f);
    fwrite(counts.get(), sizeof(unsigned long long), (size_t)A * 6, f);
    fclose(f);
    return 0;
}
