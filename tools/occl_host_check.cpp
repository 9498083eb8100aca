/*
 * occl_host_check.cpp -- the per-thread code of k_view_sweep_occl (lfbm5d_amd/csrc/lfbm5d_occl_device.h on top of
 * lfbm5d_subpel_device.h) compiled for the host and run as the kernel runs it: a grid of (tiles, synthesised SAIs) workgroups of 256
 * threads; the sets of the table row; per hypothesis the table of taps, the error phase, the two box phases with the kernel's barriers
 * as the boundaries between the loops over the threads; then the store phase and the counters' flush.  The workgroup's arrays are
 * exact-size heap blocks.  Built with the address and undefined-behaviour sanitizers by tools/occl_host_check.py, which writes the case
 * file and compares what this program writes with the numpy model: a load or a store out of bounds stops it.
 *
 * Case file: int32 A, C, H, W, n_sai, D, Q, r, hold; float32 ratio; float32 in[A*C*H*W], out[A*C*H*W] (initial contents); int8
 * disp[A*H*W], uint8 set[A*H*W] (initial contents); int32 table[n_sai*74].
 * Result file: float32 out[A*C*H*W]; int8 disp[A*H*W]; uint8 set[A*H*W]; uint64 cnt[65 + 5].
 */
#include "../lfbm5d_amd/csrc/lfbm5d_occl_device.h"

#include <cstdio>
#include <cstdlib>
#include <memory>

using namespace lfbm5d_occl;

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
    auto head = read<int>(f, 9);
    const int A = head[0], C = head[1], H = head[2], W = head[3], ns = head[4], D = head[5], Q = head[6], r = head[7], hold = head[8];
    const float ratio = read<float>(f, 1)[0];
    const size_t plane = (size_t)W * H, values = (size_t)A * C * plane;
    auto in = read<float>(f, values);
    auto out = read<float>(f, values);
    auto disp = read<signed char>(f, (size_t)A * plane);
    auto set = read<unsigned char>(f, (size_t)A * plane);
    auto table = read<int>(f, (size_t)ns * kTabStride);
    fclose(f);

    std::unique_ptr<unsigned long long[]> total(new unsigned long long[kCnt]());
    const unsigned tx_n = (W + kTW - 1) / kTW, ty_n = (H + kTH - 1) / kTH;
    const int J = D * Q;
    for (int by = 0; by < ns; by++)
        for (unsigned bx = 0; bx < tx_n * ty_n; bx++) {
            const int* tab = table.get() + (size_t)by * kTabStride;
            const int n = tab[1];
            if (n < 1 || n > kSrcMax || (hold && n > kHold)) { fprintf(stderr, "bad source count %d\n", n); return 2; }
            const Sets sets = make_sets(tab);
            const SetView s = view_of(sets);
            const unsigned ty = bx / tx_n, tx = bx - ty * tx_n;
            const int x0 = (int)(tx * kTW), y0 = (int)(ty * kTH);
            /* the workgroup's LDS: what a hypothesis does not write keeps NaN, so that a read of it shows */
            std::unique_ptr<float[]> e(new float[kEH * kEW]), h(new float[kEH * kTW]);
            for (int i = 0; i < kEH * kEW; i++) e[i] = __builtin_nanf("");
            for (int i = 0; i < kEH * kTW; i++) h[i] = __builtin_nanf("");
            std::unique_ptr<Tap[]> taps(new Tap[n]);
            std::unique_ptr<unsigned[]> cnt(new unsigned[kCnt]());
            std::unique_ptr<float[][kPer]> best(new float[kThreads][kPer]());
            std::unique_ptr<int[][kPer]> jstar(new int[kThreads][kPer]());
            for (int tid = 0; tid < n; tid++) taps[tid] = make_tap(tab, tid, 0, Q);
            for (int i = 0; i <= 2 * J; i++) {
                const int j = hypothesis(i);
                for (int tid = 0; tid < kThreads; tid++) {
                    if (hold) error_phase<true>(in.get(), taps.get(), s, n, ratio, C, W, H, x0, y0, r, tid, e.get());
                    else error_phase<false>(in.get(), taps.get(), s, n, ratio, C, W, H, x0, y0, r, tid, e.get());
                }
                for (int tid = 0; tid < kThreads; tid++) {
                    if (tid < n && i < 2 * J) taps[tid] = make_tap(tab, tid, hypothesis(i + 1), Q);
                    hbox_phase(e.get(), h.get(), r, tid);
                }
                for (int tid = 0; tid < kThreads; tid++) vbox_phase(h.get(), r, tid, i == 0, j, best[tid], jstar[tid]);
            }
            for (int tid = 0; tid < kThreads; tid++)
                store_phase(in.get(), out.get(), disp.get(), set.get(), tab, s, ratio, Q, C, W, H, x0, y0, tid, jstar[tid], 1, cnt.get(), Inc());
            for (int i = 0; i < kCnt; i++) total[i] += cnt[i];
        }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(out.get(), sizeof(float), values, f);
    fwrite(disp.get(), 1, (size_t)A * plane, f);
    fwrite(set.get(), 1, (size_t)A * plane, f);
    fwrite(total.get(), sizeof(unsigned long long), kCnt, f);
    fclose(f);
    return 0;
}
