/*
 * repair_host_check.cpp -- the per-thread code of k_repair_valid and k_repair_sweep (lfbm5d_amd/csrc/lfbm5d_repair_device.h) compiled for
 * the host and run as the kernels run it: a grid of (tiles, non-empty SAIs) workgroups of 256 threads for the validity planes, then a
 * grid of (tiles, targets) workgroups whose phases run thread after thread with the kernel's barriers between them, on planes of
 * exactly the kernel's LDS sizes.  Built with the address and undefined-behaviour sanitizers by tools/repair_host_check.py, which writes
 * the case file from the numpy model and compares what this program writes: a load or a store out of bounds stops it.
 *
 * Case file: int32 A, C, H, W, D, r, min_valid, n_sai, n_targets, has_flags; int32 sai[n_sai]; uint32 missing[A];
 *            float32 in[A*C*H*W]; uint8 flags[A*C*H*W] (if has_flags); int32 table[n_targets*74]; float32 tables[kTabFloats].
 * Result file: uint8 valid[A*H*W]; float32 mid[A*C*H*W]; uint8 rem[A*C*H*W]; int8 disp[A*H*W] (from -99); uint32 tiles[A*nt];
 *              uint64 hist[17].
 */
#include "../lfbm5d_amd/csrc/lfbm5d_repair_device.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace lfbm5d_repair;

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
    auto head = read<int>(f, 10);
    const int A = head[0], C = head[1], H = head[2], W = head[3], D = head[4], r = head[5], min_valid = head[6], ns = head[7], nt = head[8];
    const bool has_flags = head[9] != 0;
    const size_t plane = (size_t)W * H, values = (size_t)A * C * plane;
    auto sai = read<int>(f, ns);
    auto missing = read<unsigned>(f, A);
    auto in = read<float>(f, values);
    auto flags = read<unsigned char>(f, has_flags ? values : 0);
    auto table = read<int>(f, (size_t)nt * kTabStride);
    auto tables = read<float>(f, kTabFloats);
    fclose(f);

    const unsigned tx_n = (W + kTW - 1) / kTW, ty_n = (H + kTH - 1) / kTH, tiles_n = tx_n * ty_n;
    std::unique_ptr<unsigned char[]> valid(new unsigned char[A * plane]()), rem(new unsigned char[values]());
    std::unique_ptr<float[]> mid(new float[values]());
    std::unique_ptr<signed char[]> disp(new signed char[A * plane]);
    std::memset(disp.get(), -99, A * plane);
    std::unique_ptr<unsigned[]> tiles(new unsigned[(size_t)A * tiles_n]());
    unsigned long long hist[kHist] = {};

    for (int by = 0; by < ns; by++)
        for (unsigned bx = 0; bx < tiles_n; bx++) {   /* k_repair_valid */
            const int q = sai[by];
            const unsigned ty = bx / tx_n, tx = bx - ty * tx_n;
            unsigned total = 0;
            for (int tid = 0; tid < kThreads; tid++)
                total += valid_thread(in.get(), has_flags ? flags.get() : nullptr, missing[q] != 0, q, C, W, H, (int)(tx * kTW), (int)(ty * kTH), tid,
                                      valid.get(), mid.get(), rem.get());
            tiles[(size_t)q * tiles_n + bx] = total;
        }

    for (int by = 0; by < nt; by++)
        for (unsigned bx = 0; bx < tiles_n; bx++) {   /* k_repair_sweep */
            const int* tab = table.get() + (size_t)by * kTabStride;
            const int m = tab[0];
            if (!tiles[(size_t)m * tiles_n + bx]) continue;
            const Sweep s = {in.get(), valid.get(), tab, tables.get(), tab[1], C, W, H};
            const unsigned ty = bx / tx_n, tx = bx - ty * tx_n;
            const int x0 = (int)(tx * kTW), y0 = (int)(ty * kTH);
            std::unique_ptr<float[]> e(new float[kEH * kEW]), h(new float[kEH * kTW]);
            std::unique_ptr<unsigned short[]> ke(new unsigned short[kEH * kEW]), kh(new unsigned short[kEH * kTW]);
            std::unique_ptr<unsigned[]> wg_hist(new unsigned[kHist]());
            std::unique_ptr<float[]> best(new float[kThreads * kPer]());
            std::unique_ptr<int[]> dstar(new int[kThreads * kPer]());
            std::unique_ptr<float[]> dlds(new float[kThreads * kPer]);
            for (int j = 0; j <= 2 * D; j++) {
                const int d = hypothesis(j);
                for (int tid = 0; tid < kThreads; tid++) error_phase(s, d, x0, y0, r, tid, e.get(), ke.get());
                for (int tid = 0; tid < kThreads; tid++) hbox_phase(e.get(), ke.get(), h.get(), kh.get(), r, tid);
                for (int tid = 0; tid < kThreads; tid++)
                    vbox_phase(s, h.get(), kh.get(), r, tid, j == 0, d, best.get() + tid * kPer, dstar.get() + tid * kPer);
            }
            for (int tid = 0; tid < kThreads; tid++)
                for (int k = 0; k < kPer; k++) dlds[k * kThreads + tid] = (float)dstar[tid * kPer + k];   /* as the kernel lays them out in LDS */
            for (int tid = 0; tid < kThreads; tid++)
                store_phase(s, m, min_valid, mid.get(), rem.get(), disp.get(), x0, y0, tid, dlds.get() + tid, kThreads, wg_hist.get(), Inc());
            for (int i = 0; i < kHist; i++) hist[i] += wg_hist[i];
        }

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(valid.get(), 1, A * plane, f);
    fwrite(mid.get(), sizeof(float), values, f);
    fwrite(rem.get(), 1, values, f);
    fwrite(disp.get(), 1, A * plane, f);
    fwrite(tiles.get(), sizeof(unsigned), (size_t)A * tiles_n, f);
    fwrite(hist, sizeof(unsigned long long), kHist, f);
    fclose(f);
    return 0;
}
