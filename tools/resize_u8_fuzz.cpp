// resize_u8_fuzz.cpp — the host half of the 8-bit bicubic resize (csrc/rtn_resize_u8.h: the per-sample rules, the argument checks and
// the body of the CPU twin with the kernel's tile walk) as a stand-alone program for a sanitizer build.  Pages and outputs are heap
// blocks of exactly their sizes at odd offsets, so a read outside a page or a write outside an output is a sanitizer error, and an
// overflowing sum is one for -fsanitize=undefined.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Iretinanet-for-table-detection_amd/csrc tools/resize_u8_fuzz.cpp -o /tmp/resize_u8_fuzz && /tmp/resize_u8_fuzz 300
//
// Every case draws a batch of 1 .. 4 pages of random sides (1 .. 90), one or three channels, random or 0 / 255 contents, and random
// factors (0.2 .. 6, fx and fy apart) or an explicit output size; runs the twin on the path the factor chooses and with the direct
// path forced; and checks what must hold whatever the data: both runs give the same bytes, every sample equals the one computed
// straight from its 16 taps with rsz_taps, a factor of 1 copies the page, guard bytes around every output survive, and the bad
// arguments are refused.  Prints the totals; exit status 1 on a violation.
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <vector>
#include "rtn_resize_u8.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}
static int between(int a, int b) { return a + (int)rnd((uint32_t)(b - a + 1)); }
static double factor() { return 0.2 + 5.8 * (double)rnd(1000000) / 1e6; }

#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) { printf("case %d: %s failed (line %d)\n", c, #cond, __LINE__); return 1; } \
    } while (0)

constexpr int GUARD = 19;

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 100;
    long samples = 0, tiled = 0, direct = 0;
    for (int c = 0; c < cases; ++c) {
        const int n = between(1, 4);
        std::vector<std::unique_ptr<uint8_t[]>> src(n), out_a(n), out_b(n);
        std::vector<const uint8_t*> pages(n);
        std::vector<uint8_t*> outs_a(n), outs_b(n);
        std::vector<int32_t> hs(n), ws(n), cs(n), hos(n), wos(n);
        std::vector<double> ix(n), iy(n);
        std::vector<size_t> out_bytes(n);
        for (int i = 0; i < n; ++i) {
            hs[i] = c == 0 ? 1 : between(1, 90);
            ws[i] = c == 0 ? 1 : between(1, 90);
            cs[i] = rnd(2) ? 3 : 1;
            if (rnd(4) == 0) {                                                   // the size form
                hos[i] = between(1, 200);
                wos[i] = between(1, 200);
                ix[i] = (double)ws[i] / wos[i];
                iy[i] = (double)hs[i] / hos[i];
            } else {
                const double fx = rnd(8) == 0 ? 1.0 : factor(), fy = rnd(3) == 0 ? fx : factor();
                wos[i] = (int32_t)nearbyint(ws[i] * fx);
                hos[i] = (int32_t)nearbyint(hs[i] * fy);
                if (wos[i] < 1) wos[i] = 1;
                if (hos[i] < 1) hos[i] = 1;
                ix[i] = 1.0 / fx;
                iy[i] = 1.0 / fy;
            }
            const size_t sb = (size_t)hs[i] * ws[i] * cs[i];
            out_bytes[i] = (size_t)hos[i] * wos[i] * cs[i];
            src[i].reset(new uint8_t[sb]);
            const bool binary = rnd(3) == 0;
            for (size_t k = 0; k < sb; ++k) src[i][k] = binary ? (uint8_t)(255 * rnd(2)) : (uint8_t)rnd(256);
            pages[i] = src[i].get();
            out_a[i].reset(new uint8_t[out_bytes[i] + 2 * GUARD]);
            out_b[i].reset(new uint8_t[out_bytes[i] + 2 * GUARD]);
            memset(out_a[i].get(), 0xA5, out_bytes[i] + 2 * GUARD);
            memset(out_b[i].get(), 0xA5, out_bytes[i] + 2 * GUARD);
            outs_a[i] = out_a[i].get() + GUARD;
            outs_b[i] = out_b[i].get() + GUARD;
        }
        REQUIRE(rsz_host(n, pages.data(), hs.data(), ws.data(), cs.data(), hos.data(), wos.data(), ix.data(), iy.data(), outs_a.data(), 0) == nullptr);
        REQUIRE(rsz_host(n, pages.data(), hs.data(), ws.data(), cs.data(), hos.data(), wos.data(), ix.data(), iy.data(), outs_b.data(),
                         RSZ_PATH_DIRECT) == nullptr);
        for (int i = 0; i < n; ++i) {
            (rsz_choose_path(0, iy[i]) == RSZ_PATH_TILED ? tiled : direct) += 1;
            REQUIRE(memcmp(out_a[i].get(), out_b[i].get(), out_bytes[i] + 2 * GUARD) == 0);
            for (int k = 0; k < GUARD; ++k) REQUIRE(out_a[i][k] == 0xA5 && out_a[i][GUARD + out_bytes[i] + k] == 0xA5);
            for (int y = 0; y < hos[i]; ++y) {
                RszTaps ty;
                rsz_taps(y, iy[i], hs[i], &ty);
                for (int x = 0; x < wos[i]; ++x) {
                    RszTaps tx;
                    rsz_taps(x, ix[i], ws[i], &tx);
                    for (int ch = 0; ch < cs[i]; ++ch) {
                        int64_t v = 0;
                        for (int a = 0; a < 4; ++a) {
                            int64_t hsum = 0;
                            for (int b = 0; b < 4; ++b)
                                hsum += (int64_t)pages[i][((size_t)ty.idx[a] * ws[i] + tx.idx[b]) * cs[i] + ch] * tx.coef[b];
                            REQUIRE(hsum > -(1ll << 23) && hsum < (1ll << 23));
                            v += hsum * ty.coef[a];
                        }
                        REQUIRE(v + (1 << 21) < (1ll << 31) && v > -(1ll << 31));
                        REQUIRE(outs_a[i][((size_t)y * wos[i] + x) * cs[i] + ch] == rsz_output((int32_t)v));
                    }
                }
            }
            if (ix[i] == 1.0 && iy[i] == 1.0 && hos[i] == hs[i] && wos[i] == ws[i]) REQUIRE(memcmp(outs_a[i], pages[i], out_bytes[i]) == 0);
            samples += (long)out_bytes[i];
        }
        // the refusals: nothing may be touched
        std::vector<int32_t> bad(hs);
        bad[0] = c % 2 ? 0 : RSZ_MAX_SIDE + 1;
        REQUIRE(rsz_host(n, pages.data(), bad.data(), ws.data(), cs.data(), hos.data(), wos.data(), ix.data(), iy.data(), outs_a.data(), 0) != nullptr);
        std::vector<double> nan(ix);
        nan[n - 1] = c % 2 ? -1.0 : (double)NAN;
        REQUIRE(rsz_host(n, pages.data(), hs.data(), ws.data(), cs.data(), hos.data(), wos.data(), nan.data(), iy.data(), outs_a.data(), 0) != nullptr);
        std::vector<int32_t> two(cs);
        two[0] = 2;
        REQUIRE(rsz_host(n, pages.data(), hs.data(), ws.data(), two.data(), hos.data(), wos.data(), ix.data(), iy.data(), outs_a.data(), 0) != nullptr);
        REQUIRE(rsz_host(n, nullptr, hs.data(), ws.data(), cs.data(), hos.data(), wos.data(), ix.data(), iy.data(), outs_a.data(), 0) != nullptr);
        REQUIRE(rsz_host(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == nullptr);
        for (int i = 0; i < n; ++i) REQUIRE(memcmp(out_a[i].get(), out_b[i].get(), out_bytes[i] + 2 * GUARD) == 0);
    }
    printf("%d cases, %ld samples: %ld pages on the tiled path, %ld on the direct path\n", cases, samples, tiled, direct);
    return 0;
}
