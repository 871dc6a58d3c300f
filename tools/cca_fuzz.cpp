// cca_fuzz.cpp — the host half of scan analysis (csrc/rtn_cca.h: the per-element rules, the argument checks and the bodies of the
// CPU twins) as a stand-alone program for a sanitizer build.  Pages, masks and box lists are heap blocks of exactly their sizes, so
// a read outside a page or a write outside an output is a sanitizer error.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Iretinanet-for-table-detection_amd/csrc tools/cca_fuzz.cpp -o /tmp/cca_fuzz && /tmp/cca_fuzz 40
//
// Every case draws a page of random sides (30 .. 140, B,G,R or gray) of paper, rules, blobs and noise and runs main()'s chain on
// it: the line masks, the external components of both, the white boxes, the text mask, its components, the outlines.  It checks
// what must hold whatever the data: masks hold 0 and 255 only, every box lies inside the page and is not empty, no image has more
// components than ((h + 1) / 2) * ((w + 1) / 2), the external components are among all components, and a capacity of half the
// count reports the same count.  Prints the totals; exit status 1 on a violation.
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <vector>
#include "rtn_cca.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}
static int between(int a, int b) { return a + (int)rnd((uint32_t)(b - a + 1)); }

#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) { printf("case %d: %s failed (line %d)\n", c, #cond, __LINE__); return 1; } \
    } while (0)

static bool binary(const uint8_t* m, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (m[i] != 0 && m[i] != 255) return false;
    return true;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 20;
    long pixels = 0, lines = 0, texts = 0, kept = 0;
    for (int c = 0; c < cases; ++c) {
        const int h = c == 0 ? 30 : between(30, 140), w = c == 0 ? 30 : between(30, 140), ch = c % 3 == 2 ? 1 : 3;
        const size_t px = (size_t)h * w;
        std::unique_ptr<uint8_t[]> page(new uint8_t[px * ch]);
        for (size_t i = 0; i < px * ch; ++i) page[i] = (uint8_t)between(236, 250);
        for (int k = 0; k < 12; ++k) {                                              // rules and blobs of ink
            const bool rule = k < 4;
            const int bh = rule ? (k % 2 ? between(h / 3, h) : 2) : between(3, 9), bw = rule ? (k % 2 ? 2 : between(w / 3, w)) : between(3, 30);
            const int y0 = between(0, h - 1), x0 = between(0, w - 1);
            for (int y = y0; y < y0 + bh && y < h; ++y)
                for (int x = x0; x < x0 + bw && x < w; ++x)
                    for (int j = 0; j < ch; ++j) page[((size_t)y * w + x) * ch + j] = (uint8_t)between(5, 60);
        }
        const uint8_t* pages[1] = {page.get()};
        uint8_t* wpages[1] = {page.get()};
        const int32_t hs[1] = {h}, ws[1] = {w}, chs[1] = {ch};
        const int64_t offs[1] = {0};
        std::vector<CPage> pg;
        REQUIRE(cca_plan_pages(1, pages, hs, ws, chs, offs, px, &pg) == nullptr);
        REQUIRE(cca_plan_pages(1, pages, hs, ws, chs, offs, px - 1, &pg) != nullptr);
        REQUIRE(cca_plan_pages(1, pages, hs, ws, chs, offs, px, &pg) == nullptr);
        std::unique_ptr<uint8_t[]> hor(new uint8_t[px]), ver(new uint8_t[px]), bwm(new uint8_t[px]), closed(new uint8_t[px]), stages(new uint8_t[4 * px]);
        cca_lines_mask_page(pg[0], hor.get(), ver.get(), bwm.get());
        REQUIRE(binary(hor.get(), px) && binary(ver.get(), px) && binary(bwm.get(), px));
        const int cap = ((h + 1) / 2) * ((w + 1) / 2);
        std::vector<int32_t> page_of, all_boxes;
        for (const uint8_t* m : {hor.get(), ver.get()}) {
            const int64_t all = cca_label_image(m, h, w, 0, 0, nullptr);
            REQUIRE(all <= cap);
            std::unique_ptr<int32_t[]> boxes(new int32_t[4 * (size_t)(all ? all : 1)]);
            const int64_t ext = cca_label_image(m, h, w, 1, (int)all, boxes.get());
            REQUIRE(ext <= all);
            std::unique_ptr<int32_t[]> half(new int32_t[4 * (size_t)(ext / 2 + 1)]);
            REQUIRE(cca_label_image(m, h, w, 1, (int)(ext / 2), half.get()) == ext);
            for (int64_t k = 0; k < ext; ++k) {
                const int32_t* b = boxes.get() + 4 * k;
                REQUIRE(b[0] >= 0 && b[1] >= 0 && b[2] >= 1 && b[3] >= 1 && b[0] + b[2] <= w && b[1] + b[3] <= h);
                page_of.push_back(0);
                all_boxes.insert(all_boxes.end(), b, b + 4);
            }
            lines += ext;
        }
        std::vector<CPaintPage> pp;
        std::vector<CRect> rects;
        REQUIRE(cca_plan_paint(1, wpages, hs, ws, chs, (int)page_of.size(), page_of.data(), all_boxes.data(), 0, &pp, &rects) == nullptr);
        for (const CRect& r : rects)
            for (int y = r.y0; y < r.y1; ++y)
                for (int x = r.x0; x < r.x1; ++x) cca_paint_pixel(pp[r.page], 0, y, x);
        cca_text_mask_page(pg[0], closed.get(), stages.get());
        REQUIRE(binary(closed.get(), px) && binary(stages.get() + 2 * px, 2 * px));
        const int64_t n = cca_label_image(closed.get(), h, w, 1, 0, nullptr);
        REQUIRE(n <= cap);
        std::unique_ptr<int32_t[]> boxes(new int32_t[4 * (size_t)(n ? n : 1)]);
        REQUIRE(cca_label_image(closed.get(), h, w, 1, (int)n, boxes.get()) == n);
        page_of.assign((size_t)n, 0);
        REQUIRE(cca_plan_paint(1, wpages, hs, ws, chs, (int)n, page_of.data(), boxes.get(), 1, &pp, &rects) == nullptr);
        for (const CRect& r : rects) {
            REQUIRE(r.x0 >= 0 && r.y0 >= 0 && r.x1 <= w && r.y1 <= h && r.x0 < r.x1 && r.y0 < r.y1);
            for (int y = r.y0; y < r.y1; ++y)
                for (int x = r.x0; x < r.x1; ++x) cca_paint_pixel(pp[r.page], 1, y, x);
        }
        for (int64_t k = 0; k < n; ++k) kept += boxes[4 * k + 2] > boxes[4 * k + 3] && boxes[4 * k + 2] * boxes[4 * k + 3] > 500;
        texts += n;
        pixels += (long)px;
    }
    printf("%d cases, %ld pixels: %ld line components, %ld text components, %ld kept\n", cases, pixels, lines, texts, kept);
    return 0;
}
