// preview_list_check — the tap-list builder of preview_gather_kernel (opencv-octvr_amd/csrc/preview_list.hpp)
// against a plain per-pixel loop, built with -fsanitize=address,undefined (make -C opencv-octvr_amd
// lib/preview_list_check) and run on the CPU: down-scale, identity, up-scale and odd sizes; the clamps of the
// last row and column; padding to whole workgroups; every listed entry is the LUT's own entry of an in-frame
// result pixel, so the list reads no source tap the composite does not read (the footprint stays).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "preview_list.hpp"

struct Entry {
    uint32_t xy, code;
};
static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("line %d: %s\n", __LINE__, #c);                \
            fails++;                                              \
        }                                                         \
    } while (0)

static uint32_t rnd(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

// resize_rgba_rgb_kernel's coordinates of one axis, written out per pixel
static void coords(int x, int d, int s, int* lo, int* hi) {
    const float f = (float)(1.0 / ((double)d / s));
    const float src = (float)x * f;
    const int x1 = (int)floorf(src);
    const int x2 = x1 + 1;
    *lo = x1;
    *hi = x2 < s - 1 ? x2 : s - 1;
}

static void run(int W, int H, int dw, int dh, int block, uint32_t seed) {
    // a LUT whose every entry is distinct (xy = the pixel's index), so an entry names its result pixel
    std::vector<Entry> lut((size_t)W * H);
    for (size_t k = 0; k < lut.size(); k++) lut[k] = Entry{(uint32_t)k, rnd(seed) | 0x8000u};
    lut[lut.size() / 2].code = 0;  // a pixel no camera claims stays what it is: an entry that evaluates to black
    const auto b = octvr::build_preview_list(lut, W, H, dw, dh, block);
    const size_t n = 4 * (size_t)dw * dh;
    CHECK(b.pixels == (size_t)dw * dh);
    CHECK(b.entries.size() >= n && b.entries.size() % (size_t)block == 0 && b.entries.size() - n < (size_t)block);
    CHECK(b.fx == (float)(1.0 / ((double)dw / W)) && b.fy == (float)(1.0 / ((double)dh / H)));
    if (b.entries.size() < n) return;
    int clamped_x = 0, clamped_y = 0;
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            int x1, x2r, y1, y2r;
            coords(x, dw, W, &x1, &x2r);
            coords(y, dh, H, &y1, &y2r);
            CHECK(x1 >= 0 && x1 < W && x2r >= x1 && x2r < W && y1 >= 0 && y1 < H && y2r >= y1 && y2r < H);
            clamped_x += x2r == x1;
            clamped_y += y2r == y1;
            const size_t want[4] = {(size_t)y1 * W + x1, (size_t)y1 * W + x2r, (size_t)y2r * W + x1, (size_t)y2r * W + x2r};
            const Entry* e = &b.entries[4 * ((size_t)y * dw + x)];
            for (int t = 0; t < 4; t++) {
                // the LUT's own entry of that in-frame result pixel, bit for bit: its taps are the composite's
                CHECK(want[t] < lut.size());
                CHECK(e[t].xy == lut[want[t]].xy && e[t].code == lut[want[t]].code);
            }
        }
    // the last column and row read their own pixel twice whenever floor(x f) is the source's last one
    int lx, hx, ly, hy;
    coords(dw - 1, dw, W, &lx, &hx);
    coords(dh - 1, dh, H, &ly, &hy);
    CHECK((lx == W - 1) == (hx == lx) && (ly == H - 1) == (hy == ly));
    if (dw >= W) CHECK(clamped_x >= dh);  // identity and up-scale: at least the last column clamps
    if (dh >= H) CHECK(clamped_y >= dw);
    for (size_t k = n; k < b.entries.size(); k++) CHECK(b.entries[k].xy == 0 && b.entries[k].code == 0);  // claims nothing
}

int main() {
    run(384, 192, 320, 180, 256, 1);   // down-scale
    run(384, 192, 384, 192, 256, 2);   // identity: every pixel's upper taps are its neighbours', the last clamp
    run(384, 192, 1000, 500, 256, 3);  // up-scale
    run(384, 192, 301, 201, 256, 4);   // odd sizes, 4 * 301 * 201 no multiple of 256
    run(512, 256, 1280, 640, 256, 5);
    run(13, 7, 5, 3, 256, 6);          // less than one workgroup
    run(2, 2, 64, 1, 256, 7);          // exactly one workgroup: no padding
    run(1, 1, 3, 3, 4, 8);             // a one-pixel source: every tap clamps
    run(7680, 8, 1280, 2, 256, 9);     // the C2 width
    const std::vector<Entry> none;
    CHECK(octvr::build_preview_list(none, 16, 16, 8, 8, 256).entries.empty());  // a LUT that is too small
    const std::vector<Entry> one(256);
    CHECK(octvr::build_preview_list(one, 16, 16, 0, 8, 256).entries.empty());
    CHECK(octvr::build_preview_list(one, 16, 16, 8, 8, 6).entries.empty());  // a workgroup holds whole pixels
    printf(fails ? "preview_list_check: %d checks FAILED\n" : "preview_list_check: ok\n", fails);
    return fails ? 1 : 0;
}
