// overlay_list_check — the work-list builder of overlay_apply_kernel (opencv-octvr_amd/csrc/overlay_list.hpp)
// against a direct scan, built with -fsanitize=address,undefined (make -C opencv-octvr_amd
// lib/overlay_list_check) and run on the CPU: widths that are no multiple of 8, covered pixels in the last
// partial group, on the first and last row, an empty LUT, padding to whole workgroups.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "overlay_list.hpp"

struct Entry {
    uint32_t xy, code;
};
static const uint32_t kCovered = 1u << 29;
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

static void run(int W, int H, int percent, int block, uint32_t seed) {
    std::vector<Entry> lut((size_t)W * H);
    size_t covered = 0;
    for (auto& e : lut) {
        e.xy = rnd(seed);
        e.code = rnd(seed) & ~kCovered;
        if ((int)(rnd(seed) % 100) < percent) {
            e.code |= kCovered;
            covered++;
        }
    }
    if (percent > 0 && percent < 100) {  // corners
        for (size_t k : {(size_t)0, (size_t)W - 1, lut.size() - 1})
            if (!(lut[k].code & kCovered)) {
                lut[k].code |= kCovered;
                covered++;
            }
    }
    const auto b = octvr::build_overlay_list(lut, W, H, kCovered, block);
    CHECK(b.covered == covered);
    CHECK(b.groups.size() % (size_t)block == 0 && b.entries.size() == 8 * b.groups.size());
    // every listed covered entry is the LUT's, at its position; uncovered slots are zero; order is row-major
    size_t seen = 0;
    uint64_t last = 0;
    bool pad = false;
    for (size_t g = 0; g < b.groups.size(); g++) {
        const int gx = (int)(b.groups[g] & 0xFFFFu), y = (int)(b.groups[g] >> 16);
        int hit = 0;
        for (int i = 0; i < 8; i++) hit += (b.entries[8 * g + i].code & kCovered) ? 1 : 0;
        if (!hit) pad = true;  // padding groups come last, sit at (0, 0) and hold nothing
        for (int i = 0; i < 8; i++) {
            const Entry& e = b.entries[8 * g + i];
            const int x = 8 * gx + i;
            if (e.code & kCovered) {
                CHECK(x < W && y < H);
                if (x < W && y < H) CHECK(e.xy == lut[(size_t)y * W + x].xy && e.code == lut[(size_t)y * W + x].code);
            } else {
                CHECK(e.xy == 0 && e.code == 0);
                if (x < W && y < H && !pad) CHECK(!(lut[(size_t)y * W + x].code & kCovered));
            }
        }
        seen += (size_t)hit;
        if (!hit) CHECK(b.groups[g] == 0u);
        else {
            CHECK(!pad);
            const uint64_t key = ((uint64_t)y << 32) | (uint64_t)gx;
            CHECK(g == 0 || key > last);
            last = key;
        }
    }
    CHECK(seen == covered);
    if (covered == 0) CHECK(b.groups.empty());
}

int main() {
    run(512, 256, 30, 32, 1);
    run(13, 7, 50, 32, 2);
    run(9, 1, 100, 4, 3);
    run(8, 3, 0, 32, 4);
    run(250, 64, 1, 32, 5);
    run(1, 1, 100, 1, 6);
    const std::vector<Entry> none;
    CHECK(octvr::build_overlay_list(none, 16, 16, kCovered, 32).groups.empty());  // a LUT that is too small
    printf(fails ? "overlay_list_check: %d checks FAILED\n" : "overlay_list_check: ok\n", fails);
    return fails ? 1 : 0;
}
