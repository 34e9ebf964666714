// async_host_check — the AsyncMultiMapper pipeline's host arithmetic (opencv-octvr_amd/csrc/frame_layout.hpp
// pack_run, async_host.hpp merge_pin_ranges) in a stand-alone program, meant to be built with
// -fsanitize=address,undefined (make -C opencv-octvr_amd lib/async_host_check) and run on the CPU.  Source planes
// and the packed buffer are heap blocks of exactly the needed size, so any byte read or written past a plane's last
// row end or past a run's packed size is reported.  check_pack: the two 4:2:0 layouts against each other and the
// planes.  check_pack_layouts: every run of small frames of all ten layouts against a per-sample reference that
// indexes the planes itself, from the formats' definitions written out here.  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "async_host.hpp"

using namespace octvr;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                               \
        }                                                          \
    } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// a plane of `rows` rows of `w` bytes at `pitch`, allocated to end with its last row's last byte
struct Plane {
    std::vector<uint8_t> b;
    size_t pitch;
    Plane(int w, int rows, size_t pitch_) : b(pitch_ * (size_t)(rows - 1) + (size_t)w), pitch(pitch_) {
        for (uint8_t& x : b) x = (uint8_t)rnd();
    }
};

static void check_pack(int w, int h) {
    Plane y(w, h, (size_t)w + 5), u(w / 2, h / 2, (size_t)w / 2 + 3), v(w / 2, h / 2, (size_t)w / 2), uv(w, h / 2, (size_t)w + 2);
    for (int r = 0; r < h / 2; r++)
        for (int c = 0; c < w / 2; c++) {
            uv.b[r * uv.pitch + 2 * c] = u.b[r * u.pitch + c];
            uv.b[r * uv.pitch + 2 * c + 1] = v.b[r * v.pitch + c];
        }
    const uint8_t* pl[3] = {y.b.data(), u.b.data(), v.b.data()};
    const size_t pp[3] = {y.pitch, u.pitch, v.pitch};
    const uint8_t* nl[3] = {y.b.data(), uv.b.data(), nullptr};
    const size_t np[3] = {y.pitch, uv.pitch, 0};
    const int G = (w + 7) / 8;
    for (int it = 0; it < 400; it++) {
        int rp = (int)(rnd() % (uint32_t)(h / 2)), g0 = (int)(rnd() % (uint32_t)G), ng = 1 + (int)(rnd() % (uint32_t)(G - g0));
        if (it == 0) rp = h / 2 - 1, g0 = G - 1, ng = 1;  // the last group of the last row pair
        if (it == 1) rp = h / 2 - 1, g0 = 0, ng = G;
        const int yb = run_px(w, g0, ng);
        std::vector<uint8_t> a((size_t)3 * yb), b((size_t)3 * yb);
        CHECK(pack_run(layout_of(0), a.data(), w, rp, g0, ng, pl, pp) == a.size());
        CHECK(pack_run(layout_of(1), b.data(), w, rp, g0, ng, nl, np) == b.size());
        for (int k = 0; k < 2 * yb; k++) CHECK(a[k] == b[k] && a[k] == y.b[(size_t)(2 * rp + k / yb) * y.pitch + 8 * g0 + k % yb]);
        for (int c = 0; c < yb / 2; c++) {
            CHECK(b[2 * yb + 2 * c] == a[2 * yb + c] && a[2 * yb + c] == u.b[rp * u.pitch + 4 * g0 + c]);
            CHECK(b[2 * yb + 2 * c + 1] == a[2 * yb + yb / 2 + c] && a[2 * yb + yb / 2 + c] == v.b[rp * v.pitch + 4 * g0 + c]);
        }
    }
}

// The ten layouts, written out: the OCTVR_PIX_* value, bytes per sample, the chroma kind (0: one packed plane with
// luma and chroma bytes alternating; 1: Y and a plane of U,V pairs; 2: Y, U and V planes) and chroma rows per row pair.
struct Fmt {
    int pix;
    const char* name;
    int S, kind, cr;
};
static const Fmt kFmts[10] = {{0, "YUV420P", 1, 2, 1},  {1, "NV12", 1, 1, 1},     {16, "UYVY422", 1, 0, 2}, {17, "YUYV422", 1, 0, 2},
                              {18, "YUV422P", 1, 2, 2}, {19, "NV16", 1, 1, 2},    {32, "P010", 2, 1, 1},    {33, "YUV420P10", 2, 2, 1},
                              {34, "P210", 2, 1, 2},    {35, "YUV422P10", 2, 2, 2}};

// Every run (row pair, first group, groups) of a w x h frame of the layout: pack_run's bytes are the run's samples
// in the packed order — the two luma rows (for the packed kind the two packed rows, 2 bytes per pixel), then per
// chroma row its U,V pairs, or its U samples and then its V samples.  extra: bytes of pitch past a row.  joined:
// U and V are the column halves of one array (V starts half a row into U's rows).
static void check_pack_layout(const Fmt& f, int w, int h, int extra, bool joined) {
    const int S = f.S, crows = f.cr * (h / 2);
    const int luma_w = (f.kind == 0 ? 2 : 1) * S * w, chroma_w = f.kind == 2 ? S * w / 2 : S * w;
    Plane y(luma_w, h, (size_t)(luma_w + extra));
    Plane c1(chroma_w, crows, (size_t)(chroma_w + extra)), c2(chroma_w, crows, (size_t)(chroma_w + 2 * extra));
    Plane both(2 * chroma_w, crows, (size_t)(2 * chroma_w + extra));
    const uint8_t* pl[3] = {y.b.data(), nullptr, nullptr};
    size_t pp[3] = {y.pitch, 0, 0};
    if (f.kind == 1) pl[1] = c1.b.data(), pp[1] = c1.pitch;
    if (f.kind == 2 && !joined) pl[1] = c1.b.data(), pp[1] = c1.pitch, pl[2] = c2.b.data(), pp[2] = c2.pitch;
    if (f.kind == 2 && joined) pl[1] = both.b.data(), pl[2] = both.b.data() + chroma_w, pp[1] = pp[2] = both.pitch;
    const LayoutDesc d = layout_of(f.pix);
    const int G = (w + 7) / 8;
    for (int rp = 0; rp < h / 2; rp++)
        for (int g0 = 0; g0 < G; g0++)
            for (int ng = 1; ng <= G - g0; ng++) {
                const int x0 = 8 * g0, n = (8 * (g0 + ng) < w ? 8 * (g0 + ng) : w) - x0;
                std::vector<uint8_t> want;
                auto sample = [&](int plane, int row, int idx) {
                    for (int b = 0; b < S; b++) want.push_back(pl[plane][(size_t)row * pp[plane] + (size_t)(S * idx + b)]);
                };
                for (int row = 0; row < 2; row++)
                    for (int x = 0; x < n; x++) {
                        if (f.kind == 0) {  // the pixel's two bytes, luma and chroma
                            want.push_back(pl[0][(size_t)(2 * rp + row) * pp[0] + (size_t)(2 * (x0 + x))]);
                            want.push_back(pl[0][(size_t)(2 * rp + row) * pp[0] + (size_t)(2 * (x0 + x) + 1)]);
                        } else {
                            sample(0, 2 * rp + row, x0 + x);
                        }
                    }
                for (int cr = 0; cr < (f.kind == 0 ? 0 : f.cr); cr++) {
                    const int row = f.cr * rp + cr;
                    if (f.kind == 1) {
                        for (int x = 0; x < n; x++) sample(1, row, x0 + x);  // sample x0 + x of the pairs: U or V of pair (x0 + x) / 2
                    } else {
                        for (int x = 0; x < n / 2; x++) sample(1, row, x0 / 2 + x);
                        for (int x = 0; x < n / 2; x++) sample(2, row, x0 / 2 + x);
                    }
                }
                std::vector<uint8_t> got(want.size(), 0);  // exact size: a byte too many is reported
                const size_t size = pack_run(d, got.data(), w, rp, g0, ng, pl, pp);
                if (size != want.size() || got != want) {
                    fprintf(stderr, "pack_run %s w=%d h=%d extra=%d joined=%d rp=%d g0=%d ng=%d\n", f.name, w, h, extra, (int)joined, rp,
                            g0, ng);
                    fails++;
                }
            }
}

static void check_pack_layouts() {
    for (const Fmt& f : kFmts)
        for (int w : {2, 6, 8, 10, 18, 64})  // below one group, a short last group, one group, several groups
            for (int h : {2, 4})
                for (int extra : {0, 6}) {
                    check_pack_layout(f, w, h, extra, false);
                    if (f.kind == 2) check_pack_layout(f, w, h, extra, true);
                }
}

static void check_merge() {
    const uintptr_t P = 4096;
    // three planes in separate allocations: as given (sorted)
    auto r = merge_pin_ranges({{10 * P + 16, 12 * P}, {40 * P, 41 * P + 7}, {20 * P + 1, 20 * P + 2}}, P);
    CHECK(r.size() == 3 && r[0].begin == 10 * P + 16 && r[0].end == 12 * P && r[1].begin == 20 * P + 1 &&
          r[1].end == 20 * P + 2 && r[2].begin == 40 * P && r[2].end == 41 * P + 7);
    // a contiguous NV12 frame: Y then U,V, adjacent, sharing a page
    r = merge_pin_ranges({{8 * P + 64, 8 * P + 64 + 131072}, {8 * P + 64 + 131072, 8 * P + 64 + 196608}}, P);
    CHECK(r.size() == 1 && r[0].begin == 8 * P + 64 && r[0].end == 8 * P + 64 + 196608);
    // U and V as column halves of one array (overlapping), Y elsewhere; given out of order
    r = merge_pin_ranges({{100 * P + 256, 100 * P + 256 + 65536 - 256}, {50 * P, 60 * P}, {100 * P, 100 * P + 65536 - 256}}, P);
    CHECK(r.size() == 2 && r[0].begin == 50 * P && r[0].end == 60 * P && r[1].begin == 100 * P &&
          r[1].end == 100 * P + 65536);
    // page-rounded extents that touch without sharing a page merge too; a page apart they do not
    r = merge_pin_ranges({{4 * P, 5 * P}, {5 * P, 6 * P}}, P);
    CHECK(r.size() == 1 && r[0].begin == 4 * P && r[0].end == 6 * P);
    r = merge_pin_ranges({{4 * P, 5 * P - 1}, {6 * P, 7 * P}}, P);
    CHECK(r.size() == 2);
    // a range inside another, a chain of three, an empty range, a range at the top of the address space
    r = merge_pin_ranges({{4 * P, 9 * P}, {5 * P, 6 * P}, {9 * P + 5, 10 * P}, {3 * P, 3 * P}}, P);
    CHECK(r.size() == 1 && r[0].begin == 4 * P && r[0].end == 10 * P);
    r = merge_pin_ranges({{UINTPTR_MAX - 100, UINTPTR_MAX - 1}, {P, 2 * P}}, P);
    CHECK(r.size() == 2 && r[1].end == UINTPTR_MAX - 1);
    CHECK(merge_pin_ranges({}, P).empty());
    // random sets: the result is sorted, page-disjoint with a free page between neighbours' extents or more,
    // and covers exactly the inputs
    for (int it = 0; it < 2000; it++) {
        std::vector<PinRange> in;
        const int n = 1 + (int)(rnd() % 5);
        for (int k = 0; k < n; k++) {
            const uintptr_t b = P + rnd() % (40 * P);
            in.push_back({b, b + rnd() % (6 * P)});
        }
        r = merge_pin_ranges(in, P);
        for (size_t k = 0; k < r.size(); k++) {
            CHECK(r[k].begin < r[k].end);
            if (k) CHECK((r[k - 1].end + P - 1) / P * P < r[k].begin / P * P);
        }
        for (const PinRange& x : in) {
            if (x.end <= x.begin) continue;
            bool inside = false;
            for (const PinRange& m : r) inside |= m.begin <= x.begin && x.end <= m.end;
            CHECK(inside);
        }
        for (const PinRange& m : r) {  // each merged range starts and ends with an input's
            bool b = false, e = false;
            for (const PinRange& x : in) b |= x.begin == m.begin, e |= x.end == m.end;
            CHECK(b && e);
        }
    }
}

int main() {
    check_pack(324, 240);  // w % 8 == 4: a partial last group
    check_pack(256, 144);
    check_pack(16, 2);
    check_pack(2, 2);
    check_pack_layouts();
    check_merge();
    printf(fails ? "async_host_check: %d checks FAILED\n" : "async_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
