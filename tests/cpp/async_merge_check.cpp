// async_merge_check — the device-frame merge's host arithmetic (opencv-octvr_amd/csrc/async_host.hpp:
// build_merge_table and merge_item, the function merge_regions_kernel runs per work item) in a stand-alone
// program, meant to be built with -fsanitize=address,undefined (make -C opencv-octvr_amd lib/async_merge_check)
// and run on the CPU.  The region frames and the merged frame are heap blocks of exactly the needed size (the
// merged frame ends with its last row's last byte, not with its pitch), so a work item that reads or writes
// outside them is reported.  Every work item of a table is executed as the kernel executes it (a copy of its
// span), at every alignment of the merged frame's base; then: each byte of each region was written exactly
// once with the byte the layout asks for, no other byte was written, and every 16-byte span is 16-byte
// aligned.  check_placement: region_pieces, the one table the D2H copies, the copy-out and the merge table place a
// region by, applied with memcpy to planes of their own at pitches above the width (every byte of a region is
// the region frame's byte the layout asks for, every other byte keeps its guard value), and the merge table built
// from the pieces against the table recorded from build_merge_table before it used them.  Exit status 0 = every
// check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static uint32_t rng_state = 2468;
static uint8_t rnd8() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 13);
}

// _rect_mul_size of the pipeline (async.cpp): the rectangle of the fractions f in a W x H plane
static PlaneRect rect_mul_size(const double* f, int W, int H) {
    PlaneRect o{(int)std::round(f[0] * W), (int)std::round(f[1] * H), (int)std::round(f[2] * W), (int)std::round(f[3] * H)};
    if (o.x + o.w >= W) o.w = W - o.x;
    if (o.y + o.h >= H) o.h = H - o.y;
    return o;
}

static void run_case(int OW, int OH, size_t pitch, int nv12, const std::vector<std::vector<double>>& fr) {
    const int n = (int)fr.size();
    std::vector<PlaneRect> r, c;
    std::vector<std::vector<uint8_t>> src(n);
    std::vector<const uint8_t*> sp;
    for (int k = 0; k < n; k++) {
        r.push_back(rect_mul_size(fr[k].data(), OW, OH));
        c.push_back(rect_mul_size(fr[k].data(), OW / 2, OH / 2));
        // octvr_async_create's region rule
        CHECK(r[k].w > 0 && r[k].h > 0 && r[k].w % 2 == 0 && r[k].h % 2 == 0 && c[k].w == r[k].w / 2 && c[k].h == r[k].h / 2);
        src[k].resize((size_t)r[k].w * (r[k].h / 2 * 3));
        for (uint8_t& b : src[k]) b = rnd8();
        sp.push_back(src[k].data());
    }
    MergeTable t;
    CHECK(build_merge_table(r.data(), c.data(), sp.data(), n, OW, OH, pitch, nv12, t));
    CHECK(t.n == n && t.pitch == pitch && t.nv12 == nv12);
    uint64_t items = 0;
    for (int k = 0; k < n; k++) {
        CHECK(t.r[k].first == items);
        CHECK(t.r[k].y_off == (size_t)r[k].y * pitch + r[k].x);
        if (nv12) {
            CHECK(t.r[k].u_off == (size_t)(OH + c[k].y) * pitch + 2 * c[k].x);
        } else {
            CHECK(t.r[k].u_off == (size_t)(OH + c[k].y) * pitch + c[k].x);
            CHECK(t.r[k].v_off == (size_t)(OH + c[k].y) * pitch + OW / 2 + c[k].x);
        }
        items += merge_region_items(r[k].w, r[k].h, nv12);
    }
    CHECK(t.items == items);

    // the merged frame the layout asks for, and which bytes belong to a region
    const size_t rows = (size_t)OH / 2 * 3, bytes = pitch * (rows - 1) + (size_t)OW;
    std::vector<uint8_t> want(bytes, 0xA7);
    std::vector<int> owner(bytes, 0);
    auto put = [&](size_t off, uint8_t v) {
        want[off] = v;
        owner[off]++;
    };
    for (int k = 0; k < n; k++) {
        const int w = r[k].w, h = r[k].h;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) put((size_t)(r[k].y + y) * pitch + r[k].x + x, src[k][(size_t)y * w + x]);
        for (int y = 0; y < h / 2; y++)
            for (int x = 0; x < w; x++) {
                const uint8_t v = src[k][(size_t)(h + y) * w + x];
                const size_t row = (size_t)(OH + c[k].y + y) * pitch;
                if (nv12)
                    put(row + 2 * c[k].x + x, v);
                else
                    put(row + (x < w / 2 ? c[k].x + x : OW / 2 + c[k].x + x - w / 2), v);
            }
    }
    for (size_t i = 0; i < bytes; i++) CHECK(owner[i] <= 1);  // the cases' regions do not overlap

    for (int align = 0; align < 16; align++) {
        const uintptr_t base = 0x10000u + (uintptr_t)align;  // the merged frame's address: its low four bits matter
        std::vector<uint8_t> out(bytes, 0xA7);  // exact size: the copies below go here, at the spans' offsets
        std::vector<int> hits(bytes, 0);
        int bad_align = 0, bad_len = 0;
        for (uint32_t id = 0; id < t.items; id++) {
            const MergeSpan s = merge_item(t, id, base);
            if (s.len < 0 || s.len > kChunk) bad_len++;
            if (s.len == kChunk && ((base + s.dst) & 15u)) bad_align++;
            for (int i = 0; i < s.len; i++) {
                out.at(s.dst + (size_t)i) = s.src[i];  // s.src past a region frame's end: AddressSanitizer
                hits.at(s.dst + (size_t)i)++;
            }
        }
        CHECK(bad_align == 0 && bad_len == 0);
        size_t wrong = 0, miscounted = 0;
        for (size_t i = 0; i < bytes; i++) {
            wrong += out[i] != want[i];
            miscounted += hits[i] != owner[i];
        }
        CHECK(wrong == 0);
        CHECK(miscounted == 0);
    }
}

// ---- region_pieces ------------------------------------------------------------------------------------------
// The merge table of a case as build_merge_table produced it when it spelled the offsets out itself: pitch, n,
// nv12, items, and per region w, h, y_off, u_off, v_off, first.
struct Recorded {
    uint32_t pitch;
    int n, nv12;
    uint32_t items;
    struct {
        int w, h;
        uint32_t y_off, u_off, v_off, first;
    } r[kMergeMaxRegions];
};
static const Recorded kOddChroma_planar = {27, 2, 0, 64, {
    {10, 8, 0, 216, 226, 0}, {10, 8, 10, 221, 231, 32},
}};
static const Recorded kOddChroma_nv12 = {27, 2, 1, 48, {
    {10, 8, 0, 216, 216, 0}, {10, 8, 10, 226, 226, 24},
}};
static const Recorded kWidth2_planar = {23, 2, 0, 48, {
    {2, 8, 2, 185, 195, 0}, {10, 4, 102, 235, 245, 32},
}};
static const Recorded kWidth2_nv12 = {23, 2, 1, 36, {
    {2, 8, 2, 186, 186, 0}, {10, 4, 102, 240, 240, 24},
}};
static const Recorded kWhole_planar = {17, 1, 0, 24, {
    {12, 6, 0, 102, 108, 0},
}};
static const Recorded kWhole_nv12 = {17, 1, 1, 18, {
    {12, 6, 0, 102, 102, 0},
}};
static const Recorded kMany_planar = {70, 32, 0, 512, {
    {4, 4, 0, 560, 592, 0}, {4, 4, 4, 562, 594, 16}, {4, 4, 8, 564, 596, 32}, {4, 4, 12, 566, 598, 48},
    {4, 4, 16, 568, 600, 64}, {4, 4, 20, 570, 602, 80}, {4, 4, 24, 572, 604, 96}, {4, 4, 28, 574, 606, 112},
    {4, 4, 32, 576, 608, 128}, {4, 4, 36, 578, 610, 144}, {4, 4, 40, 580, 612, 160}, {4, 4, 44, 582, 614, 176},
    {4, 4, 48, 584, 616, 192}, {4, 4, 52, 586, 618, 208}, {4, 4, 56, 588, 620, 224}, {4, 4, 60, 590, 622, 240},
    {4, 4, 280, 700, 732, 256}, {4, 4, 284, 702, 734, 272}, {4, 4, 288, 704, 736, 288}, {4, 4, 292, 706, 738, 304},
    {4, 4, 296, 708, 740, 320}, {4, 4, 300, 710, 742, 336}, {4, 4, 304, 712, 744, 352}, {4, 4, 308, 714, 746, 368},
    {4, 4, 312, 716, 748, 384}, {4, 4, 316, 718, 750, 400}, {4, 4, 320, 720, 752, 416}, {4, 4, 324, 722, 754, 432},
    {4, 4, 328, 724, 756, 448}, {4, 4, 332, 726, 758, 464}, {4, 4, 336, 728, 760, 480}, {4, 4, 340, 730, 762, 496},
}};
static const Recorded kMany_nv12 = {70, 32, 1, 384, {
    {4, 4, 0, 560, 560, 0}, {4, 4, 4, 564, 564, 12}, {4, 4, 8, 568, 568, 24}, {4, 4, 12, 572, 572, 36},
    {4, 4, 16, 576, 576, 48}, {4, 4, 20, 580, 580, 60}, {4, 4, 24, 584, 584, 72}, {4, 4, 28, 588, 588, 84},
    {4, 4, 32, 592, 592, 96}, {4, 4, 36, 596, 596, 108}, {4, 4, 40, 600, 600, 120}, {4, 4, 44, 604, 604, 132},
    {4, 4, 48, 608, 608, 144}, {4, 4, 52, 612, 612, 156}, {4, 4, 56, 616, 616, 168}, {4, 4, 60, 620, 620, 180},
    {4, 4, 280, 700, 700, 192}, {4, 4, 284, 704, 704, 204}, {4, 4, 288, 708, 708, 216}, {4, 4, 292, 712, 712, 228},
    {4, 4, 296, 716, 716, 240}, {4, 4, 300, 720, 720, 252}, {4, 4, 304, 724, 724, 264}, {4, 4, 308, 728, 728, 276},
    {4, 4, 312, 732, 732, 288}, {4, 4, 316, 736, 736, 300}, {4, 4, 320, 740, 740, 312}, {4, 4, 324, 744, 744, 324},
    {4, 4, 328, 748, 748, 336}, {4, 4, 332, 752, 752, 348}, {4, 4, 336, 756, 756, 360}, {4, 4, 340, 760, 760, 372},
}};

static void check_placement(int OW, int OH, size_t pitch, const std::vector<std::vector<double>>& fr, const Recorded& planar,
                            const Recorded& nv12_table) {
    const int n = (int)fr.size();
    std::vector<PlaneRect> r, c;
    std::vector<std::vector<uint8_t>> src(n);
    std::vector<const uint8_t*> sp;
    for (int k = 0; k < n; k++) {
        r.push_back(rect_mul_size(fr[k].data(), OW, OH));
        c.push_back(rect_mul_size(fr[k].data(), OW / 2, OH / 2));
        CHECK(r[k].w > 0 && r[k].h > 0 && r[k].w % 2 == 0 && r[k].h % 2 == 0 && c[k].w == r[k].w / 2 && c[k].h == r[k].h / 2);
        src[k].resize((size_t)r[k].w * (r[k].h / 2 * 3));
        for (size_t i = 0; i < src[k].size(); i++) src[k][i] = (uint8_t)(1 + 41 * k + 3 * i);  // a ramp of its own
        sp.push_back(src[k].data());
    }
    for (int nv12 = 0; nv12 < 2; nv12++) {
        // planes of their own, pitches above the width: Y; U and V of OW / 2 bytes, or the U,V plane of OW
        const int np = nv12 ? 2 : 3;
        const size_t pw[3] = {(size_t)OW, nv12 ? (size_t)OW : (size_t)OW / 2, (size_t)OW / 2};
        const size_t pp[3] = {(size_t)OW + 7, pw[1] + 3, pw[2] + 5}, ph[3] = {(size_t)OH, (size_t)OH / 2, (size_t)OH / 2};
        std::vector<uint8_t> got[3], want[3];
        for (int k = 0; k < np; k++) {
            got[k].assign(pp[k] * (ph[k] - 1) + pw[k], 0xEE);  // exact size: a row copy past the plane is reported
            want[k] = got[k];
        }
        for (int k = 0; k < n; k++) {
            const RegionPieces pc = region_pieces(r[k], c[k], nv12);
            CHECK(pc.n == np);
            for (int i = 0; i < pc.n; i++) {
                const RegionPiece& p = pc.p[i];
                CHECK(p.plane >= 0 && p.plane < np && p.x + p.bytes <= pw[p.plane] && p.y + p.rows <= ph[p.plane]);
                if (!(p.plane >= 0 && p.plane < np && p.x + p.bytes <= pw[p.plane] && p.y + p.rows <= ph[p.plane])) continue;
                for (size_t y = 0; y < p.rows; y++)
                    memcpy(got[p.plane].data() + (p.y + y) * pp[p.plane] + p.x, src[k].data() + p.src + y * (size_t)r[k].w, p.bytes);
            }
            // what the layouts ask for, byte by byte
            const int w = r[k].w, h = r[k].h;
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) want[0][(size_t)(r[k].y + y) * pp[0] + r[k].x + x] = src[k][(size_t)y * w + x];
            for (int y = 0; y < h / 2; y++)
                for (int x = 0; x < w; x++) {
                    const uint8_t v = src[k][(size_t)(h + y) * w + x];
                    if (nv12)
                        want[1][(size_t)(c[k].y + y) * pp[1] + 2 * c[k].x + x] = v;
                    else if (x < w / 2)
                        want[1][(size_t)(c[k].y + y) * pp[1] + c[k].x + x] = v;
                    else
                        want[2][(size_t)(c[k].y + y) * pp[2] + c[k].x + x - w / 2] = v;
                }
        }
        for (int k = 0; k < np; k++) CHECK(got[k] == want[k]);

        const Recorded& rec = nv12 ? nv12_table : planar;
        MergeTable t;
        CHECK(build_merge_table(r.data(), c.data(), sp.data(), n, OW, OH, pitch, nv12, t));
        CHECK(t.pitch == rec.pitch && t.n == rec.n && t.nv12 == rec.nv12 && t.items == rec.items && rec.n == n && rec.nv12 == nv12);
        for (int k = 0; k < kMergeMaxRegions; k++) {
            const MergeRegion& m = t.r[k];
            if (k < n)
                CHECK(m.src == sp[k] && m.w == rec.r[k].w && m.h == rec.r[k].h && m.y_off == rec.r[k].y_off &&
                      m.u_off == rec.r[k].u_off && m.v_off == rec.r[k].v_off && m.first == rec.r[k].first);
            else
                CHECK(m.src == nullptr && m.w == 0 && m.h == 0 && m.y_off == 0 && m.u_off == 0 && m.v_off == 0 && m.first == rec.items);
        }
        run_case(OW, OH, pitch, nv12, fr);  // and the work items of that table
    }
}

int main() {
    const std::vector<std::vector<double>> top_bottom = {{0, 0, 1, .5}, {0, .5, 1, .5}};
    const std::vector<std::vector<double>> left_right = {{0, 0, .5, 1}, {.5, 0, .5, 1}};
    for (int nv12 = 0; nv12 < 2; nv12++) {
        run_case(768, 768, 768, nv12, top_bottom);
        // r.x = r.w = 518 = 6 (mod 16), c.x = c.w = 259: planar chroma halves off every vector boundary
        run_case(1036, 512, 1036, nv12, left_right);
        run_case(1036, 512, 1036 + 6, nv12, left_right);
        run_case(64, 36, 70, nv12, {{0, 0, .5, .5}, {.5, .5, .5, .5}});  // a gap: bytes no region owns
        run_case(20, 4, 23, nv12, {{.1, 0, .2, 1}, {.5, 0, .5, .5}});    // rows shorter than a chunk
    }
    {
        // 20 x 8 in halves: r.x = 10 and an odd chroma column c.x = 5; a region 2 pixels wide; a single region that
        // is the whole frame; the 32 regions of one merge launch
        check_placement(20, 8, 27, {{0, 0, .5, 1}, {.5, 0, .5, 1}}, kOddChroma_planar, kOddChroma_nv12);
        const PlaneRect half = rect_mul_size(std::vector<double>{.5, 0, .5, 1}.data(), 20, 8);
        const PlaneRect half_c = rect_mul_size(std::vector<double>{.5, 0, .5, 1}.data(), 10, 4);
        CHECK(half.x == 10 && half_c.x == 5);
        check_placement(20, 8, 23, {{.1, 0, .1, 1}, {.5, .5, .5, .5}}, kWidth2_planar, kWidth2_nv12);
        CHECK(rect_mul_size(std::vector<double>{.1, 0, .1, 1}.data(), 20, 8).w == 2);
        check_placement(12, 6, 17, {{0, 0, 1, 1}}, kWhole_planar, kWhole_nv12);
        std::vector<std::vector<double>> many;
        for (int k = 0; k < kMergeMaxRegions; k++) many.push_back({(k % 16) / 16., (k / 16) * .5, 1 / 16., .5});
        check_placement(64, 8, 70, many, kMany_planar, kMany_nv12);
    }
    {  // 1036 x 512 in halves: the numbers the pipeline's tests rely on
        const double f[4] = {.5, 0, .5, 1};
        const PlaneRect r = rect_mul_size(f, 1036, 512), c = rect_mul_size(f, 518, 256);
        CHECK(r.x == 518 && r.w == 518 && r.h == 512 && c.x == 259 && c.w == 259 && c.h == 256 && r.x % 16 == 6);
    }
    {  // refused tables
        MergeTable t;
        std::vector<PlaneRect> r(kMergeMaxRegions + 1, PlaneRect{0, 0, 2, 2}), c(kMergeMaxRegions + 1, PlaneRect{0, 0, 1, 1});
        std::vector<const uint8_t*> s(kMergeMaxRegions + 1, nullptr);
        CHECK(build_merge_table(r.data(), c.data(), s.data(), kMergeMaxRegions, 64, 64, 64, 0, t));
        CHECK(!build_merge_table(r.data(), c.data(), s.data(), kMergeMaxRegions + 1, 64, 64, 64, 0, t));
        CHECK(!build_merge_table(r.data(), c.data(), s.data(), 0, 64, 64, 64, 0, t));
        CHECK(!build_merge_table(r.data(), c.data(), s.data(), 1, 64, 64, 63, 0, t));  // pitch below the width
        r[0] = PlaneRect{60, 0, 6, 2};  // past the right edge
        c[0] = PlaneRect{30, 0, 3, 1};
        CHECK(!build_merge_table(r.data(), c.data(), s.data(), 1, 64, 64, 64, 0, t));
        r[0] = PlaneRect{0, 0, 4, 2};  // chroma rectangle not half the luma rectangle
        c[0] = PlaneRect{0, 0, 1, 1};
        CHECK(!build_merge_table(r.data(), c.data(), s.data(), 1, 64, 64, 64, 0, t));
        r[0] = PlaneRect{0, 0, 2, 2};  // 2 GiB: 32768 x 43692 rows at pitch 32768 >= 0x7FFFFF80
        c[0] = PlaneRect{0, 0, 1, 1};
        CHECK(build_merge_table(r.data(), c.data(), s.data(), 1, 32768, 43688, 32768, 0, t));
        CHECK(!build_merge_table(r.data(), c.data(), s.data(), 1, 32768, 43692, 32768, 0, t));
    }
    printf(fails ? "async_merge_check: %d checks FAILED\n" : "async_merge_check: ok\n", fails);
    return fails ? 1 : 0;
}
