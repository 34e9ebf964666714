// async_merge_pack_check — the converted-output merge of the AsyncMultiMapper pipeline on the CPU
// (opencv-octvr_amd/csrc/async_host.hpp build_merge_pack_table, merge_pack_item, region_rects and
// csrc/frame_layout.hpp pack_item_at, pack_lane: the functions merge_pack_kernel runs per work item), a stand-alone
// program meant to be built with -fsanitize=address,undefined (make -C opencv-octvr_amd lib/async_merge_pack_check)
// and run directly.  The NV12 region frames and the merged frame are heap blocks of exactly the needed size (the
// merged frame ends with its last row's last byte, not with its pitch), the memory policy is memcpy, so a work item
// that reads or writes outside them is reported.  For all eight converted layouts every work item of a table is
// executed as the kernel executes it, at every alignment of the merged frame's base (the even ones for 16-bit
// layouts) and at pitch = row and row + 6; then every byte of the merged frame is compared with a sample-by-sample
// restatement of the out rule and the placement, bytes outside every region must still hold the fill and must not
// have been written, every covered byte was written exactly once, and every 16-byte span is 16-byte aligned.
// Further: region_rects applied with memcpy to host planes of their own against the same restatement, the table
// builder's refusals, and pack_item_at on a whole-frame placement against the pack_item it generalises, item by
// item.  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "async_host.hpp"

using namespace octvr;

static int fails = 0;
#define CHECK(c, ...)                                       \
    do {                                                    \
        if (!(c)) {                                         \
            if (fails < 40) {                               \
                fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c); \
                fprintf(stderr, __VA_ARGS__);               \
                fprintf(stderr, "\n");                      \
            }                                               \
            fails++;                                        \
        }                                                   \
    } while (0)

static uint32_t rng_state = 97531;
static uint8_t rnd8() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 13);
}

struct HostMem {
    Words2 load8(const uint8_t* p) const {
        Words2 v;
        memcpy(&v, p, 8);
        return v;
    }
    Words4 load16(const uint8_t* p) const {
        Words4 v;
        memcpy(&v, p, 16);
        return v;
    }
    void store16(uint8_t* p, const Words4& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 15u) == 0, "a 16-byte store is not aligned");
        memcpy(p, &v, 16);
    }
};

// ---- the eight layouts, written out ------------------------------------------------------------------------------
enum Pix { UYVY = 16, YUYV = 17, YUV422P = 18, NV16 = 19, P010 = 32, YUV420P10 = 33, P210 = 34, YUV422P10 = 35 };
static const int kPix[8] = {UYVY, YUYV, YUV422P, NV16, P010, YUV420P10, P210, YUV422P10};
static bool ref_packed(int p) { return p == UYVY || p == YUYV; }
static bool ref_halves(int p) { return p == YUV422P || p == YUV420P10 || p == YUV422P10; }
static int ref_S(int p) { return p >= 32 ? 2 : 1; }
static int ref_cr(int p) { return p == P010 || p == YUV420P10 ? 1 : 2; }
static int ref_shift(int p) { return p == P010 || p == P210 ? 8 : 2; }  // a 10-bit sample of v8: v8 << shift
static int ref_row_bytes(int p, int w) { return ref_packed(p) ? 2 * w : ref_S(p) * w; }
static int ref_rows(int p, int h) { return ref_packed(p) ? h : h + ref_cr(p) * (h / 2); }
static int ref_planes(int p) { return ref_packed(p) ? 1 : ref_halves(p) ? 3 : 2; }

// One sample of the out rule at byte `off`: a byte, or a little-endian word with the other bits 0.
struct Sink {
    std::vector<uint8_t>* bytes;
    std::vector<int>* owner;
    int pix;
    void put(size_t off, uint8_t v8) const {
        if (ref_S(pix) == 1) {
            bytes->at(off) = v8;
            owner->at(off)++;
            return;
        }
        const unsigned v = (unsigned)v8 << ref_shift(pix);
        bytes->at(off) = (uint8_t)(v & 0xFF);
        bytes->at(off + 1) = (uint8_t)(v >> 8);
        owner->at(off)++;
        owner->at(off + 1)++;
    }
};

// Region r (its NV12 frame src, pitch = r.w) in the one-piece frame of an OW x OH picture of layout pix at `pitch`.
static void ref_place_frame(int pix, const PlaneRect& r, const uint8_t* src, int OW, int OH, size_t pitch, const Sink& s) {
    const int w = r.w, h = r.h, S = ref_S(pix), cr = ref_cr(pix);
    auto Y = [&](int x, int y) { return src[(size_t)y * w + x]; };
    auto C = [&](int px, int py, int v) { return src[(size_t)(h + py) * w + 2 * px + v]; };
    if (ref_packed(pix)) {
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t pair = (size_t)(r.y + y) * pitch + 4 * (size_t)((r.x + x) / 2);
                const int second = x & 1;  // of the pair's two pixels (r.x is even)
                if (pix == UYVY) {
                    s.put(pair + 1 + 2 * second, Y(x, y));
                    if (!second) s.put(pair, C(x / 2, y / 2, 0)), s.put(pair + 2, C(x / 2, y / 2, 1));
                } else {
                    s.put(pair + 2 * second, Y(x, y));
                    if (!second) s.put(pair + 1, C(x / 2, y / 2, 0)), s.put(pair + 3, C(x / 2, y / 2, 1));
                }
            }
        return;
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) s.put((size_t)(r.y + y) * pitch + (size_t)S * (r.x + x), Y(x, y));
    for (int j = 0; j < cr * (h / 2); j++) {
        const size_t row = (size_t)(OH + cr * r.y / 2 + j) * pitch;
        const int py = j / cr;  // with two chroma rows per row pair each NV12 chroma row is written twice
        for (int px = 0; px < w / 2; px++) {
            if (ref_halves(pix)) {
                s.put(row + (size_t)S * (r.x / 2 + px), C(px, py, 0));
                s.put(row + (size_t)S * (OW / 2) + (size_t)S * (r.x / 2 + px), C(px, py, 1));
            } else {
                s.put(row + (size_t)S * (r.x + 2 * px), C(px, py, 0));
                s.put(row + (size_t)S * (r.x + 2 * px + 1), C(px, py, 1));
            }
        }
    }
}

struct Case {
    int OW, OH;
    std::vector<PlaneRect> r;
};
static std::vector<PlaneRect> halves_of(const std::vector<PlaneRect>& r) {
    std::vector<PlaneRect> c;
    for (const PlaneRect& a : r) c.push_back(PlaneRect{a.x / 2, a.y / 2, a.w / 2, a.h / 2});
    return c;
}

template <class L>
static void run_case(int pix, const Case& cs, int extra) {
    constexpr LayoutDesc d = L::desc;
    const int n = (int)cs.r.size(), OW = cs.OW, OH = cs.OH, S = ref_S(pix);
    CHECK(d.row_bytes(OW) == ref_row_bytes(pix, OW) && d.rows(OH) == ref_rows(pix, OH) && d.planes() == ref_planes(pix) &&
              d.bytes == S && d.chroma_rows == ref_cr(pix),
          "descriptor of %d", pix);
    const std::vector<PlaneRect> c = halves_of(cs.r);
    std::vector<uint8_t*> src(n);
    std::vector<const uint8_t*> sp;
    for (int k = 0; k < n; k++) {
        const size_t bytes = (size_t)cs.r[k].w * (cs.r[k].h / 2 * 3);
        src[k] = (uint8_t*)malloc(bytes);  // exact size
        for (size_t i = 0; i < bytes; i++) src[k][i] = rnd8();
        src[k][0] = 255;
        src[k][1] = 0;
        sp.push_back(src[k]);
    }
    const size_t row = (size_t)ref_row_bytes(pix, OW), pitch = row + (size_t)extra;
    const size_t bytes = pitch * (size_t)(ref_rows(pix, OH) - 1) + row;
    std::vector<uint8_t> want(bytes, 0xA7);
    std::vector<int> owner(bytes, 0);
    for (int k = 0; k < n; k++) ref_place_frame(pix, cs.r[k], src[k], OW, OH, pitch, Sink{&want, &owner, pix});
    for (size_t i = 0; i < bytes; i++) CHECK(owner[i] <= 1, "the case's regions overlap at byte %zu", i);

    MergePackTable t;
    CHECK(build_merge_pack_table(d, cs.r.data(), c.data(), sp.data(), n, OW, OH, pitch, t), "table of %d refused", pix);
    uint64_t items = 0;
    for (int k = 0; k < n; k++) {
        CHECK(t.r[k].first == items && t.r[k].src == src[k] && t.r[k].w == cs.r[k].w && t.r[k].h == cs.r[k].h, "region %d", k);
        items += pack_items(d, cs.r[k].w, cs.r[k].h);
    }
    CHECK(t.items == items && t.n == n && t.pitch == pitch, "table header");

    for (int align = 0; align < 16; align += S) {
        uint8_t* raw = (uint8_t*)malloc(bytes + (size_t)align);  // the frame's last byte is the block's last byte
        CHECK((reinterpret_cast<uintptr_t>(raw) & 15u) == 0, "malloc is not 16-byte aligned");
        uint8_t* out = raw + align;
        memset(out, 0xA7, bytes);
        std::vector<int> hits(bytes, 0);
        int bad = 0;
        for (uint32_t id = 0; id < t.items; id++) {
            int k = -1;
            const LayoutSpan s = merge_pack_item(d, t, id, reinterpret_cast<uintptr_t>(out), k);
            if (k < 0 || k >= n || s.len < 0 || s.len > kChunk || s.len % S || s.b0 % S || s.dst + (size_t)s.len > bytes ||
                (s.len == kChunk && ((reinterpret_cast<uintptr_t>(out) + s.dst) & 15u))) {
                bad++;
                continue;
            }
            pack_lane<L>(HostMem{}, t.r[k].src, out, t.r[k].w, t.r[k].h, s);
            for (int i = 0; i < s.len; i++) hits[s.dst + (size_t)i]++;
        }
        CHECK(bad == 0, "pix %d: %d bad spans", pix, bad);
        size_t wrong = 0, miscounted = 0;
        for (size_t i = 0; i < bytes; i++) {
            wrong += out[i] != want[i];
            miscounted += hits[i] != owner[i];
        }
        CHECK(wrong == 0, "pix %d %dx%d extra %d align %d: %zu bytes differ", pix, OW, OH, extra, align, wrong);
        CHECK(miscounted == 0, "pix %d %dx%d extra %d align %d: %zu bytes written another number of times", pix, OW, OH, extra,
              align, miscounted);
        free(raw);
    }

    // region_rects: the same bytes in host planes of their own (the download and the copy-out), copied from the
    // one-piece frame `want` at (fx, fy); every other byte of a plane keeps its fill
    {
        size_t pw[3], ph[3], pp[3];
        std::vector<uint8_t> got[3], exp[3];
        for (int k = 0; k < d.planes(); k++) {
            pw[k] = (size_t)d.plane_row_bytes(k, OW);
            ph[k] = (size_t)d.plane_rows(k, OH);
            pp[k] = pw[k] + 2 * (size_t)(k + 1);
            got[k].assign(pp[k] * (ph[k] - 1) + pw[k], 0xEE);
            exp[k] = got[k];
        }
        // expected planes: the frame's bytes that belong to a region, at the plane's own coordinates
        for (size_t y = 0; y < (size_t)ref_rows(pix, OH); y++)
            for (size_t x = 0; x < row; x++) {
                if (!owner[y * pitch + x]) continue;
                int k = 0;
                size_t px = x, py = y;
                if (y >= (size_t)OH && !ref_packed(pix)) {
                    py = y - (size_t)OH;
                    k = 1;
                    if (ref_halves(pix) && x >= row / 2) k = 2, px = x - row / 2;
                }
                exp[k].at(py * pp[k] + px) = want[y * pitch + x];
            }
        for (int r = 0; r < n; r++) {
            const LayoutRects rc = region_rects(d, cs.r[r], OW, OH);
            CHECK(rc.n == d.planes(), "rects of %d", pix);
            for (int i = 0; i < rc.n; i++) {
                const LayoutRect& p = rc.p[i];
                const bool in = p.plane == i && p.x + p.bytes <= pw[i] && p.y + p.rows <= ph[i] && p.fx + p.bytes <= row &&
                                p.fy + p.rows <= (size_t)ref_rows(pix, OH);
                CHECK(in, "pix %d region %d rect %d outside its plane", pix, r, i);
                if (!in) continue;
                for (size_t y = 0; y < p.rows; y++)
                    memcpy(got[i].data() + (p.y + y) * pp[i] + p.x, want.data() + (p.fy + y) * pitch + p.fx, p.bytes);
            }
        }
        for (int k = 0; k < d.planes(); k++) CHECK(got[k] == exp[k], "pix %d: host plane %d by region_rects", pix, k);
    }
    for (uint8_t* p : src) free(p);
}

static void all_layouts(const Case& cs, int extra) {
    for (int pix : kPix) {
        const bool known = with_layout(pix, [&](auto tag) { run_case<decltype(tag)>(pix, cs, extra); });
        CHECK(known, "with_layout(%d)", pix);
    }
}

// pack_item as it stood before pack_item_at generalised it
static LayoutSpan pack_item_present(const LayoutDesc& d, int w, int h, size_t pitch, uintptr_t out_base, uint32_t id) {
    LayoutSpan sp{0, 0, 0, 0, 0};
    int chunk;
    const int n_full = d.row_bytes(w), full = full_rows(d, h);
    const uint32_t per_full = row_items(n_full), per_half = row_items(n_full / 2);
    const uint32_t first_half = (uint32_t)full * per_full;
    if (!d.halves() || id < first_half) {
        sp.row = (int)(id / per_full);
        if (!d.halves() && sp.row >= full) return sp;
        chunk = (int)(id - (uint32_t)sp.row * per_full);
        sp.n = n_full;
        sp.dst = (size_t)sp.row * pitch;
    } else {
        const uint32_t q = (id - first_half) / per_half;
        if (q >= (uint32_t)half_rows(d, h)) return sp;
        chunk = (int)(id - first_half - q * per_half);
        sp.row = h + (int)q;
        sp.n = n_full / 2;
        sp.dst = (size_t)(h + (int)(q >> 1)) * pitch + (size_t)((q & 1u) ? n_full / 2 : 0);
    }
    const RowChunk c = row_chunk(out_base + sp.dst, sp.n, chunk);
    if (chunk == 0) {
        sp.len = c.head;
        return sp;
    }
    if (c.b0 >= sp.n) return sp;
    sp.b0 = c.b0;
    sp.len = c.len(sp.n);
    sp.dst += (size_t)c.b0;
    return sp;
}

static void check_whole_frame(int pix, int w, int h, int extra) {
    const LayoutDesc d = layout_of(pix);
    const size_t pitch = (size_t)d.row_bytes(w) + (size_t)extra;
    const uint32_t items = (uint32_t)pack_items(d, w, h);
    for (int align = 0; align < 16; align += d.bytes) {
        const uintptr_t base = 0x40000u + (uintptr_t)align;
        size_t differ = 0;
        for (uint32_t id = 0; id < items + 3; id++) {
            const LayoutSpan a = pack_item_present(d, w, h, pitch, base, id);
            const LayoutSpan b = pack_item_at(d, w, h, pitch, whole_frame_place(d, w, h, pitch), base, id);
            const LayoutSpan c = pack_item(d, w, h, pitch, base, id);
            differ += a.row != b.row || a.n != b.n || a.b0 != b.b0 || a.len != b.len || a.dst != b.dst;
            differ += a.row != c.row || a.n != c.n || a.b0 != c.b0 || a.len != c.len || a.dst != c.dst;
        }
        CHECK(differ == 0, "pix %d %dx%d extra %d align %d: %zu items differ from the present pack_item", pix, w, h, extra, align,
              differ);
    }
}

int main() {
    // the left and right half of 1036 x 512: r.x = 518, so a packed row of the right half starts 2 * 518 = 12 (mod
    // 16) bytes past a 16-byte boundary and its 8-bit U half at byte 259
    const Case halves{1036, 512, {{0, 0, 518, 512}, {518, 0, 518, 512}}};
    CHECK((2 * 518) % 16 == 12 && 518 / 2 == 259, "the numbers above");
    // one region with a gap beside it (and below), another diagonally opposite
    const Case gap{64, 36, {{0, 0, 32, 18}, {32, 18, 32, 18}}};
    // a 2 x 2 region; a region narrower than 16 bytes of a row in every layout (6 pixels: 12 or 6 bytes); bytes no
    // region owns all around
    const Case tiny{20, 8, {{6, 4, 2, 2}, {10, 0, 6, 4}}};
    // a single region that is the whole frame
    const Case whole{24, 6, {{0, 0, 24, 6}}};
    for (int extra : {0, 6}) {
        all_layouts(halves, extra);
        all_layouts(gap, extra);
        all_layouts(tiny, extra);
        all_layouts(whole, extra);
    }
    for (int pix : kPix)
        for (int extra : {0, 6}) {
            check_whole_frame(pix, 40, 6, extra);
            check_whole_frame(pix, 1036, 4, extra);
            check_whole_frame(pix, 6, 2, extra);
        }
    {  // refused tables
        const LayoutDesc d = layout_of(UYVY), p = layout_of(P210);
        MergePackTable t;
        std::vector<PlaneRect> r(kMergeMaxRegions + 1, PlaneRect{0, 0, 2, 2}), c(kMergeMaxRegions + 1, PlaneRect{0, 0, 1, 1});
        std::vector<const uint8_t*> s(kMergeMaxRegions + 1, nullptr);
        CHECK(build_merge_pack_table(d, r.data(), c.data(), s.data(), kMergeMaxRegions, 64, 64, 128, t), "32 regions");
        CHECK(!build_merge_pack_table(d, r.data(), c.data(), s.data(), kMergeMaxRegions + 1, 64, 64, 128, t), "33 regions");
        CHECK(!build_merge_pack_table(d, r.data(), c.data(), s.data(), 0, 64, 64, 128, t), "no region");
        CHECK(!build_merge_pack_table(d, r.data(), c.data(), s.data(), 1, 64, 64, 127, t), "pitch below a row");
        CHECK(!build_merge_pack_table(layout_of(1), r.data(), c.data(), s.data(), 1, 64, 64, 128, t), "a native layout");
        r[0] = PlaneRect{3, 0, 2, 2};  // odd r.x, which creation accepts (c from its own rounding)
        c[0] = PlaneRect{2, 0, 1, 1};
        CHECK(!build_merge_pack_table(d, r.data(), c.data(), s.data(), 1, 64, 64, 128, t), "odd r.x");
        r[0] = PlaneRect{4, 0, 2, 2};  // c.x != r.x / 2
        c[0] = PlaneRect{3, 0, 1, 1};
        CHECK(!build_merge_pack_table(d, r.data(), c.data(), s.data(), 1, 64, 64, 128, t), "c.x != r.x / 2");
        r[0] = PlaneRect{4, 2, 2, 2};  // c.y != r.y / 2
        c[0] = PlaneRect{2, 0, 1, 1};
        CHECK(!build_merge_pack_table(d, r.data(), c.data(), s.data(), 1, 64, 64, 128, t), "c.y != r.y / 2");
        r[0] = PlaneRect{60, 0, 6, 2};  // past the right edge
        c[0] = PlaneRect{30, 0, 3, 1};
        CHECK(!build_merge_pack_table(d, r.data(), c.data(), s.data(), 1, 64, 64, 128, t), "outside the frame");
        r[0] = PlaneRect{0, 0, 2, 2};  // 2 GiB: 16384 x 2 h rows of 32768 bytes reach 0x7FFFFF80 at h = 32768
        c[0] = PlaneRect{0, 0, 1, 1};
        CHECK(build_merge_pack_table(p, r.data(), c.data(), s.data(), 1, 16384, 32766, 32768, t), "below 2 GiB");
        CHECK(!build_merge_pack_table(p, r.data(), c.data(), s.data(), 1, 16384, 32768, 32768, t), "2 GiB");
        CHECK(region_is_subpicture(PlaneRect{518, 0, 518, 512}, PlaneRect{259, 0, 259, 256}), "the right half of 1036 x 512");
    }
    printf(fails ? "async_merge_pack_check: %d checks FAILED\n" : "async_merge_pack_check: ok\n", fails);
    return fails ? 1 : 0;
}
