// yuv422_check.cpp — the arithmetic of the YUYV / YUV422P / NV16 conversions (csrc/yuv422_host.hpp) executed on
// the CPU for every work item of small geometries, against exactly sized heap blocks under the address and
// undefined-behaviour sanitizers: the lane bodies here are the templates yuv422_unpack_kernel and
// yuv422_pack_kernel instantiate, with memcpy as the memory policy.  For each of the three layouts:
//   unpack: widths 8k, 8k + 2, 8k + 4, 8k + 6; pitches minimal and minimal + 6; every base alignment 0-15 of
//     the source and both source kinds (the caller's frame, the packed upload buffer); runs at the first and the
//     last group of a row, a one-group run, a run longer than one table piece.  Every footprint byte of the NV12
//     frame is written exactly once with the value of the rule, nothing else is written, and every read lies in
//     the source block (the sanitizer's part: the blocks end where the frame or the packed runs end).
//   yuv422_pack_run, from the three host plane shapes of a push, equals a byte-wise reference of the layout the
//     unpack item's offsets describe.
//   pack: the same widths, pitches (and + 10) and base alignments: every byte below a row's width written exactly
//     once with the value of the rule, the bytes between the width and the pitch never.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "yuv422_host.hpp"

using namespace octvr;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (g_fail++ < 20) {              \
                fprintf(stderr, "FAIL: ");    \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");        \
            }                                 \
        }                                     \
    } while (0)

uint32_t rng_state = 4242u;
uint8_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

struct Run {
    uint32_t cam, g0, ng, off;
};

// n bytes whose first byte has address = align (mod 16) and whose last byte is the allocation's last byte: an
// access past the end is a heap overflow for the sanitizer (before the start, `align` bytes of slack).
uint8_t* tail_block(std::vector<void*>& keep, size_t n, int align) {
    uint8_t* raw = (uint8_t*)malloc(n + (size_t)align);
    keep.push_back(raw);
    CHECK((reinterpret_cast<uintptr_t>(raw) & 15u) == 0, "malloc is not 16-byte aligned");
    return raw + align;
}

struct HostMem {
    uint32_t load4(const uint8_t* p) const {
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    Yuv422Pair load8(const uint8_t* p) const {
        Yuv422Pair v;
        memcpy(&v, p, 8);
        return v;
    }
    UyvyWords load16(const uint8_t* p) const {
        UyvyWords v;
        memcpy(&v, p, 16);
        return v;
    }
    void store8(uint8_t* p, const Yuv422Pair& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 7u) == 0, "an 8-byte store is not aligned");
        memcpy(p, &v, 8);
    }
    void store16(uint8_t* p, const UyvyWords& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 15u) == 0, "a 16-byte store is not aligned");
        memcpy(p, &v, 16);
    }
};

// The 4:2:2 picture behind a frame of any layout: luma (x, y) and the chroma byte x of row y as U,V pairs.
struct Picture {
    int layout, w, h;
    const uint8_t* f;
    size_t pitch;
    uint8_t luma(int x, int y) const { return layout == kYuv422Yuyv ? f[(size_t)y * pitch + 2 * x] : f[(size_t)y * pitch + x]; }
    uint8_t chroma(int x, int y) const {
        if (layout == kYuv422Yuyv) return f[(size_t)y * pitch + 2 * x + 1];
        const uint8_t* row = f + (size_t)(h + y) * pitch;
        return layout == kYuv422Nv16 ? row[x] : row[(x & 1) * (w / 2) + x / 2];
    }
};

template <int L>
void check_unpack(int w, int h, int extra, int align, bool packed_mode) {
    std::vector<void*> keep;
    const int G = (w + 7) / 8;
    const size_t pitch = (size_t)yuv422_frame_row_bytes(L, w) + extra;
    const int rows = yuv422_frame_rows(L, h);
    const size_t frame_bytes = (size_t)(rows - 1) * pitch + (size_t)yuv422_frame_row_bytes(L, w);
    uint8_t* frame = tail_block(keep, frame_bytes, align);
    for (size_t i = 0; i < frame_bytes; i++) frame[i] = rnd();
    // carry cases of the average in the first row pair's chroma: 0 + 1, 255 + 254
    for (int x = 0; x < w; x++) {
        const size_t c0 = L == kYuv422Yuyv ? (size_t)2 * x + 1 : (size_t)h * pitch + x;
        frame[c0] = (x & 2) ? 255 : 0;
        frame[c0 + pitch] = (x & 2) ? 254 : 1;
    }
    const Picture pic{L, w, h, frame, pitch};
    std::vector<Run> runs;
    const int rp_n = h / 2;
    runs.push_back(Run{0u | 0u << 8, 0u, (uint32_t)(G > 1 ? 2 : 1), 0});
    runs.push_back(Run{0u | (uint32_t)(rp_n - 1) << 8, (uint32_t)(G - 1), 1u, 0});
    if (G > 4) runs.push_back(Run{0u | 1u << 8, (uint32_t)(G / 2), 1u, 0});
    if (rp_n > 2) runs.push_back(Run{0u | 2u << 8, 0u, (uint32_t)G, 0});
    if (G > 6) runs.push_back(Run{0u | 1u << 8, (uint32_t)(G - 3), 3u, 0});
    size_t bytes = 0;
    const std::vector<int> in_w{w};
    const std::vector<UyvyRun> table = uyvy_run_table(runs, in_w, bytes);
    // the host planes of a push: YUYV the frame; NV16 Y and the U,V plane; YUV422P Y, U, V (exactly sized copies
    // of the V plane, which is no block of its own inside the frame)
    const uint8_t* planes[3] = {frame, nullptr, nullptr};
    size_t pitches[3] = {pitch, 0, 0};
    if (L == kYuv422Nv16) {
        planes[1] = frame + (size_t)h * pitch;
        pitches[1] = pitch;
    } else if (L == kYuv422Planar) {
        for (int k = 0; k < 2; k++) {
            const size_t pp = (size_t)(w / 2 + (extra ? 3 : 0));
            uint8_t* p = tail_block(keep, (size_t)(h - 1) * pp + w / 2, align);
            for (int y = 0; y < h; y++) memcpy(p + (size_t)y * pp, frame + (size_t)(h + y) * pitch + k * (w / 2), w / 2);
            planes[1 + k] = p;
            pitches[1 + k] = pp;
        }
    }
    // the packed upload buffer: exactly `bytes`; each piece against a byte-wise reference of its layout
    uint8_t* packed = tail_block(keep, bytes ? bytes : 1, align);
    size_t expect_off = 0;
    for (const UyvyRun& t : table) {
        CHECK(t.off == expect_off, "table offsets are not back to back");
        CHECK(t.ng >= 1 && t.ng <= (uint32_t)kUyvyWave, "piece of %u groups", t.ng);
        const int rp = (int)(t.cam >> 8), x0 = 8 * (int)t.g0;
        const size_t got = yuv422_pack_run(L, packed + t.off, w, rp, (int)t.g0, (int)t.ng, planes, pitches);
        const int px = uyvy_run_px(w, (int)t.g0, (int)t.ng);
        CHECK(got == (size_t)4 * px, "pack_run size %zu for %d pixels", got, px);
        const uint8_t* p = packed + t.off;
        for (int row = 0; row < 2; row++)
            for (int x = 0; x < px; x++) {
                const int y = 2 * rp + row;
                uint8_t ly, ch;
                if (L == kYuv422Yuyv) {
                    ly = p[(size_t)row * 2 * px + 2 * x];
                    ch = p[(size_t)row * 2 * px + 2 * x + 1];
                } else {
                    ly = p[(size_t)row * px + x];
                    const uint8_t* c = p + 2 * px + (size_t)row * px;
                    ch = L == kYuv422Nv16 ? c[x] : c[(x & 1) * (px / 2) + x / 2];
                }
                CHECK(ly == pic.luma(x0 + x, y) && ch == pic.chroma(x0 + x, y), "pack_run L=%d w=%d rp=%d row=%d x=%d", L, w,
                      rp, row, x);
            }
        expect_off += got;
    }
    CHECK(expect_off == bytes, "table bytes");
    const size_t dst_bytes = (size_t)w * (h / 2 * 3);
    uint8_t* dst = tail_block(keep, dst_bytes, 0);
    memset(dst, 0x5A, dst_bytes);
    std::vector<int> writes(dst_bytes, 0);
    const uint8_t* src = packed_mode ? packed : frame;
    for (const UyvyRun& t : table)
        for (int k = -1; k <= (int)t.ng; k++) {
            const Yuv422Item it = yuv422_unpack_item(L, w, h, packed_mode ? 0 : pitch, t, k);
            if (k < 0 || k >= (int)t.ng) {
                CHECK(it.px <= 0, "an item outside its piece has pixels");
                continue;
            }
            CHECK(it.px > 0 && it.px <= 8 && !(it.px & 1), "item px %d", it.px);
            if (it.px <= 0) continue;
            CHECK(it.y0 + it.px <= dst_bytes && it.y1 + it.px <= dst_bytes && it.c + it.px <= dst_bytes, "store outside");
            if (it.y0 + it.px > dst_bytes || it.y1 + it.px > dst_bytes || it.c + it.px > dst_bytes) continue;
            yuv422_unpack_lane<L>(HostMem{}, src, dst, w, it);
            for (int p = 0; p < it.px; p++) {
                writes[it.y0 + p]++;
                writes[it.y1 + p]++;
                writes[it.c + p]++;
            }
        }
    std::vector<int> want_writes(dst_bytes, 0);
    std::vector<uint8_t> want(dst_bytes, 0x5A);
    for (const Run& r : runs) {
        const int rp = (int)(r.cam >> 8);
        const int px = uyvy_run_px(w, (int)r.g0, (int)r.ng);
        for (int p = 0; p < px; p++) {
            const int x = 8 * (int)r.g0 + p;
            const size_t y0 = (size_t)(2 * rp) * w + x, y1 = y0 + w, c = (size_t)(h + rp) * w + x;
            want[y0] = pic.luma(x, 2 * rp);
            want[y1] = pic.luma(x, 2 * rp + 1);
            want[c] = (uint8_t)((pic.chroma(x, 2 * rp) + pic.chroma(x, 2 * rp + 1) + 1) >> 1);
            want_writes[y0]++;
            want_writes[y1]++;
            want_writes[c]++;
        }
    }
    for (size_t i = 0; i < dst_bytes; i++) {
        CHECK(writes[i] == want_writes[i], "L=%d w=%d extra=%d align=%d packed=%d: byte %zu written %d times, want %d", L, w,
              extra, align, (int)packed_mode, i, writes[i], want_writes[i]);
        CHECK(dst[i] == want[i], "L=%d w=%d extra=%d align=%d packed=%d: byte %zu = %d, want %d", L, w, extra, align,
              (int)packed_mode, i, dst[i], want[i]);
    }
    for (void* p : keep) free(p);
}

template <int L>
void check_pack(int w, int h, int extra, int align) {
    std::vector<void*> keep;
    const size_t src_bytes = (size_t)w * (h / 2 * 3);
    uint8_t* src = tail_block(keep, src_bytes, 0);
    for (size_t i = 0; i < src_bytes; i++) src[i] = rnd();
    const int n = yuv422_frame_row_bytes(L, w), rows = yuv422_frame_rows(L, h);
    const size_t pitch = (size_t)n + extra;
    const size_t out_bytes = (size_t)(rows - 1) * pitch + (size_t)n;
    uint8_t* out = tail_block(keep, out_bytes, align);
    memset(out, 0xA5, out_bytes);
    std::vector<int> writes(out_bytes, 0);
    const uint32_t items = (uint32_t)yuv422_pack_items(L, w, h);
    for (uint32_t id = 0; id < items + 3; id++) {
        const Yuv422Span sp = yuv422_pack_item(L, w, h, pitch, reinterpret_cast<uintptr_t>(out), id);
        if (id >= items) {
            CHECK(sp.len == 0, "an item past the last one writes");
            continue;
        }
        if (sp.len == 0) continue;
        CHECK(sp.len > 0 && sp.len <= 16 && sp.b0 + sp.len <= sp.n && sp.row < yuv422_pack_rows(L, h), "span");
        CHECK(sp.dst + sp.len <= out_bytes, "span outside the frame");
        if (sp.dst + sp.len > out_bytes) continue;
        for (int i = 0; i < sp.len; i++)
            CHECK(yuv422_pack_src(L, w, h, sp.row, sp.b0 + i) < src_bytes, "source byte outside the frame");
        yuv422_pack_lane<L>(HostMem{}, src, out, w, h, sp);
        for (int i = 0; i < sp.len; i++) writes[sp.dst + i]++;
    }
    const Picture pic{L, w, h, out, pitch};
    for (int y = 0; y < rows; y++)
        for (size_t b = (size_t)n; b < pitch && (size_t)y * pitch + b < out_bytes; b++)
            CHECK(writes[(size_t)y * pitch + b] == 0 && out[(size_t)y * pitch + b] == 0xA5,
                  "L=%d w=%d extra=%d align=%d: pad byte (%d, %zu) written", L, w, extra, align, y, b);
    for (int y = 0; y < rows; y++)
        for (int b = 0; b < n; b++)
            CHECK(writes[(size_t)y * pitch + b] == 1, "L=%d w=%d extra=%d align=%d: byte (%d, %d) written %d times", L, w, extra,
                  align, y, b, writes[(size_t)y * pitch + b]);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            CHECK(pic.luma(x, y) == src[(size_t)y * w + x], "L=%d w=%d extra=%d align=%d: luma (%d, %d)", L, w, extra, align, x, y);
            CHECK(pic.chroma(x, y) == src[(size_t)(h + y / 2) * w + x], "L=%d w=%d extra=%d align=%d: chroma (%d, %d) = %d, want %d",
                  L, w, extra, align, x, y, pic.chroma(x, y), src[(size_t)(h + y / 2) * w + x]);
        }
    for (void* p : keep) free(p);
}

template <int L>
void check_layout() {
    const int widths[] = {8, 16, 24, 40, 10, 18, 42, 12, 44, 14, 46, 64, 66, 8 * 70, 8 * 66 + 2};
    for (int w : widths)
        for (int extra : {0, 6})
            for (int align = 0; align < 16; align++)
                for (int packed = 0; packed < 2; packed++) check_unpack<L>(w, 8, extra, align, packed != 0);
    for (int w : widths)
        for (int extra : {0, 6, 10})
            for (int align = 0; align < 16; align++) check_pack<L>(w, 6, extra, align);
}

}  // namespace

int main() {
    check_layout<kYuv422Yuyv>();
    check_layout<kYuv422Planar>();
    check_layout<kYuv422Nv16>();
    if (g_fail) {
        fprintf(stderr, "yuv422_check: %d failures\n", g_fail);
        return 1;
    }
    printf("yuv422_check ok\n");
    return 0;
}
