// yuv10_check.cpp — the arithmetic of the 10-bit conversions (csrc/yuv10_host.hpp: P010, YUV420P10, P210,
// YUV422P10) executed on the CPU for every work item of small geometries, against exactly sized heap blocks
// under the address and undefined-behaviour sanitizers: the lane bodies here are the templates
// yuv10_unpack_kernel and yuv10_pack_kernel instantiate, with memcpy as the memory policy.  For each layout:
//   samples: every 16-bit word through yuv10_narrow against the rule written out, and every dword pattern of
//     the edge values through the two-samples-per-dword narrowing against the per-sample one; widening back.
//   unpack: widths 8k, 8k + 2, 8k + 4, 8k + 6 and 328, 330, 332; pitches minimal and minimal + 6; every 2-byte
//     alignment of the source base within 16 and both source kinds (the caller's frame, the packed upload
//     buffer); an NV12 frame at an 8-byte aligned and at a 2 (mod 8) base; runs at the first and the last group
//     of a row, a one-group run, a run longer than one table piece.  Every footprint byte of the NV12 frame is
//     written exactly once with the value of the rule, nothing else is written, every 8-byte store is aligned,
//     and every read lies in the source block (the sanitizer's part: the blocks end where the frame or the
//     packed runs end).  The source carries random ignored bits, the edge values and the 4:2:2 row pairs (3, 6),
//     (1023, 1021), (2, 1), (1, 2).
//   yuv10_pack_run, from the host plane shapes of a push, equals a word-wise reference of the layout the unpack
//     item's offsets describe, at the offsets of yuv10_run_table; uyvy_run_table's own results are unchanged.
//   pack: the same widths, pitches (and + 10) and base alignments: every byte below a row's 2 w written exactly
//     once with the value of the rule (ignored bits 0), the bytes between that and the pitch never, every
//     16-byte store aligned; the unpack of the packed frame is the NV12 frame again (out-then-in).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "yuv10_host.hpp"

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

uint32_t rng_state = 1010u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 16;
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
    Yuv10Pair load8(const uint8_t* p) const {
        Yuv10Pair v;
        memcpy(&v, p, 8);
        return v;
    }
    UyvyWords load16(const uint8_t* p) const {
        UyvyWords v;
        memcpy(&v, p, 16);
        return v;
    }
    void store8(uint8_t* p, const Yuv10Pair& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 7u) == 0, "an 8-byte store is not aligned");
        memcpy(p, &v, 8);
    }
    void store16(uint8_t* p, const UyvyWords& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 15u) == 0, "a 16-byte store is not aligned");
        memcpy(p, &v, 16);
    }
};

// The rule, written out: the 10-bit sample of a word and its 8-bit value.
int sample10(int layout, uint16_t word) { return yuv10_planar(layout) ? word & 0x3FF : word >> 6; }
int rule8(int v10) {
    const int v = (v10 + 2) >> 2;
    return v > 255 ? 255 : v;
}
uint16_t rd16(const uint8_t* p) {
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}
void wr16(uint8_t* p, uint16_t v) { memcpy(p, &v, 2); }
// A word carrying v10 with random ignored bits.
uint16_t word_of(int layout, int v10) {
    const uint32_t junk = rnd();
    return yuv10_planar(layout) ? (uint16_t)(v10 | (junk & 0x3Fu) << 10) : (uint16_t)(v10 << 6 | (junk & 0x3Fu));
}

// The picture behind a frame of any layout: the words of luma (x, y) and of chroma sample x (U,V pairs: U of pixel
// pair x / 2 when x is even, else V) of chroma row y.
struct Picture {
    int layout, w, h;
    const uint8_t* f;
    size_t pitch;
    uint16_t luma(int x, int y) const { return rd16(f + (size_t)y * pitch + 2 * (size_t)x); }
    uint16_t chroma(int x, int y) const {
        const uint8_t* row = f + (size_t)(h + y) * pitch;
        return rd16(yuv10_planar(layout) ? row + (size_t)((x & 1) * w + (x / 2) * 2) : row + 2 * (size_t)x);
    }
};

const int kEdge[] = {1023, 1022, 1021, 1020, 6, 5, 3, 2, 1, 0};

void check_samples() {
    for (uint32_t w = 0; w < 0x10000u; w++) {
        CHECK(yuv10_narrow((uint16_t)w, true) == rule8((int)(w >> 6)), "narrow msb %u", w);
        CHECK(yuv10_narrow((uint16_t)w, false) == rule8((int)(w & 0x3FF)), "narrow lsb %u", w);
        const int p010 = (int)((w + 128u) >> 8);
        CHECK(yuv10_narrow((uint16_t)w, true) == (p010 > 255 ? 255 : p010), "P010 word form %u", w);
    }
    for (int v = 0; v < 256; v++) {
        CHECK(yuv10_widen((uint8_t)v, true) == (v << 8) && yuv10_widen((uint8_t)v, false) == (v << 2), "widen %d", v);
        CHECK(yuv10_narrow(yuv10_widen((uint8_t)v, true), true) == v && yuv10_narrow(yuv10_widen((uint8_t)v, false), false) == v,
              "out-then-in of %d", v);
    }
    // two samples per dword: every pair of edge values (1023 beside 0: the carries) with every ignored-bit pattern
    // of one half, against the per-sample rule
    for (int a : kEdge)
        for (int b : kEdge)
            for (uint32_t junk = 0; junk < 64; junk++)
                for (int side = 0; side < 2; side++) {
                    const uint32_t ja = side ? junk : 63u - junk, jb = side ? 63u - junk : junk;
                    const uint32_t dm = ((uint32_t)a << 6 | ja) | ((uint32_t)b << 6 | jb) << 16;
                    const uint32_t dl = ((uint32_t)a | ja << 10) | ((uint32_t)b | jb << 10) << 16;
                    const uint32_t m = yuv10_narrow2<true>(dm), l = yuv10_narrow2<false>(dl);
                    CHECK(((m >> 8) & 0xFF) == (uint32_t)rule8(a) && (m >> 24) == (uint32_t)rule8(b), "narrow2 msb %d %d", a, b);
                    CHECK(((l >> 8) & 0xFF) == (uint32_t)rule8(a) && (l >> 24) == (uint32_t)rule8(b), "narrow2 lsb %d %d", a, b);
                }
    CHECK(rule8(3) == 1 && rule8(6) == 2 && ((rule8(3) + rule8(6) + 1) >> 1) == 2, "the rule's own example");
}

template <int L>
void check_unpack(int w, int h, int extra, int align, bool packed_mode, int dst_align) {
    std::vector<void*> keep;
    const int G = (w + 7) / 8;
    const size_t row_bytes = (size_t)yuv10_frame_row_bytes(w), pitch = row_bytes + extra;
    const int rows = yuv10_frame_rows(L, h), c_rows = yuv10_chroma_rows(L, h), cpr = yuv10_is422(L) ? 2 : 1;
    const size_t frame_bytes = (size_t)(rows - 1) * pitch + row_bytes;
    uint8_t* frame = tail_block(keep, frame_bytes, align);
    for (size_t i = 0; i < frame_bytes; i++) frame[i] = (uint8_t)rnd();
    // row 0 and 1 of luma and chroma: the edge values, then 1023 beside 0; the 4:2:2 chroma row pairs of the rule
    for (int x = 0; x < w; x++) {
        wr16(frame + 2 * (size_t)x, word_of(L, kEdge[x % 10]));
        wr16(frame + pitch + 2 * (size_t)x, word_of(L, (x & 1) ? 0 : 1023));
        wr16(frame + (size_t)h * pitch + 2 * (size_t)x, word_of(L, (x & 1) ? 1023 : 0));
        if (cpr == 2) {
            const int pa[] = {3, 1023, 2, 1}, pb[] = {6, 1021, 1, 2};
            wr16(frame + (size_t)(h + 2) * pitch + 2 * (size_t)x, word_of(L, pa[(x / 2) % 4]));
            wr16(frame + (size_t)(h + 3) * pitch + 2 * (size_t)x, word_of(L, pb[(x / 2) % 4]));
        }
    }
    const Picture pic{L, w, h, frame, pitch};
    std::vector<Run> runs;
    const int rp_n = h / 2;
    runs.push_back(Run{0u | 0u << 8, 0u, (uint32_t)(G > 1 ? 2 : 1), 0});
    runs.push_back(Run{0u | (uint32_t)(rp_n - 1) << 8, (uint32_t)(G - 1), 1u, 0});
    if (G > 4) runs.push_back(Run{0u | 1u << 8, (uint32_t)(G / 2), 1u, 0});
    if (rp_n > 2) runs.push_back(Run{0u | 2u << 8, 0u, (uint32_t)G, 0});
    if (G > 6) runs.push_back(Run{0u | 1u << 8, (uint32_t)(G - 3), 3u, 0});
    size_t bytes = 0, bytes4 = 0;
    const std::vector<int> in_w{w};
    const std::vector<UyvyRun> table = yuv10_run_table(L, runs, in_w, bytes);
    const std::vector<UyvyRun> table4 = uyvy_run_table(runs, in_w, bytes4);
    CHECK(table.size() == table4.size() && bytes * 4 == bytes4 * (size_t)yuv10_run_bpp(L), "the table's pieces are UYVY's");
    // the host planes of a push: Y; the U,V plane, or U and V (exactly sized copies of the halves, which are no
    // blocks of their own inside the frame)
    const uint8_t* planes[3] = {frame, frame + (size_t)h * pitch, nullptr};
    size_t pitches[3] = {pitch, pitch, 0};
    if (yuv10_planar(L))
        for (int k = 0; k < 2; k++) {
            const size_t pp = (size_t)(w + (extra ? 4 : 0));
            uint8_t* p = tail_block(keep, (size_t)(c_rows - 1) * pp + w, align);
            for (int y = 0; y < c_rows; y++) memcpy(p + (size_t)y * pp, frame + (size_t)(h + y) * pitch + (size_t)k * w, w);
            planes[1 + k] = p;
            pitches[1 + k] = pp;
        }
    // the packed upload buffer: exactly `bytes`; each piece against a word-wise reference of its layout
    uint8_t* packed = tail_block(keep, bytes ? bytes : 1, align);
    size_t expect_off = 0;
    for (size_t ti = 0; ti < table.size(); ti++) {
        const UyvyRun& t = table[ti];
        CHECK(t.off == expect_off, "table offsets are not back to back");
        CHECK(t.cam == table4[ti].cam && t.g0 == table4[ti].g0 && t.ng == table4[ti].ng, "piece %zu differs from UYVY's", ti);
        CHECK(t.ng >= 1 && t.ng <= (uint32_t)kUyvyWave, "piece of %u groups", t.ng);
        const int rp = (int)(t.cam >> 8), x0 = 8 * (int)t.g0;
        const size_t got = yuv10_pack_run(L, packed + t.off, w, rp, (int)t.g0, (int)t.ng, planes, pitches);
        const int px = uyvy_run_px(w, (int)t.g0, (int)t.ng);
        CHECK(got == (size_t)yuv10_run_bpp(L) * px, "pack_run size %zu for %d pixels", got, px);
        const uint8_t* p = packed + t.off;
        for (int row = 0; row < 2; row++)
            for (int x = 0; x < px; x++)
                CHECK(rd16(p + (size_t)row * 2 * px + 2 * (size_t)x) == pic.luma(x0 + x, 2 * rp + row), "pack_run luma L=%d w=%d", L, w);
        for (int row = 0; row < cpr; row++)
            for (int x = 0; x < px; x++) {
                const uint8_t* c = p + (size_t)4 * px + (size_t)row * 2 * px;
                const uint16_t ch = rd16(yuv10_planar(L) ? c + (size_t)((x & 1) * px + (x / 2) * 2) : c + 2 * (size_t)x);
                CHECK(ch == pic.chroma(x0 + x, cpr * rp + row), "pack_run chroma L=%d w=%d rp=%d row=%d x=%d", L, w, rp, row, x);
            }
        expect_off += got;
    }
    CHECK(expect_off == bytes, "table bytes");
    const size_t dst_bytes = (size_t)w * (h / 2 * 3);
    uint8_t* dst = tail_block(keep, dst_bytes, dst_align);
    memset(dst, 0x5A, dst_bytes);
    std::vector<int> writes(dst_bytes, 0);
    const uint8_t* src = packed_mode ? packed : frame;
    for (const UyvyRun& t : table)
        for (int k = -1; k <= (int)t.ng; k++) {
            const Yuv10Item it = yuv10_unpack_item(L, w, h, packed_mode ? 0 : pitch, t, k);
            if (k < 0 || k >= (int)t.ng) {
                CHECK(it.px <= 0, "an item outside its piece has pixels");
                continue;
            }
            CHECK(it.px > 0 && it.px <= 8 && !(it.px & 1), "item px %d", it.px);
            if (it.px <= 0) continue;
            CHECK(it.y0 + it.px <= dst_bytes && it.y1 + it.px <= dst_bytes && it.c + it.px <= dst_bytes, "store outside");
            if (it.y0 + it.px > dst_bytes || it.y1 + it.px > dst_bytes || it.c + it.px > dst_bytes) continue;
            yuv10_unpack_lane<L>(HostMem{}, src, dst, w, it);
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
            want[y0] = (uint8_t)rule8(sample10(L, pic.luma(x, 2 * rp)));
            want[y1] = (uint8_t)rule8(sample10(L, pic.luma(x, 2 * rp + 1)));
            if (cpr == 2)
                want[c] = (uint8_t)((rule8(sample10(L, pic.chroma(x, 2 * rp))) + rule8(sample10(L, pic.chroma(x, 2 * rp + 1))) + 1) >> 1);
            else
                want[c] = (uint8_t)rule8(sample10(L, pic.chroma(x, rp)));
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
    for (size_t i = 0; i < src_bytes; i++) src[i] = (uint8_t)rnd();
    for (int x = 0; x < w && x < 4; x++) src[x] = (uint8_t)(x & 1 ? 255 : 0);
    const int n = yuv10_frame_row_bytes(w), rows = yuv10_frame_rows(L, h), cpr = yuv10_is422(L) ? 2 : 1;
    const size_t pitch = (size_t)n + extra;
    const size_t out_bytes = (size_t)(rows - 1) * pitch + (size_t)n;
    uint8_t* out = tail_block(keep, out_bytes, align);
    memset(out, 0xA5, out_bytes);
    std::vector<int> writes(out_bytes, 0);
    const uint32_t items = (uint32_t)yuv10_pack_items(L, w, h);
    for (uint32_t id = 0; id < items + 3; id++) {
        const Yuv10Span sp = yuv10_pack_item(L, w, h, pitch, reinterpret_cast<uintptr_t>(out), id);
        if (id >= items) {
            CHECK(sp.len == 0, "an item past the last one writes");
            continue;
        }
        if (sp.len == 0) continue;
        CHECK(sp.len > 0 && sp.len <= 16 && !(sp.len & 1) && !(sp.b0 & 1) && sp.b0 + sp.len <= sp.n && sp.row < yuv10_pack_rows(L, h),
              "span");
        CHECK(sp.dst + sp.len <= out_bytes, "span outside the frame");
        if (sp.dst + sp.len > out_bytes) continue;
        for (int i = 0; i < sp.len; i += 2)
            CHECK(yuv10_pack_src(L, w, h, sp.row, (sp.b0 + i) >> 1) < src_bytes, "source byte outside the frame");
        yuv10_pack_lane<L>(HostMem{}, src, out, w, h, sp);
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
    const int sh = yuv10_planar(L) ? 2 : 8;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            CHECK(pic.luma(x, y) == (uint16_t)(src[(size_t)y * w + x] << sh), "L=%d w=%d extra=%d align=%d: luma (%d, %d)", L, w,
                  extra, align, x, y);
            for (int k = 0; k < cpr; k++) {
                const int cy = cpr * (y / 2) + k;
                CHECK(pic.chroma(x, cy) == (uint16_t)(src[(size_t)(h + y / 2) * w + x] << sh),
                      "L=%d w=%d extra=%d align=%d: chroma (%d, %d) = %d, want %d", L, w, extra, align, x, cy, pic.chroma(x, cy),
                      src[(size_t)(h + y / 2) * w + x] << sh);
            }
        }
    // out-then-in: the whole packed frame through the unpack items is the NV12 frame again
    uint8_t* back = tail_block(keep, src_bytes, 0);
    memset(back, 0x5A, src_bytes);
    for (int rp = 0; rp < h / 2; rp++) {
        const UyvyRun r{(uint32_t)rp << 8, 0u, (uint32_t)((w + 7) / 8), 0u};
        for (int k = 0; k < (int)r.ng; k++) yuv10_unpack_lane<L>(HostMem{}, out, back, w, yuv10_unpack_item(L, w, h, pitch, r, k));
    }
    CHECK(memcmp(back, src, src_bytes) == 0, "L=%d w=%d extra=%d align=%d: out-then-in is not the identity", L, w, extra, align);
    for (void* p : keep) free(p);
}

template <int L>
void check_layout() {
    const int widths[] = {8, 16, 24, 40, 10, 18, 42, 12, 44, 14, 46, 64, 66, 328, 330, 332, 8 * 70, 8 * 66 + 2};
    for (int w : widths)
        for (int extra : {0, 6})
            for (int align = 0; align < 16; align += 2)
                for (int packed = 0; packed < 2; packed++) check_unpack<L>(w, 8, extra, align, packed != 0, align == 6 ? 2 : 0);
    for (int w : widths)
        for (int extra : {0, 6, 10})
            for (int align = 0; align < 16; align += 2) check_pack<L>(w, 6, extra, align);
}

}  // namespace

int main() {
    check_samples();
    check_layout<kYuv10P010>();
    check_layout<kYuv10Planar420>();
    check_layout<kYuv10P210>();
    check_layout<kYuv10Planar422>();
    if (g_fail) {
        fprintf(stderr, "yuv10_check: %d failures\n", g_fail);
        return 1;
    }
    printf("yuv10_check ok\n");
    return 0;
}
