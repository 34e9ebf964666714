// uyvy_runs_check.cpp — the packed UYVY conversions' arithmetic (csrc/uyvy_host.hpp) executed on the CPU for
// every work item of small geometries, against exactly sized heap blocks under the address and undefined-
// behaviour sanitizers: the functions here are the ones uyvy_unpack_kernel and uyvy_pack_kernel run.
//   unpack: widths 8k, 8k + 2, 8k + 4, 8k + 6; pitches 2 w and 2 w + 6; every base alignment 0-15 of the source
//     and both source kinds (the caller's frame, the packed upload buffer); runs at the first and the last
//     group of a row, a one-group run, a run longer than one wave's piece.  Every footprint byte of the 4:2:0
//     frame is written exactly once with the value of the rule, nothing else is written, and every read lies in
//     the source block (the sanitizer's part: the blocks end where the frame or the packed runs end).
//   uyvy_pack_run equals a byte-wise reference.
//   pack: the same widths, pitches and base alignments: every byte below 2 w of every row written exactly once
//     with the value of the rule, the bytes between 2 w and the pitch never.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uyvy_host.hpp"

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

uint32_t rng_state = 12345u;
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

void emulate_unpack_lane(const uint8_t* src, uint8_t* dst, int w, const UyvyItem& it, bool vector) {
    if (vector) {
        UyvyWords a, b;
        memcpy(&a, src + it.s0, 16);
        memcpy(&b, src + it.s1, 16);
        const UyvyGroupOut o = uyvy_split_group(a, b);
        memcpy(dst + it.y0, o.y0, 8);
        memcpy(dst + it.y1, o.y1, 8);
        memcpy(dst + it.c, o.c, 8);
    } else {
        uyvy_unpack_bytes(src, dst, it);
    }
}

void check_unpack(int w, int h, size_t pitch, int align, bool packed_mode) {
    std::vector<void*> keep;
    const int G = (w + 7) / 8;
    // the caller's frame: h rows at `pitch`, the last one 2 w bytes
    const size_t frame_bytes = (size_t)(h - 1) * pitch + (size_t)2 * w;
    uint8_t* frame = tail_block(keep, frame_bytes, align);
    for (size_t i = 0; i < frame_bytes; i++) frame[i] = rnd();
    // carry cases of the packed-byte average in the first row pair
    for (int x = 0; x < 2 * w; x += 2) {
        frame[x] = (x & 4) ? 255 : 0;
        frame[pitch + x] = (x & 4) ? 254 : 1;
    }
    // runs: first group, last group, a one-group run in the middle, a whole row (longer than a wave when G > 64)
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
    // the packed upload buffer: exactly `bytes`, packed by uyvy_pack_run, checked against a byte-wise reference
    uint8_t* packed = tail_block(keep, bytes ? bytes : 1, align);
    size_t expect_off = 0;
    for (const UyvyRun& t : table) {
        CHECK(t.off == expect_off, "table offsets are not back to back");
        CHECK(t.ng >= 1 && t.ng <= (uint32_t)kUyvyWave, "piece of %u groups", t.ng);
        const int rp = (int)(t.cam >> 8);
        const size_t got = uyvy_pack_run(packed + t.off, w, rp, (int)t.g0, (int)t.ng, frame, pitch);
        const int px = uyvy_run_px(w, (int)t.g0, (int)t.ng);
        CHECK(got == (size_t)4 * px, "pack_run size %zu for %d pixels", got, px);
        for (int row = 0; row < 2; row++)
            for (int b = 0; b < 2 * px; b++)
                CHECK(packed[t.off + (size_t)row * 2 * px + b] == frame[(size_t)(2 * rp + row) * pitch + 16 * t.g0 + b],
                      "pack_run byte w=%d rp=%d row=%d b=%d", w, rp, row, b);
        expect_off += got;
    }
    CHECK(expect_off == bytes, "table bytes");
    // the destination frame, exactly sized; count the writes per byte
    const size_t dst_bytes = (size_t)w * (h / 2 * 3);
    uint8_t* dst = tail_block(keep, dst_bytes, 0);
    memset(dst, 0x5A, dst_bytes);
    std::vector<int> writes(dst_bytes, 0);
    const uint8_t* src = packed_mode ? packed : frame;
    for (const UyvyRun& t : table)
        for (int k = 0; k < (int)t.ng; k++) {
            const UyvyItem it = uyvy_unpack_item(w, h, packed_mode ? 0 : pitch, t, k);
            CHECK(it.px > 0 && it.px <= 8 && !(it.px & 1), "item px %d", it.px);
            if (it.px <= 0) continue;
            CHECK(it.y0 + it.px <= dst_bytes && it.y1 + it.px <= dst_bytes && it.c + it.px <= dst_bytes, "store outside");
            if (it.y0 + it.px > dst_bytes || it.y1 + it.px > dst_bytes || it.c + it.px > dst_bytes) continue;
            emulate_unpack_lane(src, dst, w, it, uyvy_unpack_vector(w, reinterpret_cast<uintptr_t>(dst), it));
            for (int p = 0; p < it.px; p++) {
                writes[it.y0 + p]++;
                writes[it.y1 + p]++;
                writes[it.c + p]++;
            }
        }
    // expected: the runs' cells by the rule (the runs above share no cell), 0x5A elsewhere; each written once
    std::vector<int> want_writes(dst_bytes, 0);
    std::vector<uint8_t> want(dst_bytes, 0x5A);
    for (const Run& r : runs) {
        const int rp = (int)(r.cam >> 8);
        const int px = uyvy_run_px(w, (int)r.g0, (int)r.ng);
        for (int p = 0; p < px; p++) {
            const int x = 8 * (int)r.g0 + p;
            const uint8_t* a = frame + (size_t)(2 * rp) * pitch;
            const uint8_t* b = a + pitch;
            const size_t y0 = (size_t)(2 * rp) * w + x, y1 = y0 + w, c = (size_t)(h + rp) * w + x;
            want[y0] = a[2 * x + 1];
            want[y1] = b[2 * x + 1];
            want[c] = (uint8_t)((a[2 * x] + b[2 * x] + 1) >> 1);  // chroma byte x of the row: U,V pairs
            want_writes[y0]++;
            want_writes[y1]++;
            want_writes[c]++;
        }
    }
    for (size_t i = 0; i < dst_bytes; i++) {
        CHECK(writes[i] == want_writes[i], "w=%d pitch=%zu align=%d packed=%d: byte %zu written %d times, want %d", w,
              pitch, align, (int)packed_mode, i, writes[i], want_writes[i]);
        CHECK(dst[i] == want[i], "w=%d pitch=%zu align=%d packed=%d: byte %zu = %d, want %d", w, pitch, align,
              (int)packed_mode, i, dst[i], want[i]);
    }
    for (void* p : keep) free(p);
}

void check_pack(int w, int h, size_t pitch, int align) {
    std::vector<void*> keep;
    const size_t src_bytes = (size_t)w * (h / 2 * 3);
    uint8_t* src = tail_block(keep, src_bytes, 0);
    for (size_t i = 0; i < src_bytes; i++) src[i] = rnd();
    const size_t out_bytes = (size_t)(h - 1) * pitch + (size_t)2 * w;
    uint8_t* out = tail_block(keep, out_bytes, align);
    memset(out, 0xA5, out_bytes);
    std::vector<int> writes(out_bytes, 0);
    const uint32_t items = (uint32_t)h * uyvy_pack_row_items(w);
    for (uint32_t id = 0; id < items + 3; id++) {
        const UyvySpan sp = uyvy_pack_item(w, h, pitch, reinterpret_cast<uintptr_t>(out), id);
        if (id >= items) {
            CHECK(sp.len == 0, "an item past the last one writes");
            continue;
        }
        if (sp.len == 0) continue;
        CHECK(sp.len > 0 && sp.len <= 16 && sp.b0 + sp.len <= 2 * w && sp.row < h, "span");
        CHECK(sp.dst == (size_t)sp.row * pitch + sp.b0, "span dst");
        if (sp.len == kUyvyChunk) {
            CHECK(((reinterpret_cast<uintptr_t>(out) + sp.dst) & 15u) == 0, "a full chunk is not 16-byte aligned");
            const UyvyChunkSrc cs = uyvy_pack_chunk_src(w, h, sp);
            CHECK(cs.first + 8 <= src_bytes && cs.second + 8 <= src_bytes, "chunk load outside the frame");
            uint32_t f[2], g[2];
            memcpy(f, src + cs.first, 8);
            memcpy(g, src + cs.second, 8);
            const UyvyWords o = uyvy_zip(f[0], f[1], g[0], g[1]);
            memcpy(out + sp.dst, &o, 16);
        } else {
            uyvy_pack_bytes(src, out, w, h, sp);
        }
        for (int i = 0; i < sp.len; i++) writes[sp.dst + i]++;
    }
    for (int y = 0; y < h; y++)
        for (size_t b = 0; b < pitch && (size_t)y * pitch + b < out_bytes; b++) {
            const size_t i = (size_t)y * pitch + b;
            if (b >= (size_t)2 * w) {
                CHECK(writes[i] == 0 && out[i] == 0xA5, "w=%d pitch=%zu align=%d: pad byte (%d, %zu) written", w, pitch, align, y, b);
                continue;
            }
            const uint8_t want = (b & 1) ? src[(size_t)y * w + (b >> 1)] : src[(size_t)(h + y / 2) * w + (b >> 1)];
            CHECK(writes[i] == 1, "w=%d pitch=%zu align=%d: byte (%d, %zu) written %d times", w, pitch, align, y, b, writes[i]);
            CHECK(out[i] == want, "w=%d pitch=%zu align=%d: byte (%d, %zu) = %d, want %d", w, pitch, align, y, b, out[i], want);
        }
    for (void* p : keep) free(p);
}

}  // namespace

int main() {
    // the four bytes of the averaged word never borrow from each other
    for (uint32_t a = 0; a < 256; a++)
        for (uint32_t b = 0; b < 256; b++) {
            const uint32_t x = a | (255u - a) << 8 | b << 16 | 0xFFu << 24, y = b | a << 8 | (255u - b) << 16 | 0xFEu << 24;
            const uint32_t got = uyvy_avg4(x, y);
            for (int k = 0; k < 4; k++) {
                const uint32_t p = (x >> (8 * k)) & 255u, q = (y >> (8 * k)) & 255u;
                CHECK(((got >> (8 * k)) & 255u) == ((p + q + 1) >> 1), "avg4(%u, %u)", p, q);
            }
        }
    const int widths[] = {8, 16, 24, 40, 10, 18, 42, 12, 44, 14, 46, 8 * 70, 8 * 66 + 2};
    for (int w : widths)
        for (int extra : {0, 6})
            for (int align = 0; align < 16; align++)
                for (int packed = 0; packed < 2; packed++) check_unpack(w, 8, (size_t)2 * w + extra, align, packed != 0);
    for (int w : widths)
        for (int extra : {0, 6, 10})
            for (int align = 0; align < 16; align++) check_pack(w, 6, (size_t)2 * w + extra, align);
    if (g_fail) {
        fprintf(stderr, "uyvy_runs_check: %d failures\n", g_fail);
        return 1;
    }
    printf("uyvy_runs_check ok\n");
    return 0;
}
