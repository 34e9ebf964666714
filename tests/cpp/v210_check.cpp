// v210_check.cpp — the work items and lane bodies of OCTVR_PIX_V210 (csrc/v210_layout.hpp: what v210_unpack_kernel
// and v210_pack_kernel run) and its run packing (csrc/frame_layout.hpp run_table, pack_run) executed on the CPU for
// every work item of small geometries, against exactly sized heap blocks under the address and undefined-behaviour
// sanitizers, with memcpy as the memory policy.  What a v210 frame means is written out here from the format's
// definition (kBlock: the four words of a block, component by component), never taken from the header.
//   widths 48, 96, 146, 148, 150, 190, 256 (every w mod 6, w mod 8 class; 146 .. 150 and 190 with a short last
//   group, so every group word by word; 48, 96 and 256 on the vector path); heights 2 and 6; pitches row_bytes and
//   row_bytes + 4; bases 0 and 4 (mod 16).
//   check_unpack: the source is the caller's frame — its last row ends with the last block that holds a pixel, so a
//     load of a block past it is a heap overflow — or the packed upload of run_table / pack_run, sized by the table;
//     runs start at groups 0, 1 and 2 (the three phases) and end at the row's last group, one more is the last group
//     alone; the NV12 frame at an 8-byte aligned base and at 2 (mod 8) (every group word by word).  Every footprint
//     byte of the NV12 frame has the rule's value, every other byte is untouched, every 8-byte store is aligned.  The
//     source carries random bits in bits 31..30, in the absent components and in the padding blocks, the edge values
//     1023 .. 0 and the chroma row pairs (3, 6), (1023, 1021), (2, 1), (1, 2).
//   check_pack: every byte of row_bytes of every row has the rule's value (bits 31..30, absent components and padding
//     blocks 0), the bytes between row_bytes and the pitch keep the fill, every 16-byte store is 16-byte and every
//     4-byte store 4-byte aligned; the NV12 source ends with its last byte; unpacking the written frame gives the
//     NV12 frame again (out-then-in).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "v210_layout.hpp"

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

uint32_t rng_state = 210u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Run {
    uint32_t cam, g0, ng, off;
};

// n bytes whose first byte has address = align (mod 16) and whose last byte is the allocation's last byte
uint8_t* tail_block(std::vector<void*>& keep, size_t n, int align) {
    uint8_t* raw = (uint8_t*)malloc(n + (size_t)align);
    keep.push_back(raw);
    CHECK((reinterpret_cast<uintptr_t>(raw) & 15u) == 0, "malloc is not 16-byte aligned");
    return raw + align;
}
void release(std::vector<void*>& keep) {
    for (void* p : keep) free(p);
    keep.clear();
}

struct HostMem {
    uint32_t load4(const uint8_t* p) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 3u) == 0, "a word load is not aligned");
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
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
    void store4(uint8_t* p, uint32_t v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 3u) == 0, "a 4-byte store is not aligned");
        memcpy(p, &v, 4);
    }
    void store8(uint8_t* p, const Words2& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 7u) == 0, "an 8-byte store is not aligned");
        memcpy(p, &v, 8);
    }
    void store16(uint8_t* p, const Words4& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 15u) == 0, "a 16-byte store is not aligned");
        memcpy(p, &v, 16);
    }
};

// ---- the format, written out ------------------------------------------------------------------------------------
// word j of a block: its three components from bit 0, 10 and 20; 'y': luma of pixel 6 b + idx, 'b' / 'r': Cb / Cr of
// pixel pair 3 b + idx
struct Comp {
    char kind;
    int idx;
};
const Comp kBlock[4][3] = {{{'b', 0}, {'y', 0}, {'r', 0}},
                           {{'y', 1}, {'b', 1}, {'y', 2}},
                           {{'r', 1}, {'y', 3}, {'b', 2}},
                           {{'y', 4}, {'r', 2}, {'y', 5}}};
int ref_row_bytes(int w) { return 128 * ((w + 47) / 48); }
int ref_pixel_blocks(int w) { return (w + 5) / 6; }  // blocks that hold a pixel

struct Picture {  // 10-bit 4:2:2
    int w, h;
    std::vector<int> y, cb, cr;
};
const int kEdge[10] = {1023, 1022, 1021, 1020, 6, 5, 3, 2, 1, 0};
const int kPairs[4][2] = {{3, 6}, {1023, 1021}, {2, 1}, {1, 2}};
Picture make_picture(int w, int h) {
    Picture p{w, h, std::vector<int>((size_t)w * h), std::vector<int>((size_t)w / 2 * h), std::vector<int>((size_t)w / 2 * h)};
    for (int r = 0; r < h; r++) {
        for (int x = 0; x < w; x++) p.y[(size_t)r * w + x] = (r & 1) ? kEdge[(x + r) % 10] : (int)(rnd() & 1023u);
        for (int x = 0; x < w / 2; x++) {
            const int* pair = kPairs[(x + r / 2) % 4];
            p.cb[(size_t)r * (w / 2) + x] = (x % 3 == 0) ? pair[r & 1] : (r % 4 < 2) ? kEdge[(x + r) % 10] : (int)(rnd() & 1023u);
            p.cr[(size_t)r * (w / 2) + x] = (x % 3 == 1) ? pair[r & 1] : (int)(rnd() & 1023u);
        }
    }
    return p;
}
// the 10-bit component, or -1 where the picture has none (a pixel >= w)
int ref_comp(const Picture& p, int row, int b, const Comp& c) {
    if (c.kind == 'y') {
        const int x = 6 * b + c.idx;
        return x < p.w ? p.y[(size_t)row * p.w + x] : -1;
    }
    const int k = 3 * b + c.idx;
    if (k >= p.w / 2) return -1;
    return (c.kind == 'b' ? p.cb : p.cr)[(size_t)row * (p.w / 2) + k];
}
// the frame's word (row, block b, word j): junk = random bits wherever the format ignores them, else 0 there
uint32_t ref_word(const Picture& p, int row, int b, int j, bool junk) {
    uint32_t word = junk ? (rnd() & 3u) << 30 : 0u;
    for (int f = 0; f < 3; f++) {
        const int v = ref_comp(p, row, b, kBlock[j][f]);
        word |= (v >= 0 ? (uint32_t)v : junk ? rnd() & 1023u : 0u) << (10 * f);
    }
    return word;
}
int ref_narrow(int v10) {
    const int v = (v10 + 2) >> 2;
    return v > 255 ? 255 : v;
}
// the NV12 frame (pitch = w) of the picture by the in rule
std::vector<uint8_t> ref_nv12(const Picture& p) {
    std::vector<uint8_t> f((size_t)p.w * (p.h / 2 * 3));
    for (int r = 0; r < p.h; r++)
        for (int x = 0; x < p.w; x++) f[(size_t)r * p.w + x] = (uint8_t)ref_narrow(p.y[(size_t)r * p.w + x]);
    for (int r = 0; r < p.h / 2; r++)
        for (int k = 0; k < p.w / 2; k++) {
            const size_t a = (size_t)(2 * r) * (p.w / 2) + k, b = a + (size_t)(p.w / 2);
            f[(size_t)(p.h + r) * p.w + 2 * k] = (uint8_t)((ref_narrow(p.cb[a]) + ref_narrow(p.cb[b]) + 1) >> 1);
            f[(size_t)(p.h + r) * p.w + 2 * k + 1] = (uint8_t)((ref_narrow(p.cr[a]) + ref_narrow(p.cr[b]) + 1) >> 1);
        }
    return f;
}

// ---- in -----------------------------------------------------------------------------------------------------
void check_unpack(int w, int h, int pad, int base) {
    std::vector<void*> keep;
    const Picture pic = make_picture(w, h);
    const std::vector<uint8_t> want = ref_nv12(pic);
    const size_t rb = (size_t)ref_row_bytes(w), pitch = rb + (size_t)pad;
    CHECK((size_t)v210_row_bytes(w) == rb && (size_t)kLayoutV210.row_bytes(w) == rb && kLayoutV210.rows(h) == h &&
              kLayoutV210.planes() == 1 && kLayoutV210.plane_row_bytes(0, w) == (int)rb && kLayoutV210.plane_rows(0, h) == h,
          "w %d: the frame's shape", w);
    // the caller's frame: the last row ends with its last block that holds a pixel
    const size_t frame_bytes = (size_t)(h - 1) * pitch + 16 * (size_t)ref_pixel_blocks(w);
    uint8_t* const frame = tail_block(keep, frame_bytes, base);
    for (size_t i = 0; i < frame_bytes; i++) frame[i] = (uint8_t)rnd();  // padding blocks and the pitch's bytes: junk
    for (int r = 0; r < h; r++)
        for (int b = 0; b < ref_pixel_blocks(w); b++)
            for (int j = 0; j < 4; j++) {
                const uint32_t word = ref_word(pic, r, b, j, true);
                memcpy(frame + (size_t)r * pitch + 16 * (size_t)b + 4 * (size_t)j, &word, 4);
            }
    CHECK(kLayoutV210.aligned(frame, pitch) && !kLayoutV210.aligned(frame + 2, pitch) && !kLayoutV210.aligned(frame, pitch + 2) &&
              !kLayoutV210.aligned(frame + 1, pitch),
          "the alignment rule");
    CHECK(frame_fault(kLayoutV210, frame, pitch, w, h, 0x7FFFFFFFull) == nullptr &&
              frame_fault(kLayoutV210, frame, rb - 4, w, h, 0x7FFFFFFFull) != nullptr &&
              frame_fault(kLayoutV210, frame + 2, pitch, w, h, 0x7FFFFFFFull) != nullptr &&
              frame_fault(kLayoutV210, frame, pitch, w, h, (uint64_t)pitch * (uint64_t)h) != nullptr,
          "frame_fault");
    // the runs: from groups 0, 1, 2 to the row's last group, and the last group alone, in every row pair
    const int G = (w + 7) / 8;
    std::vector<Run> runs;
    std::vector<uint8_t> foot((size_t)w * (h / 2 * 3), 0);
    for (int rp = 0; rp < h / 2; rp++)
        for (int g0 : {0, 1, 2, G - 1}) {
            runs.push_back(Run{(uint32_t)rp << 8, (uint32_t)g0, (uint32_t)(G - g0), 0});
            for (int x = 8 * g0; x < w; x++)
                foot[(size_t)(2 * rp) * w + x] = foot[(size_t)(2 * rp + 1) * w + x] = foot[(size_t)(h + rp) * w + x] = 1;
        }
    size_t bytes = 0;
    const std::vector<FootRun> table = run_table(kLayoutV210, runs, std::vector<int>{w}, bytes);
    // the packed upload: each piece's covering blocks, row 2 rp then row 2 rp + 1, pieces back to back
    size_t expect = 0;
    for (const FootRun& t : table) {
        CHECK(t.ng <= (uint32_t)kWave && t.off == expect, "piece at %u, expected %zu", t.off, expect);
        const int b0 = 8 * (int)t.g0 / 6, end = 8 * (int)(t.g0 + t.ng) < w ? 8 * (int)(t.g0 + t.ng) : w;
        const int nb = (end + 5) / 6 - b0;
        CHECK(kLayoutV210.run_bytes(w, (int)t.g0, (int)t.ng) == (size_t)(32 * nb), "run_bytes");
        expect += (size_t)(32 * nb);
    }
    CHECK(bytes == expect, "the table's size %zu, expected %zu", bytes, expect);
    uint8_t* const packed = tail_block(keep, bytes, 0);
    const uint8_t* planes[3] = {frame, nullptr, nullptr};
    const size_t pitches[3] = {pitch, 0, 0};
    for (const FootRun& t : table) {
        const size_t got = pack_run(kLayoutV210, packed + t.off, w, (int)(t.cam >> 8), (int)t.g0, (int)t.ng, planes, pitches);
        const int b0 = 8 * (int)t.g0 / 6;
        CHECK(got == kLayoutV210.run_bytes(w, (int)t.g0, (int)t.ng), "pack_run's size");
        for (int row = 0; row < 2; row++)  // block by block against the frame
            for (size_t b = 0; b < got / 32; b++)
                CHECK(memcmp(packed + t.off + (size_t)row * (got / 2) + 16 * b,
                             frame + (size_t)(2 * (int)(t.cam >> 8) + row) * pitch + 16 * ((size_t)b0 + b), 16) == 0,
                      "pack_run: block %zu of row %d", b, row);
    }
    for (int packed_src = 0; packed_src < 2; packed_src++)
        for (int dst_align : {0, 2}) {  // 2 (mod 8): every group sample by sample
            std::vector<void*> keep_dst;
            uint8_t* const dst = tail_block(keep_dst, want.size(), dst_align);
            memset(dst, 0x5A, want.size());
            for (const FootRun& t : table)
                for (int k = 0; k < (int)t.ng; k++) {
                    const V210Item it = v210_unpack_item(w, h, packed_src ? 0 : pitch, t, k);
                    const int left = w - 8 * (int)(t.g0 + (uint32_t)k);
                    CHECK(it.px == (left < 8 ? left : 8) && it.ph == (8 * (int)(t.g0 + (uint32_t)k)) % 6, "item: px %d phase %d", it.px, it.ph);
                    v210_unpack_lane(HostMem{}, packed_src ? packed : frame, dst, w, it);
                }
            size_t bad = 0, stray = 0;
            for (size_t i = 0; i < want.size(); i++) {
                if (foot[i]) bad += dst[i] != want[i];
                else stray += dst[i] != 0x5A;
            }
            CHECK(bad == 0 && stray == 0, "unpack w %d h %d pad %d base %d packed %d dst %d: %zu wrong, %zu stray", w, h, pad, base,
                  packed_src, dst_align, bad, stray);
            // an item outside the piece or the frame does nothing
            CHECK(v210_unpack_item(w, h, pitch, table[0], (int)table[0].ng).px <= 0 && v210_unpack_item(w, h, pitch, table[0], -1).px <= 0,
                  "items outside the piece");
            release(keep_dst);
        }
    release(keep);
}

// ---- out ----------------------------------------------------------------------------------------------------
void check_pack(int w, int h, int pad, int base) {
    std::vector<void*> keep;
    const size_t rb = (size_t)ref_row_bytes(w), pitch = rb + (size_t)pad;
    const size_t nv_bytes = (size_t)w * (h / 2 * 3);
    uint8_t* const nv = tail_block(keep, nv_bytes, 1);
    for (size_t i = 0; i < nv_bytes; i++) nv[i] = (i % 7 == 0) ? 255 : (uint8_t)rnd();
    // the picture the out rule makes of it
    Picture pic{w, h, std::vector<int>((size_t)w * h), std::vector<int>((size_t)w / 2 * h), std::vector<int>((size_t)w / 2 * h)};
    for (int r = 0; r < h; r++) {
        for (int x = 0; x < w; x++) pic.y[(size_t)r * w + x] = nv[(size_t)r * w + x] << 2;
        for (int k = 0; k < w / 2; k++) {
            pic.cb[(size_t)r * (w / 2) + k] = nv[(size_t)(h + r / 2) * w + 2 * k] << 2;
            pic.cr[(size_t)r * (w / 2) + k] = nv[(size_t)(h + r / 2) * w + 2 * k + 1] << 2;
        }
    }
    const size_t out_bytes = (size_t)(h - 1) * pitch + rb;
    uint8_t* const out = tail_block(keep, out_bytes, base);
    memset(out, 0xA5, out_bytes);
    const uint64_t items = v210_pack_items(w, h);
    CHECK(items == (uint64_t)(rb / 16) * (uint64_t)h, "pack items");
    for (uint32_t id = 0; id < (uint32_t)items; id++) v210_pack_lane(HostMem{}, nv, out, v210_pack_item(w, h, pitch, id));
    CHECK(v210_pack_item(w, h, pitch, (uint32_t)items).row < 0, "an item past the last does nothing");
    size_t bad = 0, gap = 0;
    for (int r = 0; r < h; r++) {
        for (int b = 0; b < (int)(rb / 16); b++)
            for (int j = 0; j < 4; j++) {
                const uint32_t word = ref_word(pic, r, b, j, false);
                bad += memcmp(out + (size_t)r * pitch + 16 * (size_t)b + 4 * (size_t)j, &word, 4) != 0;
            }
        if (r + 1 < h)
            for (size_t i = rb; i < pitch; i++) gap += out[(size_t)r * pitch + i] != 0xA5;
    }
    CHECK(bad == 0 && gap == 0, "pack w %d h %d pad %d base %d: %zu wrong words, %zu bytes past the row written", w, h, pad, base, bad, gap);
    // out-then-in: every group of the written frame
    std::vector<void*> keep_dst;
    uint8_t* const back = tail_block(keep_dst, nv_bytes, 0);
    memset(back, 0x5A, nv_bytes);
    for (int rp = 0; rp < h / 2; rp++) {
        const FootRun r{(uint32_t)rp << 8, 0, (uint32_t)((w + 7) / 8), 0};
        for (int k = 0; k < (int)r.ng; k++) v210_unpack_lane(HostMem{}, out, back, w, v210_unpack_item(w, h, pitch, r, k));
    }
    CHECK(memcmp(back, nv, nv_bytes) == 0, "out-then-in w %d h %d pad %d base %d", w, h, pad, base);
    release(keep_dst);
    release(keep);
}

void check_words() {
    // every 10-bit value in each of a word's three places, beside the values that carry (1023) and that do not (0)
    for (int v = 0; v < 1024; v++)
        for (int f = 0; f < 3; f++)
            for (uint32_t other : {0u, 1023u}) {
                uint32_t word = 0xC0000000u;
                for (int k = 0; k < 3; k++) word |= (k == f ? (uint32_t)v : other) << (10 * k);
                const uint32_t t = v210_narrow3(word);
                for (int k = 0; k < 3; k++)
                    CHECK(((t >> (8 * k)) & 0xFFu) == (uint32_t)ref_narrow(k == f ? v : (int)other), "narrow3 of %08x: byte %d", word, k);
                CHECK((t >> 24) == 0, "narrow3's byte 3");
            }
    CHECK(layout_of(48).v210() && layout_of(48).converted() && !layout_of(47).converted() && !layout_of(49).converted(),
          "layout_of: 48 is v210, 47 and 49 nothing");
    bool any = false;
    with_layout(48, [&](auto) { any = true; });
    CHECK(!any, "with_layout has no case for v210");
}

}  // namespace

int main() {
    check_words();
    for (int w : {48, 96, 146, 148, 150, 190, 256})
        for (int h : {2, 6})
            for (int pad : {0, 4})
                for (int base : {0, 4}) {
                    check_unpack(w, h, pad, base);
                    check_pack(w, h, pad, base);
                }
    if (g_fail) {
        fprintf(stderr, "v210_check: %d failures\n", g_fail);
        return 1;
    }
    printf("v210_check ok\n");
    return 0;
}
