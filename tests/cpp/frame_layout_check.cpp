// frame_layout_check.cpp — the arithmetic of the converted capture layouts (csrc/frame_layout.hpp: UYVY, YUYV,
// YUV422P, NV16, P010, YUV420P10, P210, YUV422P10) executed on the CPU for every work item of small geometries,
// against exactly sized heap blocks under the address and undefined-behaviour sanitizers: the lane bodies here are
// the templates layout_unpack_kernel and layout_pack_kernel instantiate, with memcpy as the memory policy.  What a
// frame of a layout means (Picture, ref_*) is written out here per layout from the format definitions, never taken
// from the header's descriptors.
//   check_bytes: the four-byte average against the rule for every pair of bytes in every lane; the byte permute
//     with its zero selector.
//   check_samples: every 16-bit word through the per-sample narrowing against the rule written out, every dword
//     pattern of the edge values through the two-samples-per-dword narrowing; widening and back.
//   check_descriptors: layout_of against the formats' row bytes, rows and packed bytes per pixel; the values that
//     are no converted format.
//   check_planes: for all ten layouts (the two native 4:2:0 ones included) the frame's row bytes, rows and packed
//     bytes per pixel and each host plane's row bytes and rows against the table of the header's comment, written
//     out here in numbers; frame_fault's four refusals at each call's own limit.
//   check_row_chunks: rows of 0, 1, 15, 16, 17, 31 and 33 bytes at all 16 alignments: the items tile the row exactly
//     once, in order, and a full 16-byte item is 16-byte aligned; items past the row's last are empty.
//   check_unpack, for each layout: widths 8k, 8k + 2, 8k + 4, 8k + 6 and 328, 330, 332; pitches minimal and
//     minimal + 6; every alignment of the source base within 16 (every even one for 16-bit samples) and both
//     source kinds (the caller's frame, the packed upload buffer); an NV12 frame at an 8-byte aligned and at a 2
//     (mod 8) base; runs at the first and the last group of a row, a one-group run, a run longer than one table
//     piece.  Every footprint byte of the NV12 frame is written exactly once with the value of the rule, nothing
//     else is written, every 8-byte store is aligned, and every read lies in the source block (the sanitizer's
//     part: the blocks end where the frame or the packed runs end).  The source carries the carries of the average
//     (0 + 1, 255 + 254) or, as words, random ignored bits, the edge values and the row pairs (3, 6), (1023, 1021),
//     (2, 1), (1, 2).  The run table: pieces back to back at the layout's bytes per pixel, none longer than
//     kWave, the same pieces for every layout.  pack_run, from the host plane shapes of a push, equals a
//     sample-wise reference of the piece.
//   check_pack, for each layout: the same widths, pitches (and + 10) and base alignments: every byte below a row's
//     width written exactly once with the value of the rule (ignored bits 0), the bytes between that and the pitch
//     never, every 16-byte store aligned; the unpack of the written frame is the NV12 frame again (out-then-in).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "frame_layout.hpp"

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
    uint32_t load4(const uint8_t* p) const {
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
    void store8(uint8_t* p, const Words2& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 7u) == 0, "an 8-byte store is not aligned");
        memcpy(p, &v, 8);
    }
    void store16(uint8_t* p, const Words4& v) const {
        CHECK((reinterpret_cast<uintptr_t>(p) & 15u) == 0, "a 16-byte store is not aligned");
        memcpy(p, &v, 16);
    }
};

// ---- the formats, written out ---------------------------------------------------------------------------------
enum Pix { UYVY = 16, YUYV = 17, YUV422P = 18, NV16 = 19, P010 = 32, YUV420P10 = 33, P210 = 34, YUV422P10 = 35 };
const char* name(int pix) {
    switch (pix) {
    case UYVY: return "UYVY";
    case YUYV: return "YUYV";
    case YUV422P: return "YUV422P";
    case NV16: return "NV16";
    case P010: return "P010";
    case YUV420P10: return "YUV420P10";
    case P210: return "P210";
    default: return "YUV422P10";
    }
}
bool ref_words(int pix) { return pix == P010 || pix == YUV420P10 || pix == P210 || pix == YUV422P10; }
bool ref_low_bits(int pix) { return pix == YUV420P10 || pix == YUV422P10; }  // the sample in bits 9..0, else 15..6
int ref_chroma_rows(int pix, int h) { return pix == P010 || pix == YUV420P10 ? h / 2 : h; }
int ref_row_bytes(int pix, int w) { return pix == YUV422P || pix == NV16 ? w : 2 * w; }
int ref_rows(int pix, int h) { return pix == UYVY || pix == YUYV ? h : h + ref_chroma_rows(pix, h); }
int ref_run_bpp(int pix) { return pix == P210 || pix == YUV422P10 ? 8 : pix == P010 || pix == YUV420P10 ? 6 : 4; }

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
// The 8-bit value of a stored sample by the in rule, and the stored sample of an 8-bit value by the out rule.
int ref_value8(int pix, uint16_t raw) { return !ref_words(pix) ? raw : rule8(ref_low_bits(pix) ? raw & 0x3FF : raw >> 6); }
uint16_t ref_stored(int pix, uint8_t v8) { return !ref_words(pix) ? v8 : (uint16_t)(ref_low_bits(pix) ? v8 << 2 : v8 << 8); }
// A stored sample of value v (8 or 10 bits) with random ignored bits.
uint16_t sample_of(int pix, int v) {
    const uint32_t junk = rnd();
    if (!ref_words(pix)) return (uint16_t)v;
    return ref_low_bits(pix) ? (uint16_t)(v | (junk & 0x3Fu) << 10) : (uint16_t)(v << 6 | (junk & 0x3Fu));
}

// The picture behind a frame of any layout: the stored samples of luma (x, y) and of chroma sample x (as U,V pairs:
// U of pixel pair x / 2 when x is even, else V) of chroma row y.
struct Picture {
    int pix, w, h;
    uint8_t* f;
    size_t pitch;
    uint8_t* luma_at(int x, int y) const {
        uint8_t* row = f + (size_t)y * pitch;
        switch (pix) {
        case UYVY: return row + 2 * x + 1;  // U0 Y0 V0 Y1
        case YUYV: return row + 2 * x;      // Y0 U0 Y1 V0
        case YUV422P:
        case NV16: return row + x;
        default: return row + 2 * x;  // words
        }
    }
    uint8_t* chroma_at(int x, int y) const {
        switch (pix) {
        case UYVY: return f + (size_t)y * pitch + 2 * x;
        case YUYV: return f + (size_t)y * pitch + 2 * x + 1;
        case NV16: return f + (size_t)(h + y) * pitch + x;
        case YUV422P: return f + (size_t)(h + y) * pitch + (x & 1) * (w / 2) + x / 2;  // [U | V] halves
        case P010:
        case P210: return f + (size_t)(h + y) * pitch + 2 * x;
        default: return f + (size_t)(h + y) * pitch + (x & 1) * w + (x / 2) * 2;  // [U | V] halves of words
        }
    }
    uint16_t get(const uint8_t* p) const { return ref_words(pix) ? rd16(p) : *p; }
    void set(uint8_t* p, uint16_t v) const {
        if (ref_words(pix))
            wr16(p, v);
        else
            *p = (uint8_t)v;
    }
    uint16_t luma(int x, int y) const { return get(luma_at(x, y)); }
    uint16_t chroma(int x, int y) const { return get(chroma_at(x, y)); }
};

// Sample x of row `row` (0, 1) of luma, or of chroma row `row`, of a packed piece of px pixels at p: two packed
// rows; or two luma rows, then the chroma row(s), a [U | V] layout's U part before its V part.
uint16_t piece_sample(int pix, const uint8_t* p, int px, bool chroma, int row, int x) {
    const int S = ref_words(pix) ? 2 : 1;
    const uint8_t* at;
    if (pix == UYVY || pix == YUYV) {
        at = p + (size_t)row * 2 * px + 2 * x + ((pix == UYVY) != chroma ? 1 : 0);
    } else if (!chroma) {
        at = p + (size_t)row * S * px + (size_t)S * x;
    } else {
        const uint8_t* c = p + (size_t)2 * S * px + (size_t)row * S * px;
        const bool halves = pix == YUV422P || pix == YUV420P10 || pix == YUV422P10;
        at = halves ? c + (size_t)(x & 1) * (S * px / 2) + (size_t)S * (x / 2) : c + (size_t)S * x;
    }
    return S == 2 ? rd16(at) : *at;
}

const int kEdge[] = {1023, 1022, 1021, 1020, 6, 5, 3, 2, 1, 0};

void check_bytes() {
    // the four bytes of the averaged word never borrow from each other
    for (uint32_t a = 0; a < 256; a++)
        for (uint32_t b = 0; b < 256; b++) {
            const uint32_t x = a | (255u - a) << 8 | b << 16 | 0xFFu << 24, y = b | a << 8 | (255u - b) << 16 | 0xFEu << 24;
            const uint32_t got = avg4(x, y);
            for (int k = 0; k < 4; k++) {
                const uint32_t p = (x >> (8 * k)) & 255u, q = (y >> (8 * k)) & 255u;
                CHECK(((got >> (8 * k)) & 255u) == ((p + q + 1) >> 1), "avg4(%u, %u)", p, q);
            }
            CHECK(avg1((uint8_t)a, (uint8_t)b) == ((a + b + 1) >> 1), "avg1(%u, %u)", a, b);
        }
    CHECK(perm(0x77665544u, 0x33221100u, 0x07050301u) == 0x77553311u && perm(0x77665544u, 0x33221100u, 0x06040200u) == 0x66442200u,
          "perm selects bytes");
    CHECK(perm(0x77665544u, 0x33221100u, 0x0c010c00u) == 0x00110000u && perm(0, 0xDDCCBBAAu, 0x030c010cu) == 0xDD00BB00u,
          "perm's selector 0x0c is a zero byte");
}

void check_samples() {
    const LayoutDesc msb = LayoutP010::desc, lsb = LayoutYuv420p10::desc;
    for (uint32_t w = 0; w < 0x10000u; w++) {
        uint8_t b[2];
        wr16(b, (uint16_t)w);
        CHECK(narrow_at(msb, b) == rule8((int)(w >> 6)), "narrow msb %u", w);
        CHECK(narrow_at(lsb, b) == rule8((int)(w & 0x3FF)), "narrow lsb %u", w);
        const int p010 = (int)((w + 128u) >> 8);
        CHECK(narrow_at(msb, b) == (p010 > 255 ? 255 : p010), "P010 word form %u", w);
    }
    for (int v = 0; v < 256; v++) {
        uint8_t m[2], l[2], one[1];
        widen_at(msb, m, (uint8_t)v);
        widen_at(lsb, l, (uint8_t)v);
        widen_at(LayoutNv16::desc, one, (uint8_t)v);
        CHECK(rd16(m) == (v << 8) && rd16(l) == (v << 2) && one[0] == v, "widen %d", v);
        CHECK(narrow_at(msb, m) == v && narrow_at(lsb, l) == v && narrow_at(LayoutNv16::desc, one) == v, "out-then-in of %d", v);
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
                    const uint32_t m = narrow2<true>(dm), l = narrow2<false>(dl);
                    CHECK(((m >> 8) & 0xFF) == (uint32_t)rule8(a) && (m >> 24) == (uint32_t)rule8(b), "narrow2 msb %d %d", a, b);
                    CHECK(((l >> 8) & 0xFF) == (uint32_t)rule8(a) && (l >> 24) == (uint32_t)rule8(b), "narrow2 lsb %d %d", a, b);
                }
    CHECK(rule8(3) == 1 && rule8(6) == 2 && ((rule8(3) + rule8(6) + 1) >> 1) == 2, "the rule's own example");
}

// The header comment's table for a 16 x 4 picture, in numbers, and per host plane (Y / packed; U or U,V; V) its
// row bytes and rows: -1 = no such plane.
void check_planes() {
    const struct {
        int pix, row_bytes, rows, run_bpp, planes;
        int plane_bytes[3], plane_rows[3];
    } T[10] = {
        {0, 16, 6, 3, 3, {16, 8, 8}, {4, 2, 2}},     // YUV420P
        {1, 16, 6, 3, 2, {16, 16, -1}, {4, 2, -1}},  // NV12
        {16, 32, 4, 4, 1, {32, -1, -1}, {4, -1, -1}},  // UYVY422
        {17, 32, 4, 4, 1, {32, -1, -1}, {4, -1, -1}},  // YUYV422
        {18, 16, 8, 4, 3, {16, 8, 8}, {4, 4, 4}},      // YUV422P
        {19, 16, 8, 4, 2, {16, 16, -1}, {4, 4, -1}},   // NV16
        {32, 32, 6, 6, 2, {32, 32, -1}, {4, 2, -1}},   // P010
        {33, 32, 6, 6, 3, {32, 16, 16}, {4, 2, 2}},    // YUV420P10
        {34, 32, 8, 8, 2, {32, 32, -1}, {4, 4, -1}},   // P210
        {35, 32, 8, 8, 3, {32, 16, 16}, {4, 4, 4}},    // YUV422P10
    };
    for (const auto& t : T) {
        const LayoutDesc d = layout_of(t.pix);
        CHECK(d.bytes != 0 && d.native == (t.pix < 2) && d.converted() == (t.pix >= 16) && converted_format(t.pix) == (t.pix >= 16),
              "%d: native / converted", t.pix);
        CHECK(d.row_bytes(16) == t.row_bytes && d.rows(4) == t.rows && d.run_bpp() == t.run_bpp, "%d: frame %d x %d, %d B / pixel",
              t.pix, d.row_bytes(16), d.rows(4), d.run_bpp());
        CHECK(d.planes() == t.planes, "%d: %d planes", t.pix, d.planes());
        int frame_rows = 0;
        for (int k = 0; k < t.planes; k++) {
            CHECK(d.plane_row_bytes(k, 16) == t.plane_bytes[k] && d.plane_rows(k, 4) == t.plane_rows[k], "%d: plane %d is %d x %d", t.pix, k,
                  d.plane_row_bytes(k, 16), d.plane_rows(k, 4));
            frame_rows += k < 2 ? d.plane_rows(k, 4) : 0;  // V lies beside U in the frame's chroma rows
        }
        CHECK(frame_rows == t.rows, "%d: the planes' rows are the frame's", t.pix);
        // frame_fault: the limit is the caller's, the first byte count refused
        uint8_t* const even = reinterpret_cast<uint8_t*>(uintptr_t(0x1000));
        const size_t rb = (size_t)t.row_bytes;
        CHECK(frame_fault(d, even, rb, 16, 4, rb * t.rows + 1) == nullptr, "%d: a frame at its minimal pitch", t.pix);
        CHECK(frame_fault(d, even, rb, 16, 4, rb * t.rows) != nullptr, "%d: a frame of `limit` bytes", t.pix);
        CHECK(frame_fault(d, even, rb - 2, 16, 4, 1u << 30) != nullptr, "%d: a pitch below the row", t.pix);
        CHECK(frame_fault(d, nullptr, rb, 16, 4, 1u << 30) != nullptr, "%d: a NULL frame", t.pix);
        CHECK((frame_fault(d, even + 1, rb, 16, 4, 1u << 30) != nullptr) == (d.bytes == 2), "%d: an odd base", t.pix);
        CHECK((frame_fault(d, even, rb + 1, 16, 4, 1u << 30) != nullptr) == (d.bytes == 2), "%d: an odd pitch", t.pix);
    }
    CHECK(layout_of(2).bytes == 0 && layout_of(-1).bytes == 0 && layout_of(36).bytes == 0, "values that are no layout");
}

void check_row_chunks() {
    CHECK(kChunk == 16, "a chunk is one 16-byte store");
    for (int n : {0, 1, 15, 16, 17, 31, 33})
        for (uintptr_t align = 0; align < 16; align++) {
            const uintptr_t a = 0x4000u + align;
            const int items = (int)row_items(n);
            int next = 0;  // the first byte no item has covered yet
            for (int k = 0; k < items + 2; k++) {
                struct {
                    int b0, len;
                } c{0, 0};  // the item as the callers read it: the head, a chunk, or nothing past the row's end
                const RowChunk rc = row_chunk(a, n, k);
                if (k == 0)
                    c = {0, rc.head};
                else if (rc.b0 < n)
                    c = {rc.b0, rc.len(n)};
                CHECK(c.len >= 0 && c.len <= kChunk, "n=%d align=%d item %d: len %d", n, (int)align, k, c.len);
                if (c.len == 0) continue;
                CHECK(k < items, "n=%d align=%d: item %d past row_items writes", n, (int)align, k);
                CHECK(c.b0 == next, "n=%d align=%d item %d: starts at %d, want %d", n, (int)align, k, c.b0, next);
                CHECK(c.len != kChunk || ((a + (uintptr_t)c.b0) & 15u) == 0, "n=%d align=%d item %d: a full chunk off its boundary", n,
                      (int)align, k);
                CHECK(k == 0 || ((a + (uintptr_t)c.b0) & 15u) == 0, "n=%d align=%d item %d: a chunk off its boundary", n, (int)align, k);
                next = c.b0 + c.len;
            }
            CHECK(next == n, "n=%d align=%d: the items cover %d bytes", n, (int)align, next);
        }
}

template <class L>
void check_descriptor(int pix) {
    const LayoutDesc d = layout_of(pix), t = L::desc;
    CHECK(d.converted() && converted_format(pix), "%s is a converted format", name(pix));
    CHECK(d.bytes == t.bytes && d.msb == t.msb && d.chroma == t.chroma && d.luma_odd == t.luma_odd && d.chroma_rows == t.chroma_rows,
          "%s: layout_of is not the layout's tag", name(pix));
    for (int n : {2, 6, 8, 330})
        CHECK(d.row_bytes(n) == ref_row_bytes(pix, n) && d.rows(n) == ref_rows(pix, n), "%s: frame of size %d", name(pix), n);
    CHECK(d.run_bpp() == ref_run_bpp(pix), "%s: %d packed bytes per pixel", name(pix), d.run_bpp());
    uint8_t* const odd = reinterpret_cast<uint8_t*>(uintptr_t(0x1001)), *const even = reinterpret_cast<uint8_t*>(uintptr_t(0x1002));
    CHECK(d.aligned(even, 64) && d.aligned(odd, 64) == !ref_words(pix) && d.aligned(even, 63) == !ref_words(pix), "%s: aligned", name(pix));
}

template <class L>
void check_unpack(int pix, int w, int h, int extra, int align, bool packed_mode, int dst_align) {
    std::vector<void*> keep;
    const LayoutDesc d = L::desc;
    const int G = (w + 7) / 8, S = ref_words(pix) ? 2 : 1;
    const size_t row_bytes = (size_t)ref_row_bytes(pix, w), pitch = row_bytes + extra;
    const int rows = ref_rows(pix, h), c_rows = ref_chroma_rows(pix, h), cpr = c_rows == h ? 2 : 1;
    const size_t frame_bytes = (size_t)(rows - 1) * pitch + row_bytes;
    uint8_t* frame = tail_block(keep, frame_bytes, align);
    for (size_t i = 0; i < frame_bytes; i++) frame[i] = (uint8_t)rnd();
    const Picture pic{pix, w, h, frame, pitch};
    for (int x = 0; x < w; x++) {
        if (S == 1) {  // carry cases of the average in the first row pair's chroma: 0 + 1, 255 + 254
            pic.set(pic.chroma_at(x, 0), (x & 2) ? 255 : 0);
            pic.set(pic.chroma_at(x, 1), (x & 2) ? 254 : 1);
            continue;
        }
        // rows 0 and 1 of luma and chroma row 0: the edge values, then 1023 beside 0; the chroma row pairs of the rule
        pic.set(pic.luma_at(x, 0), sample_of(pix, kEdge[x % 10]));
        pic.set(pic.luma_at(x, 1), sample_of(pix, (x & 1) ? 0 : 1023));
        pic.set(pic.chroma_at(x, 0), sample_of(pix, (x / 2 + x) & 1 ? 1023 : 0));
        if (cpr == 2) {
            const int pa[] = {3, 1023, 2, 1}, pb[] = {6, 1021, 1, 2};
            pic.set(pic.chroma_at(x, 2), sample_of(pix, pa[(x / 2) % 4]));
            pic.set(pic.chroma_at(x, 3), sample_of(pix, pb[(x / 2) % 4]));
        }
    }
    // runs: first group, last group, a one-group run in the middle, a whole row (longer than a piece when G > 64)
    std::vector<Run> runs;
    const int rp_n = h / 2;
    runs.push_back(Run{0u | 0u << 8, 0u, (uint32_t)(G > 1 ? 2 : 1), 0});
    runs.push_back(Run{0u | (uint32_t)(rp_n - 1) << 8, (uint32_t)(G - 1), 1u, 0});
    if (G > 4) runs.push_back(Run{0u | 1u << 8, (uint32_t)(G / 2), 1u, 0});
    if (rp_n > 2) runs.push_back(Run{0u | 2u << 8, 0u, (uint32_t)G, 0});
    if (G > 6) runs.push_back(Run{0u | 1u << 8, (uint32_t)(G - 3), 3u, 0});
    size_t bytes = 0, bytes4 = 0;
    const std::vector<int> in_w{w};
    const std::vector<ConvRun> table = run_table(d, runs, in_w, bytes);
    const std::vector<ConvRun> table4 = run_table(LayoutUyvy::desc, runs, in_w, bytes4);
    CHECK(table.size() == table4.size() && bytes * 4 == bytes4 * (size_t)ref_run_bpp(pix), "%s: the table's pieces are UYVY's", name(pix));
    // the host planes of a push: the packed frame; Y and the U,V plane; or Y, U and V (exactly sized copies of the
    // halves, which are no blocks of their own inside the frame)
    const uint8_t* planes[3] = {frame, frame + (size_t)h * pitch, nullptr};
    size_t pitches[3] = {pitch, pitch, 0};
    if (pix == UYVY || pix == YUYV) planes[1] = nullptr;
    if (pix == YUV422P || pix == YUV420P10 || pix == YUV422P10)
        for (int k = 0; k < 2; k++) {
            const size_t half = (size_t)(S * w / 2), pp = half + (extra ? (S == 2 ? 4 : 3) : 0);
            uint8_t* p = tail_block(keep, (size_t)(c_rows - 1) * pp + half, align);
            for (int y = 0; y < c_rows; y++) memcpy(p + (size_t)y * pp, frame + (size_t)(h + y) * pitch + (size_t)k * half, half);
            planes[1 + k] = p;
            pitches[1 + k] = pp;
        }
    // the packed upload buffer: exactly `bytes`; each piece against a sample-wise reference of its layout
    uint8_t* packed = tail_block(keep, bytes ? bytes : 1, align);
    size_t expect_off = 0;
    for (size_t ti = 0; ti < table.size(); ti++) {
        const ConvRun& t = table[ti];
        CHECK(t.off == expect_off, "table offsets are not back to back");
        CHECK(t.cam == table4[ti].cam && t.g0 == table4[ti].g0 && t.ng == table4[ti].ng, "piece %zu differs from UYVY's", ti);
        CHECK(t.ng >= 1 && t.ng <= (uint32_t)kWave, "piece of %u groups", t.ng);
        const int rp = (int)(t.cam >> 8), x0 = 8 * (int)t.g0;
        const size_t got = pack_run(d, packed + t.off, w, rp, (int)t.g0, (int)t.ng, planes, pitches);
        const int px = run_px(w, (int)t.g0, (int)t.ng);
        CHECK(got == (size_t)ref_run_bpp(pix) * px, "pack_run size %zu for %d pixels", got, px);
        const uint8_t* p = packed + t.off;
        for (int x = 0; x < px; x++) {
            for (int row = 0; row < 2; row++)
                CHECK(piece_sample(pix, p, px, false, row, x) == pic.luma(x0 + x, 2 * rp + row), "pack_run luma %s w=%d rp=%d row=%d x=%d",
                      name(pix), w, rp, row, x);
            for (int row = 0; row < cpr; row++)
                CHECK(piece_sample(pix, p, px, true, row, x) == pic.chroma(x0 + x, cpr * rp + row),
                      "pack_run chroma %s w=%d rp=%d row=%d x=%d", name(pix), w, rp, row, x);
        }
        expect_off += got;
    }
    CHECK(expect_off == bytes, "table bytes");
    // the destination frame, exactly sized; count the writes per byte
    const size_t dst_bytes = (size_t)w * (h / 2 * 3);
    uint8_t* dst = tail_block(keep, dst_bytes, dst_align);
    memset(dst, 0x5A, dst_bytes);
    std::vector<int> writes(dst_bytes, 0);
    const uint8_t* src = packed_mode ? packed : frame;
    for (const ConvRun& t : table)
        for (int k = -1; k <= (int)t.ng; k++) {
            const LayoutItem it = unpack_item(d, w, h, packed_mode ? 0 : pitch, t, k);
            if (k < 0 || k >= (int)t.ng) {
                CHECK(it.px <= 0, "an item outside its piece has pixels");
                continue;
            }
            CHECK(it.px > 0 && it.px <= 8 && !(it.px & 1), "item px %d", it.px);
            if (it.px <= 0) continue;
            CHECK(it.y0 + it.px <= dst_bytes && it.y1 + it.px <= dst_bytes && it.c + it.px <= dst_bytes, "store outside");
            if (it.y0 + it.px > dst_bytes || it.y1 + it.px > dst_bytes || it.c + it.px > dst_bytes) continue;
            unpack_lane<L>(HostMem{}, src, dst, w, it);
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
        const int px = run_px(w, (int)r.g0, (int)r.ng);
        for (int p = 0; p < px; p++) {
            const int x = 8 * (int)r.g0 + p;
            const size_t y0 = (size_t)(2 * rp) * w + x, y1 = y0 + w, c = (size_t)(h + rp) * w + x;
            want[y0] = (uint8_t)ref_value8(pix, pic.luma(x, 2 * rp));
            want[y1] = (uint8_t)ref_value8(pix, pic.luma(x, 2 * rp + 1));
            if (cpr == 2)
                want[c] = (uint8_t)((ref_value8(pix, pic.chroma(x, 2 * rp)) + ref_value8(pix, pic.chroma(x, 2 * rp + 1)) + 1) >> 1);
            else
                want[c] = (uint8_t)ref_value8(pix, pic.chroma(x, rp));
            want_writes[y0]++;
            want_writes[y1]++;
            want_writes[c]++;
        }
    }
    for (size_t i = 0; i < dst_bytes; i++) {
        CHECK(writes[i] == want_writes[i], "unpack %s w=%d extra=%d align=%d packed=%d: byte %zu written %d times, want %d", name(pix),
              w, extra, align, (int)packed_mode, i, writes[i], want_writes[i]);
        CHECK(dst[i] == want[i], "unpack %s w=%d extra=%d align=%d packed=%d: byte %zu = %d, want %d", name(pix), w, extra, align,
              (int)packed_mode, i, dst[i], want[i]);
    }
    for (void* p : keep) free(p);
}

template <class L>
void check_pack(int pix, int w, int h, int extra, int align) {
    std::vector<void*> keep;
    const LayoutDesc d = L::desc;
    const size_t src_bytes = (size_t)w * (h / 2 * 3);
    uint8_t* src = tail_block(keep, src_bytes, 0);
    for (size_t i = 0; i < src_bytes; i++) src[i] = (uint8_t)rnd();
    for (int x = 0; x < w && x < 4; x++) src[x] = (uint8_t)(x & 1 ? 255 : 0);
    const int n = ref_row_bytes(pix, w), rows = ref_rows(pix, h), S = ref_words(pix) ? 2 : 1;
    const int cpr = ref_chroma_rows(pix, h) == h ? 2 : 1;
    const bool halves = pix == YUV422P || pix == YUV420P10 || pix == YUV422P10;
    const int list_rows = halves ? h + 2 * ref_chroma_rows(pix, h) : rows;  // a [U | V] row is two rows of the list
    const size_t pitch = (size_t)n + extra;
    const size_t out_bytes = (size_t)(rows - 1) * pitch + (size_t)n;
    uint8_t* out = tail_block(keep, out_bytes, align);
    memset(out, 0xA5, out_bytes);
    std::vector<int> writes(out_bytes, 0);
    const uint32_t items = (uint32_t)pack_items(d, w, h);
    for (uint32_t id = 0; id < items + 3; id++) {
        const LayoutSpan sp = pack_item(d, w, h, pitch, reinterpret_cast<uintptr_t>(out), id);
        if (id >= items) {
            CHECK(sp.len == 0, "an item past the last one writes");
            continue;
        }
        if (sp.len == 0) continue;
        CHECK(sp.len > 0 && sp.len <= 16 && sp.len % S == 0 && sp.b0 % S == 0 && sp.b0 + sp.len <= sp.n && sp.row < list_rows,
              "%s w=%d: span", name(pix), w);
        CHECK(sp.row >= h || sp.dst == (size_t)sp.row * pitch + sp.b0, "span dst");
        CHECK(sp.dst + sp.len <= out_bytes, "span outside the frame");
        if (sp.dst + sp.len > out_bytes) continue;
        if (sp.len == kChunk) CHECK(((reinterpret_cast<uintptr_t>(out) + sp.dst) & 15u) == 0, "a full chunk is not 16-byte aligned");
        for (int i = 0; i < sp.len; i += S)
            CHECK(pack_src(d, w, h, sp.row, (sp.b0 + i) / S) < src_bytes, "source byte outside the frame");
        pack_lane<L>(HostMem{}, src, out, w, h, sp);
        for (int i = 0; i < sp.len; i++) writes[sp.dst + i]++;
    }
    const Picture pic{pix, w, h, out, pitch};
    for (int y = 0; y < rows; y++)
        for (size_t b = (size_t)n; b < pitch && (size_t)y * pitch + b < out_bytes; b++)
            CHECK(writes[(size_t)y * pitch + b] == 0 && out[(size_t)y * pitch + b] == 0xA5,
                  "pack %s w=%d extra=%d align=%d: pad byte (%d, %zu) written", name(pix), w, extra, align, y, b);
    for (int y = 0; y < rows; y++)
        for (int b = 0; b < n; b++)
            CHECK(writes[(size_t)y * pitch + b] == 1, "pack %s w=%d extra=%d align=%d: byte (%d, %d) written %d times", name(pix), w,
                  extra, align, y, b, writes[(size_t)y * pitch + b]);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            CHECK(pic.luma(x, y) == ref_stored(pix, src[(size_t)y * w + x]), "pack %s w=%d extra=%d align=%d: luma (%d, %d)", name(pix),
                  w, extra, align, x, y);
            const int cy = cpr == 2 ? y : y / 2;  // two chroma rows per row pair: rows 2r and 2r + 1 both carry NV12 row r
            const uint16_t wantc = ref_stored(pix, src[(size_t)(h + y / 2) * w + x]);
            CHECK(pic.chroma(x, cy) == wantc, "pack %s w=%d extra=%d align=%d: chroma (%d, %d) = %d, want %d", name(pix), w, extra,
                  align, x, cy, pic.chroma(x, cy), wantc);
        }
    // out-then-in: the whole frame through the unpack items is the NV12 frame again
    uint8_t* back = tail_block(keep, src_bytes, 0);
    memset(back, 0x5A, src_bytes);
    for (int rp = 0; rp < h / 2; rp++) {
        const ConvRun r{(uint32_t)rp << 8, 0u, (uint32_t)((w + 7) / 8), 0u};
        for (int k = 0; k < (int)r.ng; k++) unpack_lane<L>(HostMem{}, out, back, w, unpack_item(d, w, h, pitch, r, k));
    }
    CHECK(memcmp(back, src, src_bytes) == 0, "%s w=%d extra=%d align=%d: out-then-in is not the identity", name(pix), w, extra, align);
    for (void* p : keep) free(p);
}

template <class L>
void check_layout(int pix) {
    check_descriptor<L>(pix);
    const int step = ref_words(pix) ? 2 : 1;  // a frame of words has an even base
    const int widths[] = {8, 16, 24, 40, 10, 18, 42, 12, 44, 14, 46, 64, 66, 328, 330, 332, 8 * 70, 8 * 66 + 2};
    for (int w : widths)
        for (int extra : {0, 6})
            for (int align = 0; align < 16; align += step)
                for (int packed = 0; packed < 2; packed++) check_unpack<L>(pix, w, 8, extra, align, packed != 0, align == 6 ? 2 : 0);
    for (int w : widths)
        for (int extra : {0, 6, 10})
            for (int align = 0; align < 16; align += step) check_pack<L>(pix, w, 6, extra, align);
}

}  // namespace

int main() {
    check_bytes();
    check_samples();
    check_planes();
    check_row_chunks();
    for (int pix : {0, 1, 2, 15, 20, 31, 36, -1}) CHECK(!converted_format(pix) && !layout_of(pix).converted(), "%d is no converted format", pix);
    check_layout<LayoutUyvy>(UYVY);
    check_layout<LayoutYuyv>(YUYV);
    check_layout<LayoutYuv422p>(YUV422P);
    check_layout<LayoutNv16>(NV16);
    check_layout<LayoutP010>(P010);
    check_layout<LayoutYuv420p10>(YUV420P10);
    check_layout<LayoutP210>(P210);
    check_layout<LayoutYuv422p10>(YUV422P10);
    if (g_fail) {
        fprintf(stderr, "frame_layout_check: %d failures\n", g_fail);
        return 1;
    }
    printf("frame_layout_check ok\n");
    return 0;
}
