// v210_layout.hpp — the work items and lane bodies of OCTVR_PIX_V210 (10-bit 4:2:2 as SDI capture cards and the
// `v210` codec store it), in and out: what v210_unpack_kernel and v210_pack_kernel (frame_layout.hip) run.  No HIP
// types, as frame_layout.hpp: the lane bodies are templates over a memory policy, so the kernels and
// tests/cpp/v210_check.cpp (memcpy against exactly sized heap blocks) execute one definition.
//
// The format.  A w x h frame (w, h even) is h rows of 16-byte blocks of four little-endian 32-bit words; a word
// carries three 10-bit components in bits 9..0, 19..10 and 29..20 (bits 31..30: ignored in, 0 out).  Block b of a
// row is its pixels [6 b, 6 b + 6), twelve components in the order
//     Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5        (component c: word c / 3, bits 10 (c % 3) + 9 .. 10 (c % 3))
// Cb_k, Cr_k being the chroma of pixels 6 b + 2 k, 6 b + 2 k + 1.  A row is v210_row_bytes(w) = 128 ceil(w / 48)
// bytes: the components of pixels >= w and the blocks past the last pixel are ignored in and written as 0 out.
// Base and pitch are multiples of 4 (LayoutDesc::aligned); nothing else is assumed of them.
// The rules are P210's (frame_layout.hpp): in v8 = min(255, (v10 + 2) >> 2), each chroma row narrowed, then the row
// pair's two averaged (a + b + 1) >> 1; out v10 = v8 << 2, chroma row r on rows 2 r and 2 r + 1.
//
// Narrowed, a block's twelve components are twelve bytes U0 Y0 V0 Y1 U1 Y2 V1 Y3 U2 Y4 V2 Y5: UYVY.  Both lane
// bodies go through that byte form, so luma and U,V pairs split and zip by UYVY's byte permutes.
#pragma once

#include "frame_layout.hpp"

namespace octvr {

OCTVR_LAYOUT_HD inline uint8_t v210_narrow(uint32_t v10) {
    const uint32_t v8 = (v10 + 2u) >> 2;
    return (uint8_t)(v8 > 255u ? 255u : v8);
}
// The three components of a word, narrowed, as bytes 0, 1, 2 (byte 3: 0).  Each field is rounded and clamped in a
// place of its own: v10 + 2 carries out of ten bits for 1022 and 1023.
OCTVR_LAYOUT_HD inline uint32_t v210_narrow3(uint32_t word) {
    const uint32_t a = (word & 0x3FF003FFu) + 0x00200002u;  // components 0 and 2, eleven bits each from bits 0 and 20
    const uint32_t b = ((word >> 10) & 0x3FFu) + 2u;
    uint32_t n0 = (a >> 2) & 0x1FFu, n1 = b >> 2, n2 = a >> 22;
    n0 = n0 > 255u ? 255u : n0;
    n1 = n1 > 255u ? 255u : n1;
    n2 = n2 > 255u ? 255u : n2;
    return n0 | n1 << 8 | n2 << 16;
}
constexpr uint32_t kSelV210A = 0x04020100u;  // bytes 0 1 2 of lo, 0 of hi: narrowed words 0, 1 of a block -> its bytes 0..3
constexpr uint32_t kSelV210B = 0x05040201u;  // bytes 1 2 of lo, 0 1 of hi: words 1, 2 -> bytes 4..7
constexpr uint32_t kSelV210C = 0x06050402u;  // byte 2 of lo, 0 1 2 of hi: words 2, 3 -> bytes 8..11
struct Words3 {
    uint32_t x, y, z;
};
// A block's twelve components narrowed: twelve bytes of UYVY
OCTVR_LAYOUT_HD inline Words3 v210_narrow_block(const Words4& b) {
    const uint32_t t0 = v210_narrow3(b.x), t1 = v210_narrow3(b.y), t2 = v210_narrow3(b.z), t3 = v210_narrow3(b.w);
    return Words3{perm(t1, t0, kSelV210A), perm(t2, t1, kSelV210B), perm(t3, t2, kSelV210C)};
}

// ---- in ------------------------------------------------------------------------------------------------------
// What the lane of group k (< r.ng) of table piece r does for a w x h camera.  Group g = r.g0 + k is pixels
// [8 g, 8 g + 8) of rows 2 rp, 2 rp + 1: they start at pixel ph = 8 g mod 6 (0, 2 or 4) of block floor(8 g / 6) and
// end in the next block.  sy0, sy1: that first block in the two source rows — of the caller's frame (src_pitch >=
// v210_row_bytes(w)), or of the packed upload (src_pitch == 0: the piece's covering blocks of row 2 rp at r.off, those
// of row 2 rp + 1 behind them; pack_run).  It writes px bytes at y0, y1 and c of the NV12 frame (pitch = w), as
// unpack_item's.  A full group (px == 8) taking the vector path loads the 32 bytes at sy0 and at sy1: its second
// block holds its pixels 6 - ph .. 7, so both lie inside the row's blocks that hold pixels, and inside the piece's
// covering blocks.  Any other item (the short last group of a width that is no multiple of 8, an NV12 frame whose rows
// are not 8-byte aligned) loads, word by word, only the words that hold one of its samples: nothing past the
// last block with a pixel.
struct V210Item {
    int px, ph;
    size_t sy0, sy1;
    size_t y0, y1, c;
};
OCTVR_LAYOUT_HD inline V210Item v210_unpack_item(int w, int h, size_t src_pitch, const FootRun& r, int k) {
    const int rp = (int)(r.cam >> 8), g = (int)r.g0 + k;
    V210Item it;
    const int left = w - 8 * g;
    it.px = (k < 0 || k >= (int)r.ng || 2 * rp + 1 >= h) ? 0 : left < 8 ? left : 8;
    const int b = v210_block0(g);
    it.ph = 8 * g - 6 * b;
    if (src_pitch) {
        it.sy0 = (size_t)(2 * rp) * src_pitch + (size_t)kV210Block * (size_t)b;
        it.sy1 = it.sy0 + src_pitch;
    } else {
        it.sy0 = (size_t)r.off + (size_t)kV210Block * (size_t)(b - v210_block0((int)r.g0));
        it.sy1 = it.sy0 + (size_t)kV210Block * (size_t)v210_blocks(w, (int)r.g0, (int)r.ng);
    }
    it.y0 = (size_t)(2 * rp) * (size_t)w + (size_t)8 * (size_t)g;
    it.y1 = it.y0 + (size_t)w;
    it.c = (size_t)(h + rp) * (size_t)w + (size_t)8 * (size_t)g;
    return it;
}

// Component c (0 .. 11, or 12 .. 23 in the next block) of the blocks at p.  Mem: load4 at a 4-byte aligned address.
template <class Mem>
OCTVR_LAYOUT_HD inline uint8_t v210_sample(const Mem& mem, const uint8_t* p, int c) {
    return v210_narrow((mem.load4(p + 4 * (c / 3)) >> (10 * (c % 3))) & 0x3FFu);
}
// The item sample by sample.
template <class Mem>
OCTVR_LAYOUT_HD inline void v210_unpack_samples(const Mem& mem, const uint8_t* src, uint8_t* dst, const V210Item& it) {
    for (int p = 0; p < it.px; p++) {
        // pixel ph + p from the first block's start: its luma is component 2 (ph + p) + 1, its chroma byte (U for an
        // even p, V for an odd) component 4 ((ph + p) / 2) + 2 (p & 1)
        const int cy = 2 * (it.ph + p) + 1, cc = 4 * ((it.ph + p) >> 1) + 2 * (p & 1);
        dst[it.y0 + p] = v210_sample(mem, src + it.sy0, cy);
        dst[it.y1 + p] = v210_sample(mem, src + it.sy1, cy);
        dst[it.c + p] = avg1(v210_sample(mem, src + it.sy0, cc), v210_sample(mem, src + it.sy1, cc));
    }
}
// The group's 16 narrowed bytes (U Y V Y of its four pixel pairs) of the two blocks at p: the 24 bytes of the two
// blocks from byte 2 ph, which is a whole dword (0, 4 or 8), so the lanes of a wave differ by selects only
template <class Mem>
OCTVR_LAYOUT_HD inline Words4 v210_group_bytes(const Mem& mem, const uint8_t* p, int ph) {
    const Words3 a = v210_narrow_block(mem.load16(p)), b = v210_narrow_block(mem.load16(p + kV210Block));
    if (ph == 0) return Words4{a.x, a.y, a.z, b.x};
    if (ph == 2) return Words4{a.y, a.z, b.x, b.y};
    return Words4{a.z, b.x, b.y, b.z};
}
// One lane of the unpack kernel.  Mem: load4 at a 4-byte aligned address, load16 at any, store8 to an 8-byte
// aligned address of the destination.
template <class Mem>
OCTVR_LAYOUT_HD inline void v210_unpack_lane(const Mem& mem, const uint8_t* src, uint8_t* dst, int w, const V210Item& it) {
    if (it.px <= 0) return;
    if (!(it.px == 8 && (w & 7) == 0 && (reinterpret_cast<uintptr_t>(dst) & 7u) == 0)) {  // unpack_vector's rule
        v210_unpack_samples(mem, src, dst, it);
        return;
    }
    const Words4 a = v210_group_bytes(mem, src + it.sy0, it.ph), b = v210_group_bytes(mem, src + it.sy1, it.ph);
    mem.store8(dst + it.y0, Words2{perm(a.y, a.x, kSelOdd), perm(a.w, a.z, kSelOdd)});
    mem.store8(dst + it.y1, Words2{perm(b.y, b.x, kSelOdd), perm(b.w, b.z, kSelOdd)});
    mem.store8(dst + it.c, Words2{avg4(perm(a.y, a.x, kSelEven), perm(b.y, b.x, kSelEven)),
                                  avg4(perm(a.w, a.z, kSelEven), perm(b.w, b.z, kSelEven))});
}

// ---- out -----------------------------------------------------------------------------------------------------
// A work item of the pack kernel is one block of one destination row: v210_row_bytes(w) / 16 items a row, h rows.
// Item id is block b = id mod that of row y = id / that: it reads the npx = min(6, w - 6 b) (0 for a padding block)
// luma bytes at sy and the npx chroma bytes (U,V pairs) at sc of the NV12 frame (pitch = w; the same byte 6 b of the
// luma row y and of the chroma row y >> 1), and writes the 16 bytes at dst of the caller's frame.  row < 0: nothing.
struct V210Span {
    int row, npx;
    bool wide;  // 8 bytes may be loaded at sy and at sc: they lie inside the rows
    size_t sy, sc, dst;
};
OCTVR_LAYOUT_HD inline uint64_t v210_pack_items(int w, int h) { return (uint64_t)(v210_row_bytes(w) / kV210Block) * (uint64_t)h; }
OCTVR_LAYOUT_HD inline V210Span v210_pack_item(int w, int h, size_t pitch, uint32_t id) {
    const uint32_t per = (uint32_t)(v210_row_bytes(w) / kV210Block);
    V210Span sp{-1, 0, false, 0, 0, 0};
    const uint32_t y = id / per, b = id - y * per;
    if (y >= (uint32_t)h) return sp;
    sp.row = (int)y;
    const int left = w - 6 * (int)b;
    sp.npx = left < 0 ? 0 : left < 6 ? left : 6;
    sp.wide = left >= 8;
    sp.sy = (size_t)y * (size_t)w + (size_t)6 * (size_t)b;
    sp.sc = (size_t)(h + (int)(y >> 1)) * (size_t)w + (size_t)6 * (size_t)b;
    sp.dst = (size_t)y * pitch + (size_t)kV210Block * (size_t)b;
    return sp;
}
// The first n (<= 6, even) bytes at p, the others 0
OCTVR_LAYOUT_HD inline Words2 v210_bytes(const uint8_t* p, int n) {
    Words2 v{0, 0};
    if (n > 0) v.x = (uint32_t)p[0] | (uint32_t)p[1] << 8;
    if (n > 2) v.x |= (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    if (n > 4) v.y = (uint32_t)p[4] | (uint32_t)p[5] << 8;
    return v;
}
OCTVR_LAYOUT_HD inline uint32_t v210_word(uint32_t c0, uint32_t c1, uint32_t c2) {
    return (c0 & 0xFFu) << 2 | (c1 & 0xFFu) << 12 | (c2 & 0xFFu) << 22;
}
// One work item of the pack kernel.  Mem: load8 of the NV12 frame at any alignment, store16 to a 16-byte aligned
// address of the caller's frame, store4 to a 4-byte aligned one (a base or a pitch that is no multiple of 16: every
// vector store stays naturally aligned).
template <class Mem>
OCTVR_LAYOUT_HD inline void v210_pack_lane(const Mem& mem, const uint8_t* src, uint8_t* out, const V210Span& sp) {
    if (sp.row < 0) return;
    const Words2 l = sp.wide ? mem.load8(src + sp.sy) : v210_bytes(src + sp.sy, sp.npx);
    const Words2 c = sp.wide ? mem.load8(src + sp.sc) : v210_bytes(src + sp.sc, sp.npx);
    // U0 Y0 V0 Y1, U1 Y2 V1 Y3, U2 Y4 V2 Y5 (bytes 6, 7 of a wide load are the next block's)
    const uint32_t z0 = perm(l.x, c.x, kSelZipLo), z1 = perm(l.x, c.x, kSelZipHi), z2 = perm(l.y, c.y, kSelZipLo);
    const Words4 o{v210_word(z0, z0 >> 8, z0 >> 16), v210_word(z0 >> 24, z1, z1 >> 8), v210_word(z1 >> 16, z1 >> 24, z2),
                   v210_word(z2 >> 8, z2 >> 16, z2 >> 24)};
    uint8_t* const d = out + sp.dst;
    if ((reinterpret_cast<uintptr_t>(d) & 15u) == 0) {
        mem.store16(d, o);
    } else {
        mem.store4(d, o.x);
        mem.store4(d + 4, o.y);
        mem.store4(d + 8, o.z);
        mem.store4(d + 12, o.w);
    }
}

}  // namespace octvr
