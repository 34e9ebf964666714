// yuv10_host.hpp — the arithmetic of the 10-bit capture layouts (OCTVR_PIX_P010, OCTVR_PIX_YUV420P10,
// OCTVR_PIX_P210, OCTVR_PIX_YUV422P10): which bytes a work item of yuv10_unpack_kernel / yuv10_pack_kernel
// (yuv10.hip) loads and which it stores, and the packing of a footprint run of such planes (async.cpp copy_in).
// No HIP types: the lane bodies are templates over a memory policy, as yuv422_host.hpp's, so the kernels
// (non-temporal / vector accesses) and tests/cpp/yuv10_check.cpp (memcpy against exactly sized heap blocks)
// execute one definition.  The run table, the byte permute and the four-byte average are uyvy_host.hpp's.
//
// Every sample is a 16-bit little-endian word; a w x h picture (w, h even) is
//   P010       h rows of w luma words, then h / 2 chroma rows of w / 2 U,V word pairs;   sample in bits 15..6
//   YUV420P10  h rows of w luma words, then h / 2 chroma rows: U in words [0, w / 2), V in [w / 2, w);  bits 9..0
//   P210       h rows of luma, then h chroma rows of U,V word pairs;                     sample in bits 15..6
//   YUV422P10  h rows of luma, then h chroma rows of [U | V] halves;                     bits 9..0
// so a row is 2 w bytes in all four.  The bits of a word outside the sample are ignored on the way in and
// written as 0 on the way out.  The 8-bit side of both conversions is NV12 at pitch = width, as for UYVY:
//   in   v8 = min(255, (v10 + 2) >> 2) per sample; for the 4:2:2 layouts then chroma row r =
//        (c8[2r] + c8[2r + 1] + 1) >> 1 of the narrowed rows
//   out  v10 = v8 << 2; the 4:2:2 layouts carry chroma row r on their chroma rows 2r and 2r + 1
#pragma once

#include "uyvy_host.hpp"

namespace octvr {

enum Yuv10Layout : int { kYuv10P010 = 0, kYuv10Planar420 = 1, kYuv10P210 = 2, kYuv10Planar422 = 3 };  // OCTVR_PIX_* - 32
constexpr int kYuv10First = 32, kYuv10Last = 35;  // OCTVR_PIX_P010 .. OCTVR_PIX_YUV422P10
inline bool yuv10_format(int pix) { return pix >= kYuv10First && pix <= kYuv10Last; }

OCTVR_UYVY_HD inline bool yuv10_is422(int layout) { return layout >= kYuv10P210; }
OCTVR_UYVY_HD inline bool yuv10_planar(int layout) { return (layout & 1) != 0; }
// rows and bytes per row of a w x h frame; packed bytes per pixel of a table piece's row (two luma rows and
// one or two chroma rows of two bytes a sample)
OCTVR_UYVY_HD inline int yuv10_frame_rows(int layout, int h) { return yuv10_is422(layout) ? 2 * h : h / 2 * 3; }
OCTVR_UYVY_HD inline int yuv10_frame_row_bytes(int w) { return 2 * w; }
OCTVR_UYVY_HD inline int yuv10_run_bpp(int layout) { return yuv10_is422(layout) ? 8 : 6; }

// ---- samples ------------------------------------------------------------------------------------------------
// One sample by the in rule: msb, the word carries it in bits 15..6 (else in bits 9..0).
OCTVR_UYVY_HD inline uint8_t yuv10_narrow(uint16_t word, bool msb) {
    const uint32_t v10 = msb ? (uint32_t)word >> 6 : (uint32_t)word & 0x3FFu;
    const uint32_t v8 = (v10 + 2u) >> 2;
    return (uint8_t)(v8 > 255u ? 255u : v8);
}
OCTVR_UYVY_HD inline uint16_t yuv10_widen(uint8_t v8, bool msb) { return (uint16_t)((uint32_t)v8 << (msb ? 8 : 2)); }

// Two samples in bits 15..6 of a dword's halves: min(0xFFFF, half + 128) of each half, so that byte 1 and byte 3
// are the two narrowed samples — min(255, (word + 128) >> 8) = min(255, (v10 + 2) >> 2), as the 6 low bits of a
// word lie below bit 7 and never carry into it.  One v_pk_add_u16 with clamp on the device.
OCTVR_UYVY_HD inline uint32_t yuv10_round2(uint32_t d) {
#ifdef __HIP_DEVICE_COMPILE__
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 r = __builtin_elementwise_add_sat(__builtin_bit_cast(u16x2, d), (u16x2){128, 128});
    return __builtin_bit_cast(uint32_t, r);
#else
    const uint32_t lo = (d & 0xFFFFu) + 128u, hi = (d >> 16) + 128u;
    return (lo > 0xFFFFu ? 0xFFFFu : lo) | (hi > 0xFFFFu ? 0xFFFFu : hi) << 16;
#endif
}
// ... of two samples in bits 9..0: moved up to bits 15..6 first.  The shift drops each half's 6 high bits except
// that the low half's land in bits 21..16, the ignored low bits of the high half.
template <bool MSB>
OCTVR_UYVY_HD inline uint32_t yuv10_narrow2(uint32_t d) {
    return yuv10_round2(MSB ? d : d << 6);
}
constexpr uint32_t kYuv10SelOdd = 0x07050301u;     // bytes 1, 3 of lo, then of hi: four narrowed samples
constexpr uint32_t kYuv10SelOddZip = 0x07030501u;  // byte 1 of lo, of hi, byte 3 of lo, of hi: u0 v0 u1 v1

// v_perm_b32 with the selector byte 0x0c (a zero byte) as well as 0-7; uyvy_perm otherwise.
OCTVR_UYVY_HD inline uint32_t yuv10_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = (uint64_t)hi << 32 | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) {
        const uint32_t s = (sel >> (8 * k)) & 0xFFu;
        if (s < 8u) r |= (uint32_t)((both >> (8 * s)) & 0xFFu) << (8 * k);
    }
    return r;
#endif
}
// Two bytes of a dword as two words: selectors for bytes (0, 1), (2, 3), (0, 2), (1, 3) into the words' low
// bytes (the planar layouts, then << 2) or high bytes (P010 / P210: v8 << 8).
constexpr uint32_t kYuv10Wide01Lo = 0x0c010c00u, kYuv10Wide23Lo = 0x0c030c02u, kYuv10Wide02Lo = 0x0c020c00u,
                   kYuv10Wide13Lo = 0x0c030c01u;
constexpr uint32_t kYuv10Wide01Hi = 0x010c000cu, kYuv10Wide23Hi = 0x030c020cu;
template <bool MSB>
OCTVR_UYVY_HD inline UyvyWords yuv10_widen8(uint32_t a, uint32_t b) {  // 8 bytes -> 8 words
    if (MSB)
        return UyvyWords{yuv10_perm(0, a, kYuv10Wide01Hi), yuv10_perm(0, a, kYuv10Wide23Hi), yuv10_perm(0, b, kYuv10Wide01Hi),
                         yuv10_perm(0, b, kYuv10Wide23Hi)};
    return UyvyWords{yuv10_perm(0, a, kYuv10Wide01Lo) << 2, yuv10_perm(0, a, kYuv10Wide23Lo) << 2,
                     yuv10_perm(0, b, kYuv10Wide01Lo) << 2, yuv10_perm(0, b, kYuv10Wide23Lo) << 2};
}

// ---- in: the unpack kernel's work items -----------------------------------------------------------------------
// What the lane of group k (< r.ng) of table piece r (uyvy_host.hpp UyvyRun) does for a w x h camera.  It writes
// px bytes at y0, at y1 and at c of the camera's NV12 frame (pitch = w), exactly as a UYVY item, and reads
//   2 px bytes of luma at sy0 and at sy1 (rows 2 rp, 2 rp + 1);
//   P010       2 px bytes of U,V pairs at su0 (chroma row rp);
//   YUV420P10  px bytes of U at su0 and px of V at sv0;
//   P210       2 px bytes of U,V pairs at su0 and at su1 (chroma rows 2 rp, 2 rp + 1);
//   YUV422P10  px bytes of U at su0, su1 and px of V at sv0, sv1.
// The source is the caller's frame (src_pitch > 0) or the pipeline's packed upload buffer (src_pitch == 0): at
// r.off the piece's two luma rows, then its chroma row(s) in the layout's order (the U part before the V part
// for the planar layouts): yuv10_run_bpp bytes per pixel of the piece's row (yuv10_pack_run, yuv10_run_table).
struct Yuv10Item {
    int px;
    size_t sy0, sy1, su0, su1, sv0, sv1;
    size_t y0, y1, c;
};
OCTVR_UYVY_HD inline Yuv10Item yuv10_unpack_item(int layout, int w, int h, size_t src_pitch, const UyvyRun& r, int k) {
    const int rp = (int)(r.cam >> 8), g = (int)r.g0 + k;
    const bool planar = yuv10_planar(layout), c422 = yuv10_is422(layout);
    Yuv10Item it;
    const int left = w - 8 * g;
    it.px = (k < 0 || k >= (int)r.ng || 2 * rp + 1 >= h) ? 0 : left < 8 ? left : 8;
    it.su1 = it.sv0 = it.sv1 = 0;
    const size_t cg = planar ? 8 : 16;  // bytes of a group in a chroma (half) row
    if (src_pitch) {
        it.sy0 = (size_t)(2 * rp) * src_pitch + (size_t)16 * (size_t)g;
        it.sy1 = it.sy0 + src_pitch;
        it.su0 = (size_t)(h + (c422 ? 2 * rp : rp)) * src_pitch + cg * (size_t)g;
        if (planar) it.sv0 = it.su0 + (size_t)w;
        if (c422) {
            it.su1 = it.su0 + src_pitch;
            if (planar) it.sv1 = it.sv0 + src_pitch;
        }
    } else {
        const size_t n = (size_t)uyvy_run_px(w, (int)r.g0, (int)r.ng);
        it.sy0 = (size_t)r.off + (size_t)16 * (size_t)k;
        it.sy1 = it.sy0 + 2 * n;
        it.su0 = (size_t)r.off + 4 * n + cg * (size_t)k;
        if (planar) it.sv0 = it.su0 + n;
        if (c422) {
            it.su1 = it.su0 + 2 * n;
            if (planar) it.sv1 = it.su1 + n;
        }
    }
    it.y0 = (size_t)(2 * rp) * (size_t)w + (size_t)8 * (size_t)g;
    it.y1 = it.y0 + (size_t)w;
    it.c = (size_t)(h + rp) * (size_t)w + (size_t)8 * (size_t)g;
    return it;
}

OCTVR_UYVY_HD inline uint16_t yuv10_word(const uint8_t* p) { return (uint16_t)(p[0] | p[1] << 8); }

// The item's per-sample path (the short last group; an NV12 frame whose rows are not 8-byte aligned).
template <int L>
OCTVR_UYVY_HD inline void yuv10_unpack_samples(const uint8_t* src, uint8_t* dst, const Yuv10Item& it) {
    constexpr bool msb = !(L & 1), planar = (L & 1) != 0, c422 = L >= kYuv10P210;
    for (int p = 0; p < it.px; p++) {
        dst[it.y0 + p] = yuv10_narrow(yuv10_word(src + it.sy0 + 2 * p), msb);
        dst[it.y1 + p] = yuv10_narrow(yuv10_word(src + it.sy1 + 2 * p), msb);
        // chroma byte p of the group: U (p even) or V (p odd) of pixel pair p / 2
        const size_t o = planar ? (size_t)(p >> 1) * 2 : (size_t)2 * p;
        const uint8_t a = yuv10_narrow(yuv10_word(src + (planar && (p & 1) ? it.sv0 : it.su0) + o), msb);
        if (c422) {
            const uint8_t b = yuv10_narrow(yuv10_word(src + (planar && (p & 1) ? it.sv1 : it.su1) + o), msb);
            dst[it.c + p] = (uint8_t)(((int)a + (int)b + 1) >> 1);
        } else {
            dst[it.c + p] = a;
        }
    }
}

// True when the item takes the vector path: a full group whose three stores are 8-byte aligned (the NV12
// frame's rows are when w is a multiple of 8 and its base is 8-byte aligned; the loads need no alignment).
OCTVR_UYVY_HD inline bool yuv10_unpack_vector(int w, uintptr_t dst_base, const Yuv10Item& it) {
    return it.px == 8 && (w & 7) == 0 && (dst_base & 7u) == 0;
}

struct Yuv10Pair {
    uint32_t x, y;
};
// 8 words -> 8 bytes; 4 words of U and 4 of V -> 8 bytes of U,V pairs
template <bool MSB>
OCTVR_UYVY_HD inline Yuv10Pair yuv10_narrow8(const UyvyWords& a) {
    return Yuv10Pair{uyvy_perm(yuv10_narrow2<MSB>(a.y), yuv10_narrow2<MSB>(a.x), kYuv10SelOdd),
                     uyvy_perm(yuv10_narrow2<MSB>(a.w), yuv10_narrow2<MSB>(a.z), kYuv10SelOdd)};
}
template <bool MSB>
OCTVR_UYVY_HD inline Yuv10Pair yuv10_narrow_zip(const Yuv10Pair& u, const Yuv10Pair& v) {
    return Yuv10Pair{uyvy_perm(yuv10_narrow2<MSB>(v.x), yuv10_narrow2<MSB>(u.x), kYuv10SelOddZip),
                     uyvy_perm(yuv10_narrow2<MSB>(v.y), yuv10_narrow2<MSB>(u.y), kYuv10SelOddZip)};
}

// One lane of the unpack kernel.  Mem: load8 / load16 of the source at any alignment, store8 to an 8-byte
// aligned address of the destination.
template <int L, class Mem>
OCTVR_UYVY_HD inline void yuv10_unpack_lane(const Mem& mem, const uint8_t* src, uint8_t* dst, int w, const Yuv10Item& it) {
    constexpr bool msb = !(L & 1), planar = (L & 1) != 0, c422 = L >= kYuv10P210;
    if (it.px <= 0) return;
    if (!yuv10_unpack_vector(w, reinterpret_cast<uintptr_t>(dst), it)) {
        yuv10_unpack_samples<L>(src, dst, it);
        return;
    }
    const Yuv10Pair y0 = yuv10_narrow8<msb>(mem.load16(src + it.sy0)), y1 = yuv10_narrow8<msb>(mem.load16(src + it.sy1));
    Yuv10Pair c;
    if (planar) {
        c = yuv10_narrow_zip<msb>(mem.load8(src + it.su0), mem.load8(src + it.sv0));
        if (c422) {
            const Yuv10Pair b = yuv10_narrow_zip<msb>(mem.load8(src + it.su1), mem.load8(src + it.sv1));
            c = Yuv10Pair{uyvy_avg4(c.x, b.x), uyvy_avg4(c.y, b.y)};
        }
    } else {
        c = yuv10_narrow8<msb>(mem.load16(src + it.su0));
        if (c422) {
            const Yuv10Pair b = yuv10_narrow8<msb>(mem.load16(src + it.su1));
            c = Yuv10Pair{uyvy_avg4(c.x, b.x), uyvy_avg4(c.y, b.y)};
        }
    }
    mem.store8(dst + it.y0, y0);
    mem.store8(dst + it.y1, y1);
    mem.store8(dst + it.c, c);
}

// The unpack kernel's table for a 10-bit layout: uyvy_run_table's pieces (the same cut into at most kUyvyWave
// groups) with each piece's `off` its place in a packed upload buffer of yuv10_pack_run's pieces.
template <class Run>
inline std::vector<UyvyRun> yuv10_run_table(int layout, const std::vector<Run>& runs, const std::vector<int>& in_w, size_t& bytes) {
    size_t bytes4 = 0;
    std::vector<UyvyRun> t = uyvy_run_table(runs, in_w, bytes4);
    bytes = 0;
    for (UyvyRun& r : t) {
        r.off = (uint32_t)bytes;
        bytes += (size_t)yuv10_run_bpp(layout) * (size_t)uyvy_run_px(in_w[r.cam & 31u], (int)r.g0, (int)r.ng);
    }
    return t;
}

// Packs piece (row pair rp, groups [g0, g0 + ng)) of a w-wide camera at d from host planes laid out as
// octvr_async_push's: P010 / P210 planes[0] = Y, planes[1] = U,V word pairs (2 w bytes a row; h / 2 or h rows);
// the planar layouts planes[0 / 1 / 2] = Y, U, V (U and V w bytes a row; h / 2 or h rows).  The layout the
// packed-source items above read; returns its size, yuv10_run_bpp bytes per pixel of the piece's row.
inline size_t yuv10_pack_run(int layout, uint8_t* d, int w, int rp, int g0, int ng, const uint8_t* const* planes,
                             const size_t* pitches) {
    const size_t n = (size_t)uyvy_run_px(w, g0, ng);
    for (int row = 0; row < 2; row++, d += 2 * n)
        memcpy(d, planes[0] + (size_t)(2 * rp + row) * pitches[0] + (size_t)16 * (size_t)g0, 2 * n);
    const int c_rows = yuv10_is422(layout) ? 2 : 1;
    for (int row = 0; row < c_rows; row++, d += 2 * n) {
        const size_t cr = (size_t)(c_rows * rp + row);
        if (yuv10_planar(layout)) {
            memcpy(d, planes[1] + cr * pitches[1] + (size_t)8 * (size_t)g0, n);
            memcpy(d + n, planes[2] + cr * pitches[2] + (size_t)8 * (size_t)g0, n);
        } else {
            memcpy(d, planes[1] + cr * pitches[1] + (size_t)16 * (size_t)g0, 2 * n);
        }
    }
    return (size_t)yuv10_run_bpp(layout) * n;
}

// ---- out: the pack kernel's work items -----------------------------------------------------------------------
// The destination is a list of rows, each with yuv422_pack_item's head / chunk / tail arithmetic (the bytes
// before the row's first 16-byte boundary, then 16-byte chunks, the last one possibly short; all even, as the
// base, the pitch and a half row's start are):
//   P010 / P210   3 h / 2 or 2 h rows of 2 w bytes: luma rows, then chroma rows;
//   the planar layouts   h luma rows of 2 w bytes, then h or 2 h half rows of w bytes: half row q is the U (q even)
//                 or V (q odd) half of chroma row q >> 1, at byte (q & 1) w of frame row h + (q >> 1).
OCTVR_UYVY_HD inline int yuv10_chroma_rows(int layout, int h) { return yuv10_is422(layout) ? h : h / 2; }
OCTVR_UYVY_HD inline int yuv10_pack_rows(int layout, int h) {
    return h + (yuv10_planar(layout) ? 2 : 1) * yuv10_chroma_rows(layout, h);
}
OCTVR_UYVY_HD inline uint32_t yuv10_row_items(int n) { return (uint32_t)((n + kUyvyChunk - 1) / kUyvyChunk + 1); }
OCTVR_UYVY_HD inline uint64_t yuv10_pack_items(int layout, int w, int h) {
    if (!yuv10_planar(layout)) return (uint64_t)yuv10_pack_rows(layout, h) * yuv10_row_items(2 * w);
    return (uint64_t)h * yuv10_row_items(2 * w) + (uint64_t)(2 * yuv10_chroma_rows(layout, h)) * yuv10_row_items(w);
}

// What item `id` writes: len bytes (0: nothing) from byte b0 of list row `row` (n bytes long), at dst of the
// caller's frame (first byte at address out_base).  len = 16 only with dst 16-byte aligned.
struct Yuv10Span {
    int row, n, b0, len;
    size_t dst;
};
OCTVR_UYVY_HD inline Yuv10Span yuv10_pack_item(int layout, int w, int h, size_t pitch, uintptr_t out_base, uint32_t id) {
    Yuv10Span sp{0, 0, 0, 0, 0};
    int chunk;
    const uint32_t per_y = yuv10_row_items(2 * w);
    if (yuv10_planar(layout)) {
        const uint32_t per_c = yuv10_row_items(w);
        const uint32_t ny = (uint32_t)h * per_y;
        if (id < ny) {
            sp.row = (int)(id / per_y);
            chunk = (int)(id - (uint32_t)sp.row * per_y);
            sp.n = 2 * w;
            sp.dst = (size_t)sp.row * pitch;
        } else {
            const uint32_t q = (id - ny) / per_c;
            if (q >= (uint32_t)(2 * yuv10_chroma_rows(layout, h))) return sp;
            chunk = (int)(id - ny - q * per_c);
            sp.row = h + (int)q;
            sp.n = w;
            sp.dst = (size_t)(h + (int)(q >> 1)) * pitch + (size_t)((q & 1u) ? w : 0);
        }
    } else {
        sp.n = 2 * w;
        sp.row = (int)(id / per_y);
        if (sp.row >= yuv10_pack_rows(layout, h)) return sp;
        chunk = (int)(id - (uint32_t)sp.row * per_y);
        sp.dst = (size_t)sp.row * pitch;
    }
    const int head = (int)((0 - (out_base + sp.dst)) & (uintptr_t)(kUyvyChunk - 1));
    const int hd = head < sp.n ? head : sp.n;
    if (chunk == 0) {
        sp.len = hd;
        return sp;
    }
    const int b0 = hd + kUyvyChunk * (chunk - 1);
    if (b0 >= sp.n) return sp;
    sp.b0 = b0;
    sp.len = sp.n - b0 < kUyvyChunk ? sp.n - b0 : kUyvyChunk;
    sp.dst += (size_t)b0;
    return sp;
}

// Where word i of list row `row` comes from in the NV12 frame (pitch = w).
OCTVR_UYVY_HD inline size_t yuv10_pack_src(int layout, int w, int h, int row, int i) {
    if (row < h) return (size_t)row * (size_t)w + (size_t)i;
    const int q = row - h;
    const int sh = yuv10_is422(layout) ? 1 : 0;  // a 4:2:2 chroma row is written twice
    if (!yuv10_planar(layout)) return (size_t)(h + (q >> sh)) * (size_t)w + (size_t)i;
    return (size_t)(h + (q >> (1 + sh))) * (size_t)w + (size_t)(2 * i + (q & 1));
}

// One work item of the pack kernel.  Mem: load8 / load16 of the NV12 frame at any alignment, store16 to a
// 16-byte aligned address of the caller's frame.  A full chunk is 8 words from
//   a luma row, a P010 / P210 chroma row: 8 bytes of the NV12 row;
//   a planar half row: the even (U) or odd (V) bytes of 16 bytes of the NV12 chroma row.
template <int L, class Mem>
OCTVR_UYVY_HD inline void yuv10_pack_lane(const Mem& mem, const uint8_t* src, uint8_t* out, int w, int h, const Yuv10Span& sp) {
    constexpr bool msb = !(L & 1), planar = (L & 1) != 0;
    if (sp.len <= 0) return;
    if (sp.len != kUyvyChunk) {  // heads and tails, word by word
        for (int i = 0; i < sp.len; i += 2) {
            const uint16_t v = yuv10_widen(src[yuv10_pack_src(L, w, h, sp.row, (sp.b0 + i) >> 1)], msb);
            out[sp.dst + i] = (uint8_t)(v & 0xFFu);
            out[sp.dst + i + 1] = (uint8_t)(v >> 8);
        }
        return;
    }
    UyvyWords o;
    if (!planar || sp.row < h) {
        const Yuv10Pair s = mem.load8(src + yuv10_pack_src(L, w, h, sp.row, sp.b0 >> 1));
        o = yuv10_widen8<msb>(s.x, s.y);
    } else {
        const int half = (sp.row - h) & 1;
        const UyvyWords a = mem.load16(src + yuv10_pack_src(L, w, h, sp.row, sp.b0 >> 1) - half);  // row bytes [b0, b0 + 16)
        const uint32_t sel = half ? kYuv10Wide13Lo : kYuv10Wide02Lo;
        o = UyvyWords{yuv10_perm(0, a.x, sel) << 2, yuv10_perm(0, a.y, sel) << 2, yuv10_perm(0, a.z, sel) << 2,
                      yuv10_perm(0, a.w, sel) << 2};
    }
    mem.store16(out + sp.dst, o);
}

}  // namespace octvr
