// yuv422_host.hpp — the arithmetic of the 8-bit 4:2:2 capture layouts beside UYVY (OCTVR_PIX_YUYV422,
// OCTVR_PIX_YUV422P, OCTVR_PIX_NV16): which bytes a work item of yuv422_unpack_kernel / yuv422_pack_kernel
// (yuv422.hip) loads and which it stores, and the packing of a footprint run of such planes (async.cpp copy_in).
// No HIP types: the lane bodies are templates over a memory policy, so the kernels (non-temporal / vector
// accesses) and tests/cpp/yuv422_check.cpp (memcpy against exactly sized heap blocks) execute one definition.
// The run table, the byte permute and the four-byte average are uyvy_host.hpp's.
//
// A w x h picture (w, h even) is
//   YUYV     h rows of 2 w bytes, Y0 U0 Y1 V0 per pixel pair: byte b of a row is luma Y[b >> 1] when b is even
//            and, when b is odd, byte b >> 1 of the row's chroma as U,V pairs;
//   YUV422P  h rows of Y, then h chroma rows: U in bytes [0, w / 2), V in bytes [w / 2, w);
//   NV16     h rows of Y, then h chroma rows of w / 2 U,V pairs.
// The 4:2:0 side of both conversions is NV12 at pitch = width, as for UYVY, and the rules are the same two:
//   in  (4:2:2 -> 4:2:0): chroma row r = (c[2r] + c[2r + 1] + 1) >> 1 per byte; luma copied
//   out (4:2:0 -> 4:2:2): chroma rows 2r and 2r + 1 both carry chroma row r; luma copied
#pragma once

#include "uyvy_host.hpp"

namespace octvr {

enum Yuv422Layout : int { kYuv422Yuyv = 0, kYuv422Planar = 1, kYuv422Nv16 = 2 };  // OCTVR_PIX_* - 17
constexpr int kYuv422First = 17, kYuv422Last = 19;                                // OCTVR_PIX_YUYV422 .. OCTVR_PIX_NV16
inline bool yuv422_format(int pix) { return pix >= kYuv422First && pix <= kYuv422Last; }

// rows and bytes per row of a w x h frame
OCTVR_UYVY_HD inline int yuv422_frame_rows(int layout, int h) { return layout == kYuv422Yuyv ? h : 2 * h; }
OCTVR_UYVY_HD inline int yuv422_frame_row_bytes(int layout, int w) { return layout == kYuv422Yuyv ? 2 * w : w; }

constexpr uint32_t kYuv422SelEven = 0x06040200u;  // bytes 0, 2, 4, 6 of {hi, lo}: YUYV's luma, a U,V row's U
constexpr uint32_t kYuv422SelOdd = 0x07050301u;   // bytes 1, 3, 5, 7:             YUYV's chroma, a U,V row's V

// ---- in: the unpack kernel's work items -----------------------------------------------------------------------
// What the lane of group k (< r.ng) of table piece r (uyvy_host.hpp UyvyRun, uyvy_run_table) does for a w x h
// camera.  It writes px bytes at y0, at y1 and at c of the camera's NV12 frame (pitch = w), exactly as a UYVY
// item, and reads
//   YUYV     2 px bytes at sy0 and at sy1 (the packed rows 2 rp, 2 rp + 1);
//   NV16     px luma bytes at sy0, sy1 and px bytes of U,V pairs at su0, su1 (chroma rows 2 rp, 2 rp + 1);
//   YUV422P  px luma bytes at sy0, sy1, px / 2 bytes of U at su0, su1 and px / 2 of V at sv0, sv1.
// The source is the caller's frame (src_pitch > 0) or the pipeline's packed upload buffer (src_pitch == 0): at
// r.off the piece's two luma rows, then its chroma rows 2 rp and 2 rp + 1 in the layout's order (the U part
// before the V part for YUV422P); for YUYV its two packed rows.  Either way 4 bytes per pixel of the piece's row
// (yuv422_pack_run), so the table's offsets are UYVY's.
struct Yuv422Item {
    int px;
    size_t sy0, sy1, su0, su1, sv0, sv1;
    size_t y0, y1, c;
};
OCTVR_UYVY_HD inline Yuv422Item yuv422_unpack_item(int layout, int w, int h, size_t src_pitch, const UyvyRun& r, int k) {
    const int rp = (int)(r.cam >> 8), g = (int)r.g0 + k;
    Yuv422Item it;
    const int left = w - 8 * g;
    it.px = (k < 0 || k >= (int)r.ng || 2 * rp + 1 >= h) ? 0 : left < 8 ? left : 8;
    it.su0 = it.su1 = it.sv0 = it.sv1 = 0;
    if (src_pitch) {
        const size_t lb = layout == kYuv422Yuyv ? 16 : 8;  // bytes of a group in a luma (packed) row
        it.sy0 = (size_t)(2 * rp) * src_pitch + lb * (size_t)g;
        it.sy1 = it.sy0 + src_pitch;
        const size_t c0 = (size_t)(h + 2 * rp) * src_pitch;
        if (layout == kYuv422Nv16) {
            it.su0 = c0 + (size_t)8 * (size_t)g;
            it.su1 = it.su0 + src_pitch;
        } else if (layout == kYuv422Planar) {
            it.su0 = c0 + (size_t)4 * (size_t)g;
            it.su1 = it.su0 + src_pitch;
            it.sv0 = it.su0 + (size_t)(w / 2);
            it.sv1 = it.sv0 + src_pitch;
        }
    } else {
        const size_t n = (size_t)uyvy_run_px(w, (int)r.g0, (int)r.ng);
        if (layout == kYuv422Yuyv) {
            it.sy0 = (size_t)r.off + (size_t)16 * (size_t)k;
            it.sy1 = it.sy0 + 2 * n;
        } else {
            it.sy0 = (size_t)r.off + (size_t)8 * (size_t)k;
            it.sy1 = it.sy0 + n;
            if (layout == kYuv422Nv16) {
                it.su0 = (size_t)r.off + 2 * n + (size_t)8 * (size_t)k;
                it.su1 = it.su0 + n;
            } else {
                it.su0 = (size_t)r.off + 2 * n + (size_t)4 * (size_t)k;
                it.sv0 = it.su0 + n / 2;
                it.su1 = it.su0 + n;
                it.sv1 = it.su1 + n / 2;
            }
        }
    }
    it.y0 = (size_t)(2 * rp) * (size_t)w + (size_t)8 * (size_t)g;
    it.y1 = it.y0 + (size_t)w;
    it.c = (size_t)(h + rp) * (size_t)w + (size_t)8 * (size_t)g;
    return it;
}

OCTVR_UYVY_HD inline uint8_t yuv422_avg(uint8_t a, uint8_t b) { return (uint8_t)(((int)a + (int)b + 1) >> 1); }

// The item's byte path (the short last group; a frame whose rows are not 8-byte aligned): pixel pair by pair.
template <int L>
OCTVR_UYVY_HD inline void yuv422_unpack_bytes(const uint8_t* src, uint8_t* dst, const Yuv422Item& it) {
    for (int p = 0; p < it.px; p += 2) {
        if (L == kYuv422Yuyv) {
            const uint8_t* a = src + it.sy0 + 2 * p;
            const uint8_t* b = src + it.sy1 + 2 * p;
            dst[it.y0 + p] = a[0];
            dst[it.y0 + p + 1] = a[2];
            dst[it.y1 + p] = b[0];
            dst[it.y1 + p + 1] = b[2];
            dst[it.c + p] = yuv422_avg(a[1], b[1]);
            dst[it.c + p + 1] = yuv422_avg(a[3], b[3]);
            continue;
        }
        dst[it.y0 + p] = src[it.sy0 + p];
        dst[it.y0 + p + 1] = src[it.sy0 + p + 1];
        dst[it.y1 + p] = src[it.sy1 + p];
        dst[it.y1 + p + 1] = src[it.sy1 + p + 1];
        if (L == kYuv422Nv16) {
            dst[it.c + p] = yuv422_avg(src[it.su0 + p], src[it.su1 + p]);
            dst[it.c + p + 1] = yuv422_avg(src[it.su0 + p + 1], src[it.su1 + p + 1]);
        } else {
            dst[it.c + p] = yuv422_avg(src[it.su0 + p / 2], src[it.su1 + p / 2]);
            dst[it.c + p + 1] = yuv422_avg(src[it.sv0 + p / 2], src[it.sv1 + p / 2]);
        }
    }
}

// True when the item takes the vector path: a full group whose three stores are 8-byte aligned (the frame's
// rows are when w is a multiple of 8 and its base is 8-byte aligned; the loads need no alignment).  A multiple
// of 8 also puts YUV422P's V half, at byte w / 2, on a 4-byte boundary of its row.
OCTVR_UYVY_HD inline bool yuv422_unpack_vector(int w, uintptr_t dst_base, const Yuv422Item& it) {
    return it.px == 8 && (w & 7) == 0 && ((w / 2) & 3) == 0 && (dst_base & 7u) == 0;
}

struct Yuv422Pair {
    uint32_t x, y;
};
// One lane of the unpack kernel.  Mem: load4 / load8 / load16 of the source at any alignment, store8 to an
// 8-byte aligned address of the destination.
template <int L, class Mem>
OCTVR_UYVY_HD inline void yuv422_unpack_lane(const Mem& mem, const uint8_t* src, uint8_t* dst, int w, const Yuv422Item& it) {
    if (it.px <= 0) return;
    if (!yuv422_unpack_vector(w, reinterpret_cast<uintptr_t>(dst), it)) {
        yuv422_unpack_bytes<L>(src, dst, it);
        return;
    }
    if (L == kYuv422Yuyv) {
        const UyvyWords a = mem.load16(src + it.sy0), b = mem.load16(src + it.sy1);
        mem.store8(dst + it.y0, Yuv422Pair{uyvy_perm(a.y, a.x, kYuv422SelEven), uyvy_perm(a.w, a.z, kYuv422SelEven)});
        mem.store8(dst + it.y1, Yuv422Pair{uyvy_perm(b.y, b.x, kYuv422SelEven), uyvy_perm(b.w, b.z, kYuv422SelEven)});
        mem.store8(dst + it.c, Yuv422Pair{uyvy_avg4(uyvy_perm(a.y, a.x, kYuv422SelOdd), uyvy_perm(b.y, b.x, kYuv422SelOdd)),
                                          uyvy_avg4(uyvy_perm(a.w, a.z, kYuv422SelOdd), uyvy_perm(b.w, b.z, kYuv422SelOdd))});
        return;
    }
    const Yuv422Pair y0 = mem.load8(src + it.sy0), y1 = mem.load8(src + it.sy1);
    Yuv422Pair c;
    if (L == kYuv422Nv16) {
        const Yuv422Pair a = mem.load8(src + it.su0), b = mem.load8(src + it.su1);
        c = Yuv422Pair{uyvy_avg4(a.x, b.x), uyvy_avg4(a.y, b.y)};
    } else {
        const uint32_t u = uyvy_avg4(mem.load4(src + it.su0), mem.load4(src + it.su1));
        const uint32_t v = uyvy_avg4(mem.load4(src + it.sv0), mem.load4(src + it.sv1));
        c = Yuv422Pair{uyvy_perm(v, u, kUyvySelZipLo), uyvy_perm(v, u, kUyvySelZipHi)};  // u0 v0 u1 v1, u2 v2 u3 v3
    }
    mem.store8(dst + it.y0, y0);
    mem.store8(dst + it.y1, y1);
    mem.store8(dst + it.c, c);
}

// Packs piece (row pair rp, groups [g0, g0 + ng)) of a w-wide camera at d from host planes laid out as
// octvr_async_push's: YUYV planes[0] (2 w bytes a row); NV16 planes[0] = Y, planes[1] = U,V pairs (w bytes a
// row, h rows); YUV422P planes[0 / 1 / 2] = Y, U, V (w / 2 bytes a row, h rows).  The layout the packed-source
// items above read; returns its size, 4 bytes per pixel of the piece's row.
inline size_t yuv422_pack_run(int layout, uint8_t* d, int w, int rp, int g0, int ng, const uint8_t* const* planes,
                              const size_t* pitches) {
    const size_t n = (size_t)uyvy_run_px(w, g0, ng);
    if (layout == kYuv422Yuyv) return uyvy_pack_run(d, w, rp, g0, ng, planes[0], pitches[0]);  // two packed rows
    for (int row = 0; row < 2; row++)
        memcpy(d + (size_t)row * n, planes[0] + (size_t)(2 * rp + row) * pitches[0] + (size_t)8 * (size_t)g0, n);
    d += 2 * n;
    for (int row = 0; row < 2; row++, d += n) {
        if (layout == kYuv422Nv16) {
            memcpy(d, planes[1] + (size_t)(2 * rp + row) * pitches[1] + (size_t)8 * (size_t)g0, n);
        } else {
            memcpy(d, planes[1] + (size_t)(2 * rp + row) * pitches[1] + (size_t)4 * (size_t)g0, n / 2);
            memcpy(d + n / 2, planes[2] + (size_t)(2 * rp + row) * pitches[2] + (size_t)4 * (size_t)g0, n / 2);
        }
    }
    return 4 * n;
}

// ---- out: the pack kernel's work items -----------------------------------------------------------------------
// The destination is a list of rows, each with its own head / chunk / tail arithmetic (uyvy_pack_item's: the
// bytes before the row's first 16-byte boundary, then 16-byte chunks, the last one possibly short):
//   YUYV     h rows of 2 w bytes;
//   NV16     2 h rows of w bytes: luma rows, then chroma rows;
//   YUV422P  h luma rows of w bytes, then 2 h half rows of w / 2 bytes: half row q is the U (q even) or V (q odd)
//            half of chroma row q >> 1, at byte (q & 1) w / 2 of frame row h + (q >> 1).
OCTVR_UYVY_HD inline int yuv422_pack_rows(int layout, int h) { return layout == kYuv422Yuyv ? h : layout == kYuv422Nv16 ? 2 * h : 3 * h; }
OCTVR_UYVY_HD inline uint32_t yuv422_row_items(int n) { return (uint32_t)((n + kUyvyChunk - 1) / kUyvyChunk + 1); }
OCTVR_UYVY_HD inline uint64_t yuv422_pack_items(int layout, int w, int h) {
    if (layout == kYuv422Yuyv) return (uint64_t)h * yuv422_row_items(2 * w);
    if (layout == kYuv422Nv16) return (uint64_t)(2 * h) * yuv422_row_items(w);
    return (uint64_t)h * yuv422_row_items(w) + (uint64_t)(2 * h) * yuv422_row_items(w / 2);
}

// What item `id` writes: len bytes (0: nothing) from byte b0 of list row `row` (n bytes long), at dst of the
// caller's frame (first byte at address out_base).  len = 16 only with dst 16-byte aligned.
struct Yuv422Span {
    int row, n, b0, len;
    size_t dst;
};
OCTVR_UYVY_HD inline Yuv422Span yuv422_pack_item(int layout, int w, int h, size_t pitch, uintptr_t out_base, uint32_t id) {
    Yuv422Span sp{0, 0, 0, 0, 0};
    int chunk;
    if (layout == kYuv422Planar) {
        const uint32_t per_y = yuv422_row_items(w), per_c = yuv422_row_items(w / 2);
        const uint32_t ny = (uint32_t)h * per_y;
        if (id < ny) {
            sp.row = (int)(id / per_y);
            chunk = (int)(id - (uint32_t)sp.row * per_y);
            sp.n = w;
            sp.dst = (size_t)sp.row * pitch;
        } else {
            const uint32_t q = (id - ny) / per_c;
            if (q >= (uint32_t)(2 * h)) return sp;
            chunk = (int)(id - ny - q * per_c);
            sp.row = h + (int)q;
            sp.n = w / 2;
            sp.dst = (size_t)(h + (int)(q >> 1)) * pitch + (size_t)((q & 1u) ? w / 2 : 0);
        }
    } else {
        sp.n = yuv422_frame_row_bytes(layout, w);
        const uint32_t per = yuv422_row_items(sp.n);
        sp.row = (int)(id / per);
        if (sp.row >= yuv422_frame_rows(layout, h)) return sp;
        chunk = (int)(id - (uint32_t)sp.row * per);
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

// Where byte b of list row `row` comes from in the NV12 frame (pitch = w).
OCTVR_UYVY_HD inline size_t yuv422_pack_src(int layout, int w, int h, int row, int b) {
    if (layout == kYuv422Yuyv)
        return (b & 1) ? (size_t)(h + (row >> 1)) * (size_t)w + (size_t)(b >> 1) : (size_t)row * (size_t)w + (size_t)(b >> 1);
    if (row < h) return (size_t)row * (size_t)w + (size_t)b;
    const int q = row - h;
    if (layout == kYuv422Nv16) return (size_t)(h + (q >> 1)) * (size_t)w + (size_t)b;
    return (size_t)(h + (q >> 2)) * (size_t)w + (size_t)(2 * b + (q & 1));
}

// One work item of the pack kernel.  Mem: load8 / load16 of the NV12 frame at any alignment, store16 to a
// 16-byte aligned address of the caller's frame.  A full chunk is
//   YUYV     8 bytes of the luma row zipped with 8 of the chroma row (the first from byte b0 >> 1, the second
//            from byte (b0 + 1) >> 1: which row comes first depends on b0's parity, uyvy_pack_chunk_src);
//   a luma row, an NV16 chroma row: 16 bytes copied;
//   a YUV422P half row: the even (U) or odd (V) bytes of 32 bytes of the chroma row.
template <int L, class Mem>
OCTVR_UYVY_HD inline void yuv422_pack_lane(const Mem& mem, const uint8_t* src, uint8_t* out, int w, int h, const Yuv422Span& sp) {
    if (sp.len <= 0) return;
    if (sp.len != kUyvyChunk) {  // heads and tails
        for (int i = 0; i < sp.len; i++) out[sp.dst + i] = src[yuv422_pack_src(L, w, h, sp.row, sp.b0 + i)];
        return;
    }
    UyvyWords o;
    if (L == kYuv422Yuyv) {
        const Yuv422Pair f = mem.load8(src + yuv422_pack_src(L, w, h, sp.row, sp.b0));
        const Yuv422Pair g = mem.load8(src + yuv422_pack_src(L, w, h, sp.row, sp.b0 + 1));
        o = uyvy_zip(f.x, f.y, g.x, g.y);
    } else if (L == kYuv422Nv16 || sp.row < h) {
        o = mem.load16(src + yuv422_pack_src(L, w, h, sp.row, sp.b0));
    } else {
        const int half = (sp.row - h) & 1;
        const uint8_t* const p = src + yuv422_pack_src(L, w, h, sp.row, sp.b0) - half;  // the row's bytes [2 b0, 2 b0 + 32)
        const UyvyWords a = mem.load16(p), b = mem.load16(p + 16);
        const uint32_t sel = half ? kYuv422SelOdd : kYuv422SelEven;
        o = UyvyWords{uyvy_perm(a.y, a.x, sel), uyvy_perm(a.w, a.z, sel), uyvy_perm(b.y, b.x, sel), uyvy_perm(b.w, b.z, sel)};
    }
    mem.store16(out + sp.dst, o);
}

}  // namespace octvr
