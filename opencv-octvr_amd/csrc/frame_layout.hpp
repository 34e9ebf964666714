// frame_layout.hpp — the arithmetic of the frame layouts (the eleven OCTVR_PIX_* values): the planes of a frame and the
// packing of a footprint run from them (async.cpp copy_in), for every layout; and for the eight capture layouts of
// byte and 16-bit samples the Mapper and the pipeline convert to and from their internal 8-bit NV12 frames (the
// values 16 .. 35) which bytes a work item of layout_unpack_kernel / layout_pack_kernel (frame_layout.hip) loads and
// which it stores, and the split of footprint runs into the unpack kernel's table.  v210 (48), whose samples are 10
// bits of a 32-bit word, shares the frame arithmetic, the runs and the table here; its work items and lane bodies
// are v210_layout.hpp's.
// No HIP types: the lane bodies are templates over a layout descriptor and a memory policy, so the kernels
// (non-temporal / vector accesses) and tests/cpp/frame_layout_check.cpp (memcpy against exactly sized heap blocks)
// execute one definition.
//
// A w x h picture (w, h even) in a layout is described by four properties:
//   bytes        1: a sample is a byte; 2: a 16-bit little-endian word that carries a 10-bit sample in bits 15..6
//                (msb) or in bits 9..0.  The bits of a word outside the sample are ignored on the way in and
//                written as 0 on the way out.
//   chroma       kChromaPacked: h rows of 2 w bytes, luma and chroma bytes alternating (luma_odd: luma is the odd
//                byte, U0 Y0 V0 Y1; else Y0 U0 Y1 V0), the chroma bytes of a row being its U,V pairs;
//                kChromaPairs: h rows of luma, then chroma rows of w / 2 U,V pairs;
//                kChromaHalves: h rows of luma, then chroma rows with U in samples [0, w / 2), V in [w / 2, w).
//   luma_odd     the packed kind only.
//   chroma_rows  chroma rows per row pair: 1 (4:2:0) or 2 (4:2:2).
//
//                       bytes  msb  chroma  luma_odd  chroma_rows   row bytes  rows     packed B / pixel of a run
//   YUV420P               1     -   halves     -          1             w      3 h / 2        3
//   NV12                  1     -   pairs      -          1             w      3 h / 2        3
//   UYVY422               1     -   packed    yes         2           2 w      h              4
//   YUYV422               1     -   packed    no          2           2 w      h              4
//   YUV422P               1     -   halves     -          2             w      2 h            4
//   NV16                  1     -   pairs      -          2             w      2 h            4
//   P010                  2    yes  pairs      -          1           2 w      3 h / 2        6
//   YUV420P10             2    no   halves     -          1           2 w      3 h / 2        6
//   P210                  2    yes  pairs      -          2           2 w      2 h            8
//   YUV422P10             2    no   halves     -          2           2 w      2 h            8
//   V210                  three 10-bit samples a 32-bit word, six pixels a 16-byte block (v210_layout.hpp):
//                         128 ceil(w / 48) row bytes, h rows, a run packs its covering blocks (run_bytes)
// YUV420P and NV12 are native: the kernels read and write them in place, nothing converts them (converted() is
// false, with_layout has no case for them).  On the host a frame is planes() planes, as octvr_async_push takes
// them: the packed kind one plane; pairs Y and the U,V plane; halves Y, U and V, each half a row's bytes wide.
//
// The 8-bit side of both conversions is NV12 at pitch = width ("Y over U,V pairs": h rows of Y, h / 2 rows of
// U,V pairs), so the 8-pixel group g of row pair r is luma bytes [8 g, 8 g + 8) of rows 2r, 2r + 1 and chroma
// bytes [8 g, 8 g + 8) of row h + r: the footprint's cell.  The rules:
//   in   a 10-bit sample narrows to v8 = min(255, (v10 + 2) >> 2); with two chroma rows per row pair then chroma
//        row r = (c8[2r] + c8[2r + 1] + 1) >> 1 per byte; luma copied
//   out  v10 = v8 << 2; with two chroma rows per row pair, rows 2r and 2r + 1 both carry chroma row r
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define OCTVR_LAYOUT_HD __host__ __device__
#else
#define OCTVR_LAYOUT_HD
#endif

namespace octvr {

// ---- the layouts ---------------------------------------------------------------------------------------------
enum ChromaKind : int { kChromaPacked = 0, kChromaPairs = 1, kChromaHalves = 2, kChromaV210 = 3 };
// v210: block b of a row is its pixels [6 b, 6 b + 6) in 16 bytes; a row is padded to 48 pixels.  The blocks that
// hold the samples of groups [g0, g0 + ng) of a w-wide row (8 pixels a group, cut at the width) are
// [v210_block0(g0), v210_block0(g0) + v210_blocks(w, g0, ng)).
constexpr int kV210Block = 16;
OCTVR_LAYOUT_HD constexpr int v210_row_bytes(int w) { return 128 * ((w + 47) / 48); }
OCTVR_LAYOUT_HD constexpr int v210_block0(int g0) { return 8 * g0 / 6; }
OCTVR_LAYOUT_HD constexpr int v210_blocks(int w, int g0, int ng) {
    return ((8 * (g0 + ng) < w ? 8 * (g0 + ng) : w) + 5) / 6 - v210_block0(g0);
}
struct LayoutDesc {
    int bytes;        // 0: no OCTVR_PIX_* value; 4: v210's word of three samples
    bool msb;
    int chroma;
    bool luma_odd;
    int chroma_rows;
    bool native = false;  // YUV420P, NV12
    OCTVR_LAYOUT_HD constexpr bool converted() const { return bytes != 0 && !native; }
    OCTVR_LAYOUT_HD constexpr bool packed() const { return chroma == kChromaPacked; }
    OCTVR_LAYOUT_HD constexpr bool halves() const { return chroma == kChromaHalves; }
    OCTVR_LAYOUT_HD constexpr bool v210() const { return chroma == kChromaV210; }
    // bytes per row and rows of a w x h frame
    OCTVR_LAYOUT_HD constexpr int row_bytes(int w) const { return v210() ? v210_row_bytes(w) : (packed() ? 2 : 1) * bytes * w; }
    OCTVR_LAYOUT_HD constexpr int rows(int h) const { return packed() || v210() ? h : h + chroma_rows * (h / 2); }
    // the host planes of such a frame, and bytes per row and rows of plane k
    constexpr int planes() const { return packed() || v210() ? 1 : halves() ? 3 : 2; }
    constexpr int plane_row_bytes(int k, int w) const { return k && halves() ? row_bytes(w) / 2 : row_bytes(w); }
    constexpr int plane_rows(int k, int h) const { return k ? chroma_rows * (h / 2) : h; }
    // packed bytes per pixel of a table piece's row: its two luma rows and its chroma row(s) (pack_run)
    // (v210: 0, a run packs whole blocks)
    OCTVR_LAYOUT_HD constexpr int run_bpp() const { return v210() ? 0 : packed() ? 4 : bytes * (2 + chroma_rows); }
    // packed bytes of groups [g0, g0 + ng) of a row pair of a w-wide frame: run_bpp() per pixel of the run's row;
    // v210: the covering blocks of its two rows.  run_key: what the sizes of a table's pieces depend on.
    OCTVR_LAYOUT_HD constexpr size_t run_bytes(int w, int g0, int ng) const {
        return v210() ? (size_t)(2 * kV210Block) * (size_t)v210_blocks(w, g0, ng)
                      : (size_t)run_bpp() * (size_t)((8 * (g0 + ng) < w ? 8 * (g0 + ng) : w) - 8 * g0);
    }
    constexpr int run_key() const { return v210() ? -210 : run_bpp(); }
    // a frame of 16-bit (32-bit) words has a base and a pitch that are multiples of 2 (4): a word's natural alignment
    bool aligned(const void* base, size_t pitch) const {
        return bytes < 2 || ((reinterpret_cast<uintptr_t>(base) | pitch) & (uintptr_t)(bytes - 1)) == 0;
    }
};
// One compile-time descriptor per layout, the tag of the lane bodies' instantiations.
template <int Bytes, bool Msb, int Chroma, bool LumaOdd, int ChromaRows>
struct Layout {
    static constexpr LayoutDesc desc{Bytes, Msb, Chroma, LumaOdd, ChromaRows};
};
using LayoutUyvy = Layout<1, false, kChromaPacked, true, 2>;
using LayoutYuyv = Layout<1, false, kChromaPacked, false, 2>;
using LayoutYuv422p = Layout<1, false, kChromaHalves, false, 2>;
using LayoutNv16 = Layout<1, false, kChromaPairs, false, 2>;
using LayoutP010 = Layout<2, true, kChromaPairs, false, 1>;
using LayoutYuv420p10 = Layout<2, false, kChromaHalves, false, 1>;
using LayoutP210 = Layout<2, true, kChromaPairs, false, 2>;
using LayoutYuv422p10 = Layout<2, false, kChromaHalves, false, 2>;
// v210 is no instance of the lane bodies below (with_layout has no case for it): v210_layout.hpp
constexpr LayoutDesc kLayoutV210{4, false, kChromaV210, false, 2};

// f(tag) of the OCTVR_PIX_* value's layout; false when `pix` is no converted format.
template <class F>
inline bool with_layout(int pix, F&& f) {
    switch (pix) {
    case 16: f(LayoutUyvy{}); return true;       // OCTVR_PIX_UYVY422
    case 17: f(LayoutYuyv{}); return true;       // OCTVR_PIX_YUYV422
    case 18: f(LayoutYuv422p{}); return true;    // OCTVR_PIX_YUV422P
    case 19: f(LayoutNv16{}); return true;       // OCTVR_PIX_NV16
    case 32: f(LayoutP010{}); return true;       // OCTVR_PIX_P010
    case 33: f(LayoutYuv420p10{}); return true;  // OCTVR_PIX_YUV420P10
    case 34: f(LayoutP210{}); return true;       // OCTVR_PIX_P210
    case 35: f(LayoutYuv422p10{}); return true;  // OCTVR_PIX_YUV422P10
    }
    return false;
}
// The run-time lookup of all eleven layouts; bytes == 0 for any other value.
inline LayoutDesc layout_of(int pix) {
    if (pix == 0) return LayoutDesc{1, false, kChromaHalves, false, 1, true};  // OCTVR_PIX_YUV420P
    if (pix == 1) return LayoutDesc{1, false, kChromaPairs, false, 1, true};   // OCTVR_PIX_NV12
    if (pix == 48) return kLayoutV210;                                         // OCTVR_PIX_V210
    LayoutDesc d{0, false, 0, false, 0};
    with_layout(pix, [&](auto tag) { d = decltype(tag)::desc; });
    return d;
}
inline bool converted_format(int pix) { return layout_of(pix).converted(); }

// Why (base, pitch) is no whole w x h device frame of the layout below `limit` bytes (what the kernels that touch
// it address with 32 bits); NULL when it is one.
inline const char* frame_fault(const LayoutDesc& d, const void* base, size_t pitch, int w, int h, uint64_t limit) {
    if (!base) return "frame is NULL";
    if (!d.aligned(base, pitch))
        return d.v210() ? "frame address and pitch must be multiples of 4 for v210's 32-bit words"
                        : "frame address and pitch must be multiples of 2 for 16-bit samples";
    if (pitch < (size_t)d.row_bytes(w)) return "pitch smaller than a row of the format";
    if ((uint64_t)pitch * (uint64_t)d.rows(h) >= limit) return "frame larger than 2 GiB";
    return nullptr;
}

// ---- rows in 16-byte chunks ----------------------------------------------------------------------------------
// The copy kernels (layout_pack_kernel, merge_regions_kernel) cut a destination row of n bytes whose first byte is
// at address a into work items: item 0 is the bytes before the row's first 16-byte boundary (at most 15, possibly
// none), then 16-byte chunks, the last one possibly short.  row_items: an upper bound over every alignment.
// row_chunk: item 0 is `head` bytes from byte 0; item `chunk` > 0 is len(n) bytes from byte b0, nothing when b0 >= n.
// len = 16 only at a 16-byte aligned address.  The caller branches on the three cases itself: its work item differs
// per case, and the kernels keep the code they had.
constexpr int kChunk = 16;
OCTVR_LAYOUT_HD inline uint32_t row_items(int n) { return (uint32_t)((n + kChunk - 1) / kChunk + 1); }
struct RowChunk {
    int head, b0;
    OCTVR_LAYOUT_HD int len(int n) const { return n - b0 < kChunk ? n - b0 : kChunk; }
};
OCTVR_LAYOUT_HD inline RowChunk row_chunk(uintptr_t a, int n, int chunk) {
    const int to_boundary = (int)((0 - a) & (uintptr_t)(kChunk - 1));
    const int head = to_boundary < n ? to_boundary : n;
    return RowChunk{head, head + kChunk * (chunk - 1)};
}

// ---- bytes ---------------------------------------------------------------------------------------------------
struct Words4 {
    uint32_t x, y, z, w;
};
struct Words2 {
    uint32_t x, y;
};
// v_perm_b32: byte k of the result is byte sel[k] of the eight bytes {hi, lo} (0-3: lo, 4-7: hi); the selector
// byte 0x0c gives a zero byte
OCTVR_LAYOUT_HD inline uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
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
constexpr uint32_t kSelEven = 0x06040200u;    // bytes 0, 2, 4, 6 of {hi, lo}: YUYV's luma, UYVY's chroma, a U,V row's U
constexpr uint32_t kSelOdd = 0x07050301u;     // bytes 1, 3, 5, 7: UYVY's luma, YUYV's chroma, a U,V row's V, narrowed samples
constexpr uint32_t kSelOddZip = 0x07030501u;  // byte 1 of lo, of hi, byte 3 of lo, of hi: narrowed u0 v0 u1 v1
constexpr uint32_t kSelZipLo = 0x05010400u;   // a0 a1 a2 a3, b0 b1 b2 b3 (lo = a, hi = b) -> a0 b0 a1 b1
constexpr uint32_t kSelZipHi = 0x07030602u;   //                                            -> a2 b2 a3 b3
// Two bytes of a dword as two words: bytes (0, 1), (2, 3), (0, 2), (1, 3) into the words' low bytes (a sample in
// bits 9..0, then << 2) or high bytes (a sample in bits 15..6: v8 << 8)
constexpr uint32_t kWide01Lo = 0x0c010c00u, kWide23Lo = 0x0c030c02u, kWide02Lo = 0x0c020c00u, kWide13Lo = 0x0c030c01u;
constexpr uint32_t kWide01Hi = 0x010c000cu, kWide23Hi = 0x030c020cu, kWide02Hi = 0x020c000cu, kWide13Hi = 0x030c010cu;

// (a + b + 1) >> 1 of each of the four bytes: a + b = 2 (a | b) - (a ^ b), so the rounded-up half is
// (a | b) - ((a ^ b) >> 1); the shift's bits that crossed a byte boundary are masked off, and no byte borrows
// ((a ^ b) >> 1 <= a | b per byte).
OCTVR_LAYOUT_HD inline uint32_t avg4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) >> 1) & 0x7F7F7F7Fu); }
OCTVR_LAYOUT_HD inline Words2 avg8(const Words2& a, const Words2& b) { return Words2{avg4(a.x, b.x), avg4(a.y, b.y)}; }
OCTVR_LAYOUT_HD inline uint8_t avg1(uint8_t a, uint8_t b) { return (uint8_t)(((int)a + (int)b + 1) >> 1); }

// ---- samples -------------------------------------------------------------------------------------------------
// One sample at p by the in rule, and one 8-bit value as the sample written at p by the out rule.
OCTVR_LAYOUT_HD inline uint8_t narrow_at(const LayoutDesc& d, const uint8_t* p) {
    if (d.bytes == 1) return p[0];
    const uint32_t word = (uint32_t)p[0] | (uint32_t)p[1] << 8;
    const uint32_t v10 = d.msb ? word >> 6 : word & 0x3FFu;
    const uint32_t v8 = (v10 + 2u) >> 2;
    return (uint8_t)(v8 > 255u ? 255u : v8);
}
OCTVR_LAYOUT_HD inline void widen_at(const LayoutDesc& d, uint8_t* p, uint8_t v8) {
    if (d.bytes == 1) {
        p[0] = v8;
        return;
    }
    const uint32_t v = (uint32_t)v8 << (d.msb ? 8 : 2);
    p[0] = (uint8_t)(v & 0xFFu);
    p[1] = (uint8_t)(v >> 8);
}

// Two samples in bits 15..6 of a dword's halves: min(0xFFFF, half + 128) of each half, so that byte 1 and byte 3
// are the two narrowed samples — min(255, (word + 128) >> 8) = min(255, (v10 + 2) >> 2), as the 6 low bits of a
// word lie below bit 7 and never carry into it.  One v_pk_add_u16 with clamp on the device.
OCTVR_LAYOUT_HD inline uint32_t round2(uint32_t d) {
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
OCTVR_LAYOUT_HD inline uint32_t narrow2(uint32_t d) {
    return round2(MSB ? d : d << 6);
}
// 8 words -> 8 bytes; 4 words of U and 4 of V -> 8 bytes of U,V pairs
template <bool MSB>
OCTVR_LAYOUT_HD inline Words2 narrow8(const Words4& a) {
    return Words2{perm(narrow2<MSB>(a.y), narrow2<MSB>(a.x), kSelOdd), perm(narrow2<MSB>(a.w), narrow2<MSB>(a.z), kSelOdd)};
}
template <bool MSB>
OCTVR_LAYOUT_HD inline Words2 narrow_zip(const Words2& u, const Words2& v) {
    return Words2{perm(narrow2<MSB>(v.x), narrow2<MSB>(u.x), kSelOddZip), perm(narrow2<MSB>(v.y), narrow2<MSB>(u.y), kSelOddZip)};
}
// 8 bytes -> 8 words; of a dword's four bytes the even (odd == 0) or the odd ones -> 2 words
template <bool MSB>
OCTVR_LAYOUT_HD inline Words4 widen8(uint32_t a, uint32_t b) {
    if (MSB) return Words4{perm(0, a, kWide01Hi), perm(0, a, kWide23Hi), perm(0, b, kWide01Hi), perm(0, b, kWide23Hi)};
    return Words4{perm(0, a, kWide01Lo) << 2, perm(0, a, kWide23Lo) << 2, perm(0, b, kWide01Lo) << 2, perm(0, b, kWide23Lo) << 2};
}
template <bool MSB>
OCTVR_LAYOUT_HD inline uint32_t widen_alternate(uint32_t a, int odd) {
    if (MSB) return perm(0, a, odd ? kWide13Hi : kWide02Hi);
    return perm(0, a, odd ? kWide13Lo : kWide02Lo) << 2;
}

// ---- in: the unpack kernel's table and work items ------------------------------------------------------------
// A run is ng consecutive 8-pixel groups from group g0 of row pair rp of camera cam (host_common.hpp
// SourceFootprint), the entry of every upload table: the native layouts' (mapper.cpp footprint_runs;
// unpack_runs_kernel, unpack_runs_nv12_kernel) and the converted layouts' (run_table below).  The source of an
// unpack is either the caller's frame (src_pitch >= the layout's row bytes) or the pipeline's packed upload buffer
// (src_pitch == 0: the run's bytes at `off`, pack_run's layout).
struct FootRun {
    uint32_t cam;  // camera | row pair << 8
    uint32_t g0, ng;
    uint32_t off;
};
using ConvRun = FootRun;  // a piece of run_table: a run of at most kWave groups

// Luma samples of one row of the run: its groups cut at the width.
OCTVR_LAYOUT_HD inline int run_px(int w, int g0, int ng) { return (8 * (g0 + ng) < w ? 8 * (g0 + ng) : w) - 8 * g0; }

// What the lane of group k (< r.ng) of table piece r does for a w x h camera.  It writes px bytes at y0, at y1 and
// at c of the camera's NV12 frame (pitch = w) and reads, with S the layout's bytes per sample,
//   packed   2 px bytes at sy0 and at sy1 (the packed rows 2 rp, 2 rp + 1);
//   pairs    S px bytes of luma at sy0, sy1 and S px bytes of U,V pairs at su0 (and at su1 with two chroma rows);
//   halves   S px bytes of luma at sy0, sy1, S px / 2 bytes of U at su0 (su1) and S px / 2 of V at sv0 (sv1).
// px = 8, or 2, 4 or 6 in the short last group of a width that is no multiple of 8; px <= 0: nothing (no such
// group is built).  In the packed upload buffer a piece is its two luma rows, then its chroma row(s) in the
// layout's order (the U part before the V part for the halves kind); for the packed kind its two packed rows:
// run_bpp() bytes per pixel of the piece's row.  Offsets a layout does not read are 0.
struct LayoutItem {
    int px;
    size_t sy0, sy1, su0, su1, sv0, sv1;
    size_t y0, y1, c;
};
OCTVR_LAYOUT_HD inline LayoutItem unpack_item(const LayoutDesc& d, int w, int h, size_t src_pitch, const FootRun& r, int k) {
    const int rp = (int)(r.cam >> 8), g = (int)r.g0 + k;
    const size_t S = (size_t)d.bytes;
    LayoutItem it;
    const int left = w - 8 * g;
    it.px = (k < 0 || k >= (int)r.ng || 2 * rp + 1 >= h) ? 0 : left < 8 ? left : 8;
    it.su0 = it.su1 = it.sv0 = it.sv1 = 0;
    const size_t lg = d.packed() ? 16 : 8 * S;  // bytes of a group in a luma (packed) row
    const size_t cg = d.halves() ? 4 * S : 8 * S;  // ... in a chroma (half) row
    size_t row, half;  // from a row of the piece to its next; from a chroma row's U part to its V part
    if (src_pitch) {
        it.sy0 = (size_t)(2 * rp) * src_pitch + lg * (size_t)g;
        it.su0 = (size_t)(h + d.chroma_rows * rp) * src_pitch + cg * (size_t)g;
        row = src_pitch;
        half = (size_t)(d.bytes * w / 2);
        it.sy1 = it.sy0 + row;
    } else {
        const size_t n = (size_t)run_px(w, (int)r.g0, (int)r.ng);
        it.sy0 = (size_t)r.off + lg * (size_t)k;
        row = S * n;
        half = d.bytes == 2 ? n : n / 2;
        it.sy1 = it.sy0 + (d.packed() ? 2 * n : row);
        it.su0 = (size_t)r.off + 2 * row + cg * (size_t)k;
    }
    if (d.packed()) it.su0 = 0;
    if (d.halves()) it.sv0 = it.su0 + half;
    if (!d.packed() && d.chroma_rows == 2) {
        it.su1 = it.su0 + row;
        if (d.halves()) it.sv1 = it.su1 + half;
    }
    it.y0 = (size_t)(2 * rp) * (size_t)w + (size_t)8 * (size_t)g;
    it.y1 = it.y0 + (size_t)w;
    it.c = (size_t)(h + rp) * (size_t)w + (size_t)8 * (size_t)g;
    return it;
}

// The item sample by sample (the short last group; an NV12 frame whose rows are not 8-byte aligned).
template <class L>
OCTVR_LAYOUT_HD inline void unpack_samples(const uint8_t* src, uint8_t* dst, const LayoutItem& it) {
    constexpr LayoutDesc d = L::desc;
    for (int p = 0; p < it.px; p++) {
        // chroma byte p of the group is U (p even) or V (p odd) of pixel pair p / 2
        size_t y, c0, c1;
        if (d.packed()) {
            y = (size_t)(2 * p + (d.luma_odd ? 1 : 0));
            c0 = it.sy0 + (size_t)(2 * p + (d.luma_odd ? 0 : 1));
            c1 = it.sy1 + (size_t)(2 * p + (d.luma_odd ? 0 : 1));
        } else {
            y = (size_t)(d.bytes * p);
            const size_t o = (size_t)d.bytes * (size_t)(d.halves() ? p >> 1 : p);
            c0 = (d.halves() && (p & 1) ? it.sv0 : it.su0) + o;
            c1 = (d.halves() && (p & 1) ? it.sv1 : it.su1) + o;
        }
        dst[it.y0 + p] = narrow_at(d, src + it.sy0 + y);
        dst[it.y1 + p] = narrow_at(d, src + it.sy1 + y);
        const uint8_t a = narrow_at(d, src + c0);
        dst[it.c + p] = d.chroma_rows == 2 ? avg1(a, narrow_at(d, src + c1)) : a;
    }
}

// True when the item takes the vector path: a full group whose three stores are 8-byte aligned (the NV12
// frame's rows are when w is a multiple of 8 and its base is 8-byte aligned; the loads need no alignment).  A
// multiple of 8 also puts a byte frame's V half, at byte w / 2, on a 4-byte boundary of its row.
OCTVR_LAYOUT_HD inline bool unpack_vector(int w, uintptr_t dst_base, const LayoutItem& it) {
    return it.px == 8 && (w & 7) == 0 && (dst_base & 7u) == 0;
}

// One lane of the unpack kernel.  Mem: load4 / load8 / load16 of the source at any alignment, store8 to an
// 8-byte aligned address of the destination.  8 samples of a row are 8 bytes or, narrowed, 16.
template <class L, class Mem>
OCTVR_LAYOUT_HD inline Words2 load_narrow8(const Mem& mem, const uint8_t* p) {
    if (L::desc.bytes == 1) return mem.load8(p);
    return narrow8<L::desc.msb>(mem.load16(p));
}
template <class L, class Mem>
OCTVR_LAYOUT_HD inline void unpack_lane(const Mem& mem, const uint8_t* src, uint8_t* dst, int w, const LayoutItem& it) {
    constexpr LayoutDesc d = L::desc;
    if (it.px <= 0) return;
    if (!unpack_vector(w, reinterpret_cast<uintptr_t>(dst), it)) {
        unpack_samples<L>(src, dst, it);
        return;
    }
    Words2 y0, y1, c;
    if (d.packed()) {  // byte permutes split luma from chroma
        constexpr uint32_t sel_y = d.luma_odd ? kSelOdd : kSelEven, sel_c = d.luma_odd ? kSelEven : kSelOdd;
        const Words4 a = mem.load16(src + it.sy0), b = mem.load16(src + it.sy1);
        y0 = Words2{perm(a.y, a.x, sel_y), perm(a.w, a.z, sel_y)};
        y1 = Words2{perm(b.y, b.x, sel_y), perm(b.w, b.z, sel_y)};
        c = Words2{avg4(perm(a.y, a.x, sel_c), perm(b.y, b.x, sel_c)), avg4(perm(a.w, a.z, sel_c), perm(b.w, b.z, sel_c))};
    } else {
        y0 = load_narrow8<L>(mem, src + it.sy0);
        y1 = load_narrow8<L>(mem, src + it.sy1);
        if (!d.halves()) {
            c = load_narrow8<L>(mem, src + it.su0);
            if (d.chroma_rows == 2) c = avg8(c, load_narrow8<L>(mem, src + it.su1));
        } else if (d.bytes == 1) {  // averaged as 4 bytes of U and 4 of V, then zipped into U,V pairs
            uint32_t u = mem.load4(src + it.su0), v = mem.load4(src + it.sv0);
            if (d.chroma_rows == 2) {
                u = avg4(u, mem.load4(src + it.su1));
                v = avg4(v, mem.load4(src + it.sv1));
            }
            c = Words2{perm(v, u, kSelZipLo), perm(v, u, kSelZipHi)};  // u0 v0 u1 v1, u2 v2 u3 v3
        } else {  // the permute that gathers the narrowed samples also zips U with V
            c = narrow_zip<d.msb>(mem.load8(src + it.su0), mem.load8(src + it.sv0));
            if (d.chroma_rows == 2) c = avg8(c, narrow_zip<d.msb>(mem.load8(src + it.su1), mem.load8(src + it.sv1)));
        }
    }
    mem.store8(dst + it.y0, y0);
    mem.store8(dst + it.y1, y1);
    mem.store8(dst + it.c, c);
}

// Packs run (row pair rp, groups [g0, g0 + ng)) of a w-wide camera at d from host planes laid out as
// octvr_async_push's: the packed kind and v210 planes[0]; pairs planes[0] = Y, planes[1] = U,V pairs; halves
// planes[0 / 1 / 2] = Y, U, V.  Any of the ten layouts: what the packed-source items above read, and for the native
// two what unpack_runs_kernel / unpack_runs_nv12_kernel read (w is even, so the U and the V part are half the pair
// row each and both pack 3 bytes per pixel).  Returns its size, run_bytes().
inline size_t pack_run(const LayoutDesc& l, uint8_t* d, int w, int rp, int g0, int ng, const uint8_t* const* planes,
                       const size_t* pitches) {
    if (l.v210()) {  // the covering blocks of the two rows, rows back to back
        const size_t nb = (size_t)kV210Block * (size_t)v210_blocks(w, g0, ng);
        for (int row = 0; row < 2; row++, d += nb)
            memcpy(d, planes[0] + (size_t)(2 * rp + row) * pitches[0] + (size_t)kV210Block * (size_t)v210_block0(g0), nb);
        return 2 * nb;
    }
    const size_t S = (size_t)l.bytes, n = (size_t)run_px(w, g0, ng), G = (size_t)g0;
    const size_t ln = l.packed() ? 2 * n : S * n;  // bytes of the piece in a luma (packed) row
    for (int row = 0; row < 2; row++, d += ln)
        memcpy(d, planes[0] + (size_t)(2 * rp + row) * pitches[0] + (l.packed() ? 16 : 8 * S) * G, ln);
    for (int row = 0; row < (l.packed() ? 0 : l.chroma_rows); row++, d += S * n) {
        const size_t cr = (size_t)(l.chroma_rows * rp + row);
        if (l.halves()) {
            memcpy(d, planes[1] + cr * pitches[1] + 4 * S * G, S * n / 2);
            memcpy(d + S * n / 2, planes[2] + cr * pitches[2] + 4 * S * G, S * n / 2);
        } else {
            memcpy(d, planes[1] + cr * pitches[1] + 8 * S * G, S * n);
        }
    }
    return (size_t)l.run_bpp() * n;
}

// The unpack kernel's table of a set of footprint runs: each run cut into pieces of at most kWave groups (a
// group of lanes takes one piece, a lane a group), each piece's `off` its place in the packed upload buffer
// (pieces back to back, pack_run's layout each).  bytes: the packed size, which is also the packed bytes a
// frame's unpack reads.
constexpr int kWave = 64;
template <class Run>
inline std::vector<FootRun> run_table(const LayoutDesc& l, const std::vector<Run>& runs, const std::vector<int>& in_w,
                                      size_t& bytes) {
    std::vector<FootRun> t;
    bytes = 0;
    for (const Run& r : runs) {
        const int w = in_w[r.cam & 31u];
        for (uint32_t k = 0; k < r.ng; k += kWave) {
            const uint32_t ng = r.ng - k < (uint32_t)kWave ? r.ng - k : (uint32_t)kWave;
            t.push_back(FootRun{r.cam, r.g0 + k, ng, (uint32_t)bytes});
            bytes += l.run_bytes(w, (int)(r.g0 + k), (int)ng);
        }
    }
    return t;
}

// ---- out: the pack kernel's work items -----------------------------------------------------------------------
// The destination is a list of rows, each cut into row_chunk's items (all even for 16-bit samples, as the base,
// the pitch and a half row's start are):
//   packed   h rows of 2 w bytes;
//   pairs    rows(h) rows of S w bytes: luma rows, then chroma rows;
//   halves   h luma rows of S w bytes, then half rows of S w / 2 bytes, two per chroma row: half row q is the U
//            (q even) or V (q odd) half of chroma row q >> 1, at byte (q & 1) S w / 2 of frame row h + (q >> 1).
OCTVR_LAYOUT_HD inline int full_rows(const LayoutDesc& d, int h) { return d.halves() ? h : d.rows(h); }
OCTVR_LAYOUT_HD inline int half_rows(const LayoutDesc& d, int h) { return d.halves() ? 2 * d.chroma_rows * (h / 2) : 0; }
OCTVR_LAYOUT_HD inline uint64_t pack_items(const LayoutDesc& d, int w, int h) {
    return (uint64_t)full_rows(d, h) * row_items(d.row_bytes(w)) + (uint64_t)half_rows(d, h) * row_items(d.row_bytes(w) / 2);
}

// What item `id` writes: len bytes (0: nothing) from byte b0 of list row `row` (n bytes long), at dst of the
// caller's frame (first byte at address out_base).  len = 16 only with dst 16-byte aligned.
struct LayoutSpan {
    int row, n, b0, len;
    size_t dst;
};
// Where the rows of a w x h picture start in the frame it is written to, as byte offsets from the frame's first
// byte: y its first luma (packed) row; u its first chroma row (the halves kind: that row's U half); v the halves
// kind's first V half.  The rows of each follow at the frame's pitch.  A picture that is the whole frame is
// whole_frame_place; a sub-picture placed in a larger frame (the pipeline's merged frame: async_host.hpp
// region_rects) has its own three offsets, and the list rows, their lengths and the chunks are the picture's own.
struct PackPlace {
    size_t y, u, v;
};
OCTVR_LAYOUT_HD inline PackPlace whole_frame_place(const LayoutDesc& d, int w, int h, size_t pitch) {
    return PackPlace{0, (size_t)h * pitch, (size_t)h * pitch + (size_t)(d.row_bytes(w) / 2)};
}
OCTVR_LAYOUT_HD inline LayoutSpan pack_item_at(const LayoutDesc& d, int w, int h, size_t pitch, const PackPlace& at,
                                               uintptr_t out_base, uint32_t id) {
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
        sp.dst = sp.row < h ? at.y + (size_t)sp.row * pitch : at.u + (size_t)(sp.row - h) * pitch;
    } else {
        const uint32_t q = (id - first_half) / per_half;
        if (q >= (uint32_t)half_rows(d, h)) return sp;
        chunk = (int)(id - first_half - q * per_half);
        sp.row = h + (int)q;
        sp.n = n_full / 2;
        sp.dst = ((q & 1u) ? at.v : at.u) + (size_t)(q >> 1) * pitch;
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
OCTVR_LAYOUT_HD inline LayoutSpan pack_item(const LayoutDesc& d, int w, int h, size_t pitch, uintptr_t out_base, uint32_t id) {
    return pack_item_at(d, w, h, pitch, whole_frame_place(d, w, h, pitch), out_base, id);
}

// Where sample i of list row `row` comes from in the NV12 frame (pitch = w); a packed row's samples are its bytes.
OCTVR_LAYOUT_HD inline size_t pack_src(const LayoutDesc& d, int w, int h, int row, int i) {
    if (d.packed())
        return ((i & 1) != 0) == d.luma_odd ? (size_t)row * (size_t)w + (size_t)(i >> 1)
                                            : (size_t)(h + (row >> 1)) * (size_t)w + (size_t)(i >> 1);
    if (row < h) return (size_t)row * (size_t)w + (size_t)i;
    const int q = row - h;
    const int sh = d.chroma_rows == 2 ? 1 : 0;  // with two chroma rows per row pair, each NV12 chroma row is written twice
    if (!d.halves()) return (size_t)(h + (q >> sh)) * (size_t)w + (size_t)i;
    return (size_t)(h + (q >> (1 + sh))) * (size_t)w + (size_t)(2 * i + (q & 1));
}

// One work item of the pack kernel.  Mem: load8 / load16 of the NV12 frame at any alignment, store16 to a
// 16-byte aligned address of the caller's frame.  A full chunk is
//   a packed row: 8 bytes of the luma row zipped with 8 of the chroma row (the first from byte b0 >> 1, the
//            second from byte (b0 + 1) >> 1: which row comes first depends on b0's parity and on luma_odd);
//   a luma row, a chroma row of pairs: 16 bytes copied, or 8 bytes widened to 8 words;
//   a half row: the even (U) or odd (V) bytes of 32 bytes of the NV12 chroma row, or of 16 bytes, widened.
// Heads and tails go sample by sample.
template <class L, class Mem>
OCTVR_LAYOUT_HD inline void pack_lane(const Mem& mem, const uint8_t* src, uint8_t* out, int w, int h, const LayoutSpan& sp) {
    constexpr LayoutDesc d = L::desc;
    if (sp.len <= 0) return;
    if (sp.len != kChunk) {
        for (int i = 0; i < sp.len; i += d.bytes)
            widen_at(d, out + sp.dst + i, src[pack_src(d, w, h, sp.row, (sp.b0 + i) >> (d.bytes - 1))]);
        return;
    }
    const uint8_t* const p = src + pack_src(d, w, h, sp.row, sp.b0 >> (d.bytes - 1));
    const int half = (sp.row - h) & 1;  // of a half row
    Words4 o;
    if (d.packed()) {
        const Words2 f = mem.load8(p), g = mem.load8(src + pack_src(d, w, h, sp.row, sp.b0 + 1));
        o = Words4{perm(g.x, f.x, kSelZipLo), perm(g.x, f.x, kSelZipHi), perm(g.y, f.y, kSelZipLo), perm(g.y, f.y, kSelZipHi)};
    } else if (!d.halves() || sp.row < h) {
        if (d.bytes == 1) {
            o = mem.load16(p);
        } else {
            const Words2 s = mem.load8(p);
            o = widen8<d.msb>(s.x, s.y);
        }
    } else if (d.bytes == 1) {
        const Words4 a = mem.load16(p - half), b = mem.load16(p - half + 16);  // the row's bytes [2 b0, 2 b0 + 32)
        const uint32_t sel = half ? kSelOdd : kSelEven;
        o = Words4{perm(a.y, a.x, sel), perm(a.w, a.z, sel), perm(b.y, b.x, sel), perm(b.w, b.z, sel)};
    } else {
        const Words4 a = mem.load16(p - half);  // the row's bytes [b0, b0 + 16)
        o = Words4{widen_alternate<d.msb>(a.x, half), widen_alternate<d.msb>(a.y, half), widen_alternate<d.msb>(a.z, half),
                   widen_alternate<d.msb>(a.w, half)};
    }
    mem.store16(out + sp.dst, o);
}

}  // namespace octvr
