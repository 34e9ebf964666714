// async_host.hpp — the AsyncMultiMapper pipeline's pure host arithmetic (no HIP, no device) on its output side:
// the merge of the output planes' byte ranges before they are page-locked (octvr_async_register_output), where
// the pieces of a region frame land in the output planes (region_pieces: the D2H copies, the copy-out and the
// merge table all place them by it), and the region table and work-item arithmetic of the device-frame merge
// (octvr_async_push_device), which merge_regions_kernel shares; and for a merged frame in a converted layout
// (octvr_async_set_output_format) the region rule, a region's rectangles per plane (region_rects) and the table and
// work items merge_pack_kernel shares.  The input side (the layouts' planes, pack_run) is frame_layout.hpp's.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "frame_layout.hpp"

namespace octvr {

// A byte range [begin, end) of host memory.
struct PinRange {
    uintptr_t begin, end;
};

// The ranges to page-lock for a set of plane ranges: ranges whose page-rounded extents touch or overlap
// (two planes of one allocation: an NV12 frame's Y and U,V, or U and V as column halves of one array) become
// one range from the lowest begin to the highest end of the group, so no page is locked twice; a range that
// shares no page with another stays exactly as given.  Empty ranges are dropped.  Sorted by address.
inline std::vector<PinRange> merge_pin_ranges(std::vector<PinRange> in, uintptr_t page) {
    std::vector<PinRange> out;
    in.erase(std::remove_if(in.begin(), in.end(), [](const PinRange& r) { return r.end <= r.begin; }), in.end());
    std::sort(in.begin(), in.end(), [](const PinRange& a, const PinRange& b) { return a.begin < b.begin; });
    uintptr_t page_end = 0;  // page-rounded end of out.back()
    for (const PinRange& r : in) {
        const uintptr_t lo = r.begin / page * page;
        const uintptr_t hi = r.end > UINTPTR_MAX - page ? UINTPTR_MAX : (r.end + page - 1) / page * page;
        if (!out.empty() && lo <= page_end) {
            out.back().end = std::max(out.back().end, r.end);
            page_end = std::max(page_end, hi);
        } else {
            out.push_back(r);
            page_end = hi;
        }
    }
    return out;
}

// ---- where a region lands ------------------------------------------------------------------------------------
struct PlaneRect {  // a rectangle of a plane, in the plane's own pixels
    int x, y, w, h;
};

// A mapper writes its region as a frame of its own, pitch = w: h rows of Y, then h / 2 chroma rows, each [U | V]
// halves of w / 2 bytes (planar output) or w bytes of U,V pairs (NV12).  A piece of it is `rows` rows of `bytes`
// bytes from byte `src` of that frame, which land at byte column x, row y of output plane `plane` (0: Y; 1: U,
// or the U,V plane; 2: V).
struct RegionPiece {
    int plane;
    size_t x, y, src, bytes, rows;
};
struct RegionPieces {
    int n;  // 3, or 2 with NV12
    RegionPiece p[3];  // the luma piece first; the chroma pieces have the same rows
};
// The pieces of the region with rectangle r in the Y plane and c in the U / V planes (c.w = r.w / 2 and
// c.h = r.h / 2, octvr_async_create); in the U,V plane chroma column c.x is byte column 2 c.x.
inline RegionPieces region_pieces(const PlaneRect& r, const PlaneRect& c, int nv12) {
    const size_t w = (size_t)r.w, luma = (size_t)r.h * w, cw = (size_t)c.w, ch = (size_t)c.h;
    RegionPieces o{nv12 ? 2 : 3, {{0, (size_t)r.x, (size_t)r.y, 0, w, (size_t)r.h}, {}, {}}};
    if (nv12) {
        o.p[1] = RegionPiece{1, 2 * (size_t)c.x, (size_t)c.y, luma, w, ch};
    } else {
        o.p[1] = RegionPiece{1, (size_t)c.x, (size_t)c.y, luma, cw, ch};
        o.p[2] = RegionPiece{2, (size_t)c.x, (size_t)c.y, luma + w / 2, cw, ch};
    }
    return o;
}

// ---- the merge of the regions into one device frame (octvr_async_push_device, async_merge.hip) ----------
// merge_region_items and merge_item run on the host and, compiled by hipcc, in merge_regions_kernel: one
// definition of the arithmetic, checked on the CPU (tests/cpp/async_merge_check.cpp).
constexpr int kMergeMaxRegions = 32;  // regions of one merge launch (the table is a kernel argument)

// One region of the merged frame; src is the mapper's region frame.
struct MergeRegion {
    const uint8_t* src;
    int w, h;
    uint32_t y_off;  // byte offsets in the merged frame: the region's first Y byte,
    uint32_t u_off;  // planar: its first U byte; NV12: the first byte of its first chroma row
    uint32_t v_off;  // planar: its first V byte; NV12: unused (= u_off)
    uint32_t first;  // index of the region's first work item
};
struct MergeTable {
    uint32_t pitch;  // of the merged frame
    int n, nv12;
    uint32_t items;  // work items of all regions
    MergeRegion r[kMergeMaxRegions];
};

// Work items of a region (frame_layout.hpp row_chunk's), in order: h luma rows of row_items(w); then per chroma
// row, NV12: row_items(w), planar: the U half's row_items(w / 2), then the V half's.
OCTVR_LAYOUT_HD inline uint64_t merge_region_items(int w, int h, int nv12) {
    const uint64_t luma = (uint64_t)h * row_items(w);
    const uint64_t chroma = nv12 ? (uint64_t)(h / 2) * row_items(w) : (uint64_t)(h / 2) * 2 * row_items(w / 2);
    return luma + chroma;
}

// The table for regions r (their rectangles in the Y plane) and c (in the U / V planes; c.w = r.w / 2 and
// c.h = r.h / 2, octvr_async_create) of an out_w x out_h merged frame "Y over [U|V]" or NV12 at `pitch`.
// false: more than kMergeMaxRegions regions, a rectangle outside the frame, or a frame of 2 GiB or more.
inline bool build_merge_table(const PlaneRect* r, const PlaneRect* c, const uint8_t* const* src, int n, int out_w, int out_h,
                              size_t pitch, int nv12, MergeTable& t) {
    if (n <= 0 || n > kMergeMaxRegions || out_w <= 0 || out_h <= 0 || pitch < (size_t)out_w) return false;
    if ((uint64_t)pitch * (uint64_t)(out_h + out_h / 2) >= 0x7FFFFF80ull) return false;
    t.pitch = (uint32_t)pitch;
    t.n = n;
    t.nv12 = nv12 ? 1 : 0;
    uint64_t items = 0;
    for (int k = 0; k < n; k++) {
        const PlaneRect &a = r[k], &b = c[k];
        if (a.x < 0 || a.y < 0 || a.w <= 0 || a.h <= 0 || (a.w & 1) || (a.h & 1) || a.x + a.w > out_w || a.y + a.h > out_h)
            return false;
        if (b.x < 0 || b.y < 0 || b.w != a.w / 2 || b.h != a.h / 2 || b.x + b.w > out_w / 2 || b.y + b.h > out_h / 2)
            return false;
        // the merged frame's planes: Y at its first byte, below it the U,V plane or U with V at byte out_w / 2
        const size_t origin[3] = {0, (size_t)out_h * pitch, (size_t)out_h * pitch + (size_t)(out_w / 2)};
        const RegionPieces pc = region_pieces(a, b, nv12);
        auto off = [&](const RegionPiece& p) { return (uint32_t)(origin[p.plane] + p.y * pitch + p.x); };
        MergeRegion& m = t.r[k];
        m.src = src[k];
        m.w = a.w;
        m.h = a.h;
        m.y_off = off(pc.p[0]);
        m.u_off = off(pc.p[1]);
        m.v_off = off(pc.p[pc.n - 1]);
        m.first = (uint32_t)items;
        items += merge_region_items(a.w, a.h, t.nv12);
        if (items >= 0x7FFFFFFFull) return false;
    }
    for (int k = n; k < kMergeMaxRegions; k++) t.r[k] = MergeRegion{nullptr, 0, 0, 0, 0, 0, (uint32_t)items};
    t.items = (uint32_t)items;
    return true;
}

// What work item `id` (< t.items) copies: len bytes (0: nothing) from src to byte offset dst of the merged
// frame, whose first byte is at address out_base (only its low four bits matter).  len = 16 only with dst
// 16-byte aligned: the full chunks of a row start at the destination's first boundary.
struct MergeSpan {
    const uint8_t* src;
    size_t dst;
    int len;
};
OCTVR_LAYOUT_HD inline MergeSpan merge_item(const MergeTable& t, uint32_t id, uintptr_t out_base) {
    int k = 0;
    for (int i = 1; i < t.n; i++)
        if (id >= t.r[i].first) k = i;
    const MergeRegion m = t.r[k];
    uint32_t local = id - m.first;
    const uint32_t per_luma = row_items(m.w), luma = (uint32_t)m.h * per_luma;
    const uint8_t* s;
    size_t d;
    int n;
    uint32_t chunk;
    if (local < luma) {
        const uint32_t row = local / per_luma;
        chunk = local - row * per_luma;
        s = m.src + (size_t)row * (size_t)m.w;
        d = (size_t)m.y_off + (size_t)row * t.pitch;
        n = m.w;
    } else if (t.nv12) {
        local -= luma;
        const uint32_t row = local / per_luma;
        chunk = local - row * per_luma;
        s = m.src + ((size_t)m.h + row) * (size_t)m.w;
        d = (size_t)m.u_off + (size_t)row * t.pitch;
        n = m.w;
    } else {
        local -= luma;
        const uint32_t per_half = row_items(m.w / 2);
        const uint32_t half_row = local / per_half;  // 2 * chroma row + (0: U, 1: V)
        chunk = local - half_row * per_half;
        const uint32_t row = half_row >> 1, v = half_row & 1u;
        s = m.src + ((size_t)m.h + row) * (size_t)m.w + (v ? (size_t)(m.w / 2) : 0);
        d = (size_t)(v ? m.v_off : m.u_off) + (size_t)row * t.pitch;
        n = m.w / 2;
    }
    const RowChunk c = row_chunk(out_base + d, n, (int)chunk);
    if (chunk == 0) return MergeSpan{s, d, c.head};
    if (c.b0 >= n) return MergeSpan{s, d, 0};
    return MergeSpan{s + c.b0, d + (size_t)c.b0, c.len(n)};
}

// ---- the merged frame in a converted layout (octvr_async_set_output_format, async_merge_pack.hip) -------------
// With a converted output layout D the mappers write NV12 region frames and one launch of merge_pack_kernel<D>
// writes every region into the merged frame of layout D: frame_layout.hpp's out rule (pack_lane) per region, the
// region a sub-picture of the frame (pack_item_at).

// A region must be a whole sub-picture of the layout: a pixel pair of a packed row, a U,V pair and a chroma row
// cannot be split, so the luma origin is even and the chroma origin is its half (creation's looser rule places
// luma and chroma independently).
inline bool region_is_subpicture(const PlaneRect& r, const PlaneRect& c) {
    return (r.x & 1) == 0 && (r.y & 1) == 0 && c.x == r.x / 2 && c.y == r.y / 2;
}

// The rectangles of region r (its luma rectangle; region_is_subpicture) in the planes of layout d, the converted
// counterpart of region_pieces: `bytes` bytes of `rows` rows at byte column x, row y of host plane `plane` (one
// packed plane; Y and the U,V plane; or Y, U and V), which in the one-piece frame of an out_w x out_h picture (the
// Mapper's layout of d: a device frame, the slots' staging) is byte column fx of row fy.  The download, the
// copy-out, the kernel's table and the CPU check all place a region by it.
struct LayoutRect {
    int plane;
    size_t x, y, bytes, rows;
    size_t fx, fy;
};
struct LayoutRects {
    int n;  // d.planes()
    LayoutRect p[3];  // the luma (packed) rectangle first
};
inline LayoutRects region_rects(const LayoutDesc& d, const PlaneRect& r, int out_w, int out_h) {
    const size_t S = (size_t)d.bytes, x = (size_t)r.x, y = (size_t)r.y, w = (size_t)r.w, h = (size_t)r.h;
    LayoutRects o{d.planes(), {{}, {}, {}}};
    if (d.packed()) {
        o.p[0] = LayoutRect{0, 2 * x, y, 2 * w, h, 2 * x, y};
        return o;
    }
    const size_t cr = (size_t)d.chroma_rows, cy = cr * (y / 2), ch = cr * (h / 2);
    o.p[0] = LayoutRect{0, S * x, y, S * w, h, S * x, y};
    if (!d.halves()) {
        o.p[1] = LayoutRect{1, S * x, cy, S * w, ch, S * x, (size_t)out_h + cy};
    } else {
        o.p[1] = LayoutRect{1, S * x / 2, cy, S * w / 2, ch, S * x / 2, (size_t)out_h + cy};
        o.p[2] = LayoutRect{2, S * x / 2, cy, S * w / 2, ch, S * (size_t)out_w / 2 + S * x / 2, (size_t)out_h + cy};
    }
    return o;
}

// One region of a merge_pack launch; src is the mapper's NV12 region frame (pitch = w).
struct MergePackRegion {
    const uint8_t* src;
    int w, h;
    uint32_t y_off, u_off, v_off;  // PackPlace of the region in the merged frame
    uint32_t first;                // index of the region's first work item
};
struct MergePackTable {
    uint32_t pitch;  // of the merged frame
    int n;
    uint32_t items;
    MergePackRegion r[kMergeMaxRegions];
};

// The table for regions r / c (octvr_async_create's rectangles) of an out_w x out_h merged frame of layout d at
// `pitch`.  false: no converted layout, more than kMergeMaxRegions regions, a rectangle outside the frame, a region
// that is no sub-picture, a pitch below a row, 2^31 - 1 work items or more, or a frame of 2 GiB or more.
inline bool build_merge_pack_table(const LayoutDesc& d, const PlaneRect* r, const PlaneRect* c, const uint8_t* const* src, int n,
                                   int out_w, int out_h, size_t pitch, MergePackTable& t) {
    if (!d.converted() || n <= 0 || n > kMergeMaxRegions || out_w <= 0 || out_h <= 0 || (out_w & 1) || (out_h & 1)) return false;
    if (pitch < (size_t)d.row_bytes(out_w)) return false;
    if ((uint64_t)pitch * (uint64_t)d.rows(out_h) >= 0x7FFFFF80ull) return false;
    t.pitch = (uint32_t)pitch;
    t.n = n;
    uint64_t items = 0;
    for (int k = 0; k < n; k++) {
        const PlaneRect &a = r[k], &b = c[k];
        if (a.x < 0 || a.y < 0 || a.w <= 0 || a.h <= 0 || (a.w & 1) || (a.h & 1) || a.x + a.w > out_w || a.y + a.h > out_h)
            return false;
        if (b.w != a.w / 2 || b.h != a.h / 2 || !region_is_subpicture(a, b)) return false;
        const LayoutRects rc = region_rects(d, a, out_w, out_h);
        auto off = [&](const LayoutRect& p) { return (uint32_t)(p.fy * pitch + p.fx); };
        MergePackRegion& m = t.r[k];
        m.src = src[k];
        m.w = a.w;
        m.h = a.h;
        m.y_off = off(rc.p[0]);
        m.u_off = off(rc.p[rc.n > 1 ? 1 : 0]);
        m.v_off = off(rc.p[rc.n - 1]);
        m.first = (uint32_t)items;
        items += pack_items(d, a.w, a.h);
        if (items >= 0x7FFFFFFFull) return false;
    }
    for (int k = n; k < kMergeMaxRegions; k++) t.r[k] = MergePackRegion{nullptr, 0, 0, 0, 0, 0, (uint32_t)items};
    t.items = (uint32_t)items;
    return true;
}

// What work item `id` (< t.items) writes: the span of pack_item_at for its region, and the region in k; the
// caller's lane is pack_lane(mem, t.r[k].src, out, t.r[k].w, t.r[k].h, span).  The region is found as merge_item
// finds it, by the regions' first items.
OCTVR_LAYOUT_HD inline LayoutSpan merge_pack_item(const LayoutDesc& d, const MergePackTable& t, uint32_t id, uintptr_t out_base,
                                                  int& k) {
    k = 0;
    for (int i = 1; i < t.n; i++)
        if (id >= t.r[i].first) k = i;
    const MergePackRegion& m = t.r[k];
    return pack_item_at(d, m.w, m.h, t.pitch, PackPlace{m.y_off, m.u_off, m.v_off}, out_base, id - m.first);
}

}  // namespace octvr
