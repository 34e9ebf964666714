// async_host.hpp — the AsyncMultiMapper pipeline's pure host arithmetic (no HIP, no device): the packing of
// one footprint run from the caller's planes (async.cpp copy_in; debug_abi.cpp octvr_debug_pack_runs) and the
// merge of the output planes' byte ranges before they are page-locked (octvr_async_register_output).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace octvr {

// Bytes of the luma part of one row of a run: groups [g0, g0 + ng) of 8 pixels, cut at the width.
inline int run_luma_bytes(int w, int g0, int ng) { return std::min(8 * (g0 + ng), w) - 8 * g0; }

// Packs the run (row pair rp, groups [g0, g0 + ng)) of a w-wide camera at d: luma row 2 rp, luma row
// 2 rp + 1 (yb bytes each), then its chroma row — planar (nv12 == 0): cb bytes of U and cb of V, from
// planes[1] / planes[2] at byte 4 g0; NV12: the yb bytes at byte 8 g0 of the U,V plane planes[1] (planes[2]
// is not read).  w is even, so yb = 2 cb and both layouts pack 3 yb bytes.  Returns that size.
inline size_t pack_run(uint8_t* d, int w, int rp, int g0, int ng, const uint8_t* const* planes, const size_t* pitches,
                       int nv12) {
    const int x0 = 8 * g0, yb = run_luma_bytes(w, g0, ng);
    memcpy(d, planes[0] + (size_t)(2 * rp) * pitches[0] + x0, (size_t)yb);
    memcpy(d + yb, planes[0] + (size_t)(2 * rp + 1) * pitches[0] + x0, (size_t)yb);
    if (nv12) {
        memcpy(d + 2 * yb, planes[1] + (size_t)rp * pitches[1] + x0, (size_t)yb);
        return (size_t)(3 * yb);
    }
    const int c0 = 4 * g0, cb = std::max(0, std::min(4 * (g0 + ng), w / 2) - c0);
    memcpy(d + 2 * yb, planes[1] + (size_t)rp * pitches[1] + c0, (size_t)cb);
    memcpy(d + 2 * yb + cb, planes[2] + (size_t)rp * pitches[2] + c0, (size_t)cb);
    return (size_t)(2 * yb + 2 * cb);
}

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

}  // namespace octvr
