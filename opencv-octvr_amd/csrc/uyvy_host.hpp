// uyvy_host.hpp — the arithmetic of the packed UYVY 4:2:2 conversions (OCTVR_PIX_UYVY422): which bytes a work
// item of uyvy_unpack_kernel / uyvy_pack_kernel (uyvy.hip) loads and which it stores, the packing of a footprint
// run of a UYVY plane (async.cpp copy_in) and the split of footprint runs into the unpack kernel's table.  No
// HIP types: the functions run on the host and, compiled by hipcc, in the kernels — one definition, executed
// on the CPU against exactly sized heap blocks by tests/cpp/uyvy_runs_check.cpp.
//
// A UYVY frame of a w x h picture (w, h even) is h rows of 2 w bytes, U0 Y0 V0 Y1 per pixel pair: byte b of a
// row is luma Y[b >> 1] when b is odd and, when b is even, byte b >> 1 of the row's chroma as U,V pairs.  The
// 4:2:0 side of both conversions is NV12 at pitch = width ("Y over U,V pairs": h rows of Y, h / 2 rows of U,V
// pairs), so the 8-pixel group g of row pair r — packed bytes [16 g, 16 g + 16) of rows 2r and 2r + 1 — is luma
// bytes [8 g, 8 g + 8) of rows 2r, 2r + 1 and chroma bytes [8 g, 8 g + 8) of row h + r: the footprint's cell.
//   in  (4:2:2 -> 4:2:0): chroma row r = (c[2r] + c[2r + 1] + 1) >> 1 per byte; luma copied
//   out (4:2:0 -> 4:2:2): packed rows 2r and 2r + 1 both carry chroma row r; luma copied
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define OCTVR_UYVY_HD __host__ __device__
#else
#define OCTVR_UYVY_HD
#endif

namespace octvr {

// ---- bytes ----------------------------------------------------------------------------------------------
// v_perm_b32: byte k of the result is byte sel[k] of the eight bytes {hi, lo} (0-3: lo, 4-7: hi)
OCTVR_UYVY_HD inline uint32_t uyvy_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = (uint64_t)hi << 32 | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) r |= (uint32_t)((both >> (8 * ((sel >> (8 * k)) & 7u))) & 0xFFu) << (8 * k);
    return r;
#endif
}
constexpr uint32_t kUyvySelLuma = 0x07050301u;    // U Y V Y, U Y V Y -> Y Y Y Y
constexpr uint32_t kUyvySelChroma = 0x06040200u;  //                  -> U V U V
constexpr uint32_t kUyvySelZipLo = 0x05010400u;   // a0 a1 a2 a3, b0 b1 b2 b3 (lo = a, hi = b) -> a0 b0 a1 b1
constexpr uint32_t kUyvySelZipHi = 0x07030602u;   //                                            -> a2 b2 a3 b3

// (a + b + 1) >> 1 of each of the four bytes: a + b = 2 (a | b) - (a ^ b), so the rounded-up half is
// (a | b) - ((a ^ b) >> 1); the shift's bits that crossed a byte boundary are masked off, and no byte borrows
// ((a ^ b) >> 1 <= a | b per byte).
OCTVR_UYVY_HD inline uint32_t uyvy_avg4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) >> 1) & 0x7F7F7F7Fu); }

struct UyvyWords {
    uint32_t x, y, z, w;
};
struct UyvyGroupOut {
    uint32_t y0[2], y1[2], c[2];  // 8 luma bytes of each row, 8 chroma bytes (U,V pairs)
};
// One full group: the 16 packed bytes of its two rows -> its 4:2:0 bytes.
OCTVR_UYVY_HD inline UyvyGroupOut uyvy_split_group(const UyvyWords& a, const UyvyWords& b) {
    UyvyGroupOut o;
    o.y0[0] = uyvy_perm(a.y, a.x, kUyvySelLuma);
    o.y0[1] = uyvy_perm(a.w, a.z, kUyvySelLuma);
    o.y1[0] = uyvy_perm(b.y, b.x, kUyvySelLuma);
    o.y1[1] = uyvy_perm(b.w, b.z, kUyvySelLuma);
    o.c[0] = uyvy_avg4(uyvy_perm(a.y, a.x, kUyvySelChroma), uyvy_perm(b.y, b.x, kUyvySelChroma));
    o.c[1] = uyvy_avg4(uyvy_perm(a.w, a.z, kUyvySelChroma), uyvy_perm(b.w, b.z, kUyvySelChroma));
    return o;
}

// ---- in: the unpack kernel's table and work items ------------------------------------------------------------
// A run is ng consecutive 8-pixel groups from group g0 of row pair rp of camera cam (kernels.hpp FootRun, the
// same four words).  The source is either the caller's frame (src_pitch >= 2 w: rows 2 rp and 2 rp + 1 at byte
// 16 g0) or the pipeline's packed upload buffer (src_pitch == 0: at byte `off`, the run's bytes of row 2 rp,
// then those of row 2 rp + 1, uyvy_pack_run).
struct UyvyRun {
    uint32_t cam;  // camera | row pair << 8
    uint32_t g0, ng;
    uint32_t off;
};

// Luma bytes of one row of the run: its groups cut at the width (async_host.hpp run_luma_bytes).
OCTVR_UYVY_HD inline int uyvy_run_px(int w, int g0, int ng) { return (8 * (g0 + ng) < w ? 8 * (g0 + ng) : w) - 8 * g0; }

// What the lane of group k (< r.ng) of run r does for a w x h camera: it reads 2 px bytes at s0 and at s1 of
// the source and writes px bytes at y0, at y1 and at c of the camera's 4:2:0 frame (NV12, pitch = w).
// px = 8, or 2, 4 or 6 in the short last group of a width that is no multiple of 8; px <= 0: nothing (no such
// group is built).
struct UyvyItem {
    int px;
    size_t s0, s1;
    size_t y0, y1, c;
};
OCTVR_UYVY_HD inline UyvyItem uyvy_unpack_item(int w, int h, size_t src_pitch, const UyvyRun& r, int k) {
    const int rp = (int)(r.cam >> 8), g = (int)r.g0 + k;
    UyvyItem it;
    const int left = w - 8 * g;
    it.px = (k < 0 || k >= (int)r.ng || 2 * rp + 1 >= h) ? 0 : left < 8 ? left : 8;
    if (src_pitch) {
        it.s0 = (size_t)(2 * rp) * src_pitch + (size_t)16 * (size_t)g;
        it.s1 = it.s0 + src_pitch;
    } else {
        it.s0 = (size_t)r.off + (size_t)16 * (size_t)k;
        it.s1 = it.s0 + (size_t)2 * (size_t)uyvy_run_px(w, (int)r.g0, (int)r.ng);
    }
    it.y0 = (size_t)(2 * rp) * (size_t)w + (size_t)8 * (size_t)g;
    it.y1 = it.y0 + (size_t)w;
    it.c = (size_t)(h + rp) * (size_t)w + (size_t)8 * (size_t)g;
    return it;
}

// The item's byte path (the short last group; a frame whose rows are not 8-byte aligned): pixel pair by pair.
OCTVR_UYVY_HD inline void uyvy_unpack_bytes(const uint8_t* src, uint8_t* dst, const UyvyItem& it) {
    for (int p = 0; p < it.px; p += 2) {
        const uint8_t* a = src + it.s0 + 2 * p;
        const uint8_t* b = src + it.s1 + 2 * p;
        dst[it.y0 + p] = a[1];
        dst[it.y0 + p + 1] = a[3];
        dst[it.y1 + p] = b[1];
        dst[it.y1 + p + 1] = b[3];
        dst[it.c + p] = (uint8_t)((a[0] + b[0] + 1) >> 1);
        dst[it.c + p + 1] = (uint8_t)((a[2] + b[2] + 1) >> 1);
    }
}

// True when the item takes the vector path: a full group whose three stores are 8-byte aligned (the frame's
// rows are when w is a multiple of 8 and its base is 8-byte aligned; the loads need no alignment).
OCTVR_UYVY_HD inline bool uyvy_unpack_vector(int w, uintptr_t dst_base, const UyvyItem& it) {
    return it.px == 8 && (w & 7) == 0 && (dst_base & 7u) == 0;
}

// Packs the run (row pair rp, groups [g0, g0 + ng)) of a w-wide UYVY plane at d: its 2 px bytes of row 2 rp,
// then those of row 2 rp + 1 (4 px bytes, against 3 px for a 4:2:0 plane).  Returns that size.
inline size_t uyvy_pack_run(uint8_t* d, int w, int rp, int g0, int ng, const uint8_t* plane, size_t pitch) {
    const size_t n = (size_t)2 * (size_t)uyvy_run_px(w, g0, ng);
    memcpy(d, plane + (size_t)(2 * rp) * pitch + (size_t)16 * (size_t)g0, n);
    memcpy(d + n, plane + (size_t)(2 * rp + 1) * pitch + (size_t)16 * (size_t)g0, n);
    return 2 * n;
}

// The unpack kernel's table of a set of footprint runs: each run cut into pieces of at most kUyvyWave groups
// (a group of lanes takes one piece, a lane a group), each piece's `off` its place in the packed upload buffer
// (pieces back to back, uyvy_pack_run's layout each).  bytes: the packed size, which is also the packed
// bytes a frame's unpack reads.
constexpr int kUyvyWave = 64;
template <class Run>
inline std::vector<UyvyRun> uyvy_run_table(const std::vector<Run>& runs, const std::vector<int>& in_w, size_t& bytes) {
    std::vector<UyvyRun> t;
    bytes = 0;
    for (const Run& r : runs) {
        const int w = in_w[r.cam & 31u];
        for (uint32_t k = 0; k < r.ng; k += kUyvyWave) {
            const uint32_t ng = r.ng - k < (uint32_t)kUyvyWave ? r.ng - k : (uint32_t)kUyvyWave;
            t.push_back(UyvyRun{r.cam, r.g0 + k, ng, (uint32_t)bytes});
            bytes += (size_t)4 * (size_t)uyvy_run_px(w, (int)(r.g0 + k), (int)ng);
        }
    }
    return t;
}

// ---- out: the pack kernel's work items -----------------------------------------------------------------------
// A work item is (packed row, 16-byte chunk of the row counted from the destination's first 16-byte boundary),
// as the device-frame merge's (async_host.hpp merge_item): item 0 of a row is the bytes before the boundary
// (at most 15, possibly none), then whole chunks, the last one possibly short.
constexpr int kUyvyChunk = 16;
OCTVR_UYVY_HD inline uint32_t uyvy_pack_row_items(int w) { return (uint32_t)((2 * w + kUyvyChunk - 1) / kUyvyChunk + 1); }

// What item `id` of a w x h frame writes: len bytes (0: nothing) at byte b0 of packed row `row`, at dst of the
// caller's frame (first byte at address out_base, pitch >= 2 w).  Packed byte b of the row is the 4:2:0 frame's
// luma byte (row, b >> 1) when b is odd, else its chroma byte (h + row / 2, b >> 1).  len = 16 only with dst
// 16-byte aligned.
struct UyvySpan {
    int row, b0, len;
    size_t dst;
};
OCTVR_UYVY_HD inline UyvySpan uyvy_pack_item(int w, int h, size_t pitch, uintptr_t out_base, uint32_t id) {
    const uint32_t per = uyvy_pack_row_items(w);
    const int row = (int)(id / per), chunk = (int)(id - (uint32_t)row * per), n = 2 * w;
    UyvySpan sp{row, 0, 0, (size_t)row * pitch};
    if (row >= h) return sp;
    const int head = (int)((0 - (out_base + sp.dst)) & (uintptr_t)(kUyvyChunk - 1));
    const int hd = head < n ? head : n;
    if (chunk == 0) {
        sp.len = hd;
        return sp;
    }
    const int b0 = hd + kUyvyChunk * (chunk - 1);
    if (b0 >= n) return sp;
    sp.b0 = b0;
    sp.len = n - b0 < kUyvyChunk ? n - b0 : kUyvyChunk;
    sp.dst += (size_t)b0;
    return sp;
}

// The span's bytes one by one (heads and tails), from the NV12 frame `src` at pitch = w.
OCTVR_UYVY_HD inline void uyvy_pack_bytes(const uint8_t* src, uint8_t* out, int w, int h, const UyvySpan& sp) {
    const uint8_t* const y = src + (size_t)sp.row * (size_t)w;
    const uint8_t* const c = src + (size_t)(h + (sp.row >> 1)) * (size_t)w;
    for (int i = 0; i < sp.len; i++) {
        const int b = sp.b0 + i;
        out[sp.dst + i] = ((b & 1) ? y : c)[b >> 1];
    }
}

// A full chunk: packed bytes [b0, b0 + 16) alternate between two 8-byte runs of the source rows — the first
// (the chroma row when b0 is even, else the luma row) from byte b0 >> 1, the second (the other row) from byte
// (b0 + 1) >> 1.  first / second: the byte offsets of those runs in the NV12 frame.
struct UyvyChunkSrc {
    size_t first, second;
};
OCTVR_UYVY_HD inline UyvyChunkSrc uyvy_pack_chunk_src(int w, int h, const UyvySpan& sp) {
    const size_t y = (size_t)sp.row * (size_t)w, c = (size_t)(h + (sp.row >> 1)) * (size_t)w;
    const bool odd = (sp.b0 & 1) != 0;
    return UyvyChunkSrc{(odd ? y : c) + (size_t)(sp.b0 >> 1), (odd ? c : y) + (size_t)((sp.b0 + 1) >> 1)};
}
OCTVR_UYVY_HD inline UyvyWords uyvy_zip(uint32_t f0, uint32_t f1, uint32_t s0, uint32_t s1) {
    return UyvyWords{uyvy_perm(s0, f0, kUyvySelZipLo), uyvy_perm(s0, f0, kUyvySelZipHi),
                     uyvy_perm(s1, f1, kUyvySelZipLo), uyvy_perm(s1, f1, kUyvySelZipHi)};
}

}  // namespace octvr
