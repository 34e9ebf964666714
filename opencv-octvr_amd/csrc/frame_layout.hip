// frame_layout.hip — the converted capture layouts, in and out (OCTVR_PIX_UYVY422, _YUYV422, _YUV422P, _NV16, _P010,
// _YUV420P10, _P210, _YUV422P10): layout_unpack_kernel<L> converts the footprint of input frames of layout L into
// the 8-bit NV12 frames the stitch kernels read, layout_pack_kernel<L> a stitched NV12 frame into the caller's
// frame.  A translation unit of its own, like overlay.hip and the device-frame merge.  The lane bodies are
// frame_layout.hpp's templates, the functions the CPU check runs; this file supplies the memory accesses.
//
// layout_unpack_kernel: sixteen lanes per table piece (at most 64 groups of one run, run_table; a footprint's
//   runs are short, 4.7 groups on the C2 rig, so a whole wave per piece would idle most lanes), sixteen pieces
//   per workgroup, one lane per 8-pixel group of the row pair (a longer piece in rounds of sixteen).  Per group
//     packed (UYVY, YUYV)   two 16-byte loads (one per packed row), byte permutes split luma from chroma, the two
//                chroma rows are averaged four bytes at a time (avg4);
//     NV16       two 8-byte luma loads, two 8-byte chroma loads averaged four bytes at a time;
//     YUV422P    two 8-byte luma loads, 4 bytes of U and 4 of V from each of the two chroma rows, averaged, then
//                zipped into U,V pairs by two permutes;
//     P010 / P210        two 16-byte luma loads, one or two 16-byte chroma loads, narrowed (then averaged);
//     YUV420P10 / YUV422P10   two 16-byte luma loads, 8 bytes of U and 8 of V from each chroma row, narrowed and
//                zipped (then averaged);
//   a dword's two 10-bit samples are narrowed by one packed 16-bit add with clamp (a left shift before it for the
//   layouts with the sample in bits 9..0) and gathered by the byte permute that also zips U with V; then two
//   8-byte luma stores and one 8-byte chroma store into the NV12 frame.  Global loads need no alignment on gfx950,
//   so any base and pitch (for 16-bit samples the host refuses odd ones: a sample's natural alignment).  For the
//   planar layouts the luma is copied although it is already planar: the composite takes one pointer per camera
//   with the chroma below the luma.
//   Cache policy: the caller's frame (or the packed upload) is read once and never again: non-temporal loads, it
//   should not displace what the composite is about to read.  The NV12 destination is read by the gain feed and
//   the composite right after: plain stores, which keep the lines in L2 and the Infinity Cache.
//   Sample path: the short last group of a width that is no multiple of 8, and every group of an NV12 frame
//   whose rows are not 8-byte aligned (w % 8 != 0): unpack_samples.
//   Bounds: a run has row pair rp < h / 2 and groups inside the row (checked where the runs are built: async.cpp
//   footprint_runs), unpack_item yields px <= 0 for anything else; a group's loads are its own samples of its
//   rows (inside the row's bytes <= pitch, inside the frame's rows; a V part ends at the row's width), its stores
//   px bytes inside the NV12 frame's rows.
// layout_pack_kernel: a work item is a 16-byte chunk of one destination row (for the halves kind's chroma: of the
//   U or the V half of a row) counted from that row's first 16-byte boundary (pack_item), so every full chunk is
//   one aligned 16-byte store whatever the base and pitch.  A packed row zips 8 luma and 8 chroma bytes (two
//   8-byte loads, unaligned in general, two permutes per word); 8-bit luma rows and NV16's chroma rows are 16-byte
//   copies; a YUV422P half row takes the even or odd bytes of 32 bytes of the NV12 chroma row; a row of words
//   takes 8 bytes of the NV12 row, or the even or odd bytes of 16, each placed in its word by one permute with
//   zero bytes.  With two chroma rows per row pair each NV12 chroma row is read for two destination rows (the
//   second from L2).  Heads and tails are samples.  Plain loads (the frame was written by the kernel just before)
//   and plain stores (the caller's next kernel or copy reads the frame).
// v210_unpack_kernel / v210_pack_kernel (OCTVR_PIX_V210; lane bodies: v210_layout.hpp): the same table, lanes, cache
//   policy and bounds.  A lane of the unpack takes two 16-byte loads per packed row (the group's two blocks, at any
//   alignment), narrows each word's three fields where they stand (clamped before they can touch: v10 + 2 carries
//   out of ten bits), gathers a block's twelve bytes by three permutes, which are UYVY bytes, picks the group's
//   sixteen by its phase (whole dwords: selects, no divergence), then UYVY's permutes and avg4 and the same three
//   8-byte stores.  A full group's second block always holds pixels of the group, so no load leaves the row's blocks
//   that hold pixels; the short last group goes word by word.  A work item of the pack is one 16-byte block of a
//   destination row: 8 luma and 8 chroma bytes from the same byte offset of their NV12 rows (the last two blocks
//   with pixels byte by byte), zipped, widened into four words, one 16-byte store, or four dword stores where the
//   caller's base or pitch puts the block off a 16-byte boundary; the padding blocks are zero stores.
#include "frame_layout.hpp"
#include "v210_layout.hpp"
#include "kernels.hpp"
#include "octvr_hip.h"

namespace octvr {

static_assert(OCTVR_PIX_UYVY422 == 16 && OCTVR_PIX_YUYV422 == 17 && OCTVR_PIX_YUV422P == 18 && OCTVR_PIX_NV16 == 19 &&
                  OCTVR_PIX_P010 == 32 && OCTVR_PIX_YUV420P10 == 33 && OCTVR_PIX_P210 == 34 && OCTVR_PIX_YUV422P10 == 35,
              "with_layout's cases are the OCTVR_PIX_* values");
static_assert(OCTVR_PIX_V210 == 48, "layout_of's v210 case is the OCTVR_PIX_* value");

namespace {

typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct UnpackMem {  // the caller's frame, read once
    __device__ __forceinline__ uint32_t load4(const uint8_t* p) const {
        return __builtin_nontemporal_load(reinterpret_cast<const u32_u*>(p));
    }
    __device__ __forceinline__ Words2 load8(const uint8_t* p) const {
        const u32x2_u v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_u*>(p));
        return Words2{v.x, v.y};
    }
    __device__ __forceinline__ Words4 load16(const uint8_t* p) const {
        const u32x4_u v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(p));
        return Words4{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void store8(uint8_t* p, const Words2& v) const { *reinterpret_cast<u32x2*>(p) = u32x2{v.x, v.y}; }
};

struct PackMem {  // the NV12 frame the kernel before wrote
    __device__ __forceinline__ Words2 load8(const uint8_t* p) const {
        const u32x2_u v = *reinterpret_cast<const u32x2_u*>(p);
        return Words2{v.x, v.y};
    }
    __device__ __forceinline__ Words4 load16(const uint8_t* p) const {
        const u32x4_u v = *reinterpret_cast<const u32x4_u*>(p);
        return Words4{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void store16(uint8_t* p, const Words4& v) const {
        *reinterpret_cast<u32x4*>(p) = u32x4{v.x, v.y, v.z, v.w};
    }
    // the compiler barrier keeps four neighbouring dword stores four (they would otherwise be merged into one 16-byte
    // store at a 4-byte aligned address)
    __device__ __forceinline__ void store4(uint8_t* p, uint32_t v) const {
        *reinterpret_cast<uint32_t*>(p) = v;
        asm volatile("" ::: "memory");
    }
};

constexpr uint32_t kUnpackLanes = 16;  // lanes of one table piece

}  // namespace

template <class L>
__global__ void __launch_bounds__(256) layout_unpack_kernel(const FootRun* __restrict__ table, int n_pieces, ConvSources src,
                                                            FootFrames fr) {
    constexpr LayoutDesc d = L::desc;
    const int piece = (int)(blockIdx.x * (256u / kUnpackLanes) + threadIdx.x / kUnpackLanes);
    if (piece >= n_pieces) return;
    const FootRun r = table[piece];
    const int cam = (int)(r.cam & 31u);
    const int w = fr.w[cam], h = fr.h[cam];
    const uint8_t* const s = src.packed ? src.packed : src.f[cam];
    const size_t pitch = src.packed ? 0 : src.pitch[cam];
    uint8_t* const dst = fr.f[cam];
    for (int k = (int)(threadIdx.x % kUnpackLanes); k < (int)r.ng; k += (int)kUnpackLanes)
        unpack_lane<L>(UnpackMem{}, s, dst, w, unpack_item(d, w, h, pitch, r, k));
}

template <class L>
__global__ void __launch_bounds__(256) layout_pack_kernel(const uint8_t* __restrict__ src, int w, int h,
                                                          uint8_t* __restrict__ out, size_t pitch, uint32_t items) {
    constexpr LayoutDesc d = L::desc;
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= items) return;
    pack_lane<L>(PackMem{}, src, out, w, h, pack_item(d, w, h, pitch, reinterpret_cast<uintptr_t>(out), id));
}

__global__ void __launch_bounds__(256) v210_unpack_kernel(const FootRun* __restrict__ table, int n_pieces, ConvSources src,
                                                          FootFrames fr) {
    const int piece = (int)(blockIdx.x * (256u / kUnpackLanes) + threadIdx.x / kUnpackLanes);
    if (piece >= n_pieces) return;
    const FootRun r = table[piece];
    const int cam = (int)(r.cam & 31u);
    const int w = fr.w[cam], h = fr.h[cam];
    const uint8_t* const s = src.packed ? src.packed : src.f[cam];
    const size_t pitch = src.packed ? 0 : src.pitch[cam];
    uint8_t* const dst = fr.f[cam];
    for (int k = (int)(threadIdx.x % kUnpackLanes); k < (int)r.ng; k += (int)kUnpackLanes)
        v210_unpack_lane(UnpackMem{}, s, dst, w, v210_unpack_item(w, h, pitch, r, k));
}

__global__ void __launch_bounds__(256) v210_pack_kernel(const uint8_t* __restrict__ src, int w, int h, uint8_t* __restrict__ out,
                                                        size_t pitch, uint32_t items) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= items) return;
    v210_pack_lane(PackMem{}, src, out, v210_pack_item(w, h, pitch, id));
}

hipError_t launch_layout_unpack(int pix, const FootRun* table, int n_pieces, const ConvSources& src, const FootFrames& frames,
                                hipStream_t s) {
    if (!converted_format(pix)) return hipErrorInvalidValue;
    if (n_pieces <= 0) return hipSuccess;
    constexpr unsigned per_block = 256u / kUnpackLanes;
    const dim3 grid(((unsigned)n_pieces + per_block - 1u) / per_block);
    if (pix == OCTVR_PIX_V210) hipLaunchKernelGGL(v210_unpack_kernel, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    with_layout(pix, [&](auto tag) {
        hipLaunchKernelGGL(layout_unpack_kernel<decltype(tag)>, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    });
    return hipGetLastError();
}

hipError_t launch_layout_pack(int pix, const uint8_t* src, int w, int h, uint8_t* out, size_t pitch, hipStream_t s) {
    const LayoutDesc d = layout_of(pix);
    if (!d.converted()) return hipErrorInvalidValue;
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || pitch < (size_t)d.row_bytes(w)) return hipErrorInvalidValue;
    if (!d.aligned(out, pitch)) return hipErrorInvalidValue;  // heads and tails are samples
    const uint64_t items = d.v210() ? v210_pack_items(w, h) : pack_items(d, w, h);
    if (items >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((items + 255u) / 256u));
    if (d.v210()) hipLaunchKernelGGL(v210_pack_kernel, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    with_layout(pix, [&](auto tag) {
        hipLaunchKernelGGL(layout_pack_kernel<decltype(tag)>, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    });
    return hipGetLastError();
}

}  // namespace octvr
