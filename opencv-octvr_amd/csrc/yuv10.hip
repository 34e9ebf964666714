// yuv10.hip — the 10-bit capture layouts, in and out (OCTVR_PIX_P010, OCTVR_PIX_YUV420P10, OCTVR_PIX_P210,
// OCTVR_PIX_YUV422P10): yuv10_unpack_kernel<L> narrows the footprint of input frames of layout L into the 8-bit
// NV12 frames the stitch kernels read, yuv10_pack_kernel<L> widens a stitched NV12 frame into the caller's frame.
// A translation unit of its own, like uyvy.hip and yuv422.hip: no existing code object moves.  The lane bodies
// are yuv10_host.hpp's templates, the functions the CPU check runs; this file supplies the memory accesses.
//
// yuv10_unpack_kernel: the geometry of yuv422_unpack_kernel (sixteen lanes per table piece, sixteen pieces per
//   workgroup, one lane per 8-pixel group of the row pair, a longer piece in rounds of sixteen).  Per group two
//   16-byte luma loads and
//     P010       one 16-byte chroma load;
//     YUV420P10  8 bytes of U and 8 of V;
//     P210       two 16-byte chroma loads, narrowed, then averaged four bytes at a time;
//     YUV422P10  8 bytes of U and 8 of V from each of the two chroma rows, narrowed and zipped, then averaged;
//   a dword's two samples are narrowed by one packed 16-bit add with clamp (a left shift before it for the
//   layouts with the sample in bits 9..0) and gathered by the byte permute that also zips U with V; then two
//   8-byte luma stores and one 8-byte chroma store into the NV12 frame.  Global loads need no alignment on
//   gfx950, so any even base and pitch (the host refuses odd ones: a sample's natural alignment).
//   Cache policy, as uyvy.hip argues: the caller's frame is read once (non-temporal loads), the NV12 frame is
//   read by the gain feed and the composite right after (plain stores).
//   Per-sample path: the short last group of a width that is no multiple of 8, and every group of an NV12
//   frame whose rows are not 8-byte aligned.
//   Bounds: a run has row pair rp < h / 2 and groups inside the row (checked where the runs are built),
//   yuv10_unpack_item yields px <= 0 for anything else; a group's loads are its own 2 px bytes of its rows
//   (inside the row's 2 w bytes <= pitch, inside the frame's 3 h / 2 or 2 h rows; a planar V part ends at byte
//   2 w), its stores px bytes inside the NV12 frame's rows.
// yuv10_pack_kernel: a work item is a 16-byte chunk of one destination row (for the planar layouts' chroma: of
//   the U or the V half of a row) counted from that row's first 16-byte boundary (yuv10_pack_item), so every
//   full chunk is one aligned 16-byte store of 8 words whatever the base and pitch: 8 bytes of a luma or U,V
//   row, or the even or odd bytes of 16 bytes of the NV12 chroma row, each placed in its word by one permute
//   with zero bytes.  Each chroma row of a 4:2:2 layout is read for two destination rows (the second from L2).
//   Heads and tails are words.  Plain loads and stores, as uyvy_pack_kernel's.
#include "kernels.hpp"
#include "yuv10_host.hpp"

namespace octvr {

namespace {

typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct UnpackMem {  // the caller's frame, read once
    __device__ __forceinline__ Yuv10Pair load8(const uint8_t* p) const {
        const u32x2_u v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_u*>(p));
        return Yuv10Pair{v.x, v.y};
    }
    __device__ __forceinline__ UyvyWords load16(const uint8_t* p) const {
        const u32x4_u v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(p));
        return UyvyWords{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void store8(uint8_t* p, const Yuv10Pair& v) const {
        *reinterpret_cast<u32x2*>(p) = u32x2{v.x, v.y};
    }
};

struct PackMem {  // the NV12 frame the kernel before wrote
    __device__ __forceinline__ Yuv10Pair load8(const uint8_t* p) const {
        const u32x2_u v = *reinterpret_cast<const u32x2_u*>(p);
        return Yuv10Pair{v.x, v.y};
    }
    __device__ __forceinline__ UyvyWords load16(const uint8_t* p) const {
        const u32x4_u v = *reinterpret_cast<const u32x4_u*>(p);
        return UyvyWords{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void store16(uint8_t* p, const UyvyWords& v) const {
        *reinterpret_cast<u32x4*>(p) = u32x4{v.x, v.y, v.z, v.w};
    }
};

constexpr uint32_t kUnpackLanes = 16;  // lanes of one table piece

}  // namespace

template <int L>
__global__ void __launch_bounds__(256) yuv10_unpack_kernel(const UyvyRun* __restrict__ table, int n_pieces, UyvySources src,
                                                           FootFrames fr) {
    const int piece = (int)(blockIdx.x * (256u / kUnpackLanes) + threadIdx.x / kUnpackLanes);
    if (piece >= n_pieces) return;
    const UyvyRun r = table[piece];
    const int cam = (int)(r.cam & 31u);
    const int w = fr.w[cam], h = fr.h[cam];
    const uint8_t* const s = src.packed ? src.packed : src.f[cam];
    const size_t pitch = src.packed ? 0 : src.pitch[cam];
    uint8_t* const d = fr.f[cam];
    for (int k = (int)(threadIdx.x % kUnpackLanes); k < (int)r.ng; k += (int)kUnpackLanes)
        yuv10_unpack_lane<L>(UnpackMem{}, s, d, w, yuv10_unpack_item(L, w, h, pitch, r, k));
}

template <int L>
__global__ void __launch_bounds__(256) yuv10_pack_kernel(const uint8_t* __restrict__ src, int w, int h,
                                                         uint8_t* __restrict__ out, size_t pitch, uint32_t items) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= items) return;
    yuv10_pack_lane<L>(PackMem{}, src, out, w, h, yuv10_pack_item(L, w, h, pitch, reinterpret_cast<uintptr_t>(out), id));
}

hipError_t launch_yuv10_unpack(int layout, const UyvyRun* table, int n_pieces, const UyvySources& src,
                               const FootFrames& frames, hipStream_t s) {
    if (layout < kYuv10P010 || layout > kYuv10Planar422) return hipErrorInvalidValue;
    if (n_pieces <= 0) return hipSuccess;
    constexpr unsigned per_block = 256u / kUnpackLanes;
    const dim3 grid(((unsigned)n_pieces + per_block - 1u) / per_block);
    if (layout == kYuv10P010)
        hipLaunchKernelGGL(yuv10_unpack_kernel<kYuv10P010>, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    else if (layout == kYuv10Planar420)
        hipLaunchKernelGGL(yuv10_unpack_kernel<kYuv10Planar420>, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    else if (layout == kYuv10P210)
        hipLaunchKernelGGL(yuv10_unpack_kernel<kYuv10P210>, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    else
        hipLaunchKernelGGL(yuv10_unpack_kernel<kYuv10Planar422>, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    return hipGetLastError();
}

hipError_t launch_yuv10_pack(int layout, const uint8_t* src, int w, int h, uint8_t* out, size_t pitch, hipStream_t s) {
    if (layout < kYuv10P010 || layout > kYuv10Planar422) return hipErrorInvalidValue;
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || pitch < (size_t)yuv10_frame_row_bytes(w)) return hipErrorInvalidValue;
    if ((pitch & 1) || (reinterpret_cast<uintptr_t>(out) & 1)) return hipErrorInvalidValue;  // heads and tails are words
    const uint64_t items = yuv10_pack_items(layout, w, h);
    if (items >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((items + 255u) / 256u));
    if (layout == kYuv10P010)
        hipLaunchKernelGGL(yuv10_pack_kernel<kYuv10P010>, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    else if (layout == kYuv10Planar420)
        hipLaunchKernelGGL(yuv10_pack_kernel<kYuv10Planar420>, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    else if (layout == kYuv10P210)
        hipLaunchKernelGGL(yuv10_pack_kernel<kYuv10P210>, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    else
        hipLaunchKernelGGL(yuv10_pack_kernel<kYuv10Planar422>, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    return hipGetLastError();
}

}  // namespace octvr
