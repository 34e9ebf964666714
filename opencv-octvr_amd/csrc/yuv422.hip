// yuv422.hip — the 8-bit 4:2:2 capture layouts beside UYVY, in and out (OCTVR_PIX_YUYV422, OCTVR_PIX_YUV422P,
// OCTVR_PIX_NV16): yuv422_unpack_kernel<L> converts the footprint of input frames of layout L into the NV12
// frames the stitch kernels read, yuv422_pack_kernel<L> a stitched NV12 frame into the caller's frame.  A
// translation unit of its own, like uyvy.hip: no existing code object moves.  The lane bodies are
// yuv422_host.hpp's templates, the functions the CPU check runs; this file supplies the memory accesses.
//
// yuv422_unpack_kernel: the geometry of uyvy_unpack_kernel (sixteen lanes per table piece, sixteen pieces per
//   workgroup, one lane per 8-pixel group of the row pair, a longer piece in rounds of sixteen).  Per group
//     YUYV     two 16-byte loads, byte permutes split luma from chroma (UYVY's selectors, swapped), uyvy_avg4;
//     NV16     two 8-byte luma loads, two 8-byte chroma loads averaged four bytes at a time;
//     YUV422P  two 8-byte luma loads, 4 bytes of U and 4 of V from each of the two chroma rows, averaged, then
//              zipped into U,V pairs by two permutes;
//   then two 8-byte luma stores and one 8-byte chroma store into the NV12 frame.  Global loads need no alignment
//   on gfx950, so any base and pitch.  For the planar layouts the luma is copied although it is already planar:
//   the composite takes one pointer per camera with the chroma below the luma.
//   Cache policy, as uyvy.hip argues: the caller's frame is read once (non-temporal loads), the NV12 frame is
//   read by the gain feed and the composite right after (plain stores).
//   Byte path: the short last group of a width that is no multiple of 8, and every group of a frame whose rows
//   are not 8-byte aligned (then YUV422P's V half, at byte w / 2, is not 4-byte aligned either).
//   Bounds: a run has row pair rp < h / 2 and groups inside the row (checked where the runs are built),
//   yuv422_unpack_item yields px <= 0 for anything else; a group's loads are its own bytes of its rows (inside
//   the row's width <= pitch, inside the frame's 2 h rows), stores px bytes inside the NV12 frame's rows.
// yuv422_pack_kernel: a work item is a 16-byte chunk of one destination row (for YUV422P's chroma: of the U or
//   the V half of a row) counted from that row's first 16-byte boundary (yuv422_pack_item), so every full chunk
//   is one aligned 16-byte store whatever the base and pitch.  YUYV zips 8 luma and 8 chroma bytes; luma rows
//   and NV16's chroma rows are 16-byte copies; a YUV422P half row takes the even or odd bytes of 32 bytes of
//   the NV12 chroma row.  Each chroma row is read for two destination rows (the second from L2).  Heads and
//   tails are bytes.  Plain loads and stores, as uyvy_pack_kernel's.
#include "kernels.hpp"
#include "yuv422_host.hpp"

namespace octvr {

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
    __device__ __forceinline__ Yuv422Pair load8(const uint8_t* p) const {
        const u32x2_u v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_u*>(p));
        return Yuv422Pair{v.x, v.y};
    }
    __device__ __forceinline__ UyvyWords load16(const uint8_t* p) const {
        const u32x4_u v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(p));
        return UyvyWords{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void store8(uint8_t* p, const Yuv422Pair& v) const {
        *reinterpret_cast<u32x2*>(p) = u32x2{v.x, v.y};
    }
};

struct PackMem {  // the NV12 frame the kernel before wrote
    __device__ __forceinline__ Yuv422Pair load8(const uint8_t* p) const {
        const u32x2_u v = *reinterpret_cast<const u32x2_u*>(p);
        return Yuv422Pair{v.x, v.y};
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
__global__ void __launch_bounds__(256) yuv422_unpack_kernel(const UyvyRun* __restrict__ table, int n_pieces, UyvySources src,
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
        yuv422_unpack_lane<L>(UnpackMem{}, s, d, w, yuv422_unpack_item(L, w, h, pitch, r, k));
}

template <int L>
__global__ void __launch_bounds__(256) yuv422_pack_kernel(const uint8_t* __restrict__ src, int w, int h,
                                                          uint8_t* __restrict__ out, size_t pitch, uint32_t items) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= items) return;
    yuv422_pack_lane<L>(PackMem{}, src, out, w, h, yuv422_pack_item(L, w, h, pitch, reinterpret_cast<uintptr_t>(out), id));
}

hipError_t launch_yuv422_unpack(int layout, const UyvyRun* table, int n_pieces, const UyvySources& src,
                                const FootFrames& frames, hipStream_t s) {
    if (layout < kYuv422Yuyv || layout > kYuv422Nv16) return hipErrorInvalidValue;
    if (n_pieces <= 0) return hipSuccess;
    constexpr unsigned per_block = 256u / kUnpackLanes;
    const dim3 grid(((unsigned)n_pieces + per_block - 1u) / per_block);
    if (layout == kYuv422Yuyv)
        hipLaunchKernelGGL(yuv422_unpack_kernel<kYuv422Yuyv>, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    else if (layout == kYuv422Planar)
        hipLaunchKernelGGL(yuv422_unpack_kernel<kYuv422Planar>, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    else
        hipLaunchKernelGGL(yuv422_unpack_kernel<kYuv422Nv16>, grid, dim3(256), 0, s, table, n_pieces, src, frames);
    return hipGetLastError();
}

hipError_t launch_yuv422_pack(int layout, const uint8_t* src, int w, int h, uint8_t* out, size_t pitch, hipStream_t s) {
    if (layout < kYuv422Yuyv || layout > kYuv422Nv16) return hipErrorInvalidValue;
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || pitch < (size_t)yuv422_frame_row_bytes(layout, w)) return hipErrorInvalidValue;
    const uint64_t items = yuv422_pack_items(layout, w, h);
    if (items >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((items + 255u) / 256u));
    if (layout == kYuv422Yuyv)
        hipLaunchKernelGGL(yuv422_pack_kernel<kYuv422Yuyv>, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    else if (layout == kYuv422Planar)
        hipLaunchKernelGGL(yuv422_pack_kernel<kYuv422Planar>, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    else
        hipLaunchKernelGGL(yuv422_pack_kernel<kYuv422Nv16>, grid, dim3(256), 0, s, src, w, h, out, pitch, (uint32_t)items);
    return hipGetLastError();
}

}  // namespace octvr
