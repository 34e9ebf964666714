// async_merge_pack.hip — merge_pack_kernel<L>: the NV12 region frames of an AsyncMultiMapper frame into the merged
// frame in a converted layout L (octvr_async_set_output_format, async.cpp): UYVY, YUYV, YUV422P, NV16, P010,
// YUV420P10, P210 or YUV422P10.  The merge (async_merge.hip) and the out rule (frame_layout.hip
// layout_pack_kernel) in one pass: no merged 4:2:0 intermediate, no per-region converted frame.  A translation
// unit of its own: no existing code object moves.
//
// One launch per frame for all regions, destination-driven.  A work item is (region, destination list row of the
// region's sub-picture, 16-byte chunk of that row counted from the row's first 16-byte boundary in the merged
// frame): async_host.hpp merge_pack_item, which finds the region by the regions' first items (at most 32, the
// table is a kernel argument) and cuts the row by frame_layout.hpp pack_item_at; the lane body is
// frame_layout.hpp pack_lane, the function layout_pack_kernel and the CPU check run.  Consecutive lanes take
// consecutive chunks of one row.
//   full chunk: one aligned 16-byte store of 16 bytes built from the region frame: 8 luma and 8 chroma bytes
//     zipped (packed rows), a 16-byte copy, 8 bytes widened to 8 words, or the even / odd bytes of 32 (16,
//     widened) bytes of an NV12 chroma row (a U or V half row).  The loads are at whatever alignment the region's
//     column and the frame's base give: global loads need no alignment on gfx950.
//   heads and tails: sample by sample (for 16-bit layouts the base, the pitch and every row start are even).
// Plain loads (the region frames were written by the kernels just before) and plain stores (the merged frame is
// what the caller's next kernel, or the download, reads).  With two chroma rows per row pair each NV12 chroma row
// of a region frame is read for two destination rows, the second from L2.
// Bounds: build_merge_pack_table admits only regions inside the merged frame that are whole sub-pictures of the
// layout, a pitch of at least a row and a frame below 2 GiB; pack_item_at yields [dst, dst + len) inside the
// region's bytes of one row of the merged frame, pack_lane reads the region frame's samples of those bytes only;
// ids at or past t.items return at once.
#include "async_host.hpp"
#include "kernels.hpp"

namespace octvr {

namespace {

typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct MergePackMem {
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
};

}  // namespace

template <class L>
__global__ void __launch_bounds__(256) merge_pack_kernel(uint8_t* __restrict__ out, const MergePackTable t) {
    constexpr LayoutDesc d = L::desc;
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= t.items) return;
    int k;
    const LayoutSpan sp = merge_pack_item(d, t, id, reinterpret_cast<uintptr_t>(out), k);
    pack_lane<L>(MergePackMem{}, t.r[k].src, out, t.r[k].w, t.r[k].h, sp);
}

hipError_t launch_merge_pack(int pix, uint8_t* out, const MergePackTable& t, hipStream_t s) {
    const LayoutDesc d = layout_of(pix);
    if (!d.converted() || d.v210() || !out || !d.aligned(out, t.pitch)) return hipErrorInvalidValue;  // heads and tails are samples
    if (t.items == 0) return hipSuccess;
    const dim3 grid((t.items + 255u) / 256u);
    with_layout(pix, [&](auto tag) { hipLaunchKernelGGL(merge_pack_kernel<decltype(tag)>, grid, dim3(256), 0, s, out, t); });
    return hipGetLastError();
}

}  // namespace octvr
