// async_merge.hip — merge_regions_kernel: the regions of an AsyncMultiMapper frame into the caller's merged
// device frame (octvr_async_push_device, async.cpp).  A translation unit of its own, like overlay.hip and the
// NV12 unpack: no existing code object moves.
//
// A pure copy, one launch per frame for all regions.  A work item is (region, row, 16-byte chunk of the row,
// counted from the destination's first 16-byte boundary): async_host.hpp merge_item, the same function the
// CPU check runs.  Consecutive lanes take consecutive chunks of one row, so a wave's accesses are contiguous.
//   full chunk: the destination is 16-byte aligned by construction: one 16-byte store.  The source row's
//     alignment relative to it is whatever the region's width and column make it (constant along a row): the
//     16 bytes come from the widest naturally aligned loads the source address allows (16, 8, 4, 2 or 1 bytes),
//     as load16 spells out; for gfx950, where global loads need no alignment, hipcc folds its five cases into
//     one global_load_dwordx4.
//   ragged head (before the first boundary) and tail (after the last whole chunk): bytes.
// A planar region's chroma row is two such rows, its U half and its V half, each of w / 2 bytes at its own
// column of the merged chroma rows: odd widths and odd columns in general, hence mostly the narrow loads.
// Addressing is flat: a buffer resource buys nothing on a bandwidth-bound copy (no bounds to lean on, the
// offsets are checked on the host), and the sources differ per region.  The stores are plain: unlike the
// composite's frame (stored `nt`: nothing on the device reads it back) the merged frame is what the caller's
// next kernel reads, so its lines may as well stay in L2 and the Infinity Cache; the loads are plain too, the
// region frames were written by the kernels just before.
// Bounds: build_merge_table admits only regions inside the merged frame and a frame below 2 GiB; merge_item
// yields [src, src + len) inside the region frame's row and [dst, dst + len) inside the region's row of the
// merged frame; ids at or past t.items return at once.
#include "async_host.hpp"
#include "kernels.hpp"

namespace octvr {

namespace {

__device__ __forceinline__ uint32_t pack4(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// 16 bytes at p with naturally aligned loads only
__device__ __forceinline__ uint4 load16(const uint8_t* p) {
    const uint32_t a = (uint32_t)reinterpret_cast<uintptr_t>(p);
    if ((a & 15u) == 0) return *reinterpret_cast<const uint4*>(p);
    if ((a & 7u) == 0) {
        const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + 8);
        return make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
    if ((a & 3u) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        return make_uint4(q[0], q[1], q[2], q[3]);
    }
    if ((a & 1u) == 0) {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
        return make_uint4((uint32_t)q[0] | (uint32_t)q[1] << 16, (uint32_t)q[2] | (uint32_t)q[3] << 16,
                          (uint32_t)q[4] | (uint32_t)q[5] << 16, (uint32_t)q[6] | (uint32_t)q[7] << 16);
    }
    return make_uint4(pack4(p), pack4(p + 4), pack4(p + 8), pack4(p + 12));
}

}  // namespace

__global__ void __launch_bounds__(256) merge_regions_kernel(uint8_t* __restrict__ out, const MergeTable t) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= t.items) return;
    const MergeSpan sp = merge_item(t, id, reinterpret_cast<uintptr_t>(out));
    uint8_t* const d = out + sp.dst;
    if (sp.len == kChunk) {
        *reinterpret_cast<uint4*>(d) = load16(sp.src);
        return;
    }
    for (int i = 0; i < sp.len; i++) d[i] = sp.src[i];
}

hipError_t launch_merge_regions(uint8_t* out, const MergeTable& t, hipStream_t s) {
    if (t.items == 0) return hipSuccess;
    hipLaunchKernelGGL(merge_regions_kernel, dim3((t.items + 255u) / 256u), dim3(256), 0, s, out, t);
    return hipGetLastError();
}

}  // namespace octvr
