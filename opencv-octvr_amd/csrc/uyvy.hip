// uyvy.hip — packed UYVY 4:2:2 frames in and out (OCTVR_PIX_UYVY422): uyvy_unpack_kernel converts the footprint
// of packed input frames into 4:2:0 frames the stitch kernels read, uyvy_pack_kernel a stitched 4:2:0 frame into
// the caller's packed frame.  A translation unit of its own, like overlay.hip and the device-frame merge: no
// existing code object moves.  The byte arithmetic is uyvy_host.hpp's, the functions the CPU check runs.
//
// uyvy_unpack_kernel: sixteen lanes per table piece (at most 64 groups of one run, uyvy_run_table; a footprint's
//   runs are short, 4.7 groups on the C2 rig, so a whole wave per piece would idle most lanes), sixteen pieces
//   per workgroup, one lane per 8-pixel group of the row pair (a longer piece in rounds of sixteen): two 16-byte
//   loads (one per packed row; global loads need no alignment on gfx950, so any base and pitch), byte permutes
//   split luma from chroma, the two chroma rows are averaged four bytes at a time (uyvy_avg4), then two 8-byte
//   luma stores and one 8-byte chroma store into the NV12 frame.
//   Cache policy: the packed source is read once and never again: non-temporal loads, it should not displace
//   what the composite is about to read.  The 4:2:0 destination is read by the gain feed and the composite
//   right after: plain stores, which keep the lines in L2 and the Infinity Cache.
//   Byte path: the short last group of a width that is no multiple of 8, and every group of a frame whose
//   rows are not 8-byte aligned (w % 8 != 0): uyvy_unpack_bytes.
//   Bounds: a run has row pair rp < h / 2 and groups inside the row (checked by the launcher's callers when the
//   runs are built: async.cpp footprint_runs), uyvy_unpack_item yields px <= 0 for anything else; loads are
//   the 2 px bytes of the group in its two rows (inside 2 w <= pitch), stores px bytes inside the frame's rows.
// uyvy_pack_kernel: a work item is a 16-byte chunk of one packed row counted from the destination's first 16-byte
//   boundary (uyvy_pack_item), so every full chunk is one aligned 16-byte store whatever the base and pitch;
//   its bytes alternate between 8 bytes of the luma row and 8 of the chroma row (two 8-byte loads, unaligned
//   in general), zipped by two permutes per word.  Heads and tails are bytes.  Each chroma row is read for two
//   packed rows (the second from L2).  Plain loads (the frame was written by the kernel just before) and plain
//   stores (the caller's next kernel or copy reads the packed frame).
#include "kernels.hpp"
#include "uyvy_host.hpp"

namespace octvr {

namespace {

typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ UyvyWords load16_once(const uint8_t* p) {
    const u32x4_u v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(p));
    return UyvyWords{v.x, v.y, v.z, v.w};
}

}  // namespace

constexpr uint32_t kUnpackLanes = 16;  // lanes of one table piece

__global__ void __launch_bounds__(256) uyvy_unpack_kernel(const UyvyRun* __restrict__ table, int n_pieces, UyvySources src,
                                                          FootFrames fr) {
    const int piece = (int)(blockIdx.x * (256u / kUnpackLanes) + threadIdx.x / kUnpackLanes);
    if (piece >= n_pieces) return;
    const UyvyRun r = table[piece];
    const int cam = (int)(r.cam & 31u);
    const int w = fr.w[cam], h = fr.h[cam];
    const uint8_t* const s = src.packed ? src.packed : src.f[cam];
    const size_t pitch = src.packed ? 0 : src.pitch[cam];
    uint8_t* const d = fr.f[cam];
    for (int k = (int)(threadIdx.x % kUnpackLanes); k < (int)r.ng; k += (int)kUnpackLanes) {
        const UyvyItem it = uyvy_unpack_item(w, h, pitch, r, k);
        if (it.px <= 0) continue;
        if (uyvy_unpack_vector(w, reinterpret_cast<uintptr_t>(d), it)) {
            const UyvyGroupOut o = uyvy_split_group(load16_once(s + it.s0), load16_once(s + it.s1));
            *reinterpret_cast<u32x2*>(d + it.y0) = u32x2{o.y0[0], o.y0[1]};
            *reinterpret_cast<u32x2*>(d + it.y1) = u32x2{o.y1[0], o.y1[1]};
            *reinterpret_cast<u32x2*>(d + it.c) = u32x2{o.c[0], o.c[1]};
        } else {
            uyvy_unpack_bytes(s, d, it);
        }
    }
}

__global__ void __launch_bounds__(256) uyvy_pack_kernel(const uint8_t* __restrict__ src, int w, int h,
                                                        uint8_t* __restrict__ out, size_t pitch, uint32_t items) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= items) return;
    const UyvySpan sp = uyvy_pack_item(w, h, pitch, reinterpret_cast<uintptr_t>(out), id);
    if (sp.len == kUyvyChunk) {
        const UyvyChunkSrc cs = uyvy_pack_chunk_src(w, h, sp);
        const u32x2_u f = *reinterpret_cast<const u32x2_u*>(src + cs.first);
        const u32x2_u g = *reinterpret_cast<const u32x2_u*>(src + cs.second);
        const UyvyWords o = uyvy_zip(f.x, f.y, g.x, g.y);
        *reinterpret_cast<u32x4*>(out + sp.dst) = u32x4{o.x, o.y, o.z, o.w};
        return;
    }
    uyvy_pack_bytes(src, out, w, h, sp);
}

hipError_t launch_uyvy_unpack(const UyvyRun* table, int n_pieces, const UyvySources& src, const FootFrames& frames,
                              hipStream_t s) {
    if (n_pieces <= 0) return hipSuccess;
    constexpr unsigned per_block = 256u / kUnpackLanes;
    hipLaunchKernelGGL(uyvy_unpack_kernel, dim3(((unsigned)n_pieces + per_block - 1u) / per_block), dim3(256), 0, s, table,
                       n_pieces, src, frames);
    return hipGetLastError();
}

hipError_t launch_uyvy_pack(const uint8_t* src, int w, int h, uint8_t* out, size_t pitch, hipStream_t s) {
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || pitch < (size_t)2 * (size_t)w) return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)h * uyvy_pack_row_items(w);
    if (items >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(uyvy_pack_kernel, dim3((unsigned)((items + 255u) / 256u)), dim3(256), 0, s, src, w, h, out, pitch,
                       (uint32_t)items);
    return hipGetLastError();
}

}  // namespace octvr
