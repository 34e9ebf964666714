// tensor_out.hip — octvr_mapper_stitch_tensor's kernels: the RGB result as three planes of u8, f16 or f32
// (kernels.hpp TensorPlanes).  A translation unit of its own, so that no existing code object moves.
//
// Both kernels give one workgroup one segment of one tensor row (tensor_out_index.hpp) and run in two phases.
//   compute: the segment's preview bytes P[y][x][c] into LDS, one byte per pixel and colour.
//     tensor_resize_kernel: from the RGBA result frame, one pixel per lane, resize_rgba_rgb_kernel's chain per
//       channel (weights from the unclamped x2 / y2, fmaf in the order c00, c01, c10, c11 from 0, sat_u8_rne);
//     tensor_gather_kernel: from the source frames through the prepared tap list, one tap per lane and one
//       quad per pixel, preview_gather_kernel's arithmetic instruction for instruction.
//   store: plane by plane.  A plane's row has no alignment beyond the element size, so its share of the
//     segment is a ragged head, groups of 4 elements at 4-, 8- or 16-byte boundaries, and a ragged tail
//     (tensor_item, the function tests/cpp/tensor_out_check.cpp sweeps).  Consecutive lanes store consecutive
//     groups of one plane: a wave's stores are contiguous along x, 4 elements per lane.  Head and tail go
//     element by element.  Plain stores: a model reads the tensor next, its lines may stay in L2.
// Float planes: (float)P * scale[c] + bias[c], a multiply and then an add (the library is built with
// -ffp-contract=off); f16 is that value through v_cvt_f16_f32 / v_cvt_pk_f16_f32, which follow the rounding and
// denormal modes (the defaults: round to nearest even, overflow to inf, subnormal halves kept), never the
// round-toward-zero pack v_cvt_pkrtz_f16_f32.
// Bounds: every load of the result frame is from clamped coordinates, every list index is below 4 n_pixels, and
// the stores are tensor_item's elements of [0, n) of a row the host checked (mapper.cpp check_tensor).
#include <type_traits>

#include "device_common.hpp"
#include "tensor_out_index.hpp"

namespace octvr {

namespace {

constexpr int kResizeSeg = 256;  // pixels of a workgroup of tensor_resize_kernel: one per lane
constexpr int kGatherSeg = 64;   // ... of tensor_gather_kernel: one per quad (kPvBlockEntries taps)
static_assert(3 * tensor_slots<kResizeSeg>() <= 256 && 3 * tensor_slots<kGatherSeg>() <= 256, "one slot per lane");
static_assert(kGatherSeg * 4 == kPvBlockEntries, "a tap per lane");

template <class T>
__device__ __forceinline__ T tensor_value(uint32_t p, float scale, float bias) {
    if constexpr (std::is_same_v<T, uint8_t>) {
        return (uint8_t)p;
    } else {
        const float f = (float)p * scale + bias;
        return (T)f;
    }
}

// The store phase: lane tid's slot of the segment [x0, x0 + n) of row y, from the bytes in s_px[colour][pixel].
template <class T, int S>
__device__ __forceinline__ void store_segment(const uint8_t (&s_px)[3][S], const TensorPlanes& t, int y, int x0, int n,
                                              uint32_t tid) {
    typedef T Wide __attribute__((ext_vector_type(kTensorGroup)));
    // global-address-space views: stores through a pointer held in a struct would otherwise be flat
    typedef __attribute__((address_space(1))) T GT;
    typedef __attribute__((address_space(1))) Wide GWide;
    constexpr uint32_t kSlots = (uint32_t)tensor_slots<S>();
    const uint32_t pl = tid / kSlots;
    if (pl >= 3u) return;
    const uint32_t c = t.bgr ? 2u - pl : pl;
    GT* const row = (GT*)static_cast<T*>(t.dev) + ((int64_t)pl * t.plane_stride + (int64_t)y * t.row_stride + x0);
    const int head = tensor_head((uint64_t)(uintptr_t)row, (int)sizeof(T), n);
    const TensorSpan sp = tensor_item<S>((int)(tid - pl * kSlots), n, head);
    const float sc = c == 0u ? t.scale[0] : c == 1u ? t.scale[1] : t.scale[2];
    const float bi = c == 0u ? t.bias[0] : c == 1u ? t.bias[1] : t.bias[2];
    const uint8_t* const src = &s_px[c][sp.first];
    if (sp.len == kTensorGroup) {
        const Wide v = {tensor_value<T>(src[0], sc, bi), tensor_value<T>(src[1], sc, bi), tensor_value<T>(src[2], sc, bi),
                        tensor_value<T>(src[3], sc, bi)};
        *(GWide*)(row + sp.first) = v;
        return;
    }
    for (int i = 0; i < sp.len; i++) row[sp.first + i] = tensor_value<T>(src[i], sc, bi);
}

}  // namespace

template <class T>
__global__ void __launch_bounds__(256) tensor_resize_kernel(const uint8_t* __restrict__ rgba, int sw, int sh, int64_t spitch,
                                                            float fx, float fy, TensorPlanes t) {
    __shared__ uint8_t s_px[3][kResizeSeg];
    const uint32_t tid = threadIdx.x;
    const int nseg = tensor_segments<kResizeSeg>(t.w);
    const int y = (int)(blockIdx.x / (uint32_t)nseg), sx = (int)(blockIdx.x - (uint32_t)y * (uint32_t)nseg);  // y < t.h: the grid
    const int n = tensor_segment_len<kResizeSeg>(t.w, sx);
    const int x = min(sx * kResizeSeg + (int)tid, t.w - 1);  // a lane past the row's end repeats its last pixel
    const float src_x = (float)x * fx, src_y = (float)y * fy;
    const int x1 = (int)floorf(src_x), y1 = (int)floorf(src_y);
    const int x2 = x1 + 1, y2 = y1 + 1;
    const int x1r = min(x1, sw - 1), y1r = min(y1, sh - 1), x2r = min(x2, sw - 1), y2r = min(y2, sh - 1);
    const uint32_t* r1 = reinterpret_cast<const uint32_t*>(rgba + (int64_t)y1r * spitch);
    const uint32_t* r2 = reinterpret_cast<const uint32_t*>(rgba + (int64_t)y2r * spitch);
    const uint32_t c00 = r1[x1r], c01 = r1[x2r], c10 = r2[x1r], c11 = r2[x2r];
    const float w00 = ((float)x2 - src_x) * ((float)y2 - src_y);
    const float w01 = (src_x - (float)x1) * ((float)y2 - src_y);
    const float w10 = ((float)x2 - src_x) * (src_y - (float)y1);
    const float w11 = (src_x - (float)x1) * (src_y - (float)y1);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const uint32_t sh8 = 8u * ch;
        float o = 0.f;
        o = __builtin_fmaf((float)((c00 >> sh8) & 255u), w00, o);
        o = __builtin_fmaf((float)((c01 >> sh8) & 255u), w01, o);
        o = __builtin_fmaf((float)((c10 >> sh8) & 255u), w10, o);
        o = __builtin_fmaf((float)((c11 >> sh8) & 255u), w11, o);
        s_px[ch][tid] = (uint8_t)sat_u8_rne(o);
    }
    __syncthreads();
    store_segment<T, kResizeSeg>(s_px, t, y, sx * kResizeSeg, n, tid);
}

template <class T, bool NV12>
__global__ void __launch_bounds__(256) tensor_gather_kernel(FrameSet frames, PreviewList list, const double* gains,
                                                            int use_gain, TensorPlanes t) {
    __shared__ float s_gain[kMaxCams];
    __shared__ uint8_t s_px[3][kGatherSeg];
    const uint32_t tid = threadIdx.x;
    if (tid < (uint32_t)kMaxCams) s_gain[tid] = use_gain ? (float)gains[tid] : 1.0f;
    __syncthreads();
    const uint32_t dw = (uint32_t)list.dw;
    const uint32_t nseg = (uint32_t)tensor_segments<kGatherSeg>(list.dw);
    const uint32_t y = blockIdx.x / nseg, sx = blockIdx.x - y * nseg;  // y < list.dh: the grid
    const int n = tensor_segment_len<kGatherSeg>(list.dw, (int)sx);
    const uint32_t i = tid >> 2, ch = tid & 3u;
    const uint32_t x = min(sx * (uint32_t)kGatherSeg + i, dw - 1u);  // a quad past the row's end repeats its last pixel
    const uint32_t k = y * dw + x;                                   // < list.n_pixels, so 4 k + ch < list.n_entries
    const uint2 e = reinterpret_cast<const uint2*>(list.entries)[4u * k + ch];
    Taps tp;
    gather_taps<NV12>(frames, e.x, e.y, tp);
    uint32_t rgb[3];
    if (e.y & kCodeTex)
        tex_bilerp(tp.c[0], tp.c[1], tp.c[2], tp.c[3], tp.fx, tp.fy, rgb);
    else
        bilerp_rgba(tp.c[0], tp.c[1], tp.c[2], tp.c[3], tp.fx, tp.fy, rgb);
    const float g = (e.y & kCodeNoGain) ? 1.0f : s_gain[(e.y >> 10) & 31u];
    uint32_t px = pack_u8((float)rgb[0] * g, 0, 0u);
    px = pack_u8((float)rgb[1] * g, 1, px);
    px = pack_u8((float)rgb[2] * g, 2, px);
    const uint32_t c00 = quad_lane<0>(px), c01 = quad_lane<1>(px), c10 = quad_lane<2>(px), c11 = quad_lane<3>(px);
    const float src_x = (float)x * list.fx, src_y = (float)y * list.fy;
    const float x1 = floorf(src_x), y1 = floorf(src_y);
    const float x2 = x1 + 1.f, y2 = y1 + 1.f;  // exact: the coordinates are integers below 2^24
    const float w00 = (x2 - src_x) * (y2 - src_y);
    const float w01 = (src_x - x1) * (y2 - src_y);
    const float w10 = (x2 - src_x) * (src_y - y1);
    const float w11 = (src_x - x1) * (src_y - y1);
    const uint32_t sh8 = 8u * ch;
    float o = 0.f;
    o = __builtin_fmaf((float)((c00 >> sh8) & 255u), w00, o);
    o = __builtin_fmaf((float)((c01 >> sh8) & 255u), w01, o);
    o = __builtin_fmaf((float)((c10 >> sh8) & 255u), w10, o);
    o = __builtin_fmaf((float)((c11 >> sh8) & 255u), w11, o);
    if (ch < 3u) s_px[ch][i] = (uint8_t)sat_u8_rne(o);
    __syncthreads();
    store_segment<T, kGatherSeg>(s_px, t, (int)y, (int)sx * kGatherSeg, n, tid);
}

namespace {

// blocks of a w x h tensor in segments of S, or 0 when the grid would not hold them
template <int S>
uint32_t tensor_blocks(const TensorPlanes& t) {
    if (!t.dev || t.w <= 0 || t.h <= 0 || (t.bgr != 0 && t.bgr != 1)) return 0;
    const uint64_t b = (uint64_t)tensor_segments<S>(t.w) * (uint64_t)t.h;
    return b < 0x7FFFFFFFull ? (uint32_t)b : 0;
}

}  // namespace

hipError_t launch_tensor_resize(const uint8_t* rgba, int sw, int sh, int64_t spitch, const TensorPlanes& t, hipStream_t s) {
    const uint32_t blocks = tensor_blocks<kResizeSeg>(t);
    if (!blocks || !rgba || sw <= 0 || sh <= 0) return hipErrorInvalidValue;
    const float fx = (float)(1.0 / ((double)t.w / sw)), fy = (float)(1.0 / ((double)t.h / sh));
    const dim3 grid(blocks), block(256);
    switch (t.dtype) {
        case kTensorU8:
            hipLaunchKernelGGL(tensor_resize_kernel<uint8_t>, grid, block, 0, s, rgba, sw, sh, spitch, fx, fy, t);
            break;
        case kTensorF16:
            hipLaunchKernelGGL(tensor_resize_kernel<_Float16>, grid, block, 0, s, rgba, sw, sh, spitch, fx, fy, t);
            break;
        case kTensorF32:
            hipLaunchKernelGGL(tensor_resize_kernel<float>, grid, block, 0, s, rgba, sw, sh, spitch, fx, fy, t);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <class T>
static void launch_gather_as(const FrameSet& frames, const PreviewList& list, const double* gains, int use_gain,
                             const TensorPlanes& t, hipStream_t s, int pix, uint32_t blocks) {
    const dim3 grid(blocks), block(256);
    if (pix & kPixInNv12)
        hipLaunchKernelGGL((tensor_gather_kernel<T, true>), grid, block, 0, s, frames, list, gains, use_gain, t);
    else
        hipLaunchKernelGGL((tensor_gather_kernel<T, false>), grid, block, 0, s, frames, list, gains, use_gain, t);
}

hipError_t launch_tensor_gather(const FrameSet& frames, const PreviewList& list, const double* gains, int use_gain,
                                const TensorPlanes& t, hipStream_t s, int pix) {
    const uint32_t blocks = tensor_blocks<kGatherSeg>(t);
    if (!blocks || !list.entries || t.w != list.dw || t.h != list.dh ||
        (uint64_t)list.n_pixels != (uint64_t)t.w * (uint64_t)t.h || (uint64_t)list.n_pixels * 4u > list.n_entries)
        return hipErrorInvalidValue;
    switch (t.dtype) {
        case kTensorU8:
            launch_gather_as<uint8_t>(frames, list, gains, use_gain, t, s, pix, blocks);
            break;
        case kTensorF16:
            launch_gather_as<_Float16>(frames, list, gains, use_gain, t, s, pix, blocks);
            break;
        case kTensorF32:
            launch_gather_as<float>(frames, list, gains, use_gain, t, s, pix, blocks);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace octvr
