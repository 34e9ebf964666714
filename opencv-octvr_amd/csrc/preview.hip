// preview.hip — preview_gather_kernel: the preview of a blend-0 mapper gathered straight from the source
// frames through its prepared tap list (kernels.hpp PreviewList), with no result frame in between.  A
// translation unit of its own, so that no existing code object moves.
#include "device_common.hpp"

namespace octvr {

// One lane per result tap, one quad per preview pixel, 64 preview pixels per workgroup: entry t = 4 pixel +
// tap is one coalesced 8-byte load per lane.  The lane computes what the MODE-1 composite stores into the
// result frame for its tap's result pixel — the four source taps gathered in place (gather_taps: YUV -> RGB,
// vignette, both layouts; every load issued from a clamped address before the first use), filtered by the
// entry's convention, times the camera's gain with the saturating conversion — as one packed RGB dword.  The
// quad exchanges its four dwords by DPP and lanes 0-2 each run resize_rgba_rgb_kernel's chain for one channel:
// weights from the unclamped x2 / y2, fmaf in the order c00, c01, c10, c11 from 0, sat_u8_rne, one byte out.
// An entry that claims nothing names camera 0: its lane loads from input 0's frame at clamped addresses,
// uses none of it and contributes black.  The list holds whole workgroups, so only the stores are bounded.
template <bool NV12>
__global__ void __launch_bounds__(256) preview_gather_kernel(FrameSet frames, PreviewList list, const double* gains,
                                                             int use_gain, uint8_t* out, int64_t out_pitch) {
    __shared__ float s_gain[kMaxCams];
    const uint32_t tid = threadIdx.x;
    if (tid < (uint32_t)kMaxCams) s_gain[tid] = use_gain ? (float)gains[tid] : 1.0f;
    __syncthreads();
    const uint32_t t = blockIdx.x * 256u + tid;  // < list.n_entries: the list holds whole workgroups
    const uint2 e = reinterpret_cast<const uint2*>(list.entries)[t];
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
    const uint32_t k = t >> 2, ch = t & 3u;
    const uint32_t y = k / (uint32_t)list.dw, x = k - y * (uint32_t)list.dw;
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
    if (ch < 3u && k < list.n_pixels) out[(int64_t)y * out_pitch + 3 * (int64_t)x + ch] = (uint8_t)sat_u8_rne(o);
}

hipError_t launch_preview_gather(const FrameSet& frames, const PreviewList& list, const double* gains, int use_gain,
                                 uint8_t* out, int64_t out_pitch, hipStream_t s, int pix) {
    if (list.n_entries == 0 || list.n_entries % kPvBlockEntries || list.dw <= 0 ||
        (uint64_t)list.n_pixels * 4u > list.n_entries)
        return hipErrorInvalidValue;
    const dim3 grid(list.n_entries / kPvBlockEntries), block(256);
    if (pix & kPixInNv12)
        hipLaunchKernelGGL(preview_gather_kernel<true>, grid, block, 0, s, frames, list, gains, use_gain, out, out_pitch);
    else
        hipLaunchKernelGGL(preview_gather_kernel<false>, grid, block, 0, s, frames, list, gains, use_gain, out, out_pitch);
    return hipGetLastError();
}

}  // namespace octvr
