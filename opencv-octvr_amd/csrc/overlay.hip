// overlay.hip — overlay_apply_kernel: the overlays of a multi-band / feather mapper, copied onto the RGBA
// result frame after the blend (kernels.hpp OverlayList).  A translation unit of its own, so that no
// existing code object moves.
#include "device_common.hpp"

namespace octvr {

// One lane per pixel of the work list, one wave per run of 8 groups (64 consecutive entries: one 512-byte
// load).  A covered lane gathers its four taps from the frame its entry names, in place (gather_taps ->
// gather_taps_frame: YUV -> RGB, vignette; all twelve byte loads and the four vignette loads issued from
// clamped addresses before the first use), filters them by the entry's convention (A13 fixed point, or the
// texture model) and stores one RGBA dword (alpha 0: the resizes ignore it).  No gain, no LDS.  A covered
// entry that is invalid (a texture-convention coordinate outside the plane) names camera 0: its lane still
// loads from input 0's frame at clamped addresses, uses none of it and writes black.  Uncovered lanes do
// nothing: no frame is read and the blend's pixel stays.
template <bool NV12>
__global__ void __launch_bounds__(256) overlay_apply_kernel(FrameSet frames, OverlayList list, uint8_t* rgba,
                                                            int64_t rgba_pitch) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // < 8 n_groups: the list holds whole workgroups
    const uint32_t hd = list.groups[t >> 3];
    const uint2 e = reinterpret_cast<const uint2*>(list.entries)[t];
    if (!(e.y & kCodeCovered)) return;
    Taps tp;
    gather_taps<NV12>(frames, e.x, e.y, tp);
    uint32_t rgb[3];
    if (e.y & kCodeTex)
        tex_bilerp(tp.c[0], tp.c[1], tp.c[2], tp.c[3], tp.fx, tp.fy, rgb);
    else
        bilerp_rgba(tp.c[0], tp.c[1], tp.c[2], tp.c[3], tp.fx, tp.fy, rgb);
    const uint32_t x = (hd & 0xFFFFu) * (uint32_t)kOvGroupPx + (t & 7u), y = hd >> 16;
    *reinterpret_cast<uint32_t*>(rgba + (int64_t)y * rgba_pitch + (int64_t)x * 4) = rgb[0] | rgb[1] << 8 | rgb[2] << 16;
}

hipError_t launch_overlay_apply(const FrameSet& frames, const OverlayList& list, uint8_t* rgba, int64_t rgba_pitch,
                                hipStream_t s, int pix) {
    if (list.n_groups <= 0) return hipSuccess;
    if (list.n_groups % kOvBlockGroups) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(list.n_groups / kOvBlockGroups)), block(256);
    if (pix & kPixInNv12)
        hipLaunchKernelGGL(overlay_apply_kernel<true>, grid, block, 0, s, frames, list, rgba, rgba_pitch);
    else
        hipLaunchKernelGGL(overlay_apply_kernel<false>, grid, block, 0, s, frames, list, rgba, rgba_pitch);
    return hipGetLastError();
}

}  // namespace octvr
