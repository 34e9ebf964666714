// lut_kernels.hip — gfx950 kernels of the rig build: the per-camera LUT (FP64 projection), its
// diagnostics, and the composite LUT of the no-blend copy chain.  Once per rig, never per frame.
//
// Built with -ffp-contract=off: every f32/f64 expression rounds exactly as written, matching the
// reference's non-FMA x86 arithmetic (the oracle, oracle/octvr_oracle.c, is compiled the same way).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "device_common.hpp"
#include "kernels.hpp"

namespace octvr {

// ---------------------------------------------------------------------------------------------
// LUT build: MapperTemplate::add_input (template.cpp:46-133), one thread per output pixel, FP64.
// bbox = {min_w, min_h, max_w, max_h} of valid pixels (int atomics, initialised by the host).
// fragile (optional): pixels whose outcome a last-ulp libm difference could change (LutGuard,
// camera_math.hpp) are appended as indices (fragile[0] = count, entries from fragile[1], at most
// cap kept) and left out of bbox and of the visible_mask update: the host recomputes them with glibc.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lut_build_kernel(const CameraParams* __restrict__ cams, int W, int H,
                                                        float* map1, float* map2, uint8_t* mask, int32_t* bbox,
                                                        uint8_t* visible, uint32_t* fragile, uint32_t cap) {
    const CameraParams& out = cams[0];
    const CameraParams& in = cams[1];
    __shared__ int s_bb[4];
    if (threadIdx.x < 4) s_bb[threadIdx.x] = (threadIdx.x < 2) ? INT32_MAX : -1;
    __syncthreads();
    const int64_t total = (int64_t)W * H;
    int lminw = INT32_MAX, lminh = INT32_MAX, lmaxw = -1, lmaxh = -1;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int h = (int)(idx / W), w = (int)(idx - (int64_t)h * W);
        double dx, dy;
        bool vis = false;
        LutGuard g{false};
        project_output_to_input(out, in, (double)w / W, (double)h / H, &dx, &dy, visible ? &vis : nullptr,
                                fragile ? &g : nullptr);
        const bool frag = fragile && (g.hit || f32_fragile(dx) || f32_fragile(dy));
        if (frag) {
            const uint32_t k = atomicAdd(fragile, 1u);
            if (k < cap) fragile[1 + k] = (uint32_t)idx;
        }
        const float x = (float)dx, y = (float)dy;
        // visible_mask arbitration (template.cpp:86-116): a pixel an earlier camera's include mask
        // claimed (1) is rejected; one this camera's include mask claims first is marked 2 so the host
        // clears it from the earlier cameras' masks.
        const bool claimed = visible && visible[idx] == 1;
        if (visible && vis && !claimed && !frag) visible[idx] = 2;
        if (isnan(x) || isnan(y) || x < 0 || x >= 1.0f || y < 0 || y >= 1.0f || claimed) {
            mask[idx] = 0;
            map1[idx] = -1.0f;
            map2[idx] = -1.0f;
        } else {
            mask[idx] = 255;
            map1[idx] = x;
            map2[idx] = y;
            if (!frag) {
                lminw = min(lminw, w);
                lmaxw = max(lmaxw, w);
                lminh = min(lminh, h);
                lmaxh = max(lmaxh, h);
            }
        }
    }
    if (lmaxw >= 0) {
        atomicMin(&s_bb[0], lminw);
        atomicMin(&s_bb[1], lminh);
        atomicMax(&s_bb[2], lmaxw);
        atomicMax(&s_bb[3], lmaxh);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_bb[2] >= 0) {
        atomicMin(&bbox[0], s_bb[0]);
        atomicMin(&bbox[1], s_bb[1]);
        atomicMax(&bbox[2], s_bb[2]);
        atomicMax(&bbox[3], s_bb[3]);
    }
}

hipError_t launch_lut_build(const CameraParams* cams_dev, int W, int H, float* map1, float* map2, uint8_t* mask,
                            int32_t* bbox, uint8_t* visible, uint32_t* fragile, uint32_t cap, hipStream_t s) {
    const int64_t total = (int64_t)W * H;
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(lut_build_kernel, dim3(blocks), dim3(256), 0, s, cams_dev, W, H, map1, map2, mask, bbox, visible,
                       fragile, cap);
    return hipGetLastError();
}

// Diagnostics (octvr_debug_project_f64): the FP64 projection of every output pixel before the f32
// rounding, with the guard's verdict (1 = fragile), for measuring device-vs-glibc deviations.
__global__ void __launch_bounds__(256) project_f64_kernel(const CameraParams* __restrict__ cams, int W, int H,
                                                          double* xs, double* ys, uint8_t* fragile) {
    const int64_t total = (int64_t)W * H;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int h = (int)(idx / W), w = (int)(idx - (int64_t)h * W);
        double dx, dy;
        LutGuard g{false};
        project_output_to_input(cams[0], cams[1], (double)w / W, (double)h / H, &dx, &dy, nullptr, &g);
        xs[idx] = dx;
        ys[idx] = dy;
        fragile[idx] = (g.hit || f32_fragile(dx) || f32_fragile(dy)) ? 1 : 0;
    }
}

hipError_t launch_project_f64(const CameraParams* cams_dev, int W, int H, double* x, double* y, uint8_t* fragile,
                              hipStream_t s) {
    const int64_t total = (int64_t)W * H;
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(project_f64_kernel, dim3(blocks), dim3(256), 0, s, cams_dev, W, H, x, y, fragile);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Composite LUT: the no-blend copy chain `warped_i.copyTo(result(roi_i), mask_i)` in camera order
// (mapper.cpp:268-277) resolved once per rig: the LAST camera whose ROI contains the pixel and whose
// LUT mask is non-zero wins; its map value is quantized exactly as RemapInvoker does.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) composite_lut_kernel(const CamTemplate* cams, int n, int W, int H,
                                                            CompositeEntry* lut, int tex) {
    const int64_t total = (int64_t)W * H;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(idx / W), x = (int)(idx - (int64_t)y * W);
        CompositeEntry e;
        e.xy = 0;
        e.code = 0;
        for (int i = 0; i < n; i++) {
            const CamTemplate& c = cams[i];
            const int rx = x - c.roi_x, ry = y - c.roi_y;
            if (rx < 0 || ry < 0 || rx >= c.roi_w || ry >= c.roi_h) continue;
            const int64_t k = (int64_t)ry * c.roi_w + rx;
            if (c.mask[k] == 0) continue;
            e = tex ? make_entry_tex(c.map1[k], c.map2[k], (float)c.in_w, (float)c.in_h, i)
                    : make_entry(c.map1[k], c.map2[k], (float)c.in_w, (float)c.in_h, i);
        }
        lut[idx] = e;
    }
}

hipError_t launch_composite_lut(const CamTemplate* cams_dev, int n, int W, int H, CompositeEntry* lut,
                                hipStream_t s, int tex) {
    const int64_t total = (int64_t)W * H;
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(composite_lut_kernel, dim3(blocks), dim3(256), 0, s, cams_dev, n, W, H, lut, tex);
    return hipGetLastError();
}

}  // namespace octvr
