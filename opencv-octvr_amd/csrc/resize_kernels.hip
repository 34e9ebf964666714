// resize_kernels.hip — gfx950 kernels beside the per-frame path: the standalone cv::remap, the
// morph warp, the three resizes, and the saturating-conversion self-test.
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
// Standalone cv::remap INTER_LINEAR u8 (cn = 1, 3, 4), BORDER_CONSTANT 0 — one output pixel per lane.
// ---------------------------------------------------------------------------------------------
template <int CN>
__global__ void __launch_bounds__(256) remap_u8_kernel(const uint8_t* src, int sw, int sh, int64_t spitch,
                                                       const float* map1, const float* map2, int mw, int mh,
                                                       int64_t mpitch, float scale_x, float scale_y, uint8_t* dst,
                                                       int64_t dpitch) {
    const int64_t total = (int64_t)mw * mh;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(idx / mw), x = (int)(idx - (int64_t)y * mw);
        const float X = map1[(int64_t)y * mpitch + x] * scale_x;
        const float Yv = map2[(int64_t)y * mpitch + x] * scale_y;
        const float fx32 = X * 32.0f, fy32 = Yv * 32.0f;
        // _mm_cvtps_epi32: NaN / out of int range -> INT_MIN
        const int ix = (fx32 != fx32 || fabsf(fx32) >= 2147483648.f) ? INT32_MIN : (int)__builtin_rintf(fx32);
        const int iy = (fy32 != fy32 || fabsf(fy32) >= 2147483648.f) ? INT32_MIN : (int)__builtin_rintf(fy32);
        const int sx = min(max(ix >> 5, -32768), 32767), sy = min(max(iy >> 5, -32768), 32767);
        const uint32_t fx = (uint32_t)(ix & 31), fy = (uint32_t)(iy & 31);
        uint32_t v[4][CN];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int tx = sx + (t & 1), ty = sy + (t >> 1);
            const bool in = tx >= 0 && tx < sw && ty >= 0 && ty < sh;
            const uint8_t* p = src + (int64_t)min(max(ty, 0), sh - 1) * spitch + (int64_t)min(max(tx, 0), sw - 1) * CN;
#pragma unroll
            for (int k = 0; k < CN; k++) v[t][k] = in ? p[k] : 0u;
        }
        uint8_t* d = dst + (int64_t)y * dpitch + (int64_t)x * CN;
#pragma unroll
        for (int k = 0; k < CN; k++) d[k] = (uint8_t)bilerp_ch(v[0][k], v[1][k], v[2][k], v[3][k], fx, fy);
    }
}

// ---------------------------------------------------------------------------------------------
// morph_controlpoints' piecewise-affine LUT warp (template_morph.cpp:207-231).  The reference warps
// the whole ROI three times per triangle and copies the triangle's fillPoly'd pixels; here each
// pixel is computed once, by the last triangle that covers it (owner, rasterised on the host).
// cv::warpAffine (imgwarp.cpp:5627-5745, WarpAffineInvoker :5282-5470): AB_BITS = 10 fixed-point
// source coordinates, X = (round((M1 y + M2) 1024) + 16 + round(M0 x 1024)) >> 5, then remap's
// INTER_LINEAR (remapBilinear :3812-4030): f32 planes with the float table ((1-fy)(1-fx), (1-fy)fx,
// fy(1-fx), fy fx in 1/32 steps, exact), u8 with the 15-bit table; taps outside the ROI read 0.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int cv_round_sse2(double v) {  // _mm_cvtsd_si32: ties to even, out of range -> INT_MIN
    const double r = __builtin_rint(v);
    return (r >= -2147483648.0 && r <= 2147483647.0) ? (int)r : INT32_MIN;
}

__global__ void __launch_bounds__(256) morph_warp_kernel(const float* __restrict__ map1, const float* __restrict__ map2,
                                                         const uint8_t* __restrict__ mask, int w, int h,
                                                         const int16_t* __restrict__ owner, const double* __restrict__ M,
                                                         float* out1, float* out2, uint8_t* out_mask) {
    const int64_t total = (int64_t)w * h;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int k = owner[idx];
        if (k < 0) {
            out1[idx] = map1[idx];
            out2[idx] = map2[idx];
            out_mask[idx] = mask[idx];
            continue;
        }
        const int y = (int)(idx / w), x = (int)(idx - (int64_t)y * w);
        const double* m = M + 6 * k;
        const int X0 = cv_round_sse2((m[1] * (double)y + m[2]) * 1024.0) + 16;  // round_delta = 1024 / 32 / 2
        const int Y0 = cv_round_sse2((m[4] * (double)y + m[5]) * 1024.0) + 16;
        const int ad = cv_round_sse2(m[0] * (double)x * 1024.0), bd = cv_round_sse2(m[3] * (double)x * 1024.0);
        const int X = (int)((uint32_t)X0 + (uint32_t)ad) >> 5, Y = (int)((uint32_t)Y0 + (uint32_t)bd) >> 5;
        const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);
        const uint32_t fx = (uint32_t)(X & 31), fy = (uint32_t)(Y & 31);
        float a1[4], a2[4];
        uint32_t am[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int tx = sx + (t & 1), ty = sy + (t >> 1);
            const bool in = tx >= 0 && tx < w && ty >= 0 && ty < h;
            const int64_t o = in ? (int64_t)ty * w + tx : 0;
            a1[t] = in ? map1[o] : 0.f;
            a2[t] = in ? map2[o] : 0.f;
            am[t] = in ? mask[o] : 0u;
        }
        const float vy1 = (float)fy * (1.f / 32), vy0 = 1.f - vy1, vx1 = (float)fx * (1.f / 32), vx0 = 1.f - vx1;
        const float w0 = vy0 * vx0, w1 = vy0 * vx1, w2 = vy1 * vx0, w3 = vy1 * vx1;
        out1[idx] = a1[0] * w0 + a1[1] * w1 + a1[2] * w2 + a1[3] * w3;
        out2[idx] = a2[0] * w0 + a2[1] * w1 + a2[2] * w2 + a2[3] * w3;
        out_mask[idx] = (uint8_t)bilerp_ch(am[0], am[1], am[2], am[3], fx, fy);
    }
}

hipError_t launch_morph_warp(const float* map1, const float* map2, const uint8_t* mask, int w, int h,
                             const int16_t* owner, const double* M, float* out1, float* out2, uint8_t* out_mask,
                             hipStream_t s) {
    const int64_t total = (int64_t)w * h;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 256 * 16));
    hipLaunchKernelGGL(morph_warp_kernel, dim3(blocks), dim3(256), 0, s, map1, map2, mask, w, h, owner, M, out1, out2,
                       out_mask);
    return hipGetLastError();
}

hipError_t launch_remap_u8(const uint8_t* src, int sw, int sh, int64_t spitch, int cn,
                           const float* map1, const float* map2, int mw, int mh, int64_t mpitch, float scale_x,
                           float scale_y, uint8_t* dst, int64_t dpitch, hipStream_t s) {
    const int64_t total = (int64_t)mw * mh;
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 8);
    if (blocks < 1) blocks = 1;
    switch (cn) {
        case 1:
            hipLaunchKernelGGL(remap_u8_kernel<1>, dim3(blocks), dim3(256), 0, s, src, sw, sh, spitch, map1, map2,
                               mw, mh, mpitch, scale_x, scale_y, dst, dpitch);
            break;
        case 3:
            hipLaunchKernelGGL(remap_u8_kernel<3>, dim3(blocks), dim3(256), 0, s, src, sw, sh, spitch, map1, map2,
                               mw, mh, mpitch, scale_x, scale_y, dst, dpitch);
            break;
        case 4:
            hipLaunchKernelGGL(remap_u8_kernel<4>, dim3(blocks), dim3(256), 0, s, src, sw, sh, spitch, map1, map2,
                               mw, mh, mpitch, scale_x, scale_y, dst, dpitch);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// cv::resize INTER_LINEAR u8 (CPU fixed-point rule, tables from the host) — seam-mask build.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) resize_u8_kernel(const uint8_t* __restrict__ src, int sw, int sh, int64_t spitch,
                                                        uint8_t* __restrict__ dst, int dw, int dh, int64_t dpitch,
                                                        ResizeTables t) {
    const int64_t total = (int64_t)dw * dh;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(idx / dw), x = (int)(idx - (int64_t)y * dw);
        uint32_t v;
        if (t.area2) {
            const uint8_t* s0 = src + (int64_t)(2 * y) * spitch + 2 * x;
            v = ((uint32_t)s0[0] + s0[1] + s0[spitch] + s0[spitch + 1] + 2u) >> 2;
        } else {
            const uint8_t* r0 = src + (int64_t)t.rows[2 * y] * spitch;
            const uint8_t* r1 = src + (int64_t)t.rows[2 * y + 1] * spitch;
            const int sx = t.xofs[x];
            int h0, h1;
            if (x < t.xmax) {
                const int a0 = t.ax[2 * x], a1 = t.ax[2 * x + 1];
                h0 = r0[sx] * a0 + r0[sx + 1] * a1;
                h1 = r1[sx] * a0 + r1[sx + 1] * a1;
            } else {
                h0 = r0[sx] * 2048;
                h1 = r1[sx] * 2048;
            }
            const int b0 = t.by[2 * y], b1 = t.by[2 * y + 1];
            v = (uint32_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
        }
        dst[(int64_t)y * dpitch + x] = (uint8_t)v;
    }
}

hipError_t launch_resize_u8(const uint8_t* src, int sw, int sh, int64_t spitch, uint8_t* dst, int dw, int dh,
                            int64_t dpitch, const ResizeTables& t, hipStream_t s) {
    const int64_t total = (int64_t)dw * dh;
    if (total <= 0) return hipSuccess;
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(resize_u8_kernel, dim3(blocks), dim3(256), 0, s, src, sw, sh, spitch, dst, dw, dh, dpitch, t);
    return hipGetLastError();
}

// Preview output (mapper.cpp:308-312): cv::cuda::resize(result, preview_output, preview_size,
// INTER_LINEAR) of the RGB result into a CV_8UC3 image — the same glob-kernel arithmetic as above,
// one lane per preview pixel, 3 bytes out.
__global__ void __launch_bounds__(256) resize_rgba_rgb_kernel(const uint8_t* __restrict__ rgba, int sw, int sh,
                                                              int64_t spitch, float fx, float fy, uint8_t* out, int dw,
                                                              int dh, int64_t out_pitch) {
    const int64_t total = (int64_t)dw * dh;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(k / dw), x = (int)(k - (int64_t)y * dw);
        const float src_x = (float)x * fx, src_y = (float)y * fy;
        const int x1 = (int)floorf(src_x), y1 = (int)floorf(src_y);
        const int x2 = x1 + 1, y2 = y1 + 1;
        const int x2r = min(x2, sw - 1), y2r = min(y2, sh - 1);
        const uint32_t* r1 = reinterpret_cast<const uint32_t*>(rgba + (int64_t)y1 * spitch);
        const uint32_t* r2 = reinterpret_cast<const uint32_t*>(rgba + (int64_t)y2r * spitch);
        const uint32_t c00 = r1[x1], c01 = r1[x2r], c10 = r2[x1], c11 = r2[x2r];
        const float w00 = ((float)x2 - src_x) * ((float)y2 - src_y);
        const float w01 = (src_x - (float)x1) * ((float)y2 - src_y);
        const float w10 = ((float)x2 - src_x) * (src_y - (float)y1);
        const float w11 = (src_x - (float)x1) * (src_y - (float)y1);
        uint8_t* o3 = out + (int64_t)y * out_pitch + 3 * (int64_t)x;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const uint32_t sh8 = 8u * ch;
            float o = 0.f;
            o = __builtin_fmaf((float)((c00 >> sh8) & 255u), w00, o);
            o = __builtin_fmaf((float)((c01 >> sh8) & 255u), w01, o);
            o = __builtin_fmaf((float)((c10 >> sh8) & 255u), w10, o);
            o = __builtin_fmaf((float)((c11 >> sh8) & 255u), w11, o);
            o3[ch] = (uint8_t)sat_u8_rne(o);
        }
    }
}

hipError_t launch_resize_rgba_rgb(const uint8_t* rgba, int sw, int sh, int64_t spitch, uint8_t* out, int dw, int dh,
                                  int64_t out_pitch, hipStream_t s) {
    if (dw <= 0 || dh <= 0) return hipErrorInvalidValue;
    const float fx = (float)(1.0 / ((double)dw / sw)), fy = (float)(1.0 / ((double)dh / sh));
    const int64_t total = (int64_t)dw * dh;
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(resize_rgba_rgb_kernel, dim3(blocks), dim3(256), 0, s, rgba, sw, sh, spitch, fx, fy, out, dw, dh,
                       out_pitch);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Self-test: device saturating conversions (rint + clamp vs v_cvt_pk_u8_f32).
// ---------------------------------------------------------------------------------------------
__global__ void selftest_sat_kernel(const float* in, uint8_t* out, int n, int method) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = in[i];
    out[i] = method == 0 ? (uint8_t)sat_u8_rne(v) : (uint8_t)(__builtin_amdgcn_cvt_pk_u8_f32(v, 0, 0u) & 255u);
}

hipError_t launch_selftest_sat(const float* in, uint8_t* out, int n, int method, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(selftest_sat_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n, method);
    return hipGetLastError();
}

}  // namespace octvr
