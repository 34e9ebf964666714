// async_kernels.hip — kernels of the AsyncMultiMapper pipeline (async.cpp) that are not the mappers' own.
// Kept apart from the gain feed and the composite: a kernel added to their translation units can change
// their code (DESIGN.md §4 "Source map").
#include "kernels.hpp"

namespace octvr {

// One workgroup per footprint run of an NV12 pipeline: the run's three packed rows of yb bytes (luma row
// 2r, luma row 2r + 1, chroma row r of U,V pairs) into the camera's NV12 frame ("Y over U,V pairs", pitch =
// width), all at byte column 8 g0.
//   8-byte path: the camera's width is a multiple of 8 (so yb = 8 ng and every group is whole) and the run's
//     packed offset is 8-byte aligned: one 8-byte load and one 8-byte store per group and row.  Source
//     (hipMalloc base + off + row * 8 ng + 8 g) and destination (hipMalloc base + row * w + 8 (g0 + g)) are
//     8-byte aligned by construction.
//   byte path: any other run, a byte per lane, including the partial last group of a width with w % 8 != 0.
// The branch depends on the run only: uniform over the workgroup.
// Bounds: a run has row pair r < h / 2 and groups inside the row (async.cpp footprint_runs), so the luma rows
// are 2r, 2r + 1 < h, the chroma row h + r < 3h / 2 and the columns [8 g0, 8 g0 + yb) end at or before w: every
// store lies in [f, f + w * 3h / 2).
__global__ void __launch_bounds__(256) unpack_runs_nv12_kernel(const uint8_t* __restrict__ packed,
                                                               const FootRun* __restrict__ runs, FootFrames fr) {
    const FootRun r = runs[blockIdx.x];
    const int cam = (int)(r.cam & 31u), rp = (int)(r.cam >> 8);
    const int w = fr.w[cam], h = fr.h[cam];
    const int x0 = 8 * (int)r.g0, yb = min(8 * (int)(r.g0 + r.ng), w) - x0;
    if (yb <= 0 || 2 * rp + 1 >= h) return;  // no such run is built; never store outside the frame
    const uint8_t* const src = packed + r.off;
    uint8_t* const f = fr.f[cam];
    uint8_t* const d0 = f + (size_t)(2 * rp) * (size_t)w + x0;
    uint8_t* const d1 = d0 + w;
    uint8_t* const dc = f + (size_t)(h + rp) * (size_t)w + x0;
    if ((w & 7) == 0 && (r.off & 7u) == 0) {
        const int ng = yb >> 3;
        for (int g = threadIdx.x; g < ng; g += 256) {
            const uint2 a = *reinterpret_cast<const uint2*>(src + 8 * g);
            const uint2 b = *reinterpret_cast<const uint2*>(src + yb + 8 * g);
            const uint2 c = *reinterpret_cast<const uint2*>(src + 2 * yb + 8 * g);
            *reinterpret_cast<uint2*>(d0 + 8 * g) = a;
            *reinterpret_cast<uint2*>(d1 + 8 * g) = b;
            *reinterpret_cast<uint2*>(dc + 8 * g) = c;
        }
        return;
    }
    const int tot = 3 * yb;
    for (int k = threadIdx.x; k < tot; k += 256) {
        uint8_t* d = k < yb ? d0 + k : k < 2 * yb ? d1 + (k - yb) : dc + (k - 2 * yb);
        *d = src[k];
    }
}

hipError_t launch_unpack_runs_layout(const uint8_t* packed, const FootRun* runs, int n_runs, const FootFrames& frames,
                                     int nv12, hipStream_t s) {
    if (!nv12) return launch_unpack_runs(packed, runs, n_runs, frames, s);
    if (n_runs <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_runs_nv12_kernel, dim3(n_runs), dim3(256), 0, s, packed, runs, frames);
    return hipGetLastError();
}

}  // namespace octvr
