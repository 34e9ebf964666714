// preview_list.hpp — the tap list of preview_gather_kernel (kernels.hpp PreviewList) from a blend-0 mapper's
// winner LUT: host arithmetic only, no HIP, so tests/cpp/preview_list_check.cpp runs it under the
// sanitizers.  Internal header.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace octvr {

// One axis of cv::cuda::resize INTER_LINEAR as resize_rgba_rgb_kernel evaluates it (resize_kernels.hip): for
// destination coordinate x of d, over a source of s, the two source coordinates it reads — lo = floor(x f),
// hi = min(lo + 1, s - 1), f = (float)(1.0 / ((double)d / s)).  The weights come from the unclamped lo + 1
// and stay in the kernel.
struct PreviewAxis {
    float f = 0.f;
    std::vector<int> lo, hi;
};
inline PreviewAxis preview_axis(int d, int s) {
    PreviewAxis a;
    a.f = (float)(1.0 / ((double)d / s));
    a.lo.resize((size_t)d);
    a.hi.resize((size_t)d);
    for (int x = 0; x < d; x++) {
        const float src = (float)x * a.f;
        const int x1 = (int)floorf(src);
        a.lo[(size_t)x] = x1;
        a.hi[(size_t)x] = x1 + 1 < s - 1 ? x1 + 1 : s - 1;
    }
    return a;
}

// E: an 8-byte entry {xy, code} (kernels.hpp CompositeEntry).
template <class E>
struct PreviewListBuild {
    std::vector<E> entries;  // 4 per preview pixel, raster order, then the padding
    size_t pixels = 0;       // dw * dh
    float fx = 0.f, fy = 0.f;  // the axes' scales, which the kernel forms its coordinates and weights from
};

// lut: W x H entries (the composite's winner LUT; a pixel no camera claims is an entry that evaluates to
// black).  Entry 4 (y dw + x) + tap of the list is the LUT's entry of result pixel (y1, x1), (y1, x2r),
// (y2r, x1), (y2r, x2r) for tap 0..3 — the four result pixels resize_rgba_rgb_kernel reads for preview pixel
// (x, y), nothing de-duplicated.  The list is padded with zero entries (they claim nothing) to a multiple of
// block_entries, one workgroup's share, so the kernel loads without a bound.  Empty on bad arguments,
// including a size whose floor(x f) would leave the source (never for sizes below 2^23).
template <class E>
PreviewListBuild<E> build_preview_list(const std::vector<E>& lut, int W, int H, int dw, int dh, int block_entries) {
    PreviewListBuild<E> b;
    if (W <= 0 || H <= 0 || dw <= 0 || dh <= 0 || lut.size() < (size_t)W * H || block_entries < 4 || block_entries % 4)
        return b;
    const PreviewAxis ax = preview_axis(dw, W), ay = preview_axis(dh, H);
    if (ax.lo.back() > W - 1 || ay.lo.back() > H - 1) return b;
    b.pixels = (size_t)dw * dh;
    b.fx = ax.f;
    b.fy = ay.f;
    const size_t n = 4 * b.pixels, padded = (n + (size_t)block_entries - 1) / (size_t)block_entries * (size_t)block_entries;
    b.entries.reserve(padded);
    for (int y = 0; y < dh; y++) {
        const E* r1 = lut.data() + (size_t)ay.lo[(size_t)y] * W;
        const E* r2 = lut.data() + (size_t)ay.hi[(size_t)y] * W;
        for (int x = 0; x < dw; x++) {
            const int x1 = ax.lo[(size_t)x], x2r = ax.hi[(size_t)x];
            b.entries.push_back(r1[x1]);
            b.entries.push_back(r1[x2r]);
            b.entries.push_back(r2[x1]);
            b.entries.push_back(r2[x2r]);
        }
    }
    b.entries.resize(padded, E{});
    return b;
}

}  // namespace octvr
