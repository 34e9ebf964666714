// overlay_list.hpp — the work list of overlay_apply_kernel (kernels.hpp OverlayList) from the overlays'
// winner LUT: host arithmetic only, no HIP, so tests/cpp/overlay_list_check.cpp runs it under the
// sanitizers.  Internal header.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace octvr {

// E: an 8-byte entry {xy, code} (kernels.hpp CompositeEntry).
template <class E>
struct OverlayListBuild {
    std::vector<uint32_t> groups;  // x / 8 | y << 16, row-major
    std::vector<E> entries;        // 8 per group
    size_t covered = 0;            // pixels with the covered bit
};

// lut: W x H entries, `covered_bit` set in the code of every pixel some overlay writes.  Keeps the 8-pixel
// groups holding such a pixel, in row-major order; pixels of a kept group past the row's end are uncovered
// zero entries.  The list is padded with uncovered groups at (0, 0) to a multiple of block_groups (one
// workgroup's share), so the kernel needs no bound.
template <class E>
OverlayListBuild<E> build_overlay_list(const std::vector<E>& lut, int W, int H, uint32_t covered_bit, int block_groups) {
    OverlayListBuild<E> b;
    if (W <= 0 || H <= 0 || W > 8 * 65536 || H > 65536 || lut.size() < (size_t)W * H || block_groups < 1) return b;
    const int gw = (W + 7) / 8;
    for (int y = 0; y < H; y++)
        for (int g = 0; g < gw; g++) {
            const int x0 = 8 * g, nx = W - x0 < 8 ? W - x0 : 8;
            const E* row = lut.data() + (size_t)y * W + x0;
            int hit = 0;
            for (int i = 0; i < nx; i++) hit += (row[i].code & covered_bit) ? 1 : 0;
            if (!hit) continue;
            b.covered += (size_t)hit;
            b.groups.push_back((uint32_t)g | (uint32_t)y << 16);
            for (int i = 0; i < 8; i++) {
                E e{};
                if (i < nx && (row[i].code & covered_bit)) e = row[i];
                b.entries.push_back(e);
            }
        }
    while (b.groups.size() % (size_t)block_groups) {
        b.groups.push_back(0u);
        b.entries.insert(b.entries.end(), 8, E{});
    }
    return b;
}

}  // namespace octvr
