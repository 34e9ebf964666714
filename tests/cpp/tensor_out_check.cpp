// tensor_out_check.cpp — the index arithmetic of the tensor kernels (csrc/tensor_out_index.hpp: tensor_head,
// tensor_item, the segments of a row), run on the CPU exactly as a workgroup's lanes run it, under the address
// and undefined-behaviour sanitizers (make lib/tensor_out_check; tests/test_tensor_out_host.py runs it).
//
// For every element size (1, 2, 4), every base alignment 0..15 that the element size divides, every width 1..40
// and a few around the segment sizes, and the segment sizes of the kernels (64, 256) and a small one (16) that
// cuts the short widths into several segments: the lanes of every workgroup of a row store each element of the
// row's three windows exactly once and nothing outside them; a wide store is 4 elements at an address that is a
// multiple of 4 elements; head and tail are at most 3 elements; consecutive slots store consecutive groups.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tensor_out_index.hpp"

using namespace octvr;

static long g_checks = 0;

#define CHECK(c)                                                                  \
    do {                                                                          \
        g_checks++;                                                               \
        if (!(c)) {                                                               \
            fprintf(stderr, "tensor_out_check: %s failed at line %d\n", #c, __LINE__); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

// One row of a tensor whose three planes start at byte `base`: plane stride and the row's offset are chosen so
// that the planes' rows have different phases.  Runs `threads` lanes per segment as the kernels do.
template <int S>
static void sweep_row(int es, int base, int w, int threads) {
    const int slots = tensor_slots<S>();
    CHECK(3 * slots <= threads);
    const int row_stride = w + 5, plane_stride = row_stride * 2 + w + 3;  // rows 0..2 of a plane, a gap after
    const int y = 1;
    const int guard = 8;  // elements before and after the buffer's used part
    const size_t total = (size_t)guard + 2 * (size_t)plane_stride + (size_t)y * row_stride + (size_t)w + guard;
    std::vector<int> hits(total, 0);
    const int nseg = tensor_segments<S>(w);
    CHECK(nseg >= 1 && (nseg - 1) * S < w && nseg * S >= w);
    int covered = 0;
    for (int sx = 0; sx < nseg; sx++) {
        const int n = tensor_segment_len<S>(w, sx);
        CHECK(n >= 1 && n <= S);
        covered += n;
        for (int tid = 0; tid < threads; tid++) {
            const int pl = tid / slots;
            if (pl >= 3) continue;
            const int slot = tid - pl * slots;
            const size_t e0 = (size_t)guard + (size_t)pl * plane_stride + (size_t)y * row_stride + (size_t)sx * S;
            const uint64_t addr = (uint64_t)base + (uint64_t)e0 * (uint64_t)es;
            const int head = tensor_head(addr, es, n);
            CHECK(head >= 0 && head <= 3 && head <= n);
            const TensorSpan sp = tensor_item<S>(slot, n, head);
            CHECK(sp.len >= 0 && sp.len <= kTensorGroup && sp.first >= 0 && sp.first + sp.len <= n);
            if (sp.len == kTensorGroup) {
                CHECK(slot >= 1 && slot <= S / kTensorGroup);
                CHECK((addr + (uint64_t)sp.first * es) % (uint64_t)(kTensorGroup * es) == 0);
                CHECK(sp.first == head + kTensorGroup * (slot - 1));  // consecutive slots, consecutive groups
            } else if (sp.len > 0) {
                CHECK(slot == 0 || slot == slots - 1);
                CHECK(sp.len <= 3);
            }
            for (int i = 0; i < sp.len; i++) hits[e0 + (size_t)sp.first + (size_t)i]++;
        }
    }
    CHECK(covered == w);
    for (size_t e = 0; e < total; e++) {
        bool inside = false;
        for (int pl = 0; pl < 3; pl++) {
            const size_t r0 = (size_t)guard + (size_t)pl * plane_stride + (size_t)y * row_stride;
            inside = inside || (e >= r0 && e < r0 + (size_t)w);
        }
        CHECK(hits[e] == (inside ? 1 : 0));
    }
}

int main() {
    const int widths_extra[] = {63, 64, 65, 127, 129, 255, 256, 257, 301, 513};
    for (int es = 1; es <= 4; es *= 2)
        for (int base = 0; base < 16; base += es) {
            for (int w = 1; w <= 40; w++) {
                sweep_row<16>(es, base, w, 64);
                sweep_row<64>(es, base, w, 256);
                sweep_row<256>(es, base, w, 256);
            }
            for (int w : widths_extra) {
                sweep_row<16>(es, base, w, 64);
                sweep_row<64>(es, base, w, 256);
                sweep_row<256>(es, base, w, 256);
            }
        }
    // the head of a segment shorter than its phase is the whole segment
    CHECK(tensor_head(1, 1, 2) == 2 && tensor_head(1, 1, 3) == 3 && tensor_head(1, 1, 4) == 3);
    CHECK(tensor_head(0, 4, 7) == 0 && tensor_head(4, 4, 7) == 3 && tensor_head(14, 2, 9) == 1);
    printf("tensor_out_check ok: %ld checks\n", g_checks);
    return 0;
}
