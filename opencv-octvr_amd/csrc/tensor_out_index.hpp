// tensor_out_index.hpp — which tensor elements a lane of the tensor kernels (tensor_out.hip) stores: host and
// device arithmetic, no HIP types, so tests/cpp/tensor_out_check.cpp runs the same functions under the
// sanitizers.  Internal header.
//
// A workgroup owns one segment of one tensor row: S consecutive pixels (fewer at the row's end), in all three
// planes.  It computes their bytes into LDS and then stores plane by plane.  A plane's share of the segment is
// cut relative to its own address, which has no alignment beyond the element size:
//   head: the elements before the first boundary of a wide store (4 elements: 4, 8 or 16 bytes), 0..3 of them,
//   wide: groups of 4 elements, each at such a boundary,
//   tail: what is left, 0..3 elements.
// Head and tail go element by element.  S is a multiple of 16, so every segment of a row has the row's phase.
// A plane has S / 4 + 2 slots, slot 0 the head, slots 1 .. S / 4 the wide groups in order (consecutive lanes
// store consecutive groups), the last slot the tail; lane t of the workgroup takes slot t % slots of plane
// t / slots.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define OCTVR_TENSOR_HD __host__ __device__
#else
#define OCTVR_TENSOR_HD
#endif

namespace octvr {

constexpr int kTensorGroup = 4;  // elements of a wide store

template <int S>
constexpr int tensor_slots() {
    static_assert(S > 0 && S % 16 == 0, "a segment keeps the row's phase for every element size");
    return S / kTensorGroup + 2;
}

// Elements of a plane's segment before the first wide-store boundary.  addr: the byte address of the segment's
// first element of that plane (a multiple of es); es: bytes per element (1, 2 or 4); n: elements in the segment.
OCTVR_TENSOR_HD inline int tensor_head(uint64_t addr, int es, int n) {
    const uint32_t v = (uint32_t)(kTensorGroup * es);
    const int head = (int)(((v - (uint32_t)(addr % v)) % v) / (uint32_t)es);
    return head < n ? head : n;
}

// Elements [first, first + len) of the segment; len == kTensorGroup: one wide store at an aligned address
// (head and tail are shorter), len == 0: nothing.
struct TensorSpan {
    int first, len;
};

template <int S>
OCTVR_TENSOR_HD inline TensorSpan tensor_item(int slot, int n, int head) {
    const int wide = (n - head) / kTensorGroup;
    if (slot == 0) return TensorSpan{0, head};
    if (slot <= S / kTensorGroup) return slot - 1 < wide ? TensorSpan{head + kTensorGroup * (slot - 1), kTensorGroup} : TensorSpan{0, 0};
    return TensorSpan{head + kTensorGroup * wide, n - head - kTensorGroup * wide};
}

// Segments of a row of w elements, and the elements of segment sx.
template <int S>
OCTVR_TENSOR_HD inline int tensor_segments(int w) {
    return (w + S - 1) / S;
}
template <int S>
OCTVR_TENSOR_HD inline int tensor_segment_len(int w, int sx) {
    const int left = w - sx * S;
    return left < S ? left : S;
}

}  // namespace octvr
