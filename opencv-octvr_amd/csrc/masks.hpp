// masks.hpp — host-side camera mask rasterisation (camera.cpp:72-123, 146-187); see masks.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fill_poly.hpp"  // fill_poly_u8: the polygonal areas

namespace octvr {

// cv::imdecode(png, IMREAD_COLOR) restricted to PNG; returns w*h*3 bytes in R,G,B order.
// expect_w > 0: the image must be expect_w x expect_h (checked on the IHDR, before inflating)
std::vector<uint8_t> png_decode_rgb(const uint8_t* buf, size_t n, int* w, int* h, int expect_w = 0, int expect_h = 0);

}  // namespace octvr
