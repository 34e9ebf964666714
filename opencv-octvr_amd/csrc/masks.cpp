// masks.cpp — per-camera exclude / include masks of `vr::Camera` (camera.cpp:72-123, 146-187), built
// once per rig on the host (the reference builds them on the CPU in the Camera constructor) and
// uploaded for lut_build_kernel's per-pixel lookups.
//
//  * polygonal areas: cv::fillPoly(mask, {points}, 255) with lineType 8, shift 0 (fill_poly.hpp);
//  * png areas: cv::imdecode(bytes, IMREAD_COLOR) (imgcodecs/src/grfmt_png.cpp:240-286: strip_16,
//    strip_alpha, palette_to_rgb, gray 1/2/4 -> 8 expansion, gray_to_rgb, interlace handling), red
//    channel -> exclude, green -> include (camera.cpp:174-178).
#include <zlib.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "masks.hpp"

namespace octvr {

// ---------------------------------------------------------------------------------------------
// PNG -> 8-bit RGB, as libpng delivers it to OpenCV's PngDecoder for IMREAD_COLOR.
// ---------------------------------------------------------------------------------------------
namespace {

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// Undo the per-row filters of one (sub-)image in place; returns the offset past it.
size_t unfilter(uint8_t* d, size_t avail, int w, int h, int bits_pp, std::vector<uint8_t>& rows) {
    const size_t stride = ((size_t)w * bits_pp + 7) / 8;
    const int bpp = std::max(1, bits_pp / 8);
    if (w == 0 || h == 0) return 0;
    REQUIRE(avail >= (stride + 1) * h, "png: truncated image data");
    std::vector<uint8_t> prev(stride, 0);
    rows.resize(stride * h);
    for (int y = 0; y < h; y++) {
        const uint8_t f = d[(stride + 1) * y];
        uint8_t* r = d + (stride + 1) * y + 1;
        for (size_t x = 0; x < stride; x++) {
            const int a = x >= (size_t)bpp ? r[x - bpp] : 0, b = prev[x], c = x >= (size_t)bpp ? prev[x - bpp] : 0;
            int v = r[x];
            switch (f) {
                case 0: break;
                case 1: v += a; break;
                case 2: v += b; break;
                case 3: v += (a + b) >> 1; break;
                case 4: v += paeth(a, b, c); break;
                default: throw OctvrError(OCTVR_E_INVALID, "png: bad filter type");
            }
            r[x] = (uint8_t)v;
        }
        memcpy(prev.data(), r, stride);
        memcpy(rows.data() + stride * y, r, stride);
    }
    return (stride + 1) * h;
}

}  // namespace

std::vector<uint8_t> png_decode_rgb(const uint8_t* buf, size_t n, int* out_w, int* out_h, int expect_w, int expect_h) {
    static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    REQUIRE(n >= 8 && memcmp(buf, sig, 8) == 0, "png: bad signature (only PNG masks are supported)");
    int w = 0, h = 0, depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t> idat, plte;
    for (size_t p = 8; p + 12 <= n;) {
        const uint32_t len = be32(buf + p);
        REQUIRE(p + 12 + (size_t)len <= n, "png: truncated chunk");
        const uint8_t* t = buf + p + 4;
        const uint8_t* d = buf + p + 8;
        if (!memcmp(t, "IHDR", 4)) {
            REQUIRE(len >= 13, "png: bad IHDR");
            w = (int)be32(d);
            h = (int)be32(d + 4);
            depth = d[8];
            ctype = d[9];
            interlace = d[12];
        } else if (!memcmp(t, "PLTE", 4)) {
            plte.assign(d, d + len);
        } else if (!memcmp(t, "IDAT", 4)) {
            idat.insert(idat.end(), d, d + len);
        } else if (!memcmp(t, "IEND", 4)) {
            break;
        }
        p += 12 + (size_t)len;
    }
    REQUIRE(w > 0 && h > 0, "png: missing IHDR");
    const int chans = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    REQUIRE(chans > 0, "png: bad colour type");
    // the colour type / bit depth pairs the PNG spec allows (libpng rejects the others, so
    // cv::imdecode fails and camera.cpp:175-176 asserts): gray 1/2/4/8/16, palette 1/2/4/8,
    // RGB / gray+alpha / RGBA 8/16
    const bool legal = ctype == 0   ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                       : ctype == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                                    : (depth == 8 || depth == 16);
    REQUIRE(legal, "png: bit depth not allowed for this colour type");
    // size check against the camera before anything is inflated or allocated
    if (expect_w > 0) REQUIRE(w == expect_w && h == expect_h, "png mask size differs from the camera's exclude mask");
    REQUIRE((uint64_t)w * (uint64_t)h <= ((uint64_t)1 << 28), "png: image too large for a mask");
    REQUIRE(ctype != 3 || !plte.empty(), "png: palette image without PLTE");
    const int bits_pp = chans * depth;
    // inflate the whole stream (its size is bounded by the passes' (stride + 1) * rows)
    size_t raw_n = 0;
    static const int ax0[7] = {0, 4, 0, 2, 0, 1, 0}, ay0[7] = {0, 0, 4, 0, 2, 0, 1};
    static const int adx[7] = {8, 8, 4, 4, 2, 2, 1}, ady[7] = {8, 8, 8, 4, 4, 2, 2};
    auto pass_dim = [&](int k, int* pw, int* ph) {
        *pw = interlace ? (w - ax0[k] + adx[k] - 1) / adx[k] : w;
        *ph = interlace ? (h - ay0[k] + ady[k] - 1) / ady[k] : h;
        if (*pw <= 0 || *ph <= 0) *pw = *ph = 0;
    };
    const int passes = interlace ? 7 : 1;
    for (int k = 0; k < passes; k++) {
        int pw, ph;
        pass_dim(k, &pw, &ph);
        if (pw) raw_n += (((size_t)pw * bits_pp + 7) / 8 + 1) * ph;
    }
    std::vector<uint8_t> raw(raw_n);
    uLongf got = (uLongf)raw_n;
    REQUIRE(uncompress(raw.data(), &got, idat.data(), (uLong)idat.size()) == Z_OK && got == raw_n,
            "png: corrupt image data");
    std::vector<uint8_t> rgb((size_t)w * h * 3), rows;
    size_t off = 0;
    for (int k = 0; k < passes; k++) {
        int pw, ph;
        pass_dim(k, &pw, &ph);
        if (!pw) continue;
        off += unfilter(raw.data() + off, raw_n - off, pw, ph, bits_pp, rows);
        const size_t stride = ((size_t)pw * bits_pp + 7) / 8;
        for (int y = 0; y < ph; y++) {
            const uint8_t* r = rows.data() + stride * y;
            for (int x = 0; x < pw; x++) {
                auto sample = [&](int c) -> int {  // channel c of pixel x, 8-bit (strip_16 keeps the high byte)
                    if (depth == 16) return r[((size_t)x * chans + c) * 2];
                    if (depth == 8) return r[(size_t)x * chans + c];
                    const int per = 8 / depth, sh = 8 - depth * (x % per + 1);
                    return (r[x / per] >> sh) & ((1 << depth) - 1);
                };
                uint8_t R, G, B;
                if (ctype == 3) {
                    const int idx = sample(0);
                    REQUIRE((size_t)idx * 3 + 2 < plte.size(), "png: palette index out of range");
                    R = plte[idx * 3];
                    G = plte[idx * 3 + 1];
                    B = plte[idx * 3 + 2];
                } else if (ctype == 0 || ctype == 4) {
                    int g = sample(0);
                    if (depth < 8) g = g * 255 / ((1 << depth) - 1);  // expand_gray_1_2_4_to_8
                    R = G = B = (uint8_t)g;
                } else {
                    R = (uint8_t)sample(0);
                    G = (uint8_t)sample(1);
                    B = (uint8_t)sample(2);
                }
                const int X = interlace ? ax0[k] + x * adx[k] : x, Y = interlace ? ay0[k] + y * ady[k] : y;
                uint8_t* o = rgb.data() + ((size_t)Y * w + X) * 3;
                o[0] = R;
                o[1] = G;
                o[2] = B;
            }
        }
    }
    *out_w = w;
    *out_h = h;
    return rgb;
}

}  // namespace octvr
