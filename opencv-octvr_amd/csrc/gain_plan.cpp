// gain_plan.cpp — the working-scale gain setup of a mapper, computed on the host (plan_gain) and uploaded
// (setup_gain), with the host restatements of cuda::resize it needs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <vector>

#include "mapper.hpp"

namespace octvr {

namespace {

float resize_inv_scale(int d, int s) {
    // cudawarping/src/resize.cpp:82-83,105
    double f = (double)d / s;
    return (float)(1.0 / f);
}

// cuda::resize INTER_LINEAR on u8 (glob path, resize.cu:71-103); nvcc's default FMA contraction of
// `out + src * w` is reproduced with explicit fmaf.
std::vector<uint8_t> resize_linear_u8(const uint8_t* src, int sw, int sh, int dw, int dh) {
    std::vector<uint8_t> dst((size_t)dw * dh);
    float fx = resize_inv_scale(dw, sw), fy = resize_inv_scale(dh, sh);
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            float src_x = x * fx, src_y = y * fy;
            int x1 = (int)floorf(src_x), y1 = (int)floorf(src_y);
            int x2 = x1 + 1, y2 = y1 + 1;
            int x2r = std::min(x2, sw - 1), y2r = std::min(y2, sh - 1);
            float out = 0.f;
            out = fmaf((float)src[(size_t)y1 * sw + x1], (x2 - src_x) * (y2 - src_y), out);
            out = fmaf((float)src[(size_t)y1 * sw + x2r], (src_x - x1) * (y2 - src_y), out);
            out = fmaf((float)src[(size_t)y2r * sw + x1], (x2 - src_x) * (src_y - y1), out);
            out = fmaf((float)src[(size_t)y2r * sw + x2r], (src_x - x1) * (src_y - y1), out);
            int v = !(out > 0.f) ? 0 : out >= 255.f ? 255 : (int)rintf(out);
            dst[(size_t)y * dw + x] = (uint8_t)v;
        }
    return dst;
}

}  // namespace

// cuda::resize INTER_LINEAR on f32 (the texture LinearFilter path, filters.hpp:79-117, taken for an
// upscale without a stream): same taps and weights as resize_linear with clamped borders; nvcc's FMA
// contraction of `out + src * w` reproduced with explicit fmaf.
std::vector<float> resize_linear_f32(const float* src, int sw, int sh, int dw, int dh) {
    std::vector<float> dst((size_t)dw * dh);
    float fx = resize_inv_scale(dw, sw), fy = resize_inv_scale(dh, sh);
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            float src_x = x * fx, src_y = y * fy;
            int x1 = (int)floorf(src_x), y1 = (int)floorf(src_y);
            int x2 = x1 + 1, y2 = y1 + 1;
            int x2r = std::min(x2, sw - 1), y2r = std::min(y2, sh - 1);
            float out = 0.f;
            out = fmaf(src[(size_t)y1 * sw + x1], (x2 - src_x) * (y2 - src_y), out);
            out = fmaf(src[(size_t)y1 * sw + x2r], (src_x - x1) * (y2 - src_y), out);
            out = fmaf(src[(size_t)y2r * sw + x1], (x2 - src_x) * (src_y - y1), out);
            out = fmaf(src[(size_t)y2r * sw + x2r], (src_x - x1) * (src_y - y1), out);
            dst[(size_t)y * dw + x] = out;
        }
    return dst;
}

// Working-scale gain setup: Mapper ctor (mapper.cpp:94-114,140-142) + GainCompensatorGPU ctor
// (exposure_compensate.cpp:174-221).  Produces per-pair sample entries of both cameras for every
// pixel of the bitwise-AND intersection of the resized masks, N(i,j), and chunking — on the host only
// (plan_gain), then uploaded (setup_gain).
GainPlan plan_gain(const octvr_rig& rig, int n, const std::vector<int>& in_w, const std::vector<int>& in_h, int tex) {
    double ws = std::min(1.0, std::sqrt(0.1 * 1e6 / ((double)rig.out_w * rig.out_h)));
    std::vector<std::array<int, 4>> wr(n);
    std::vector<std::vector<uint8_t>> smask(n);
    std::vector<std::vector<CompositeEntry>> samp(n);
    std::vector<int32_t> N((size_t)n * n, 0);
    for (int i = 0; i < n; i++) {
        const RigInput& in = rig.inputs[i];
        wr[i] = {(int)(in.roi[0] * ws), (int)(in.roi[1] * ws), (int)(in.roi[2] * ws), (int)(in.roi[3] * ws)};
        const int ww = wr[i][2], wh = wr[i][3];
        REQUIRE(ww > 0 && wh > 0, "working-scale ROI is empty");
        smask[i] = resize_linear_u8(in.mask.data(), in.roi[2], in.roi[3], ww, wh);
        // warped -> working scale: resize_nearest (resize.cu:57-69), src index = trunc(dst * (float)(1/f))
        float fx = resize_inv_scale(ww, in.roi[2]), fy = resize_inv_scale(wh, in.roi[3]);
        samp[i].resize((size_t)ww * wh);
        for (int y = 0; y < wh; y++)
            for (int x = 0; x < ww; x++) {
                int sx = (int)(x * fx), sy = (int)(y * fy);
                size_t k = (size_t)sy * in.roi[2] + sx;
                // The feed reads the warped image, which the remap fills whatever the LUT mask says: a pixel
                // whose mask an include mask of another camera or of an overlay cleared (template.cpp:102-116)
                // still carries its in-image map value, and the linearly resized mask can be non-zero there.
                // Mask-0 pixels whose taps all lie outside the image stay zero samples: their taps read 0 either
                // way, so the sums are the same; this only keeps the sample order and the footprint of rigs
                // without cleared masks as they were.
                CompositeEntry e = tex ? make_entry_tex(in.map1[k], in.map2[k], (float)in_w[i], (float)in_h[i], i)
                                       : make_entry(in.map1[k], in.map2[k], (float)in_w[i], (float)in_h[i], i);
                if (!in.mask[k] && !tex) {
                    const TapCell c = tap_cell(e.xy, in_w[i], in_h[i]);
                    if (!((c.ix0 || c.ix1) && (c.iy0 || c.iy1))) e = CompositeEntry{0, 0};
                }
                samp[i][(size_t)y * ww + x] = e;
            }
        int nz = 0;
        for (uint8_t v : smask[i]) nz += v != 0;
        N[(size_t)i * n + i] = std::max(1, nz);
    }
    // samples: working pixel k of camera i joins I(i,j) (exposure_compensate.cpp:262-277) for every
    // camera j whose resized-mask intersection holds it -> one entry plus a partner bit per pixel
    std::vector<std::vector<uint16_t>> partner(n);
    for (int i = 0; i < n; i++) partner[i].assign(samp[i].size(), 0);
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) {
            const auto &a = wr[i], &b = wr[j];
            int x0 = std::max(a[0], b[0]), y0 = std::max(a[1], b[1]);
            int x1 = std::min(a[0] + a[2], b[0] + b[2]), y1 = std::min(a[1] + a[3], b[1] + b[3]);
            if (x1 <= x0 || y1 <= y0) {  // overlap_roi.area() == 0
                N[(size_t)i * n + j] = N[(size_t)j * n + i] = 1;
                continue;
            }
            int nz = 0;
            for (int y = y0; y < y1; y++)
                for (int x = x0; x < x1; x++) {
                    size_t ka = (size_t)(y - a[1]) * a[2] + (x - a[0]);
                    size_t kb = (size_t)(y - b[1]) * b[2] + (x - b[0]);
                    if ((smask[i][ka] & smask[j][kb]) == 0) continue;
                    nz++;
                    partner[i][ka] |= (uint16_t)(1u << j);
                    partner[j][kb] |= (uint16_t)(1u << i);
                }
            N[(size_t)i * n + j] = N[(size_t)j * n + i] = std::max(1, nz);
        }
    // per camera: the samples with a partner, ordered by (source row, source column) so the lanes of
    // a wave gather from a few neighbouring source lines; invalid (mask 0) samples read as 0 and go last
    std::vector<CompositeEntry> uniq;
    std::vector<uint16_t> pmask;
    int n_chunks = 0;  // workgroups of kGainChunk samples (4 single-camera wave runs each)
    for (int i = 0; i < n; i++) {
        std::vector<uint32_t> ks;
        for (size_t k = 0; k < samp[i].size(); k++)
            if (partner[i][k]) ks.push_back((uint32_t)k);
        auto key = [&](uint32_t k) {
            const CompositeEntry& e = samp[i][k];
            const uint64_t valid = (e.code & 0x8000u) ? 0 : 1;
            return (valid << 60) | ((uint64_t)(e.xy >> 16) << 24) | (uint64_t)(e.xy & 0xFFFFu);
        };
        std::stable_sort(ks.begin(), ks.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
        const int begin = (int)uniq.size();
        for (uint32_t k : ks) {
            CompositeEntry e = samp[i][k];
            if (!(e.code & 0x8000u)) e.code = (uint16_t)(i << 10);  // a zero sample of camera i
            uniq.push_back(e);
            pmask.push_back(partner[i][k]);
        }
        while ((uniq.size() - begin) % kGainWaveRun) {  // pad: invalid samples of camera i, no partners
            uniq.push_back(CompositeEntry{0u, (uint32_t)(i << 10)});
            pmask.push_back(0);
        }
    }
    while (uniq.size() % kGainChunk) {  // whole workgroups
        uniq.push_back(CompositeEntry{0u, 0u});
        pmask.push_back(0);
    }
    n_chunks = (int)(uniq.size() / kGainChunk);
    // exactness bound of the fixed-point totals (gain_feed.hip): < 2^21 samples per camera
    for (int i = 0; i < n; i++) REQUIRE(samp[i].size() < (1u << 21), "working-scale ROI too large for exact gain sums");
    GainPlan g;
    g.samples = std::move(uniq);
    g.partners = std::move(pmask);
    g.N = std::move(N);
    g.n_chunks = n_chunks;
    for (uint16_t pm : g.partners) g.pairs_px += (size_t)__builtin_popcount(pm);
    return g;
}

void setup_gain(octvr_mapper& m, const octvr_rig& rig) {
    const GainPlan g = plan_gain(rig, m.n, m.in_w, m.in_h, m.tex);
    for (const CompositeEntry& e : g.samples) m.foot.mark_taps(e);
    m.samples.upload(g.samples.data(), g.samples.size());
    m.partners.upload(g.partners.data(), g.partners.size());
    m.N.upload(g.N.data(), g.N.size());
    m.n_chunks = g.n_chunks;
    m.n_samples = (int)g.samples.size();
    m.n_entries = g.pairs_px;
}

}  // namespace octvr
