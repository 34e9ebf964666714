// octvr_hip.cpp — C ABI (include/octvr_hip.h): rig (vr::MapperTemplate) and mapper (vr::Mapper).
//
// The entry points only: argument checks and calls into rig_json.cpp, rig_dat.cpp and mapper.cpp (the test
// hooks are in debug_abi.cpp).  Exceptions never cross the boundary: every entry point converts them into a
// status code + octvr_last_error() (abi_guard.hpp).
#include "octvr_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "json_lite.hpp"
#include "mapper.hpp"
#include "masks.hpp"

using namespace octvr;

extern "C" {

int octvr_abi_version(void) { return OCTVR_HIP_ABI_VERSION; }

const char* octvr_last_error(void) { return last_error().c_str(); }

int octvr_device_count(int* count) {
    return guarded([&] {
        REQUIRE(count, "count is NULL");
        HIP_CHECK(hipGetDeviceCount(count));
    });
}

int octvr_dev_malloc(int device, size_t bytes, void** ptr) {
    return guarded([&] {
        REQUIRE(ptr, "ptr is NULL");
        DeviceGuard dg(device);
        HIP_CHECK(hipMalloc(ptr, bytes));
    });
}

int octvr_dev_free(void* ptr) {
    return guarded([&] { HIP_CHECK(hipFree(ptr)); });
}

int octvr_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    return guarded([&] { HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); });
}

int octvr_fill_poly_u8(uint8_t* img, int w, int h, const int* pts, int npts, uint8_t color) {
    return guarded([&] {
        REQUIRE(img && w > 0 && h > 0 && (pts || npts == 0) && npts >= 0, "bad arguments");
        fill_poly_u8(img, w, h, pts, npts, color);
    });
}

int octvr_png_decode_rgb(const uint8_t* png, size_t n, uint8_t* rgb, size_t rgb_cap, int* w, int* h) {
    return guarded([&] {
        REQUIRE(png && w && h, "bad arguments");
        std::vector<uint8_t> v = png_decode_rgb(png, n, w, h);
        if (rgb) {
            REQUIRE(rgb_cap >= v.size(), "rgb buffer too small");
            memcpy(rgb, v.data(), v.size());
        }
    });
}

int octvr_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    return guarded([&] { HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); });
}

int octvr_stream_sync(void* stream) {
    return guarded([&] { HIP_CHECK(hipStreamSynchronize((hipStream_t)stream)); });
}

int octvr_rig_create_json(const char* json, int out_w, int out_h, int use_roi, int device, octvr_rig** out) {
    return guarded([&] {
        REQUIRE(json && out, "json/out is NULL");
        JsonValue doc = json_parse(json);
        auto rig = rig_new(doc["output"], out_w, out_h, device);
        // apps/octvr/dump.cpp:84-93: every input, then every overlay, through add_input
        const JsonValue& ins = doc["inputs"];
        for (size_t i = 0; i < ins.size(); i++) rig_add(*rig, ins[i], false, use_roi != 0);
        if (doc.has("overlays")) {
            const JsonValue& ov = doc["overlays"];
            for (size_t i = 0; i < ov.size(); i++) rig_add(*rig, ov[i], true, use_roi != 0);
        }
        *out = rig.release();
    });
}

int octvr_rig_create(const char* out_type, const char* out_opts_json, int out_w, int out_h, int device, int flags,
                     octvr_rig** out) {
    return guarded([&] {
        REQUIRE(out, "out is NULL");
        auto rig = rig_new(camera_json(out_type, out_opts_json, flags), out_w, out_h, device);
        *out = rig.release();
    });
}

int octvr_rig_add_input(octvr_rig* rig, const char* type, const char* opts_json, int overlay, int use_roi, int flags) {
    return guarded([&] {
        REQUIRE(rig, "rig is NULL");
        rig_add(*rig, camera_json(type, opts_json, flags), overlay != 0, use_roi != 0);
    });
}

int octvr_rig_create_from_arrays(int out_w, int out_h, int n, const int* rois, const float* const* map1,
                                 const float* const* map2, const uint8_t* const* masks,
                                 const uint8_t* const* seams, octvr_rig** out) {
    return guarded([&] {
        REQUIRE(out && rois && map1 && map2 && masks && n > 0 && out_w > 0 && out_h > 0, "bad arguments");
        auto rig = std::make_unique<octvr_rig>();
        rig->out_w = out_w;
        rig->out_h = out_h;
        rig->inputs.resize(n);
        for (int i = 0; i < n; i++) {
            RigInput& in = rig->inputs[i];
            memcpy(in.roi, rois + 4 * i, 4 * sizeof(int));
            REQUIRE(in.roi[0] >= 0 && in.roi[1] >= 0 && in.roi[2] > 0 && in.roi[3] > 0 &&
                        in.roi[0] <= out_w - in.roi[2] && in.roi[1] <= out_h - in.roi[3],  // no int overflow
                    "ROI outside the output frame");
            size_t k = (size_t)in.roi[2] * in.roi[3];
            in.map1.assign(map1[i], map1[i] + k);
            in.map2.assign(map2[i], map2[i] + k);
            in.mask.assign(masks[i], masks[i] + k);
        }
        if (seams) {
            rig->seam_masks.resize(n);
            for (int i = 0; i < n; i++) {
                size_t k = (size_t)rig->inputs[i].roi[2] * rig->inputs[i].roi[3];
                rig->seam_masks[i].assign(seams[i], seams[i] + k);
            }
        }
        *out = rig.release();
    });
}

int octvr_rig_load_dat(const char* path, octvr_rig** out) {
    return guarded([&] {
        REQUIRE(path && out, "path/out is NULL");
        std::ifstream f(path, std::ios::binary);
        if (!f) throw OctvrError(OCTVR_E_IO, std::string("cannot open ") + path);
        *out = dat_read(f).release();
    });
}

int octvr_rig_load_stream(octvr_read_fn read, void* ctx, octvr_rig** out) {
    return guarded([&] {
        REQUIRE(read && out, "read/out is NULL");
        *out = dat_read(read, ctx).release();
    });
}

int octvr_rig_create_masks(octvr_rig* rig, int device) {
    return guarded([&] {
        REQUIRE(rig, "rig is NULL");
        rig->device = device;
        rig_create_masks(*rig);
    });
}

int octvr_rig_dump_dat(octvr_rig* rig, const char* path) {
    return guarded([&] {
        REQUIRE(rig && path, "rig/path is NULL");
        if (rig->seam_masks.empty()) rig_create_masks(*rig);  // before opening: no half-written file on error
        std::ofstream f(path, std::ios::binary);
        if (!f) throw OctvrError(OCTVR_E_IO, std::string("cannot open ") + path);
        dat_write(*rig, f);
    });
}

int octvr_rig_dump_stream(octvr_rig* rig, octvr_write_fn write, void* ctx) {
    return guarded([&] {
        REQUIRE(rig && write, "rig/write is NULL");
        dat_write(*rig, write, ctx);
    });
}

int octvr_rig_set_vignette(octvr_rig* rig, int i, int overlay, const float* map, int w, int h) {
    return guarded([&] {
        REQUIRE(rig && i >= 0, "bad arguments");
        std::vector<RigInput>& v = overlay ? rig->overlays : rig->inputs;
        REQUIRE(i < (int)v.size(), "bad input index");
        REQUIRE(map ? (w > 0 && h > 0) : (w == 0 && h == 0), "bad vignette size");
        v[i].vignette.assign(map, map + (size_t)w * h);
        v[i].vig_w = w;
        v[i].vig_h = h;
    });
}

int octvr_rig_add_overlay_arrays(octvr_rig* rig, const int* roi, const float* map1, const float* map2,
                                 const uint8_t* mask) {
    return guarded([&] {
        REQUIRE(rig && roi && map1 && map2 && mask, "bad arguments");
        REQUIRE(rig->inputs.size() + rig->overlays.size() < (size_t)kMaxCams, "too many inputs");
        REQUIRE(roi[0] >= 0 && roi[1] >= 0 && roi[2] > 0 && roi[3] > 0 && roi[0] <= rig->out_w - roi[2] &&
                    roi[1] <= rig->out_h - roi[3],
                "ROI outside the output frame");
        RigInput in;
        memcpy(in.roi, roi, sizeof in.roi);
        const size_t k = (size_t)roi[2] * roi[3];
        in.map1.assign(map1, map1 + k);
        in.map2.assign(map2, map2 + k);
        in.mask.assign(mask, mask + k);
        rig->overlays.push_back(std::move(in));
    });
}

int octvr_rig_num_inputs(const octvr_rig* rig, int* n) {
    return guarded([&] {
        REQUIRE(rig && n, "NULL argument");
        *n = (int)rig->inputs.size();
    });
}

int octvr_rig_out_size(const octvr_rig* rig, int* w, int* h) {
    return guarded([&] {
        REQUIRE(rig && w && h, "NULL argument");
        *w = rig->out_w;
        *h = rig->out_h;
    });
}

int octvr_rig_get_input(const octvr_rig* rig, int i, octvr_input_view* v) {
    return guarded([&] {
        REQUIRE(rig && v && i >= 0 && i < (int)rig->inputs.size(), "bad input index");
        const RigInput& in = rig->inputs[i];
        v->roi_x = in.roi[0];
        v->roi_y = in.roi[1];
        v->roi_w = in.roi[2];
        v->roi_h = in.roi[3];
        v->map1 = in.map1.data();
        v->map2 = in.map2.data();
        v->mask = in.mask.data();
        v->seam_mask = i < (int)rig->seam_masks.size() ? rig->seam_masks[i].data() : nullptr;
        v->vignette = in.vignette.empty() ? nullptr : in.vignette.data();
        v->vignette_w = in.vig_w;
        v->vignette_h = in.vig_h;
    });
}

int octvr_rig_num_overlays(const octvr_rig* rig, int* n) {
    return guarded([&] {
        REQUIRE(rig && n, "NULL argument");
        *n = (int)rig->overlays.size();
    });
}

int octvr_rig_get_overlay(const octvr_rig* rig, int i, octvr_input_view* v) {
    return guarded([&] {
        REQUIRE(rig && v && i >= 0 && i < (int)rig->overlays.size(), "bad overlay index");
        const RigInput& in = rig->overlays[i];
        v->roi_x = in.roi[0];
        v->roi_y = in.roi[1];
        v->roi_w = in.roi[2];
        v->roi_h = in.roi[3];
        v->map1 = in.map1.data();
        v->map2 = in.map2.data();
        v->mask = in.mask.data();
        v->seam_mask = nullptr;
        v->vignette = in.vignette.empty() ? nullptr : in.vignette.data();
        v->vignette_w = in.vig_w;
        v->vignette_h = in.vig_h;
    });
}

int octvr_rig_morph_controlpoints(octvr_rig* rig, const char* control_points_json, int* n_used) {
    return guarded([&] {
        REQUIRE(rig && control_points_json, "NULL argument");
        if (rig->has_cameras && rig->out_cam_masks)
            throw OctvrError(OCTVR_E_UNSUPPORTED, "morph_controlpoints with output-camera masks is not implemented");
        const JsonValue cps = json_parse(control_points_json);
        const int k = rig_morph_controlpoints(*rig, cps);
        if (n_used) *n_used = k;
    });
}

int octvr_rig_get_triangles(const octvr_rig* rig, int i, float* src, float* dst, int cap, int* n) {
    return guarded([&] {
        REQUIRE(rig && n && i >= 0 && i < (int)rig->inputs.size(), "bad input index");
        const RigInput& in = rig->inputs[i];
        const int nt = (int)in.src_tris.size() / 6;
        *n = nt;
        if (src && dst) {
            REQUIRE(cap >= nt, "triangle buffer too small");
            std::copy(in.src_tris.begin(), in.src_tris.end(), src);
            std::copy(in.dst_tris.begin(), in.dst_tris.end(), dst);
        }
    });
}

void octvr_rig_destroy(octvr_rig* rig) { delete rig; }

int octvr_rig_clone(const octvr_rig* src, octvr_rig** out) {
    return guarded([&] {
        REQUIRE(src && out, "NULL argument");
        auto r = std::make_unique<octvr_rig>();
        r->out_w = src->out_w;
        r->out_h = src->out_h;
        r->device = src->device;
        r->inputs = src->inputs;
        r->overlays = src->overlays;
        r->seam_masks = src->seam_masks;
        r->has_cameras = src->has_cameras;
        r->out_cam_masks = src->out_cam_masks;
        r->out_cam = src->out_cam;
        r->cams = src->cams;
        if (src->visible.p) {  // the include-mask visibility state (template.cpp:86-116) travels with the copy
            DeviceGuard dg(src->device);
            r->visible.alloc(src->visible.n);
            HIP_CHECK(hipMemcpy(r->visible.p, src->visible.p, src->visible.n, hipMemcpyDeviceToDevice));
        }
        *out = r.release();
    });
}

int octvr_mapper_create(const octvr_rig* rig, int device, int n_inputs, const int* in_w, const int* in_h, int blend,
                        int enable_gain, int scale_w, int scale_h, octvr_mapper** out) {
    return octvr_mapper_create_ex(rig, device, n_inputs, in_w, in_h, blend, enable_gain, scale_w, scale_h, 0, out);
}

int octvr_mapper_create_ex(const octvr_rig* rig, int device, int n_inputs, const int* in_w, const int* in_h, int blend,
                           int enable_gain, int scale_w, int scale_h, int flags, octvr_mapper** out) {
    return guarded([&] {
        REQUIRE(out, "NULL argument");
        *out = mapper_create(rig, device, n_inputs, in_w, in_h, blend, enable_gain, scale_w, scale_h, flags).release();
    });
}

int octvr_mapper_stitch_yuv420p(octvr_mapper* m, const uint8_t* const* in_dev, const size_t* in_pitch,
                                uint8_t* out_dev, size_t out_pitch, const double* gains, int n_gains, void* stream) {
    return guarded([&] {
        mapper_stitch(m, in_dev, in_pitch, out_dev, out_pitch, gains, n_gains, nullptr, (hipStream_t)stream);
    });
}

int octvr_mapper_stitch_batch(octvr_mapper* m, int n_frames, const uint8_t* const* in_dev, const size_t* in_pitch,
                              uint8_t* const* out_dev, size_t out_pitch, const double* gains, void* stream) {
    return guarded([&] {
        mapper_stitch_batch(m, n_frames, in_dev, in_pitch, out_dev, out_pitch, gains, (hipStream_t)stream);
    });
}

int octvr_mapper_stitch_preview(octvr_mapper* m, const uint8_t* const* in_dev, const size_t* in_pitch,
                                uint8_t* out_dev, size_t out_pitch, uint8_t* preview_dev, int preview_w, int preview_h,
                                size_t preview_pitch, const double* gains, int n_gains, void* stream) {
    return guarded([&] {
        const PreviewOut pv{preview_dev, preview_w, preview_h, preview_pitch};
        mapper_stitch(m, in_dev, in_pitch, out_dev, out_pitch, gains, n_gains, nullptr, (hipStream_t)stream,
                      preview_dev ? &pv : nullptr);
    });
}

int octvr_mapper_stitch_tensor(octvr_mapper* m, const uint8_t* const* in_dev, const size_t* in_pitch, uint8_t* out_dev,
                               size_t out_pitch, const octvr_tensor_out* tensor, const double* gains, int n_gains,
                               void* stream) {
    return guarded([&] {
        REQUIRE(tensor && tensor->dev, "NULL tensor");
        mapper_stitch(m, in_dev, in_pitch, out_dev, out_pitch, gains, n_gains, nullptr, (hipStream_t)stream, nullptr, tensor);
    });
}

int octvr_mapper_prepare_preview(octvr_mapper* m, const octvr_rig* rig, int preview_w, int preview_h) {
    return guarded([&] { mapper_prepare_preview(m, rig, preview_w, preview_h); });
}

int octvr_mapper_gains(octvr_mapper* m, double* g, int n) {
    return guarded([&] {
        REQUIRE(m && g && n >= m->n, "bad arguments");
        DeviceGuard dg(m->device);
        if (!m->use_gain) {
            for (int i = 0; i < n; i++) g[i] = 1.0;
            return;
        }
        const octvr_mapper::FrameSlot& sl = m->slots[m->cur_slot];
        if (sl.done) HIP_CHECK(hipEventSynchronize(sl.done));
        HIP_CHECK(hipMemcpy(g, sl.gains, m->n * sizeof(double), hipMemcpyDeviceToHost));
    });
}

int octvr_mapper_set_frames_in_flight(octvr_mapper* m, int k) {
    return guarded([&] { mapper_set_frames_in_flight(m, k); });
}

int octvr_mapper_set_pixel_formats(octvr_mapper* m, int in_format, int out_format) {
    return guarded([&] {
        REQUIRE(m, "NULL argument");
        auto known = [](int f) {
            return f == OCTVR_PIX_YUV420P || f == OCTVR_PIX_NV12 || converted_format(f);
        };
        REQUIRE(known(in_format) && known(out_format),
                "pixel format must be OCTVR_PIX_YUV420P, OCTVR_PIX_NV12, OCTVR_PIX_UYVY422, OCTVR_PIX_YUYV422, "
                "OCTVR_PIX_YUV422P, OCTVR_PIX_NV16, OCTVR_PIX_P010, OCTVR_PIX_YUV420P10, OCTVR_PIX_P210, "
                "OCTVR_PIX_YUV422P10 or OCTVR_PIX_V210");
        DeviceGuard dg(m->device);
        mapper_sync(*m);  // stitches in flight keep the layouts they were issued with
        // a side in a converted layout is converted to or from NV12 frames of the frame slot: the stitch sees NV12 there
        mapper_set_conv(m, converted_format(in_format) ? in_format : 0, converted_format(out_format) ? out_format : 0);
        m->pix = (in_format != OCTVR_PIX_YUV420P ? kPixInNv12 : 0) | (out_format != OCTVR_PIX_YUV420P ? kPixOutNv12 : 0);
    });
}

int octvr_mapper_pixel_formats(const octvr_mapper* m, int* in_format, int* out_format) {
    return guarded([&] {
        REQUIRE(m && in_format && out_format, "NULL argument");
        *in_format = m->conv_in ? m->conv_fmt_in : (m->pix & kPixInNv12) ? OCTVR_PIX_NV12 : OCTVR_PIX_YUV420P;
        *out_format = m->conv_out ? m->conv_fmt_out : (m->pix & kPixOutNv12) ? OCTVR_PIX_NV12 : OCTVR_PIX_YUV420P;
    });
}

int octvr_mapper_traffic(const octvr_mapper* m, double* bytes) {
    return guarded([&] {
        REQUIRE(m && bytes, "NULL argument");
        *bytes = mapper_traffic(m);
    });
}

int octvr_mapper_traffic_parts(const octvr_mapper* m, double* lut_bytes, double* frame_bytes) {
    return guarded([&] {
        REQUIRE(m && lut_bytes && frame_bytes, "NULL argument");
        // multi-band has no batched kernels: everything is per frame
        *lut_bytes = m->mb ? 0.0 : tiled_lut_bytes(m->tiles.view, m->tiles.n_packed);
        *frame_bytes = mapper_traffic(m) - *lut_bytes;
    });
}

int octvr_mapper_set_timing(octvr_mapper* m, int enable) {
    return guarded([&] { mapper_set_timing(m, enable); });
}

int octvr_interval_union(const double* start, const double* end, int n, double* span, double* busy) {
    return guarded([&] {
        REQUIRE(n >= 0 && span && busy && (n == 0 || (start && end)), "bad arguments");
        std::vector<std::pair<double, double>> iv;
        double sp = 0;
        for (int k = 0; k < n; k++) {
            REQUIRE(end[k] >= start[k], "interval ends before it starts");
            iv.emplace_back(start[k], end[k]);
            sp += end[k] - start[k];
        }
        // sweep in start order: an interval that starts inside the current run extends it, one that
        // starts after it closes the run
        std::sort(iv.begin(), iv.end());
        double bz = 0;
        bool open = false;
        double ra = 0, rb = 0;
        for (const auto& x : iv) {
            if (open && x.first <= rb) {
                rb = std::max(rb, x.second);
            } else {
                if (open) bz += rb - ra;
                ra = x.first;
                rb = x.second;
                open = true;
            }
        }
        if (open) bz += rb - ra;
        *span = sp;
        *busy = bz;
    });
}

int octvr_mapper_kernel_time(octvr_mapper* m, double* total_ms, int* launches) {
    return guarded([&] {
        REQUIRE(m && total_ms && launches, "NULL argument");
        double t = 0;
        *launches = mapper_drain_timing(m, [&](double a, double b) { t += b - a; });
        *total_ms = t;
    });
}

int octvr_mapper_kernel_busy(octvr_mapper* m, double* span_ms, double* busy_ms, int* launches) {
    return guarded([&] {
        REQUIRE(m && span_ms && busy_ms && launches, "NULL argument");
        // [start, end] of every recorded launch relative to the first one's start (launches on several
        // streams may overlap): summed spans and the length of their union
        std::vector<double> st, en;
        *launches = mapper_drain_timing(m, [&](double a, double b) {
            st.push_back(a);
            en.push_back(b);
        });
        if (octvr_interval_union(st.data(), en.data(), (int)st.size(), span_ms, busy_ms) != OCTVR_OK)
            throw OctvrError(OCTVR_E_HIP, "kernel_busy: inconsistent event timestamps");
    });
}

int octvr_mapper_kernel_intervals(octvr_mapper* m, double* start_ms, double* end_ms, int cap, int* n) {
    return guarded([&] {
        REQUIRE(m && n && cap >= 0 && (cap == 0 || (start_ms && end_ms)), "bad arguments");
        int k = 0;
        *n = mapper_drain_timing(m, [&](double a, double b) {
            if (k < cap) {
                start_ms[k] = a;
                end_ms[k] = b;
            }
            k++;
        });
    });
}

int octvr_mapper_info(const octvr_mapper* m, char* buf, size_t len) {
    return guarded([&] {
        REQUIRE(m && buf && len > 0, "bad arguments");
        char tmp[768];
        snprintf(tmp, sizeof tmp,
                 "{\"inputs\": %d, \"out\": [%d, %d], \"blend\": %d, \"tiles\": %d, \"wide_tiles\": %d, "
                 "\"staged_bytes\": %.0f, \"source_bytes\": %.0f, \"gain\": %d, \"gain_samples\": %d, \"gain_pairs_px\": %zu, "
                 "\"gain_chunks\": %d, \"scaled_out\": [%d, %d], \"footprint_bytes\": %.0f, \"overlays\": %d, "
                 "\"overlay_groups\": %d, \"overlay_px\": %zu",
                 m->n, m->W, m->H, m->blend, m->n_tiles, m->tiles.view.n_wide,
                 m->mb ? 0.0 : m->tiles.staged_bytes, m->mb ? 0.0 : m->tiles.source_bytes, m->use_gain, m->n_samples, m->n_entries, m->n_chunks, m->SW, m->SH,
                 m->foot.bytes(), m->nc - m->n, m->ov.view.n_groups, m->ov.covered);
        std::string js = tmp;
        js += ", \"preview_prepared\": [" + std::to_string(m->pv.view.dw) + ", " + std::to_string(m->pv.view.dh) +
              "], \"preview_entries\": " + std::to_string(m->pv.view.n_entries);
        js += ", \"tensor_resized\": " + std::to_string(m->tensor_resized) + ", \"tensor_gathered\": " +
              std::to_string(m->tensor_gathered) + ", \"tensor_no_composite\": " + std::to_string(m->tensor_no_composite);
        // converted sides, per family of layouts (0: the side is not of the family): the footprint runs the unpack
        // launch converts and the packed bytes it reads per frame (run_bpp(): 4, 6 or 8 per pixel of a piece's row; v210:
        // the blocks that hold a run's pixels),
        // the bytes of the frame the pack launch writes
        const LayoutDesc li = layout_of(m->conv_in ? m->conv_fmt_in : 0), lo = layout_of(m->conv_out ? m->conv_fmt_out : 0);
        const struct {
            const char* prefix;
            bool (*is)(int pix, const LayoutDesc& d);
        } families[] = {{"uyvy", [](int pix, const LayoutDesc&) { return pix == OCTVR_PIX_UYVY422; }},
                        {"yuv422", [](int pix, const LayoutDesc& d) { return d.bytes == 1 && pix != OCTVR_PIX_UYVY422; }},
                        {"yuv10", [](int, const LayoutDesc& d) { return d.bytes == 2; }},
                        {"v210", [](int, const LayoutDesc& d) { return d.v210(); }}};
        for (const auto& f : families) {
            const bool i = m->conv_in && f.is(m->conv_fmt_in, li), o = m->conv_out && f.is(m->conv_fmt_out, lo);
            js += std::string(", \"") + f.prefix + "_runs\": " + std::to_string(i ? m->conv_runs : 0) + ", \"" + f.prefix +
                  "_in_bytes\": " + std::to_string(!i ? 0 : li.v210() ? m->conv_in_v210 : m->conv_in_px * (size_t)li.run_bpp()) + ", \"" + f.prefix +
                  "_out_bytes\": " + std::to_string(o ? (size_t)lo.row_bytes(m->SW) * (size_t)lo.rows(m->SH) : 0);
        }
        if (m->mb) js += ", " + multiband_info(*m->mb);
        else if (!m->tiles.stats.empty()) js += ", " + m->tiles.stats + ", \"items_packed\": " + std::to_string(m->tiles.n_packed);
        js += "}";
        REQUIRE(js.size() < len, "buffer too small");
        memcpy(buf, js.c_str(), js.size() + 1);
    });
}

void octvr_mapper_destroy(octvr_mapper* m) {
    if (!m) return;
    int prev = -1;
    if (hipGetDevice(&prev) == hipSuccess && prev != m->device) (void)hipSetDevice(m->device);
    delete m;
    if (prev >= 0) (void)hipSetDevice(prev);
}

int octvr_remap_u8(const uint8_t* src, int sw, int sh, size_t spitch, int cn, const float* map1, const float* map2,
                   int mw, int mh, size_t mpitch, float scale_x, float scale_y, uint8_t* dst, size_t dpitch,
                   void* stream) {
    return guarded([&] {
        REQUIRE(src && map1 && map2 && dst && sw > 0 && sh > 0 && mw >= 0 && mh >= 0, "bad arguments");
        REQUIRE(cn == 1 || cn == 3 || cn == 4, "cn must be 1, 3 or 4");
        if (mw == 0 || mh == 0) return;
        HIP_CHECK(launch_remap_u8(src, sw, sh, (int64_t)spitch, cn, map1, map2, mw, mh, (int64_t)mpitch, scale_x,
                                  scale_y, dst, (int64_t)dpitch, (hipStream_t)stream));
    });
}


}  // extern "C"
