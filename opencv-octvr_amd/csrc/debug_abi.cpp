// debug_abi.cpp — the C ABI's test hooks (octvr_debug_*, the selftest and the LUT-build counter): host
// restatements and models the tests compare the product against.  Nothing here runs in a stitch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "async_host.hpp"
#include "camera_math.hpp"
#include "json_lite.hpp"
#include "mapper.hpp"

using namespace octvr;

extern "C" {

int octvr_debug_pack_runs(int n_inputs, const int* in_w, const int* in_h, const uint32_t* runs, int n_runs,
                          const uint8_t* const* planes, const size_t* pitches, int format, uint8_t* packed, size_t cap,
                          size_t* sizes, size_t* bytes) {
    return guarded([&] {
        REQUIRE(in_w && in_h && runs && planes && pitches && packed && bytes, "NULL argument");
        REQUIRE(n_inputs > 0 && n_inputs <= kMaxCams && n_runs >= 0, "bad counts");
        REQUIRE(format == OCTVR_PIX_YUV420P || format == OCTVR_PIX_NV12 || converted_format(format),
                "pixel format must be an OCTVR_PIX_* value");
        const LayoutDesc d = layout_of(format);
        for (int i = 0; i < n_inputs; i++) {
            REQUIRE(in_w[i] > 0 && in_h[i] > 0 && in_w[i] % 2 == 0 && in_h[i] % 2 == 0, "input sizes must be even");
            for (int k = 0; k < d.planes(); k++)
                REQUIRE(planes[3 * i + k] && pitches[3 * i + k] >= (size_t)d.plane_row_bytes(k, in_w[i]), "bad input plane");
        }
        size_t off = 0;
        for (int k = 0; k < n_runs; k++) {
            const uint32_t cam = runs[4 * k], rp = runs[4 * k + 1], g0 = runs[4 * k + 2], ng = runs[4 * k + 3];
            REQUIRE(cam < (uint32_t)n_inputs, "run: no such camera");
            const int w = in_w[cam], h = in_h[cam];
            REQUIRE(rp < (uint32_t)h / 2 && ng > 0 && g0 < (uint32_t)(w + 7) / 8 && ng <= (uint32_t)(w + 7) / 8 - g0,
                    "run outside its frame");
            const size_t n = d.run_bytes(w, (int)g0, (int)ng);
            REQUIRE(off + n <= cap, "buffer too small");
            const size_t got = pack_run(d, packed + off, w, (int)rp, (int)g0, (int)ng, planes + 3 * cam, pitches + 3 * cam);
            REQUIRE(got == n, "pack_run size");
            if (sizes) sizes[k] = got;
            off += got;
        }
        *bytes = off;
    });
}

int octvr_debug_mapper_uyvy_runs(const octvr_mapper* m, uint32_t* runs, size_t cap, size_t* count) {
    return guarded([&] {
        REQUIRE(m && count, "NULL argument");
        REQUIRE(m->conv_in && m->conv_fmt_in == OCTVR_PIX_UYVY422, "the mapper's input format is not OCTVR_PIX_UYVY422");
        *count = m->conv_foot_runs.size();
        if (!runs) return;
        REQUIRE(cap >= m->conv_foot_runs.size(), "buffer too small");
        for (size_t k = 0; k < m->conv_foot_runs.size(); k++) {
            const FootRun& r = m->conv_foot_runs[k];
            runs[4 * k] = r.cam & 31u;
            runs[4 * k + 1] = r.cam >> 8;
            runs[4 * k + 2] = r.g0;
            runs[4 * k + 3] = r.ng;
        }
    });
}

int octvr_debug_gain_plan(const octvr_rig* rig, int n_inputs, const int* in_w, const int* in_h, int flags,
                          uint32_t* samples, uint16_t* partners, size_t cap, size_t* count) {
    return guarded([&] {
        REQUIRE(rig && in_w && in_h && count, "bad arguments");
        REQUIRE((flags & ~OCTVR_REMAP_TEXTURE) == 0, "unknown mapper flags");
        const int n = (int)rig->inputs.size();
        REQUIRE(n_inputs == n && n > 0 && n <= kGainMaxCams, "in_sizes must cover the inputs");
        const GainPlan g = plan_gain(*rig, n, std::vector<int>(in_w, in_w + n), std::vector<int>(in_h, in_h + n),
                                     (flags & OCTVR_REMAP_TEXTURE) ? 1 : 0);
        *count = g.samples.size();
        if (!samples || !partners) return;
        REQUIRE(cap >= g.samples.size(), "buffer too small");
        for (size_t k = 0; k < g.samples.size(); k++) {
            samples[2 * k] = g.samples[k].xy;
            samples[2 * k + 1] = g.samples[k].code;
            partners[k] = g.partners[k];
        }
    });
}

int octvr_debug_tiled_lut_info(const octvr_rig* rig, int n_inputs, const int* in_w, const int* in_h, int flags,
                               char* json, size_t len) {
    return guarded([&] {
        REQUIRE(rig && in_w && in_h && json && len > 0, "bad arguments");
        REQUIRE((flags & ~OCTVR_REMAP_TEXTURE) == 0, "unknown mapper flags");
        const bool tex = (flags & OCTVR_REMAP_TEXTURE) != 0;
        const int n = (int)rig->inputs.size();
        REQUIRE(n_inputs == n && n > 0 && n <= kMaxCams, "in_sizes must cover the inputs");
        const int W = rig->out_w, H = rig->out_h;
        // the copy chain's winner per pixel (composite_lut_kernel on the host): the last camera whose ROI
        // holds the pixel and whose LUT mask is set
        std::vector<CompositeEntry> lut((size_t)W * H, CompositeEntry{0u, 0u});
        parallel_for((size_t)H, [&](size_t y) {
            for (int i = 0; i < n; i++) {
                const RigInput& in = rig->inputs[i];
                const int ry = (int)y - in.roi[1];
                if (ry < 0 || ry >= in.roi[3]) continue;
                for (int rx = 0; rx < in.roi[2]; rx++) {
                    const size_t k = (size_t)ry * in.roi[2] + rx;
                    if (!in.mask[k]) continue;
                    lut[y * W + (size_t)(rx + in.roi[0])] =
                        tex ? make_entry_tex(in.map1[k], in.map2[k], (float)in_w[i], (float)in_h[i], i)
                            : make_entry(in.map1[k], in.map2[k], (float)in_w[i], (float)in_h[i], i);
                }
            }
        });
        const TiledLutBuild b = build_frame_tiles(lut, W, H, std::vector<int>(in_w, in_w + n), std::vector<int>(in_h, in_h + n));
        const int qpl = b.qpl;
        double box_px = 0;
        for (int t = 0; t < b.n_items; t++)
            for (int j = 0; j < (int)(b.hdr[t].nslots & 0xFFu); j++)
                box_px += (double)b.slots[(size_t)t * kTileSlots + j].bw * b.slots[(size_t)t * kTileSlots + j].bh;
        // LDS bank model of the composite's reads and staging stores (MI355X_MICROARCH.md §LDS): per
        // wave-instruction and lane group, the busiest bank's distinct dword addresses; "extra" = the cycles
        // above one per group, as SQ_LDS_BANK_CONFLICT counts them.  Taps: two ds_read2_b32 per pixel (each
        // dword as a ds_read_b32: 2 x 32 lanes, bank (a/4) mod 32); weights: ds_read_b64 (2 x 32, mod 64);
        // staging: two ds_write_b128 per group (8 x 8 lanes, mod 32).
        double tap_cyc = 0, tap_extra = 0, wt_cyc = 0, wt_extra = 0, st_cyc = 0, st_extra = 0;
        {
            const int item_px = kTilePx * qpl;
            auto group_cost = [](const uint32_t* a, int n, int lanes, int banks, double& cyc, double& extra) {
                // a: n dword addresses per lane, lanes lanes in the group
                uint32_t seen[64][16];
                int cnt[64] = {};
                int mx = 0;
                for (int l = 0; l < lanes; l++)
                    for (int i = 0; i < n; i++) {
                        const uint32_t d = a[l * n + i], bk = d % (uint32_t)banks;
                        bool dup = false;
                        for (int k = 0; k < cnt[bk]; k++) dup |= seen[bk][k] == d;
                        if (!dup && cnt[bk] < 16) seen[bk][cnt[bk]++] = d;
                        mx = std::max(mx, cnt[bk]);
                    }
                cyc += std::max(mx, 1);
                extra += std::max(mx, 1) - 1;
            };
            uint32_t a[64 * 4];
            for (int t = 0; t < b.n_items; t++) {
                const TileHdr& hd = b.hdr[t];
                const uint32_t S = hd.stride & ((1u << kStrideBits) - 1u);
                const uint32_t* E = b.entries.data() + (size_t)t * item_px;
                for (int h = 0; h < qpl; h++)
                    for (int w = 0; w < 4; w++)
                        for (int p = 0; p < 4; p++) {
                            for (int half = 0; half < 2; half++) {
                                const uint32_t* e = E + (size_t)h * kTilePx + (size_t)(w * 64 + half * 32) * 4 + p;
                                for (int r = 0; r < 2; r++)
                                    for (int c = 0; c < 2; c++) {
                                        for (int l = 0; l < 32; l++)
                                            a[l] = (b.tex ? (e[l * 4] >> 17) & 0xFFFu : ((e[l * 4] >> 13) & 0x3FFFu) / 4u) + r * S + c;
                                        group_cost(a, 1, 32, 32, tap_cyc, tap_extra);
                                    }
                                if (b.tex) continue;  // the texture filter reads no weight table
                                for (int l = 0; l < 32; l++) {
                                    const uint32_t d = (0x4000u | (e[l * 4] & 0x1FF8u)) / 4u;
                                    a[2 * l] = d;
                                    a[2 * l + 1] = d + 1;
                                }
                                group_cost(a, 2, 32, 64, wt_cyc, wt_extra);
                            }
                        }
                const int ns = (int)(hd.nslots & 0xFFu), nch = (int)((hd.nslots >> 8) & 0xFFu);
                const TileSlot* ts = b.slots.data() + (size_t)t * kTileSlots;
                for (int c = 0; c < nch; c++) {
                    int j = 0;
                    for (int k = 1; k < ns; k++)
                        if (c >= (int)ts[k].chunk0) j = k;
                    const uint16_t* G = c < kGroupFirst ? b.grp0.data() + ((size_t)t * kGroupFirst + c) * 64
                                                        : b.grp1.data() + ((size_t)(hd.stride >> kStrideBits) + c - kGroupFirst) * 64;
                    for (int sgi = 0; sgi < 2; sgi++)  // the two 16-byte stores of a group
                        for (int grp = 0; grp < 8; grp++) {
                            int n = 0;
                            for (int l = grp * 8; l < grp * 8 + 8; l++) {
                                if (!(G[l] & kGroupValid)) continue;
                                const uint32_t d = ts[j].lds + (G[l] & 255u) * S + ((G[l] >> 8) & 31u) * 8u + 4u * sgi;
                                for (int i = 0; i < 4; i++) a[n * 4 + i] = d + i;
                                n++;
                            }
                            if (n) group_cost(a, 4, n, 32, st_cyc, st_extra);
                        }
                }
            }
        }
        // the composite's source footprint (what the AsyncMultiMapper uploads, gain samples aside)
        SourceFootprint fp;
        fp.init(std::vector<int>(in_w, in_w + n), std::vector<int>(in_h, in_h + n));
        footprint_add_tiles(fp, b);
        const double foot = fp.bytes();
        double frame_bytes = 0;
        for (int i = 0; i < n; i++) frame_bytes += 1.5 * in_w[i] * in_h[i];
        char tmp[1024];
        snprintf(tmp, sizeof tmp,
                 "{\"tex\": %d, \"footprint_bytes\": %.0f, \"frame_bytes\": %.0f, \"lds_model\": {\"tap_cycles\": %.0f, \"tap_extra\": %.0f, \"wtab_cycles\": %.0f, "
                 "\"wtab_extra\": %.0f, \"stage_cycles\": %.0f, \"stage_extra\": %.0f}, "
                 "\"items\": %d, \"wide_tiles\": %d, \"staged_px\": %.0f, \"box_px\": %.0f, \"staged_bytes\": %.0f, "
                 "\"source_bytes\": %.0f, \"grp1_entries\": %zu, ",
                 b.tex, foot, frame_bytes, tap_cyc, tap_extra, wt_cyc, wt_extra, st_cyc, st_extra, b.n_items, b.n_wide, b.staged_bytes / 2.0, box_px, b.staged_bytes, b.source_bytes,
                 b.grp1.size());
        std::string js = std::string(tmp) + b.stats + "}";
        REQUIRE(js.size() < len, "buffer too small");
        memcpy(json, js.c_str(), js.size() + 1);
    });
}

int octvr_debug_entry_pack(const uint32_t* entries, int n_quads, uint32_t stride, uint64_t* records, uint8_t* ok,
                           uint32_t* unpacked) {
    return guarded([&] {
        REQUIRE(entries && records && ok && unpacked && n_quads >= 0, "bad arguments");
        REQUIRE(stride < (1u << kStrideBits), "stride exceeds its header field");
        for (int q = 0; q < n_quads; q++) {
            ok[q] = quad_pack(entries + 4 * (size_t)q, stride, &records[q]) ? 1 : 0;
            quad_unpack(records[q], stride, unpacked + 4 * (size_t)q);
        }
    });
}

int octvr_debug_json_number(const char* json, int flags, double* value) {
    return guarded([&] {
        REQUIRE(json && value, "NULL argument");
        const JsonValue v = json_parse(json, (flags & OCTVR_JSON_EXACT) != 0);
        const JsonValue& n = v.kind == JsonValue::Array ? v[0] : v;
        *value = n.as_double();
    });
}

int octvr_debug_worker_failure(int n_threads, int failing) {
    return guarded([&] {
        REQUIRE(n_threads > 0 && n_threads <= 64, "bad arguments");
        run_threads((size_t)n_threads, [&](size_t t) {
            REQUIRE((int)t != failing, "worker " + std::to_string(t) + " failed (test hook)");
        });
    });
}

int octvr_rig_lut_recomputed(const octvr_rig* rig, int i, uint64_t* n) {
    return guarded([&] {
        REQUIRE(rig && n && i >= 0 && i < (int)rig->inputs.size(), "bad arguments");
        *n = rig->inputs[i].n_fragile;
    });
}

int octvr_debug_project_f64(const char* json, int out_w, int out_h, int input, int device, int where, double* x,
                            double* y, uint8_t* fragile) {
    return guarded([&] {
        REQUIRE(json && x && y && out_w > 0 && out_h > 0 && (where == 0 || where == 1), "bad arguments");
        JsonValue doc = json_parse(json);
        const CameraParams out_cam = camera_from_json(doc["output"]);
        const JsonValue& ins = doc["inputs"];
        REQUIRE(input >= 0 && input < (int)ins.size(), "bad input index");
        const JsonValue& cam = ins[(size_t)input];
        CameraParams c = camera_from_json(cam);
        std::vector<uint8_t> excl, incl;
        if (cam.has("options")) build_camera_masks(cam["options"], excl, incl);
        if (!excl.empty() || !incl.empty()) {
            c.sel = 0;
            c.width = cam["options"]["width"].as_int();
            c.height = cam["options"]["height"].as_int();
        }
        const size_t total = (size_t)out_w * out_h;
        if (where == 1) {  // host, glibc: the evaluation build_input uses for the fragile pixels
            c.excl = excl.empty() ? nullptr : excl.data();
            c.incl = nullptr;
            parallel_for((size_t)out_h, [&](size_t h) {
                for (int w = 0; w < out_w; w++)
                    project_output_to_input(out_cam, c, (double)w / out_w, (double)h / out_h, &x[h * out_w + w],
                                            &y[h * out_w + w]);
            });
            return;
        }
        REQUIRE(fragile, "fragile is NULL");
        DeviceGuard dg(device);
        DevBuf<uint8_t> excl_d;
        if (!excl.empty()) {
            excl_d.upload(excl.data(), excl.size());
            c.excl = excl_d.p;
        }
        c.incl = nullptr;
        const CameraParams both[2] = {out_cam, c};
        DevBuf<CameraParams> cams;
        cams.upload(both, 2);
        DevBuf<double> xd, yd;
        DevBuf<uint8_t> fd;
        xd.alloc(total);
        yd.alloc(total);
        fd.alloc(total);
        HIP_CHECK(launch_project_f64(cams.p, out_w, out_h, xd.p, yd.p, fd.p, nullptr));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(x, xd.p, total * sizeof(double), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(y, yd.p, total * sizeof(double), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(fragile, fd.p, total, hipMemcpyDeviceToHost));
    });
}

int octvr_debug_gain_solve(const double* A, const double* b, int n, int count, int lean, double* x, int* ok) {
    return guarded([&] {
        REQUIRE(A && b && x && ok, "NULL argument");
        REQUIRE(n >= 1 && n <= kGainMaxCams && count >= 1 && (lean == 0 || lean == 1), "bad arguments");
        const size_t nb = (size_t)count * n, nA = nb * n;
        DevBuf<double> Ad, bd, xd;
        DevBuf<int> okd;
        Ad.upload(A, nA);
        bd.upload(b, nb);
        xd.alloc(nb);
        okd.alloc((size_t)count);
        HIP_CHECK(launch_gain_solve(Ad.p, bd.p, n, count, lean != 0, xd.p, okd.p, nullptr));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(x, xd.p, nb * sizeof(double), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ok, okd.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    });
}

int octvr_selftest_sat_u8(const float* in,uint8_t* out, int n, int method, void* stream) {
    return guarded([&] {
        REQUIRE(in && out && n >= 0 && (method == 0 || method == 1), "bad arguments");
        HIP_CHECK(launch_selftest_sat(in, out, n, method, (hipStream_t)stream));
    });
}

}  // extern "C"
