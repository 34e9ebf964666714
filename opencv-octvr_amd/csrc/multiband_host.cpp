// multiband_host.cpp — host orchestration of the multi-band blend (Mapper blend > 0):
// MultiBandGPUBlender (stitching/src/blenders.cpp:589-735) laid out for the MI355X.
//
// Build (once per rig, all on `device`): the plan of multiband_plan.hpp (rectangles, weights' activity, pyrUp tap
// tables, sub-tile kinds, required tiles, work lists, remap jobs) from the rig and the f32 weight pyramid
// (levels 1..B = K4 pyrDown of seam / 255, multiband.hip), then its upload and the level-0 remap as a tiled
// composite LUT over the plan's (camera, required tile) jobs (tiling.cpp).
// Per frame: remap (+gain) -> pyrDown levels -> blend + collapse from the top level to level 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "kernels.hpp"
#include "multiband_plan.hpp"

namespace octvr {

static_assert(sizeof(MbItem) == sizeof(uint2) && alignof(MbItem) <= alignof(uint2), "MbItem is the device's uint2");

class MultiBand {
   public:
    int n = 0, B = 0, device = 0;
    int out_w = 0, out_h = 0;
    MbRect arr;  // the level-0 grid on the output frame
    MbPlan plan;  // its counts and per-tile sets, for multiband_traffic_parts and multiband_info
    struct Level {  // what a frame reads of the plan's level, and the level's device arrays
        int W = 0, H = 0, tx_n = 0, ty_n = 0;
        size_t g_bytes = 0;
        int n_work = -1, n_down = 0, rup_rows = 0;
        DevBuf<uint8_t> g;              // all cameras' Gaussian level (u8x4)
        DevBuf<MbCamLevel> cams;
        DevBuf<uint8_t> seam0;          // level 0: u8 seams over each align_roi
        DevBuf<float> wts;              // level > 0 (feather: level 0): f32 weights over each align_roi >> l
        DevBuf<uint32_t> tile_cams;
        DevBuf<uint2> work;             // multi-band: the sub-tiles mb_blend computes (kinds 0-2), MbBlendArgs::work
        DevBuf<UpQuad> up;              // per camera: rows then cols (level < B)
        DevBuf<UpQuad> rup;             // collapse: rows then cols (level < B)
        DevBuf<int32_t> up_org;         // per camera: staged-patch origins per tile row, then per tile col
        DevBuf<int32_t> rup_org;        // collapse: the same
        DevBuf<uint2> down_items;       // level > 0
        DevBuf<int16_t> R;              // level > 0: collapsed level, s16x4
    };
    std::vector<Level> lv;
    TiledLutDev remap;
    // frames in flight (octvr_mapper_set_frames_in_flight): slot k > 0 has its own Gaussian levels,
    // collapsed levels and remap work queue; everything else above is per rig and read-only per frame
    struct FrameBufs {
        std::vector<DevBuf<uint8_t>> g;
        std::vector<DevBuf<int16_t>> R;
        DevBuf<uint32_t> queue;
    };
    std::vector<std::unique_ptr<FrameBufs>> extra;
    bool feather = false;  // FeatherGPUBlender instead of MultiBandGPUBlender
    bool deep_in_remap = false;  // deep level-0 tiles are written by the remap (kItemResult, owned 4)
    bool full_cover = true;
    int crop_w = 0, crop_h = 0;
};

void MultiBandDeleter::operator()(MultiBand* p) const { delete p; }

namespace {

// The plan's stages report a bad rig as MbPlanError; the C ABI's status codes want an OctvrError.
template <class F>
void planned(F f) {
    try {
        f();
    } catch (const MbPlanError& e) {
        throw OctvrError(OCTVR_E_INVALID, e.what());
    }
}

// Level-0 weights to the device, then (multi-band) levels 1..B = K4 pyrDown in f32 on the device; returns the
// host copy of each level >= 1, the plan's input.
std::vector<std::vector<float>> weights_to_device(MultiBand& M, const MbPlan& P) {
    std::vector<std::vector<float>> upper(P.B + 1);
    if (P.feather) {
        M.lv[0].wts.upload(P.w0.data(), P.w0.size());
        return upper;
    }
    M.lv[0].seam0.upload(P.seam0.data(), P.seam0.size());
    DevBuf<float> f0;
    f0.upload(P.w0.data(), P.w0.size());
    for (int l = 1; l <= P.B; l++) {
        const auto &L = P.lv[l], &Lp = P.lv[l - 1];
        const float* prev = l == 1 ? f0.p : M.lv[l - 1].wts.p;
        M.lv[l].wts.alloc(L.n_weights);
        for (int i = 0; i < P.n; i++)
            HIP_CHECK(launch_pyr_down_f32(prev + Lp.cams[i].w_off, Lp.cams[i].w, Lp.cams[i].h,
                                          M.lv[l].wts.p + L.cams[i].w_off, L.cams[i].w, L.cams[i].h, nullptr));
        upper[l].resize(L.n_weights);
        HIP_CHECK(hipMemcpy(upper[l].data(), M.lv[l].wts.p, L.n_weights * sizeof(float), hipMemcpyDeviceToHost));
    }
    return upper;
}

// Every device array of the plan (the weights are up already), and the cameras' records pointing into them.
void upload_plan(MultiBand& M, const MbPlan& P) {
    for (int l = 0; l <= P.B; l++) {
        const auto& L = P.lv[l];
        auto& D = M.lv[l];
        D.W = L.W, D.H = L.H, D.tx_n = L.tx_n, D.ty_n = L.ty_n;
        D.g_bytes = L.g_bytes, D.n_work = L.n_work, D.n_down = (int)L.down_items.size(), D.rup_rows = L.rup_rows;
        D.g.alloc(L.g_bytes);
        D.tile_cams.upload(L.tile_cams.data(), L.tile_cams.size());
        D.work.upload(reinterpret_cast<const uint2*>(L.work.data()), L.work.size());
        D.up.upload(L.up.data(), L.up.size());
        D.rup.upload(L.rup.data(), L.rup.size());
        D.up_org.upload(L.up_org.data(), L.up_org.size());
        D.rup_org.upload(L.rup_org.data(), L.rup_org.size());
        if (l >= 1) {
            D.down_items.upload(reinterpret_cast<const uint2*>(L.down_items.data()), L.down_items.size());
            D.R.alloc((size_t)L.W * L.H * 4);
        }
        std::vector<MbCamLevel> cams(P.n);
        for (int i = 0; i < P.n; i++) {
            const MbPlanCam& c = L.cams[i];
            MbCamLevel& d = cams[i];
            memset(&d, 0, sizeof d);
            d.g_off = c.g_off, d.g_pitch = c.g_pitch;
            d.ox = c.ox, d.oy = c.oy, d.w = c.w, d.h = c.h;
            d.weight = l == 0 && !P.feather ? (const void*)(D.seam0.p + c.w_off) : (const void*)(D.wts.p + c.w_off);
            if (l < P.B) {
                d.up_rows = D.up.p + c.up_rows;
                d.up_cols = D.up.p + c.up_cols;
                d.up_r0 = D.up_org.p + c.up_org;
                d.up_c0 = D.up_org.p + c.up_org + L.ty_n;
            }
        }
        D.cams.upload(cams.data(), cams.size());
    }
}

// The level-0 remap as a tiled composite LUT over the plan's jobs.
void build_remap(MultiBand& M, const MbPlan& P, const octvr_rig& rig, const std::vector<int>& in_w,
                 const std::vector<int>& in_h, int qpl, SourceFootprint* foot, int tex) {
    std::vector<TileJob> jobs;
    for (const MbRemapJob& j : P.jobs) jobs.push_back(TileJob{j.tx, j.ty, j.cam, j.flags});
    const MbRect arr = P.arr;
    auto entry = [&](int job, int x, int y) -> CompositeEntry {
        const int i = jobs[job].cam;
        const RigInput& in = rig.inputs[i];
        const int X = x + arr.x, Y = y + arr.y;
        const int rx = X - in.roi[0], ry = Y - in.roi[1];
        if (rx < 0 || ry < 0 || rx >= in.roi[2] || ry >= in.roi[3]) return CompositeEntry{0u, 0u};
        const size_t k = (size_t)ry * in.roi[2] + rx;
        const float m1 = in.map1[k], m2 = in.map2[k];
        auto mk = [&]() {
            return tex ? make_entry_tex(m1, m2, (float)in_w[i], (float)in_h[i], i)
                       : make_entry(m1, m2, (float)in_w[i], (float)in_h[i], i);
        };
        if (in.mask[k]) return mk();
        // LUT mask 0: the remap still runs there, without gain (mul_scalar_with_mask); a template's
        // -1 maps put every tap outside the image (black; fastRemap's fill_zero in the texture
        // convention), other values follow the remap's rule
        CompositeEntry e = mk();
        e.code |= kCodeNoGain;
        return e;
    };
    TiledLutBuild tb = build_tiled_lut(jobs, entry, in_w, in_h, qpl);
    if (foot) footprint_add_tiles(*foot, tb);
    M.remap.upload(tb, true);
}

}  // namespace

MultiBand* multiband_create(const octvr_rig& rig, int device, int bands, const std::vector<int>& in_w,
                            const std::vector<int>& in_h, int feather_border, SourceFootprint* foot, int tex) {
    auto mb = std::unique_ptr<MultiBand>(new MultiBand);
    MultiBand& M = *mb;
    MbPlan& P = M.plan;
    // (OCTVR_MB_NO_DEEP=1, OCTVR_MB_NO_REMAP_RESULT=1: measurement / cross-check knobs, mb_classify)
    MbPlanOptions opt;
    opt.no_deep = std::getenv("OCTVR_MB_NO_DEEP") != nullptr;
    opt.no_remap_result = std::getenv("OCTVR_MB_NO_REMAP_RESULT") != nullptr;
    opt.qpl = composite_qpl();
    const bool feather = feather_border > 0;
    const int n = (int)rig.inputs.size();
    std::vector<MbRect> rois;
    for (auto& in : rig.inputs) rois.push_back(MbRect{in.roi[0], in.roi[1], in.roi[2], in.roi[3]});
    planned([&] { mb_plan_rects(P, rois, rig.out_w, rig.out_h, bands, feather); });
    if (feather) {  // distanceTransform(mask_i, L2, 3) of every camera
        std::vector<std::vector<float>> dist(n);
        run_threads((size_t)n, [&](size_t i) {
            dist[i].resize((size_t)rois[i].w * rois[i].h);
            chamfer_l2_3x3(rig.inputs[i].mask.data(), rois[i].w, rois[i].h, dist[i].data());
        });
        mb_feather_weights(P, rois, std::move(dist), feather_border);
    } else {
        planned([&] { mb_seam_weights(P, rois, rig.seam_masks); });
    }
    M.n = n, M.B = P.B, M.device = device, M.feather = feather;
    M.out_w = rig.out_w, M.out_h = rig.out_h;
    M.arr = P.arr, M.crop_w = P.crop_w, M.crop_h = P.crop_h, M.full_cover = P.full_cover;

    DeviceGuard dg(device);
    M.lv.resize(P.B + 1);
    const std::vector<std::vector<float>> upper = weights_to_device(M, P);
    planned([&] { mb_plan(P, upper, opt); });
    M.deep_in_remap = P.n_result > 0;
    upload_plan(M, P);
    build_remap(M, P, rig, in_w, in_h, opt.qpl, foot, tex);
    P.drop_tables();
    return mb.release();
}

void multiband_set_slots(MultiBand& M, int k) {
    M.extra.clear();
    for (int i = 1; i < k; i++) {
        auto f = std::make_unique<MultiBand::FrameBufs>();
        f->g.resize(M.lv.size());
        f->R.resize(M.lv.size());
        for (size_t l = 0; l < M.lv.size(); l++) {
            f->g[l].alloc(M.lv[l].g.n);
            f->R[l].alloc(M.lv[l].R.n);
        }
        f->queue.alloc(M.remap.queue.n);
        HIP_CHECK(hipMemset(f->queue.p, 0, f->queue.n * sizeof(uint32_t)));
        M.extra.push_back(std::move(f));
    }
}

void multiband_run(MultiBand& M, int slot, const FrameSet& frames, const double* gains_dev, int use_gain, uint8_t* out,
                   int64_t out_pitch, hipStream_t s, uint8_t* rgba, int64_t rgba_pitch, int pix) {
    const bool out_nv12 = !rgba && (pix & kPixOutNv12);
    REQUIRE(slot >= 0 && slot <= (int)M.extra.size(), "bad frame slot");
    MultiBand::FrameBufs* fb = slot ? M.extra[slot - 1].get() : nullptr;
    auto G = [&](int l) { return fb ? fb->g[l].p : M.lv[l].g.p; };
    auto Rl = [&](int l) { return fb ? fb->R[l].p : M.lv[l].R.p; };
    auto& L0 = M.lv[0];
    TiledLut view = M.remap.view;
    if (fb) view.queue = fb->queue.p;
    // (first: the remap writes the deep tiles' results into the output)
    if (!M.full_cover) {  // result pixels outside the blended ROI stay 0 (mapper.cpp:155): Y 0, U = V = 128
        if (rgba) {
            HIP_CHECK(hipMemset2DAsync(rgba, rgba_pitch, 0, (size_t)M.out_w * 4, M.out_h, s));
        } else {
            HIP_CHECK(hipMemset2DAsync(out, out_pitch, 0, M.out_w, M.out_h, s));
            HIP_CHECK(hipMemset2DAsync(out + (int64_t)M.out_h * out_pitch, out_pitch, 128, M.out_w, M.out_h / 2, s));
        }
    }
    RgbaOut ro{};
    ro.base = G(0);
    ro.bytes = (uint32_t)L0.g_bytes;
    ro.cams = L0.cams.p;
    if (M.deep_in_remap) {  // the result frame from the level-0 grid origin (align_result_roi's top-left)
        if (rgba) {
            const int64_t o = (int64_t)M.arr.y * rgba_pitch + (int64_t)M.arr.x * 4;
            const int64_t total = rgba_pitch * M.out_h;
            REQUIRE(total < ((int64_t)1 << 31) - 64 && rgba_pitch < ((int64_t)1 << 31), "result image exceeds 2 GiB");
            ro.res = rgba + o;
            ro.res_bytes = (uint32_t)(total - o);
            ro.res_pitch = (uint32_t)rgba_pitch;
            ro.res_rgba = 1;
        } else {
            const int64_t o = (int64_t)M.arr.y * out_pitch + M.arr.x;
            const int64_t total = out_pitch * (M.out_h + M.out_h / 2);
            REQUIRE(total < ((int64_t)1 << 31) - 64, "output frame exceeds 2 GiB");
            // (NV12: the U,V pair of luma column x at chroma byte x & ~1, and res_v_off = 0 says so)
            const int64_t u = (int64_t)M.out_h * out_pitch + (int64_t)(M.arr.y / 2) * out_pitch +
                              (out_nv12 ? (M.arr.x & ~1) : M.arr.x / 2);
            ro.res = out + o;
            ro.res_bytes = (uint32_t)(total - o);
            ro.res_pitch = (uint32_t)out_pitch;
            ro.res_u_off = (uint32_t)(u - o);
            ro.res_v_off = out_nv12 ? 0u : (uint32_t)(u - o + M.out_w / 2);
        }
    }
    HIP_CHECK(launch_mb_remap(frames, view, gains_dev, use_gain, ro, s, pix));
    for (int l = 1; l <= M.B; l++) {
        auto& L = M.lv[l];
        HIP_CHECK(launch_mb_down(L.down_items.p, L.n_down, L.cams.p, M.lv[l - 1].cams.p, G(l - 1), G(l), s));
    }
    for (int l = M.B; l >= 0; l--) {
        auto& L = M.lv[l];
        MbBlendArgs a{};
        a.level = l;
        a.bands = M.B;
        a.n_cams = M.n;
        a.w_u8 = l == 0 && !M.feather;
        a.feather = M.feather;
        a.out_scale = (float)(1.0 / M.n);
        a.W = L.W;
        a.H = L.H;
        a.tiles_x = L.tx_n;
        a.tile_cams = L.tile_cams.p;
        a.owned = nullptr;  // (the tile kinds travel in the work list)
        a.work = L.n_work >= 0 ? L.work.p : nullptr;
        a.n_work = L.n_work;
        a.cams = L.cams.p;
        a.g = G(l);
        if (l < M.B) {
            auto& Ln = M.lv[l + 1];
            a.cams_next = Ln.cams.p;
            a.g_next = G(l + 1);
            a.r_next = Rl(l + 1);
            a.W_next = Ln.W;
            a.H_next = Ln.H;
            a.rup_rows = L.rup.p;
            a.rup_cols = L.rup.p + L.rup_rows;
            a.rup_r0 = L.rup_org.p;
            a.rup_c0 = L.rup_org.p + L.ty_n;
        }
        if (l > 0) {
            a.r_out = Rl(l);
        } else {
            a.out = out;
            a.out_pitch = out_pitch;
            a.out_nv12 = out_nv12 ? 1 : 0;
            a.out_w = M.out_w;
            a.out_h = M.out_h;
            a.ax = M.arr.x;
            a.ay = M.arr.y;
            a.crop_w = M.crop_w;
            a.crop_h = M.crop_h;
            a.rgba = rgba;
            a.rgba_pitch = rgba_pitch;
        }
        HIP_CHECK(launch_mb_blend(a, s));
    }
}

// Algorithmic bytes per frame, per launch of the sequence: what each launch must move, every byte
// counted once per launch that needs it (re-reads of a neighbour's halo from L2 are not counted).
//   remap:   4 B tiled entry per item pixel (8 B wide), the G0 halves it writes (4 B / px), the deep
//            tiles' results (1.5 B / px YUV420P), the unique source bytes of its staged boxes, metadata;
//   down l:  4 B written per level-l item pixel, its level-(l-1) source window with the 5 x 5 halo
//            (20 x 260 pixels of 4 B per 128 x 8 item);
//   blend l: per sub-tile by kind — unread (owned 3): nothing; deep (2): G 4 B + R 8 B (level 0: nothing
//            when the remap wrote it, else 1.5 B out); owned (1): G 4 B + coarser G taps 1 B + collapsed
//            coarser level 2 B + R 8 B / out 1.5 B; general: per weighted camera G 4 B + weight (1 B u8
//            seam at level 0, else 4 B f32) + coarser G 1 B, then coarser R 2 B + R 8 B / out 1.5 B.
std::vector<std::pair<std::string, double>> multiband_traffic_parts(const MultiBand& M) {
    std::vector<std::pair<std::string, double>> parts;
    const TiledLut& t = M.remap.view;
    const TiledLutDev& r = M.remap;
    parts.emplace_back("remap", (t.e24 ? 3.0 : 4.0) * t.n_items * kTilePx * t.qpl + 8.0 * t.n_wide * kTilePx + r.g0_bytes +
                                    1.5 * r.result_bytes + r.source_bytes +
                                    (double)t.n_items * (sizeof(TileHdr) + kTileSlots * sizeof(TileSlot)));
    // down l: per item its (2 kTileH + 4) x (2 kTileW + 4) source window (the 5 x 5 support's halo) and the
    // tile it writes
    for (int l = 1; l <= M.B; l++)
        parts.emplace_back("down" + std::to_string(l),
                           (double)M.lv[l].n_down * (4.0 * (2 * kTileH + 4) * (2 * kTileW + 4) + 4.0 * kTilePx));
    for (int l = M.B; l >= 0; l--) {
        const auto& L = M.plan.lv[l];
        const bool up = l < M.B;
        const double out_b = l ? 8.0 : 1.5;
        // per sub-tile (multi-band) or per tile (feather: every tile general)
        const bool sub = !L.sub_own.empty();
        const std::vector<uint32_t>& cams = sub ? L.sub_cams : L.tile_cams;
        const double unit_px = sub ? (double)kSubW * kTileH : (double)kTilePx;
        double b = 0;
        for (size_t k = 0; k < cams.size(); k++) {
            const uint32_t m = cams[k];
            const int o = sub ? L.sub_own[k] : 0;
            double px_b = 0;
            if (o == 3) {
                px_b = 0;
            } else if (o == 4) {
                px_b = 0;  // level 0: the remap wrote the result
            } else if (o == 2) {
                px_b = 4.0 + out_b;
            } else if (o == 1) {
                px_b = 4.0 + (up ? 1.0 + 2.0 : 0.0) + out_b;
            } else if (m) {
                px_b = __builtin_popcount(m) * (4.0 + ((l == 0 && !M.feather) ? 1.0 : 4.0) + (up ? 1.0 : 0.0)) +
                       (up ? 2.0 : 0.0) + out_b;
            } else {
                px_b = (up ? 2.0 : 0.0) + out_b;  // no camera: the collapse alone
            }
            b += px_b * unit_px;
        }
        parts.emplace_back("blend" + std::to_string(l), b);
    }
    return parts;
}

double multiband_traffic(const MultiBand& M) {
    double b = 0;
    for (const auto& p : multiband_traffic_parts(M)) b += p.second;
    return b;
}

std::string multiband_info(const MultiBand& M) {
    std::string s = std::string(M.feather ? "\"feather\": 1, " : "") + "\"bands\": " + std::to_string(M.B) + ", \"align_result_roi\": [" + std::to_string(M.plan.arr_ref.x) + ", " +
                    std::to_string(M.plan.arr_ref.y) + ", " + std::to_string(M.plan.arr_ref.w) + ", " + std::to_string(M.plan.arr_ref.h) +
                    "], \"grid_roi\": [" + std::to_string(M.arr.x) + ", " + std::to_string(M.arr.y) + ", " +
                    std::to_string(M.arr.w) + ", " + std::to_string(M.arr.h) + "], \"full_cover\": " +
                    std::to_string(M.full_cover ? 1 : 0) + ", \"crop\": [" + std::to_string(M.crop_w) + ", " +
                    std::to_string(M.crop_h) + "], \"remap_items\": " + std::to_string(M.remap.view.n_items) +
                    ", \"remap_wide\": " + std::to_string(M.remap.view.n_wide) +
                    ", \"remap_entry_bits\": " + std::to_string(M.remap.view.e24 ? 24 : 32) +
                    ", \"remap_result_subtiles\": " + std::to_string(M.plan.n_result) + ", \"traffic_parts\": {";
    {
        bool first = true;
        for (const auto& p : multiband_traffic_parts(M)) {
            char buf[96];
            snprintf(buf, sizeof buf, "%s\"%s\": %.0f", first ? "" : ", ", p.first.c_str(), p.second);
            s += buf;
            first = false;
        }
    }
    s += "}, \"level_tiles\": [";
    for (int l = 0; l <= M.B; l++) {
        const auto& L = M.plan.lv[l];
        size_t cam_tiles = 0;
        for (uint32_t m : L.tile_cams) cam_tiles += (size_t)__builtin_popcount(m);
        char buf[512];
        snprintf(buf, sizeof buf, "%s{\"tiles\": %d, \"required\": %zu, \"weight_cam_tiles\": %zu, \"down_items\": %d%s}",
                 l ? ", " : "", L.tx_n * L.ty_n, L.req_tiles, cam_tiles, M.lv[l].n_down,
                 !L.sub_own.empty() ? (", \"blend_subtiles\": " + std::to_string(L.n_work) + ", \"owned_subtiles\": " +
                              std::to_string(L.n_owned) + ", \"deep_subtiles\": " + std::to_string(L.n_deep) +
                              ", \"unread_subtiles\": " + std::to_string(L.n_skip)).c_str() : "");
        s += buf;
    }
    s += "]";
    // the level-0 remap's tiled LUT: the build statistics the blend = 0 composite reports at the top level
    if (!M.remap.stats.empty()) s += ", \"remap_lut\": {" + M.remap.stats + "}";
    return s;
}

}  // namespace octvr
