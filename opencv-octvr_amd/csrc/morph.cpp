// morph.cpp — MapperTemplate::morph_controlpoints (modules/octvr/src/template_morph.cpp:69-237).
//
// Control points pair a pixel of camera n0 with a pixel of camera n1 that should coincide in the
// output.  Both are projected to the output (input image_to_obj, output obj_to_image), pulled to a
// distance-weighted midpoint, and every camera's LUT (map1, map2, mask) is warped piecewise-affinely
// over a Delaunay triangulation of its control points plus a 40-point frame around them.
//
// Host side: control-point projection, chamfer distances and the frame (this file); per camera the
// Delaunay triangulation (cv::Subdiv2D restated), per-triangle affine matrices (cv::getAffineTransform
// + cv::solve LU) and the fillPoly'd triangle ownership of every ROI pixel (morph_plan.hpp, host
// arithmetic without HIP).  Device side (resize_kernels.hip,
// morph_warp_kernel): the cv::warpAffine bilinear resampling of the three LUT planes, one pass over
// the ROI instead of the reference's three full-ROI warps per triangle.
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <thread>

#include "host_common.hpp"
#include "json_lite.hpp"
#include "morph_plan.hpp"

namespace octvr {
namespace {

using Pt = MorphPt;
struct ControlPoint {  // template_morph.cpp:15-20
    int n0, n1;
    Pt src0, src1, dst0, dst1, mid;
};

// distanceTransform(DIST_L2, 3) of one camera's ROI mask, three side-by-side copies when the camera
// starts at column 0 and spans the union ROI (DistanceSeamFinder::find, seam_finders.cpp:97-110)
std::vector<float> camera_distance(const RigInput& in, bool wrapped) {
    const int w = in.roi[2], h = in.roi[3];
    std::vector<float> d((size_t)w * h);
    if (!wrapped) {
        chamfer_l2_3x3(in.mask.data(), w, h, d.data());
        return d;
    }
    std::vector<uint8_t> tri((size_t)3 * w * h);
    for (int y = 0; y < h; y++)
        for (int c = 0; c < 3; c++) memcpy(&tri[((size_t)y * 3 + c) * w], &in.mask[(size_t)y * w], w);
    std::vector<float> d3(tri.size());
    chamfer_l2_3x3(tri.data(), 3 * w, h, d3.data());
    for (int y = 0; y < h; y++) memcpy(&d[(size_t)y * w], &d3[((size_t)y * 3 + 1) * w], sizeof(float) * w);
    return d;
}

}  // namespace

int rig_morph_controlpoints(octvr_rig& rig, const JsonValue& cps_json) {
    const int n = (int)rig.inputs.size();
    if (!rig.has_cameras)
        throw OctvrError(OCTVR_E_UNSUPPORTED, "morph_controlpoints needs the camera models (a rig built from JSON, "
                                              "not one loaded from .dat)");
    REQUIRE(cps_json.kind == JsonValue::Array, "control_points must be an array");
    const int W = rig.out_w, H = rig.out_h;

    // _translate (template_morph.cpp:86-90): input image_to_obj, then output obj_to_image
    auto translate = [&](Pt p, int cam) {
        const CameraParams& c = rig.cams[cam];
        if (c.type == CAM_FISHEYE || c.type == CAM_PINHOLE)  // camera.hpp:101-103
            throw OctvrError(OCTVR_E_UNSUPPORTED, "control point camera has no image_to_obj (fisheye / pinhole)");
        if (c.type == CAM_FULLFRAME_FISHEYE)  // fullframe_fisheye_cam.cpp:224
            REQUIRE(c.crop_x == 0 && c.crop_y == 0 && c.crop_w == c.width && c.crop_h == c.height,
                    "control point camera: fullframe_fisheye image_to_obj needs a crop covering the image");
        double x, y;
        project_output_to_input(c, rig.out_cam, p.x, p.y, &x, &y);
        return Pt{(float)x, (float)y};
    };

    // control points (:92-136); the distances are evaluated only for the points kept
    std::vector<ControlPoint> cps;
    struct Local {
        int x0, y0, x1, y1;
    };
    std::vector<Local> local;
    for (size_t k = 0; k < cps_json.size(); k++) {
        const JsonValue& a = cps_json[k];
        REQUIRE(a.kind == JsonValue::Array && a.size() >= 6, "control point must be [n0, n1, x0, y0, x1, y1]");
        ControlPoint cp;
        cp.n0 = a[0].as_int();
        cp.n1 = a[1].as_int();
        cp.src0 = Pt{(float)a[2].as_double(), (float)a[3].as_double()};
        cp.src1 = Pt{(float)a[4].as_double(), (float)a[5].as_double()};
        REQUIRE(cp.n0 < cp.n1, "control point: n0 < n1 required");  // :102
        REQUIRE(cp.n0 >= 0 && cp.n1 < n, "control point camera index out of range");
        cp.dst0 = translate(cp.src0, cp.n0);
        cp.dst1 = translate(cp.src1, cp.n1);
        // |dst0 - dst1|_1 > 0.1 in float, compared in double (:123-124); NaN passes this test in the
        // reference and then indexes the distance maps out of bounds, so it is rejected here
        const float l1 = std::fabs(cp.dst0.x - cp.dst1.x) + std::fabs(cp.dst0.y - cp.dst1.y);
        if ((double)l1 > 0.1) continue;
        REQUIRE(!std::isnan(cp.dst0.x) && !std::isnan(cp.dst0.y) && !std::isnan(cp.dst1.x) && !std::isnan(cp.dst1.y),
                "control point does not project into the output");
        const RigInput& i0 = rig.inputs[cp.n0];
        const RigInput& i1 = rig.inputs[cp.n1];
        Local l;  // :107-110, float arithmetic truncated to int
        l.x0 = (int)(cp.dst0.x * (float)W - (float)i0.roi[0]);
        l.y0 = (int)(cp.dst0.y * (float)H - (float)i0.roi[1]);
        l.x1 = (int)(cp.dst1.x * (float)W - (float)i1.roi[0]);
        l.y1 = (int)(cp.dst1.y * (float)H - (float)i1.roi[1]);
        REQUIRE(l.x0 >= 0 && l.x0 < i0.roi[2] && l.y0 >= 0 && l.y0 < i0.roi[3] && l.x1 >= 0 && l.x1 < i1.roi[2] &&
                    l.y1 >= 0 && l.y1 < i1.roi[3],
                "control point lies outside its camera's ROI");
        cps.push_back(cp);
        local.push_back(l);
    }

    // DistanceSeamFinder(2)::find's distances (:70-79; only getDistances() is used)
    int ux0 = 0, ux1 = 0;
    for (int i = 0; i < n; i++) {
        const RigInput& in = rig.inputs[i];
        ux0 = i ? std::min(ux0, in.roi[0]) : in.roi[0];
        ux1 = i ? std::max(ux1, in.roi[0] + in.roi[2]) : in.roi[0] + in.roi[2];
    }
    std::vector<char> need(n, 0);
    for (const ControlPoint& cp : cps) need[cp.n0] = need[cp.n1] = 1;
    std::vector<std::vector<float>> dist(n);
    {
        run_threads((size_t)n, [&](size_t i) {
            if (!need[i]) return;
            const RigInput& in = rig.inputs[i];
            dist[i] = camera_distance(in, in.roi[0] == 0 && in.roi[2] == ux1 - ux0);
        });
    }
    for (size_t k = 0; k < cps.size(); k++) {  // :126-133, all float
        ControlPoint& cp = cps[k];
        const Local& l = local[k];
        float w0 = dist[cp.n0][(size_t)l.y0 * rig.inputs[cp.n0].roi[2] + l.x0];
        float w1 = dist[cp.n1][(size_t)l.y1 * rig.inputs[cp.n1].roi[2] + l.x1];
        if ((double)(w0 + w1) < 1e-3) w0 = w1 = 1.0f;
        cp.mid.x = (cp.dst0.x * w0 + cp.dst1.x * w1) / (w0 + w1);
        cp.mid.y = (cp.dst0.y * w0 + cp.dst1.y * w1) / (w0 + w1);
    }

    DeviceGuard dg(rig.device);
    for (int i = 0; i < n; i++) {
        RigInput& in = rig.inputs[i];
        std::vector<Pt> sv, dv;  // :140-151
        for (const ControlPoint& cp : cps) {
            if (cp.n0 == i) {
                sv.push_back(cp.dst0);
                dv.push_back(cp.mid);
            }
            if (cp.n1 == i) {
                sv.push_back(cp.dst1);
                dv.push_back(cp.mid);
            }
        }
        // bounding box of both vertex sets, widened by 0.05 and kept inside (0, 1) (:153-169)
        float L = 1.f, R = 0.f, T = 1.f, B = 0.f;
        for (const std::vector<Pt>* vs : {&sv, &dv})
            for (const Pt& v : *vs) {
                L = std::min(L, v.x);
                R = std::max(R, v.x);
                T = std::min(T, v.y);
                B = std::max(B, v.y);
            }
        L = (float)std::max(1e-3, (double)L - 0.05);
        T = (float)std::max(1e-3, (double)T - 0.05);
        R = (float)std::min(1 - 1e-3, (double)R + 0.05);
        B = (float)std::min(1 - 1e-3, (double)B + 0.05);
        // the fixed frame: 11 columns along the top and bottom edges, 9 rows along the sides (:171-182)
        int guard = 0;
        for (float x = L; (double)x < (double)R + 1e-3; x += (R - L) / 10) {
            REQUIRE(++guard < 100000, "morph frame does not advance");
            sv.push_back(Pt{x, T});
            sv.push_back(Pt{x, B});
            dv.push_back(Pt{x, T});
            dv.push_back(Pt{x, B});
        }
        for (float y = T + (B - T) / 10; (double)(B - (B - T) / 10) + 1e-3 > (double)y; y += (B - T) / 10) {
            REQUIRE(++guard < 100000, "morph frame does not advance");
            sv.push_back(Pt{L, y});
            sv.push_back(Pt{R, y});
            dv.push_back(Pt{L, y});
            dv.push_back(Pt{R, y});
        }

        // triangles, warp matrices and pixel owners (morph_plan.hpp)
        MorphPlan P;
        try {
            P = morph_plan(sv, dv, in.roi, W, H);
        } catch (const MorphPlanError& e) {
            throw OctvrError(OCTVR_E_INVALID, e.what());
        }
        in.src_tris = P.src_tris;
        in.dst_tris = P.dst_tris;
        if (P.nt() == 0) continue;  // nothing to warp: the LUT is copied unchanged
        const std::vector<double>& M = P.M;
        const std::vector<int16_t>& owner = P.owner;

        const int rw = in.roi[2], rh = in.roi[3];
        const size_t px = (size_t)rw * rh;
        DevBuf<float> m1, m2, o1, o2;
        DevBuf<uint8_t> mk, om;
        DevBuf<int16_t> own;
        DevBuf<double> Md;
        m1.upload(in.map1.data(), px);
        m2.upload(in.map2.data(), px);
        mk.upload(in.mask.data(), px);
        own.upload(owner.data(), px);
        Md.upload(M.data(), M.size());
        o1.alloc(px);
        o2.alloc(px);
        om.alloc(px);
        HIP_CHECK(launch_morph_warp(m1.p, m2.p, mk.p, rw, rh, own.p, Md.p, o1.p, o2.p, om.p, nullptr));
        HIP_CHECK(hipMemcpy(in.map1.data(), o1.p, px * sizeof(float), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(in.map2.data(), o2.p, px * sizeof(float), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(in.mask.data(), om.p, px, hipMemcpyDeviceToHost));
    }
    return (int)cps.size();
}

}  // namespace octvr
