// rig_json.cpp — the rig (vr::MapperTemplate) from JSON camera models: camera setup, camera masks and the
// FP64 LUT build of one input (GPU build + the fragile pixels recomputed on the host with glibc).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "camera_math.hpp"
#include "host_common.hpp"
#include "json_lite.hpp"
#include "kernels.hpp"
#include "masks.hpp"

namespace octvr {

namespace {

// ---- camera setup from JSON (camera.cpp:49-136 and the per-type constructors) ------------------
void rodrigues(double rx, double ry, double rz, double R[9]) {
    // cvRodrigues2 (calib3d/src/calibration.cpp:300-345)
    double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double c, s;
    sin_cos(theta, &s, &c);  // gcc builds cvRodrigues2's cos / sin pair as one sincos (camera_math.hpp)
    const double c1 = 1. - c;
    double itheta = theta ? 1. / theta : 0.;
    rx *= itheta;
    ry *= itheta;
    rz *= itheta;
    double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    double rx_[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; k++) R[k] = c * I[k] + c1 * rrt[k] + s * rx_[k];
}

void mul33(const double* a, const double* b, double* d) {
    // cv::gemm len==3 path (core/src/matmul.cpp:934-1000): t*1 + 0*0
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double t = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j];
            d[i * 3 + j] = t * 1.0 + 0.0 * 0.0;
        }
}

void invert33(const double* S, double* D) {
    // cv::invert 3x3 closed form (core/src/lapack.cpp:709-712, 970-990)
#define Sd(y, x) S[(y) * 3 + (x)]
    double d = Sd(0, 0) * ((double)Sd(1, 1) * Sd(2, 2) - (double)Sd(1, 2) * Sd(2, 1)) -
               Sd(0, 1) * ((double)Sd(1, 0) * Sd(2, 2) - (double)Sd(1, 2) * Sd(2, 0)) +
               Sd(0, 2) * ((double)Sd(1, 0) * Sd(2, 1) - (double)Sd(1, 1) * Sd(2, 0));
    if (d == 0.) {
        for (int k = 0; k < 9; k++) D[k] = 0;
        return;
    }
    d = 1. / d;
    D[0] = (Sd(1, 1) * Sd(2, 2) - Sd(1, 2) * Sd(2, 1)) * d;
    D[1] = (Sd(0, 2) * Sd(2, 1) - Sd(0, 1) * Sd(2, 2)) * d;
    D[2] = (Sd(0, 1) * Sd(1, 2) - Sd(0, 2) * Sd(1, 1)) * d;
    D[3] = (Sd(1, 2) * Sd(2, 0) - Sd(1, 0) * Sd(2, 2)) * d;
    D[4] = (Sd(0, 0) * Sd(2, 2) - Sd(0, 2) * Sd(2, 0)) * d;
    D[5] = (Sd(0, 2) * Sd(1, 0) - Sd(0, 0) * Sd(1, 2)) * d;
    D[6] = (Sd(1, 0) * Sd(2, 1) - Sd(1, 1) * Sd(2, 0)) * d;
    D[7] = (Sd(0, 1) * Sd(2, 0) - Sd(0, 0) * Sd(2, 1)) * d;
    D[8] = (Sd(0, 0) * Sd(1, 1) - Sd(0, 1) * Sd(1, 0)) * d;
#undef Sd
}

// CalcCorrectionRadius_copy (fullframe_fisheye_cam.cpp:20-103)
double cube_root(double x) { return x == 0.0 ? 0.0 : x > 0.0 ? pow(x, 1.0 / 3.0) : -pow(-x, 1.0 / 3.0); }
void square_zero(const double* a, int* n, double* root) {
    if (a[2] == 0.0) {
        if (a[1] == 0.0) {
            if (a[0] == 0.0) {
                *n = 1;
                root[0] = 0.0;
            } else {
                *n = 0;
            }
        } else {
            *n = 1;
            root[0] = -a[0] / a[1];
        }
    } else if (4.0 * a[2] * a[0] > a[1] * a[1]) {
        *n = 0;
    } else {
        *n = 2;
        root[0] = (-a[1] + sqrt(a[1] * a[1] - 4.0 * a[2] * a[0])) / (2.0 * a[2]);
        root[1] = (-a[1] - sqrt(a[1] * a[1] - 4.0 * a[2] * a[0])) / (2.0 * a[2]);
    }
}
void cube_zero(const double* a, int* n, double* root) {
    if (a[3] == 0.0) {
        square_zero(a, n, root);
        return;
    }
    double p = ((-1.0 / 3.0) * (a[2] / a[3]) * (a[2] / a[3]) + a[1] / a[3]) / 3.0;
    double q = ((2.0 / 27.0) * (a[2] / a[3]) * (a[2] / a[3]) * (a[2] / a[3]) - (1.0 / 3.0) * (a[2] / a[3]) * (a[1] / a[3]) +
                a[0] / a[3]) / 2.0;
    if (q * q + p * p * p >= 0.0) {
        *n = 1;
        root[0] = cube_root(-q + sqrt(q * q + p * p * p)) + cube_root(-q - sqrt(q * q + p * p * p)) - a[2] / (3.0 * a[3]);
    } else {
        double phi = acos(-q / sqrt(-p * p * p));
        *n = 3;
        root[0] = 2.0 * sqrt(-p) * cos(phi / 3.0) - a[2] / (3.0 * a[3]);
        root[1] = -2.0 * sqrt(-p) * cos(phi / 3.0 + kPi / 3.0) - a[2] / (3.0 * a[3]);
        root[2] = -2.0 * sqrt(-p) * cos(phi / 3.0 - kPi / 3.0) - a[2] / (3.0 * a[3]);
    }
}
double correction_radius(const double* coeff) {
    double a[4];
    for (int k = 0; k < 4; k++) a[k] = coeff[k] != 0.0 ? (k + 1) * coeff[k] : 0.0;
    int n = 0;
    double root[3], sroot = 1000.0;
    cube_zero(a, &n, root);
    for (int i = 0; i < n; i++)
        if (root[i] > 0.0 && root[i] < sroot) sroot = root[i];
    return sroot;
}

void reject_unsupported_options(const JsonValue& o, const std::string& type) {
    // PinholeCamera overrides obj_to_image and never consults the masks (pinhole_cam.cpp:32-50), and its
    // get_include_mask would call the base obj_to_image_single, which throws (camera.hpp:92-94)
    if ((type == "fisheye" || type == "pinhole") && (o.has("include_masks") || o.has("exclude_masks")))
        throw OctvrError(OCTVR_E_UNSUPPORTED, "camera type '" + type + "' does not support include/exclude masks");
}

}  // namespace

// The Camera constructor's mask part (camera.cpp:72-123) and draw_mask (camera.cpp:146-187): `selection`
// fills the exclude mask with 255 and clears the rectangle; `exclude_masks` areas set exclude (polygons,
// PNG red) and include (PNG green) bits; `include_masks` areas set include bits.  Empty vector = no mask.
void build_camera_masks(const JsonValue& o, std::vector<uint8_t>& excl, std::vector<uint8_t>& incl) {
    const bool any = o.has("selection") || o.has("exclude_masks") || o.has("include_masks");
    if (!any) return;
    REQUIRE(o.has("width") && o.has("height"), "camera masks need the camera's width and height");
    const int w = o["width"].as_int(), h = o["height"].as_int();
    REQUIRE(w > 0 && h > 0, "camera width/height must be positive");
    const size_t n = (size_t)w * h;
    auto prepare = [&](std::vector<uint8_t>& m, uint8_t init) {
        if (m.empty()) m.assign(n, init);
    };
    auto draw = [&](const JsonValue& areas, bool include) {
        for (size_t a = 0; a < areas.size(); a++) {
            const JsonValue& area = areas[a];
            const std::string& t = area["type"].as_string();
            const JsonValue& args = area["args"];
            if (t == "polygonal") {
                std::vector<int> pts;
                for (size_t k = 0; k + 1 < args.size(); k += 2) {
                    pts.push_back((int)args[k].as_double());
                    pts.push_back((int)args[k + 1].as_double());
                }
                fill_poly_u8(include ? incl.data() : excl.data(), w, h, pts.data(), (int)pts.size() / 2, 255);
            } else if (t == "png") {
                std::vector<uint8_t> bytes(args.size());
                for (size_t k = 0; k < args.size(); k++) bytes[k] = (uint8_t)args[k].as_int();
                int pw = 0, ph = 0;
                // CV_Assert(mask_img.size() == exclude_mask.size()) (camera.cpp:170), checked on the IHDR
                REQUIRE(!excl.empty() && w > 0 && h > 0, "png mask without a camera size");
                std::vector<uint8_t> rgb = png_decode_rgb(bytes.data(), bytes.size(), &pw, &ph, w, h);
                for (size_t k = 0; k < n; k++) {
                    if (rgb[3 * k]) excl[k] = 255;      // RED channel
                    if (rgb[3 * k + 1]) incl[k] = 255;  // GREEN channel
                }
            } else {
                throw OctvrError(OCTVR_E_INVALID, "unknown mask area type '" + t + "'");
            }
        }
    };
    if (o.has("selection")) {
        prepare(excl, 255);
        const JsonValue& sel = o["selection"];
        const int l = sel[0].as_int(), r = sel[1].as_int(), t = sel[2].as_int(), b = sel[3].as_int();
        const int rect[8] = {l, t, l, b - 1, r - 1, b - 1, r - 1, t};
        fill_poly_u8(excl.data(), w, h, rect, 4, 0);
    }
    if (o.has("exclude_masks")) {
        prepare(excl, 0);
        prepare(incl, 0);
        draw(o["exclude_masks"], false);
    }
    if (o.has("include_masks")) {
        prepare(incl, 0);
        draw(o["include_masks"], true);
    }
}

namespace {

// computeTiltProjectionMatrix (imgproc/detail/distortion_model.hpp:74-94), Matx products s += a*b.
void tilt_matrix(double tauX, double tauY, double* T) {
    auto mul = [](const double* a, const double* b, double* d) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double v = 0;
                for (int k = 0; k < 3; k++) v += a[i * 3 + k] * b[k * 3 + j];
                d[i * 3 + j] = v;
            }
    };
    const double cX = cos(tauX), sX = sin(tauX), cY = cos(tauY), sY = sin(tauY);
    const double rx[9] = {1, 0, 0, 0, cX, sX, 0, -sX, cX};
    const double ry[9] = {cY, 0, -sY, 0, 1, 0, sY, 0, cY};
    double rxy[9];
    mul(ry, rx, rxy);
    const double pz[9] = {rxy[8], 0, -rxy[2], 0, rxy[8], -rxy[5], 0, 0, 1};
    mul(pz, rxy, T);
}

// get_ocam_model (ocam_fisheye.cpp:19-80): the calibration TXT file of the OCamCalib toolbox.
void read_ocam_file(const std::string& path, CameraParams& c) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) throw OctvrError(OCTVR_E_IO, "ocam_fisheye: cannot open " + path);
    char buf[1024];
    int ok = 1;
    auto line = [&] { ok &= fgets(buf, sizeof buf, f) != nullptr; };
    line();
    ok &= fscanf(f, "\n") >= 0;
    ok &= fscanf(f, "%d", &c.len_pol) == 1;
    ok &= c.len_pol > 0 && c.len_pol <= kOcamMaxPol;
    for (int i = 0; ok && i < c.len_pol; i++) ok &= fscanf(f, " %lf", &c.pol[i]) == 1;
    ok &= fscanf(f, "\n") >= 0;
    line();
    ok &= fscanf(f, "\n") >= 0;
    ok &= fscanf(f, "%d", &c.len_invpol) == 1;
    ok &= c.len_invpol > 0 && c.len_invpol <= kOcamMaxPol;
    for (int i = 0; ok && i < c.len_invpol; i++) ok &= fscanf(f, " %lf", &c.invpol[i]) == 1;
    ok &= fscanf(f, "\n") >= 0;
    line();
    ok &= fscanf(f, "\n") >= 0;
    ok &= fscanf(f, "%lf %lf\n", &c.xc, &c.yc) == 2;
    line();
    ok &= fscanf(f, "\n") >= 0;
    ok &= fscanf(f, "%lf %lf %lf\n", &c.oc, &c.od, &c.oe) == 3;
    line();
    ok &= fscanf(f, "\n") >= 0;
    ok &= fscanf(f, "%d %d", &c.height, &c.width) == 2;
    fclose(f);
    if (!ok) throw OctvrError(OCTVR_E_PARSE, "ocam_fisheye: malformed calibration file " + path);
}

}  // namespace

CameraParams camera_from_json(const JsonValue& cam) {
    CameraParams c;
    memset(&c, 0, sizeof c);
    const std::string& type = cam["type"].as_string();
    static const JsonValue empty_obj = [] {
        JsonValue v;
        v.kind = JsonValue::Object;
        return v;
    }();
    const JsonValue& o = cam.has("options") ? cam["options"] : empty_obj;
    reject_unsupported_options(o, type);
    // rotation (camera.cpp:50-70)
    double rv[3] = {0, 0, 0};
    if (o.has("rotation")) {
        rv[0] = o["rotation"]["roll"].as_double();
        rv[1] = -o["rotation"]["yaw"].as_double();
        rv[2] = -o["rotation"]["pitch"].as_double();
    }
    double Rx[9], Ry[9], Rz[9], T[9];
    rodrigues(rv[0], 0, 0, Rx);
    rodrigues(0, rv[1], 0, Ry);
    rodrigues(0, 0, rv[2], Rz);
    mul33(Rx, Rz, T);
    mul33(T, Ry, c.R);
    if (o.has("rotation_matrix"))
        for (int k = 0; k < 9; k++) c.R[k] = o["rotation_matrix"][k].as_double();
    invert33(c.R, c.Rinv);
    if (o.has("longitude_selection")) {
        c.min_lon = o["longitude_selection"][0].as_double();
        c.max_lon = o["longitude_selection"][1].as_double();
        REQUIRE(c.max_lon > c.min_lon, "longitude_selection: max must exceed min");
    } else {
        c.min_lon = -kPi;
        c.max_lon = kPi;
    }
    if (type == "equirectangular") {
        c.type = CAM_EQUIRECT;
        c.min_lat = o.get("min_lat", -kPi / 2);
        c.max_lat = o.get("max_lat", kPi / 2);
        c.scale_lon = o.get("scale_lon", 1.0);
    } else if (type == "fullframe_fisheye") {
        c.type = CAM_FULLFRAME_FISHEYE;
        c.width = o["width"].as_int();
        c.height = o["height"].as_int();
        if (o.has("crop")) {
            const JsonValue& r = o["crop"]["rect"];
            c.crop_x = r[0].as_int();
            c.crop_y = r[2].as_int();
            c.crop_w = r[1].as_int() - r[0].as_int();
            c.crop_h = r[3].as_int() - r[2].as_int();
            c.crop_circular = o["crop"]["is_circular"].as_bool() ? 1 : 0;
        }
        if (c.crop_w * c.crop_h == 0) {
            c.crop_x = c.crop_y = 0;
            c.crop_w = c.width;
            c.crop_h = c.height;
            c.crop_circular = 0;
        }
        c.hfov = o["hfov"].as_double();
        c.center_dx = o["center_dx"].as_double();
        c.center_dy = o["center_dy"].as_double();
        const JsonValue& r = o["radial"];
        c.rad[3] = r[0].as_double();
        c.rad[2] = r[1].as_double();
        c.rad[1] = r[2].as_double();
        c.rad[0] = 1.0 - r[0].as_double() - r[1].as_double() - r[2].as_double();
        c.rad[4] = (c.crop_w < c.crop_h ? c.crop_w : c.crop_h) / 2.0;
        c.rad[5] = correction_radius(c.rad);
    } else if (type == "fisheye") {
        c.type = CAM_FISHEYE;
        c.fx = o["fx"].as_double();
        c.fy = o["fy"].as_double();
        c.cx = o["cx"].as_double();
        c.cy = o["cy"].as_double();
        REQUIRE(o["dist_coeffs"].size() == 4, "fisheye: dist_coeffs must have 4 entries (calib3d/src/fisheye.cpp:90)");
        for (int k = 0; k < 4; k++) c.k[k] = o["dist_coeffs"][k].as_double();
        c.width = o["width"].as_int();
        c.height = o["height"].as_int();
    } else if (type == "pinhole") {  // PinholeCamera (pinhole_cam.cpp:13-30) + cv::projectPoints
        c.type = CAM_PINHOLE;
        c.fx = o["fx"].as_double();
        c.fy = o["fy"].as_double();
        c.cx = o["cx"].as_double();
        c.cy = o["cy"].as_double();
        const size_t nd = o.has("dist_coeffs") ? o["dist_coeffs"].size() : 0;
        REQUIRE(nd == 0 || nd == 4 || nd == 5 || nd == 8 || nd == 12 || nd == 14,
                "pinhole: dist_coeffs must have 4, 5, 8, 12 or 14 entries (calibration.cpp:644-655)");
        for (size_t k = 0; k < nd; k++) c.dist[k] = o["dist_coeffs"][k].as_double();
        for (int k = 0; k < 9; k++) c.tilt[k] = (k % 4 == 0) ? 1.0 : 0.0;
        if (c.dist[12] != 0 || c.dist[13] != 0) tilt_matrix(c.dist[12], c.dist[13], c.tilt);
        c.width = o["width"].as_int();
        c.height = o["height"].as_int();
    } else if (type == "normal") {  // normal.cpp:13-22
        c.type = CAM_NORMAL;
        c.aspect = o["aspect_ratio"].as_double();
        c.cam_x = o["cam_opt"].as_double();
        c.cam_z = sqrt((1.0 - c.cam_x * c.cam_x) / (1.0 + 1.0 / c.aspect / c.aspect));
        c.cam_y = c.cam_z / c.aspect;
    } else if (type == "perspective") {  // perspective.cpp:14-19
        c.type = CAM_PERSPECTIVE;
        c.aspect = o["aspect_ratio"].as_double();
        c.sf = o["sf"].as_double();
    } else if (type == "ocam_fisheye") {  // ocam_fisheye.cpp:82-110
        c.type = CAM_OCAM;
        if (o.has("file")) {
            read_ocam_file(o["file"].as_string(), c);
        } else {
            const JsonValue& pol = o["pol"];
            const JsonValue& inv = o["invpol"];
            c.len_pol = (int)pol.size();
            c.len_invpol = (int)inv.size();
            REQUIRE(c.len_pol > 0 && c.len_pol <= kOcamMaxPol && c.len_invpol > 0 && c.len_invpol <= kOcamMaxPol,
                    "ocam_fisheye: pol / invpol must have 1..64 entries");
            for (int i = 0; i < c.len_pol; i++) c.pol[i] = pol[i].as_double();
            for (int i = 0; i < c.len_invpol; i++) c.invpol[i] = inv[i].as_double();
            c.xc = o["xc"].as_double();
            c.yc = o["yc"].as_double();
            c.oc = o["c"].as_double();
            c.od = o["d"].as_double();
            c.oe = o["e"].as_double();
            c.width = o["width"].as_int();
            c.height = o["height"].as_int();
        }
    } else if (type == "stupidoval") {
        c.type = CAM_STUPIDOVAL;
    } else if (type == "cubic") {
        c.type = CAM_CUBIC;
    } else if (type == "eqareanorthpole") {  // eqareanorthpole.hpp:11-18
        c.type = CAM_EQAREA_NORTH;
        c.circle = o.get("arctic_circle", kPi / 3);
    } else if (type == "eqareasouthpole") {  // eqareasouthpole.hpp:10-17
        c.type = CAM_EQAREA_SOUTH;
        c.circle = o.get("antarctic_circle", -kPi / 3);
    } else {
        throw OctvrError(OCTVR_E_UNSUPPORTED, "camera type '" + type + "' is not implemented in this ABI version");
    }
    if (o.has("selection")) {  // exclude everything outside the rectangle (camera.cpp:96-112)
        REQUIRE(o.has("width") && o.has("height"), "selection needs the camera's width and height");
        c.sel = 1;
        c.width = o["width"].as_int();
        c.height = o["height"].as_int();
        c.sel_l = o["selection"][0].as_int();
        c.sel_r = o["selection"][1].as_int();
        c.sel_t = o["selection"][2].as_int();
        c.sel_b = o["selection"][3].as_int();
    }
    return c;
}

namespace {

double aspect_ratio(const JsonValue& cam) {
    // Camera::get_aspect_ratio overrides (equirectangular.hpp:32-34, fullframe_fisheye_cam.cpp:142-144,
    // pinhole_cam.hpp:32-34, normal.hpp:26-28, perspective.hpp:24-26, ocam_fisheye.cpp:112-114,
    // stupidoval.hpp:21-23, cubic.hpp:43-45, eqarea*.hpp: 1)
    const CameraParams c = camera_from_json(cam);
    switch (c.type) {
        case CAM_EQUIRECT:
            return (2.0f * c.scale_lon) / ((c.max_lat - c.min_lat) / kPi);
        case CAM_FULLFRAME_FISHEYE:
        case CAM_FISHEYE:
        case CAM_PINHOLE:
        case CAM_OCAM:
            return double(c.width) / c.height;
        case CAM_NORMAL:
        case CAM_PERSPECTIVE:
            return c.aspect;
        case CAM_STUPIDOVAL:
            return 2.0;
        case CAM_CUBIC:
            return 3.0 / 2.0;
        default:
            return 1.0;
    }
}

// Vignette::getMap (vignette.cpp:18-54) at 512x512.
std::vector<float> vignette_map(const JsonValue& o, int width, int height) {
    if (!o.has("vignette")) return {};
    double a = o["vignette"][0].as_double(), b = o["vignette"][1].as_double(), c = o["vignette"][2].as_double(),
           d = o["vignette"][3].as_double();
    if (o.has("exposure")) {
        float ev = (float)std::pow(2.0, o["exposure"].as_double());
        a /= ev;
        b /= ev;
        c /= ev;
        d /= ev;
    }
    std::vector<float> m((size_t)width * height);
    for (int j = 0; j < height; j++)
        for (int i = 0; i < width; i++) {
#define P(X) (float(X) * float(X))
            float r = std::sqrt(P(i - width / 2) + P(j - height / 2)) / std::sqrt(P(width / 2) + P(height / 2));
#undef P
            m[(size_t)j * width + i] = (float)(1.0 / (a + r * r * (b + r * r * (c + d * r * r))));
        }
    return m;
}

// MapperTemplate::add_input (template.cpp:46-153).  `visible` (W x H device bytes, 1 = claimed by an
// include mask) is allocated by the caller once some camera has include masks; `priors` are the inputs
// added before this one, whose masks lose the pixels this camera's include mask claims (:102-116).
void build_input(const CameraParams& out_cam, const JsonValue& cam, int W, int H, bool use_roi, int device,
                 RigInput& in, DevBuf<uint8_t>* visible = nullptr, std::vector<RigInput>* priors = nullptr) {
    CameraParams c = camera_from_json(cam);
    DeviceGuard dg(device);
    std::vector<uint8_t> excl, incl;
    if (cam.has("options")) build_camera_masks(cam["options"], excl, incl);
    DevBuf<uint8_t> excl_d, incl_d;
    if (!excl.empty() || !incl.empty()) {
        c.sel = 0;  // the selection rectangle is rasterised into the exclude mask
        c.width = cam["options"]["width"].as_int();
        c.height = cam["options"]["height"].as_int();
    }
    if (!excl.empty()) {
        excl_d.upload(excl.data(), excl.size());
        c.excl = excl_d.p;
        if (!incl.empty()) {
            incl_d.upload(incl.data(), incl.size());
            c.incl = incl_d.p;
        }
    }
    const size_t total_px = (size_t)W * H;
    if (visible && c.incl && !visible->p) {
        visible->alloc(total_px);
        HIP_CHECK(hipMemset(visible->p, 0, total_px));
    }
    uint8_t* vis_p = visible ? visible->p : nullptr;
    const size_t total = (size_t)W * H;
    REQUIRE(total < ((size_t)1 << 32), "output frame must have fewer than 2^32 pixels");
    DevBuf<float> m1, m2;
    DevBuf<uint8_t> mk;
    DevBuf<int32_t> bb;
    m1.alloc(total);
    m2.alloc(total);
    mk.alloc(total);
    bb.alloc(4);
    const CameraParams both[2] = {out_cam, c};
    DevBuf<CameraParams> cams;
    cams.upload(both, 2);
    // fragile pixels (LutGuard, camera_math.hpp): a list of at most `cap` indices, grown and the kernel
    // re-run if it overflows (the build is idempotent: it writes visible_mask only with 2)
    uint32_t cap = (uint32_t)std::min<size_t>(total, std::max<size_t>(1 << 16, total / 256));
    std::vector<uint32_t> frag;
    int32_t b[4];
    for (;;) {
        DevBuf<uint32_t> fr;
        fr.alloc((size_t)cap + 1);
        HIP_CHECK(hipMemset(fr.p, 0, sizeof(uint32_t)));
        const int32_t init[4] = {INT32_MAX, INT32_MAX, -1, -1};
        HIP_CHECK(hipMemcpy(bb.p, init, sizeof init, hipMemcpyHostToDevice));
        HIP_CHECK(launch_lut_build(cams.p, W, H, m1.p, m2.p, mk.p, bb.p, vis_p, fr.p, cap, nullptr));
        HIP_CHECK(hipDeviceSynchronize());
        uint32_t count = 0;
        HIP_CHECK(hipMemcpy(&count, fr.p, sizeof count, hipMemcpyDeviceToHost));
        if (count > cap) {
            cap = count;
            continue;
        }
        frag.resize(count);
        if (count) HIP_CHECK(hipMemcpy(frag.data(), fr.p + 1, sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(b, bb.p, sizeof b, hipMemcpyDeviceToHost));
        break;
    }
    // the fragile pixels with glibc: the reference's arithmetic exactly (camera_math.hpp on the host)
    std::sort(frag.begin(), frag.end());
    CameraParams ch = c;
    ch.excl = excl.empty() ? nullptr : excl.data();
    ch.incl = (excl.empty() || incl.empty()) ? nullptr : incl.data();
    struct Fix {
        float x, y;
        bool vis;
    };
    std::vector<Fix> fix(frag.size());
    {
        const bool want_vis = vis_p != nullptr;
        std::vector<double> fx(frag.size()), fy(frag.size());
        std::vector<uint8_t> fv(frag.size());
        parallel_for(frag.size(), [&](size_t k) {
            const uint32_t idx = frag[k];
            const int h = (int)(idx / (uint32_t)W), w = (int)(idx - (uint32_t)h * (uint32_t)W);
            bool v = false;
            project_output_to_input(out_cam, ch, (double)w / W, (double)h / H, &fx[k], &fy[k], want_vis ? &v : nullptr);
            fv[k] = v ? 1 : 0;
        });
        for (size_t k = 0; k < frag.size(); k++) fix[k] = Fix{(float)fx[k], (float)fy[k], fv[k] != 0};
    }
    std::vector<uint8_t> vh;  // visible_mask on the host, when this camera reads or writes it
    if (vis_p && (!frag.empty() || c.incl)) {
        vh.resize(total);
        HIP_CHECK(hipMemcpy(vh.data(), vis_p, total, hipMemcpyDeviceToHost));
    }
    std::vector<uint8_t> fvalid(frag.size());
    for (size_t k = 0; k < frag.size(); k++) {  // lut_build_kernel's per-pixel tail, in index order
        const uint32_t idx = frag[k];
        const bool claimed = !vh.empty() && vh[idx] == 1;
        if (!vh.empty() && fix[k].vis && !claimed) vh[idx] = 2;
        const float x = fix[k].x, y = fix[k].y;
        const bool valid = !(std::isnan(x) || std::isnan(y) || x < 0 || x >= 1.0f || y < 0 || y >= 1.0f || claimed);
        fvalid[k] = valid;
        if (valid) {
            const int h = (int)(idx / (uint32_t)W), w = (int)(idx - (uint32_t)h * (uint32_t)W);
            b[0] = std::min(b[0], w);
            b[1] = std::min(b[1], h);
            b[2] = std::max(b[2], w);
            b[3] = std::max(b[3], h);
        }
    }
    in.n_fragile = frag.size();
    // CV_Assert(min_h <= max_h && min_w <= max_w) (template.cpp:124)
    if (!(b[1] <= b[3] && b[0] <= b[2])) throw OctvrError(OCTVR_E_INVALID, "input camera covers no output pixel");
    int min_w = std::max(0, b[0] - 8), min_h = std::max(0, b[1] - 8);
    int max_w = std::min(W - 1, b[2] + 8), max_h = std::min(H - 1, b[3] + 8);
    int roi[4] = {min_w, min_h, max_w + 1 - min_w, max_h + 1 - min_h};
    if (!use_roi) {
        roi[0] = roi[1] = 0;
        roi[2] = W;
        roi[3] = H;
    }
    memcpy(in.roi, roi, sizeof roi);
    const size_t rn = (size_t)roi[2] * roi[3];
    in.map1.resize(rn);
    in.map2.resize(rn);
    in.mask.resize(rn);
    const size_t off = (size_t)roi[1] * W + roi[0];
    HIP_CHECK(hipMemcpy2D(in.map1.data(), roi[2] * sizeof(float), m1.p + off, W * sizeof(float), roi[2] * sizeof(float),
                          roi[3], hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy2D(in.map2.data(), roi[2] * sizeof(float), m2.p + off, W * sizeof(float), roi[2] * sizeof(float),
                          roi[3], hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy2D(in.mask.data(), roi[2], mk.p + off, W, roi[2], roi[3], hipMemcpyDeviceToHost));
    for (size_t k = 0; k < frag.size(); k++) {  // patch the recomputed pixels (every valid one is in the ROI)
        const uint32_t idx = frag[k];
        const int h = (int)(idx / (uint32_t)W), w = (int)(idx - (uint32_t)h * (uint32_t)W);
        const int rx = w - roi[0], ry = h - roi[1];
        if (rx < 0 || ry < 0 || rx >= roi[2] || ry >= roi[3]) continue;
        const size_t j = (size_t)ry * roi[2] + rx;
        in.mask[j] = fvalid[k] ? 255 : 0;
        in.map1[j] = fvalid[k] ? fix[k].x : -1.0f;
        in.map2[j] = fvalid[k] ? fix[k].y : -1.0f;
    }
    if (c.incl && priors) {  // pixels this camera claimed first (2) leave the earlier cameras' masks
        for (RigInput& p : *priors) {
            if (&p == &in) break;
            for (int y = 0; y < p.roi[3]; y++)
                for (int x = 0; x < p.roi[2]; x++)
                    if (vh[(size_t)(y + p.roi[1]) * W + x + p.roi[0]] == 2) p.mask[(size_t)y * p.roi[2] + x] = 0;
        }
    }
    if (c.incl) {
        for (uint8_t& v : vh) v = v ? 1 : 0;
        HIP_CHECK(hipMemcpy(vis_p, vh.data(), total, hipMemcpyHostToDevice));
    }
    const JsonValue& o = cam["options"];
    in.in_w = o.has("width") ? o["width"].as_int() : 0;
    in.in_h = o.has("height") ? o["height"].as_int() : 0;
    in.vignette = vignette_map(o, 512, 512);
    if (!in.vignette.empty()) in.vig_w = in.vig_h = 512;
}

}  // namespace

// MapperTemplate(to, to_opts, w, h) (template.cpp:23-44): the output camera and size
std::unique_ptr<octvr_rig> rig_new(const JsonValue& oc, int out_w, int out_h, int device) {
    CameraParams out_cam = camera_from_json(oc);
    REQUIRE(!(out_h <= 0 && out_w <= 0), "Output width/height invalid");  // template.cpp:32-33
    double ar = aspect_ratio(oc);
    if (out_h <= 0) out_h = int(double(out_w) / ar);
    if (out_w <= 0) out_w = int(double(out_h) * ar);
    // the output camera needs image_to_obj_single: fisheye / pinhole throw NotImplemented (camera.hpp:101-103)
    if (out_cam.type == CAM_FISHEYE || out_cam.type == CAM_PINHOLE)
        throw OctvrError(OCTVR_E_UNSUPPORTED, "output camera type '" + oc["type"].as_string() + "' is not supported");
    // CV_Assert(crop.size() == size && crop.tl() == Point(0, 0)) (fullframe_fisheye_cam.cpp:224)
    if (out_cam.type == CAM_FULLFRAME_FISHEYE)
        REQUIRE(out_cam.crop_x == 0 && out_cam.crop_y == 0 && out_cam.crop_w == out_cam.width &&
                    out_cam.crop_h == out_cam.height,
                "fullframe_fisheye output camera: crop must cover the whole image");
    auto rig = std::make_unique<octvr_rig>();
    rig->out_w = out_w;
    rig->out_h = out_h;
    rig->device = device;
    // the camera models stay with the rig for add_input / morph_controlpoints
    rig->has_cameras = true;
    rig->out_cam = out_cam;
    rig->out_cam_masks = oc.has("options") && (oc["options"].has("exclude_masks") || oc["options"].has("include_masks"));
    return rig;
}

// MapperTemplate::add_input(from, from_opts, overlay, use_roi) (template.cpp:46-153)
void rig_add(octvr_rig& rig, const JsonValue& cam, bool overlay, bool use_roi) {
    REQUIRE(rig.has_cameras, "add_input needs a template built from camera models (not a .dat)");
    REQUIRE(rig.inputs.size() + rig.overlays.size() < (size_t)kMaxCams, "too many inputs");
    std::vector<RigInput>& dst = overlay ? rig.overlays : rig.inputs;
    RigInput in;
    // overlays go through the same add_input: they share visible_mask and their include masks clear
    // the (non-overlay) inputs' masks (template.cpp:102-116, 147-150)
    build_input(rig.out_cam, cam, rig.out_w, rig.out_h, use_roi, rig.device, in, &rig.visible, &rig.inputs);
    dst.push_back(std::move(in));
    if (!overlay) rig.cams.push_back(camera_from_json(cam));
    rig.seam_masks.clear();  // one seam mask per input: create_masks again (dump does)
}

// camera {"type": type, "options": opts} from the C++ API's separate type / options arguments
JsonValue camera_json(const char* type, const char* opts_json, int flags) {
    REQUIRE(type && *type, "camera type is empty");
    for (const char* c = type; *c; c++)
        REQUIRE((*c >= 'a' && *c <= 'z') || (*c >= '0' && *c <= '9') || *c == '_', "bad camera type");
    const std::string text = std::string("{\"type\":\"") + type + "\",\"options\":" +
                             (opts_json && *opts_json ? opts_json : "{}") + "}";
    return json_parse(text, (flags & OCTVR_JSON_EXACT) != 0);
}

}  // namespace octvr
