// morph_plan_check — the per-camera plan of morph_controlpoints (opencv-octvr_amd/csrc/morph_plan.hpp: Subdiv2D
// triangles, warp matrices, the owner raster over csrc/fill_poly.hpp), built with -fsanitize=address,undefined (make -C
// opencv-octvr_amd lib/morph_plan_check) and run on the CPU.  Vertex sets put destination triangle corners left of,
// above, right of and below the ROI raster, whole triangles outside it, the raster down to one pixel wide or high,
// vertices onto duplicates and collinear rows and columns, and destination triangles onto a single point.  Checked:
// every owner lies in [-1, nt); the owner map is the brute-force "last triangle whose full-raster fill covers the
// pixel"; the triangles' corners are morph vertices and move to the first matching vertex's destination; a regular
// matrix takes the destination corners back to the source corners; a singular one is all zero, so morph_warp_kernel's
// coordinates of every pixel are source (0, 0) with fraction 0 (imgwarp.cpp:5655-5666, D != 0 ? 1/D : 0).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "morph_plan.hpp"

using octvr::MorphPlan;
using octvr::MorphPt;

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("line %d: %s\n", __LINE__, #c);                \
            fails++;                                              \
        }                                                         \
    } while (0)

static uint32_t rnd(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}
static float unit(uint32_t& s) { return (float)(rnd(s) & 0xFFFF) / 65536.f; }  // [0, 1)

struct Seen {
    int left = 0, above = 0, right = 0, below = 0, outside = 0, singular = 0, regular = 0, owned = 0, nt = 0;
};

// morph_warp_kernel's source cell and fractions of pixel (x, y) under matrix m (resize_kernels.hip)
static void warp_coords(const double* m, int x, int y, int* sx, int* sy, int* fx, int* fy) {
    auto rnd_i = [](double v) {
        const double r = std::nearbyint(v);
        return (r >= -2147483648.0 && r <= 2147483647.0) ? (int)r : INT32_MIN;
    };
    const int X0 = rnd_i((m[1] * (double)y + m[2]) * 1024.0) + 16, Y0 = rnd_i((m[4] * (double)y + m[5]) * 1024.0) + 16;
    const int ad = rnd_i(m[0] * (double)x * 1024.0), bd = rnd_i(m[3] * (double)x * 1024.0);
    const int X = (int)((uint32_t)X0 + (uint32_t)ad) >> 5, Y = (int)((uint32_t)Y0 + (uint32_t)bd) >> 5;
    *sx = X >> 5;
    *sy = Y >> 5;
    *fx = X & 31;
    *fy = Y & 31;
}

static Seen run(const std::vector<MorphPt>& sv, const std::vector<MorphPt>& dv, int rx, int ry, int rw, int rh, int W,
                int H) {
    Seen seen;
    const int roi[4] = {rx, ry, rw, rh};
    const MorphPlan P = octvr::morph_plan(sv, dv, roi, W, H);
    const int nt = P.nt();
    seen.nt = nt;
    CHECK(P.dst_tris.size() == P.src_tris.size());
    if (nt == 0) {
        CHECK(P.M.empty() && P.owner.empty());
        return seen;
    }
    CHECK(P.M.size() == (size_t)6 * nt && P.owner.size() == (size_t)rw * rh);
    if (P.M.size() != (size_t)6 * nt || P.owner.size() != (size_t)rw * rh) return seen;

    std::vector<int16_t> want((size_t)rw * rh, (int16_t)-1);
    std::vector<uint8_t> full((size_t)rw * rh);
    for (int k = 0; k < nt; k++) {
        float s[6], d[6];
        for (int c = 0; c < 3; c++) {
            const float sx = P.src_tris[6 * k + 2 * c], sy = P.src_tris[6 * k + 2 * c + 1];
            // a corner is a vertex, and moves where the first vertex at that position moves
            size_t j = 0;
            while (j < sv.size() && !(sv[j].x == sx && sv[j].y == sy)) j++;
            CHECK(j < sv.size());
            if (j < sv.size()) CHECK(P.dst_tris[6 * k + 2 * c] == dv[j].x && P.dst_tris[6 * k + 2 * c + 1] == dv[j].y);
            CHECK(sx >= 0.f && sx <= 1.f && sy >= 0.f && sy <= 1.f);
            s[2 * c] = sx * (float)W - (float)rx;
            s[2 * c + 1] = sy * (float)H - (float)ry;
            d[2 * c] = P.dst_tris[6 * k + 2 * c] * (float)W - (float)rx;
            d[2 * c + 1] = P.dst_tris[6 * k + 2 * c + 1] * (float)H - (float)ry;
        }
        int pts[6];
        octvr::morph_fill_points(d, pts);
        bool all_out = true;
        for (int c = 0; c < 3; c++) {
            const int x = pts[2 * c], y = pts[2 * c + 1];
            seen.left += x < 0;
            seen.above += y < 0;
            seen.right += x >= rw;
            seen.below += y >= rh;
            all_out = all_out && (x < 0 || y < 0 || x >= rw || y >= rh);
        }
        // the literal procedure: the triangle's fill over the whole raster, copied over what is there
        std::fill(full.begin(), full.end(), (uint8_t)0);
        octvr::fill_poly_u8(full.data(), rw, rh, pts, 3, 255);
        size_t covered = 0;
        for (size_t o = 0; o < full.size(); o++)
            if (full[o]) {
                want[o] = (int16_t)k;
                covered++;
            }
        seen.outside += all_out && covered == 0;

        const double* m = &P.M[(size_t)6 * k];
        const double area2 = std::fabs(((double)d[2] - d[0]) * ((double)d[5] - d[1]) - ((double)d[3] - d[1]) * ((double)d[4] - d[0]));
        const bool one_point = d[0] == 0.f && d[1] == 0.f && d[2] == 0.f && d[3] == 0.f && d[4] == 0.f && d[5] == 0.f;
        if (one_point) {
            // getAffineTransform's right-hand side is all zero: the forward matrix is, its determinant is, and so
            // the inverse warpAffine applies
            seen.singular++;
            for (int c = 0; c < 6; c++) CHECK(m[c] == 0.0);
            for (int y = 0; y < rh; y += (rh > 7 ? rh / 7 : 1))
                for (int x = 0; x < rw; x += (rw > 7 ? rw / 7 : 1)) {
                    int sx, sy, fx, fy;
                    warp_coords(m, x, y, &sx, &sy, &fx, &fy);
                    CHECK(sx == 0 && sy == 0 && fx == 0 && fy == 0);
                }
        } else if (area2 >= 8.0) {
            seen.regular++;
            for (int c = 0; c < 3; c++) {
                const double bx = m[0] * d[2 * c] + m[1] * d[2 * c + 1] + m[2], by = m[3] * d[2 * c] + m[4] * d[2 * c + 1] + m[5];
                CHECK(std::fabs(bx - s[2 * c]) < 1e-4 && std::fabs(by - s[2 * c + 1]) < 1e-4);
            }
        }
        for (int c = 0; c < 6; c++) CHECK(std::isfinite(m[c]));
    }
    size_t diff = 0;
    for (size_t o = 0; o < want.size(); o++) {
        CHECK(P.owner[o] >= -1 && P.owner[o] < nt);
        diff += P.owner[o] != want[o];
        seen.owned += P.owner[o] >= 0;
    }
    CHECK(diff == 0);
    return seen;
}

// n random vertices, each moved by up to `move` (kept inside [0, 1))
static void scatter(std::vector<MorphPt>& sv, std::vector<MorphPt>& dv, int n, float move, uint32_t seed) {
    for (int k = 0; k < n; k++) {
        const MorphPt p{0.02f + 0.96f * unit(seed), 0.02f + 0.96f * unit(seed)};
        MorphPt q{p.x + move * (2.f * unit(seed) - 1.f), p.y + move * (2.f * unit(seed) - 1.f)};
        q.x = std::min(std::max(q.x, 0.f), 0.999f);
        q.y = std::min(std::max(q.y, 0.f), 0.999f);
        sv.push_back(p);
        dv.push_back(q);
    }
}

int main() {
    const int W = 256, H = 256;
    {  // an ROI in the middle of the output: corners off every side, triangles wholly outside
        std::vector<MorphPt> sv, dv;
        scatter(sv, dv, 70, 0.05f, 1u);
        const Seen a = run(sv, dv, 60, 50, 80, 70, W, H);
        CHECK(a.nt > 100 && a.left > 0 && a.above > 0 && a.right > 0 && a.below > 0 && a.outside > 0 && a.owned > 0 &&
              a.regular > 0);
        // the same vertices over the whole output, moved far: folds
        std::vector<MorphPt> sf, df;
        scatter(sf, df, 70, 0.2f, 2u);
        const Seen b = run(sf, df, 0, 0, W, H, W, H);
        CHECK(b.nt > 100 && b.owned > 0);
        // odd ROI, odd origin
        const Seen c = run(sf, df, 33, 17, 131, 77, W, H);
        CHECK(c.left > 0 && c.above > 0 && c.right > 0 && c.below > 0);
    }
    {  // rasters one pixel wide, one pixel high, one pixel
        std::vector<MorphPt> sv, dv;
        scatter(sv, dv, 40, 0.08f, 3u);
        const Seen a = run(sv, dv, 128, 10, 1, 200, W, H);
        const Seen b = run(sv, dv, 10, 128, 200, 1, W, H);
        const Seen c = run(sv, dv, 128, 128, 1, 1, W, H);
        CHECK(a.owned > 0 && b.owned > 0 && c.nt == a.nt && a.left > 0 && a.right > 0 && b.above > 0 && b.below > 0);
        // triangles one pixel wide: pairs of vertices whose destinations round to neighbouring columns
        std::vector<MorphPt> ss, ds;
        for (int k = 0; k < 12; k++) {
            const float y = 0.1f + 0.07f * (float)k;
            ss.push_back(MorphPt{0.3f, y});
            ds.push_back(MorphPt{0.5f, y});
            ss.push_back(MorphPt{0.7f, y + 0.03f});
            ds.push_back(MorphPt{0.5f + 1.f / 256, y + 0.03f});
        }
        const Seen d = run(ss, ds, 0, 0, W, H, W, H);
        CHECK(d.nt > 10 && d.owned > 0);
    }
    {  // duplicates (the first one's destination counts), collinear rows and columns, points on existing edges
        std::vector<MorphPt> sv, dv;
        for (int k = 0; k < 3; k++) {
            sv.push_back(MorphPt{0.4f, 0.4f});
            dv.push_back(MorphPt{0.4f + 0.05f * (float)k, 0.45f});
        }
        for (int k = 0; k < 7; k++) {
            sv.push_back(MorphPt{0.1f + 0.125f * (float)k, 0.25f});
            dv.push_back(MorphPt{0.1f + 0.125f * (float)k, 0.25f + 0.01f * (float)k});
            sv.push_back(MorphPt{0.75f, 0.1f + 0.125f * (float)k});
            dv.push_back(MorphPt{0.7f, 0.1f + 0.125f * (float)k});
        }
        for (int k = 0; k <= 10; k++) {  // a frame as the morph's: 11 points on each horizontal edge, 9 on the vertical ones
            const float t = 0.05f + 0.09f * (float)k;
            for (const MorphPt p : {MorphPt{t, 0.05f}, MorphPt{t, 0.95f}}) {
                sv.push_back(p);
                dv.push_back(p);
            }
            if (k == 0 || k == 10) continue;
            for (const MorphPt p : {MorphPt{0.05f, t}, MorphPt{0.95f, t}}) {
                sv.push_back(p);
                dv.push_back(p);
            }
        }
        const Seen a = run(sv, dv, 0, 0, W, H, W, H);
        const Seen b = run(sv, dv, 90, 40, 101, 99, W, H);
        CHECK(a.nt > 40 && a.owned > 0 && b.owned > 0);
    }
    {  // destination triangles on one point, the ROI's origin: singular, the all-zero matrix
        std::vector<MorphPt> sv, dv;
        scatter(sv, dv, 30, 0.03f, 5u);
        for (const MorphPt p : {MorphPt{0.45f, 0.45f}, MorphPt{0.55f, 0.45f}, MorphPt{0.5f, 0.55f}, MorphPt{0.5f, 0.48f}}) {
            sv.push_back(p);
            dv.push_back(MorphPt{0.25f, 0.125f});  // (64, 32) of 256 x 256
        }
        const Seen a = run(sv, dv, 64, 32, 120, 90, W, H);
        CHECK(a.singular > 0 && a.regular > 0);
        // warp_matrix alone: collinear source corners leave the LU solve without a solution
        const float s[6] = {1.f, 1.f, 2.f, 2.f, 3.f, 3.f}, d[6] = {0.f, 0.f, 5.f, 0.f, 0.f, 5.f};
        double M[6];
        octvr::warp_matrix(s, d, M);
        for (int c = 0; c < 6; c++) CHECK(M[c] == 0.0);
    }
    {  // nothing to triangulate, and what the plan refuses
        const Seen a = run({}, {}, 0, 0, W, H, W, H);
        CHECK(a.nt == 0);
        int thrown = 0;
        const int roi[4] = {0, 0, W, H}, none[4] = {0, 0, 0, H};
        for (int k = 0; k < 4; k++) {
            std::vector<MorphPt> sv{{0.2f, 0.2f}, {0.8f, 0.3f}, {0.5f, 0.9f}}, dv = sv;
            if (k == 0) sv[1].x = 1.f;  // outside Subdiv2D's [0, 1) x [0, 1)
            if (k == 1) sv[2].y = -0.01f;
            if (k == 2) dv.pop_back();
            try {
                (void)octvr::morph_plan(sv, dv, k == 3 ? none : roi, W, H);
            } catch (const octvr::MorphPlanError&) {
                thrown++;
            }
        }
        CHECK(thrown == 4);
    }
    if (fails) {
        printf("morph_plan_check: %d failures\n", fails);
        return 1;
    }
    printf("morph_plan_check ok\n");
    return 0;
}
