// morph_plan.hpp — the per-camera plan of morph_controlpoints' warp (template_morph.cpp:22-67, 184-231), on host
// arrays only: no HIP, no rig.  From a camera's source and destination vertices (control points plus frame), its
// ROI and the output size: the Delaunay triangles (cv::Subdiv2D restated), each triangle's warpAffine matrix
// (cv::getAffineTransform + cv::solve LU, inverted) and the int16 owner of every ROI pixel, the last triangle whose
// fillPoly covers it.  morph.cpp uploads the plan for morph_warp_kernel; tests/cpp/morph_plan_check.cpp runs it
// under the sanitizers.  Internal header.
#pragma once

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "fill_poly.hpp"

namespace octvr {

struct MorphPlanError : std::invalid_argument {
    using std::invalid_argument::invalid_argument;
};

// ---- cv::Subdiv2D (imgproc/src/subdivision2d.cpp), Delaunay by incremental insertion on a
// quad-edge structure.  Restated with the same edge / vertex numbering, free lists and walk order,
// because getTriangleList enumerates edges by index (including freed ones, whose stale links it
// follows) — the triangle list, its order and its corner order all depend on them.
class Subdivision {
public:
    // Subdiv2D(Rect(0, 0, 1, 1)) -> initDelaunay (:560-600)
    Subdivision() {
        const float big = 3.f;  // 3 * max(width, height)
        tl_x_ = tl_y_ = 0.f;
        br_x_ = br_y_ = 1.f;
        vtx_.push_back(Vertex());
        qe_.push_back(QuadEdge());
        free_qe_ = free_pt_ = 0;
        const int a = new_point(big, 0.f, false), b = new_point(0.f, big, false), c = new_point(-big, -big, false);
        const int ab = new_edge(), bc = new_edge(), ca = new_edge();
        set_points(ab, a, b);
        set_points(bc, b, c);
        set_points(ca, c, a);
        splice(ab, sym(ca));
        splice(bc, sym(ab));
        splice(ca, sym(bc));
        recent_ = ab;
    }

    // Subdiv2D::insert (:405-480)
    void insert(float x, float y) {
        int edge = 0, vertex = 0;
        const int loc = locate(x, y, edge, vertex);
        if (loc == kLocError) throw MorphPlanError("Subdiv2D: point location failed");
        if (loc == kLocVertex) return;
        if (loc == kLocOnEdge) {
            const int deleted = edge;
            recent_ = edge = get_edge(edge, kPrevAroundOrg);
            delete_edge(deleted);
        }
        const int pt = new_point(x, y, false);
        int base = new_edge();
        const int first = org(edge);
        set_points(base, first, pt);
        splice(base, edge);
        do {
            base = connect(edge, sym(base));
            edge = get_edge(base, kPrevAroundOrg);
        } while (dst(edge) != first);
        edge = get_edge(base, kPrevAroundOrg);
        const int max_edges = (int)qe_.size() * 4;
        for (int i = 0; i < max_edges; i++) {
            const int t = get_edge(edge, kPrevAroundOrg);
            const int t_dst = dst(t), e_org = org(edge), e_dst = dst(edge);
            if (right_of(vtx_[t_dst].x, vtx_[t_dst].y, edge) > 0 &&
                in_circle(vtx_[e_org], vtx_[t_dst], vtx_[e_dst], vtx_[pt]) < 0) {
                swap_edge(edge);
                edge = get_edge(edge, kPrevAroundOrg);
            } else if (e_org == first) {
                break;
            } else {
                edge = get_edge(next(edge), kPrevAroundLeft);
            }
        }
    }

    // Subdiv2D::getTriangleList (:735-760): every even edge not yet visited starts a left-face walk
    std::vector<std::array<float, 6>> triangles() const {
        std::vector<std::array<float, 6>> out;
        const int total = (int)qe_.size() * 4;
        std::vector<char> seen(total, 0);
        auto mark = [&](int e) {
            if (e < 0 || e >= total) throw MorphPlanError("Subdiv2D: corrupt edge list");
            seen[e] = 1;
        };
        for (int i = 4; i < total; i += 2) {
            if (seen[i]) continue;
            std::array<float, 6> t;
            int e = i;
            const Vertex& a = vtx_.at(org(e));
            mark(e);
            e = get_edge(e, kNextAroundLeft);
            const Vertex& b = vtx_.at(org(e));
            mark(e);
            e = get_edge(e, kNextAroundLeft);
            const Vertex& c = vtx_.at(org(e));
            mark(e);
            t = {a.x, a.y, b.x, b.y, c.x, c.y};
            out.push_back(t);
        }
        return out;
    }

private:
    enum { kLocError = -2, kLocInside = 0, kLocVertex = 1, kLocOnEdge = 2 };
    enum { kNextAroundLeft = 0x13, kPrevAroundOrg = 0x11, kPrevAroundDst = 0x33, kPrevAroundLeft = 0x20 };
    struct QuadEdge {
        int next[4] = {0, 0, 0, 0};
        int pt[4] = {0, 0, 0, 0};
    };
    struct Vertex {
        float x = 0.f, y = 0.f;
        int first = 0;
        int type = -1;
    };
    std::vector<QuadEdge> qe_;
    std::vector<Vertex> vtx_;
    int free_qe_ = 0, free_pt_ = 0, recent_ = 0;
    float tl_x_, tl_y_, br_x_, br_y_;

    QuadEdge& q(int e) { return qe_.at((size_t)(e >> 2)); }
    const QuadEdge& q(int e) const { return qe_.at((size_t)(e >> 2)); }
    int next(int e) const { return q(e).next[e & 3]; }
    static int rot(int e, int r) { return (e & ~3) + ((e + r) & 3); }
    static int sym(int e) { return e ^ 2; }
    int get_edge(int e, int type) const {  // :63-68
        e = q(e).next[(e + type) & 3];
        return (e & ~3) + ((e + (type >> 4)) & 3);
    }
    int org(int e) const { return q(e).pt[e & 3]; }
    int dst(int e) const { return q(e).pt[(e + 2) & 3]; }

    void splice(int a, int b) {  // :160-170
        int& an = q(a).next[a & 3];
        int& bn = q(b).next[b & 3];
        const int ar = rot(an, 1), br = rot(bn, 1);
        int& arn = q(ar).next[ar & 3];
        int& brn = q(br).next[br & 3];
        std::swap(an, bn);
        std::swap(arn, brn);
    }
    void set_points(int e, int o, int d) {  // :172-178
        q(e).pt[e & 3] = o;
        q(e).pt[(e + 2) & 3] = d;
        vtx_.at(o).first = e;
        vtx_.at(d).first = e ^ 2;
    }
    int connect(int a, int b) {  // :180-189
        const int e = new_edge();
        splice(e, get_edge(a, kNextAroundLeft));
        splice(sym(e), b);
        set_points(e, dst(a), org(b));
        return e;
    }
    void swap_edge(int e) {  // :191-204
        const int s = sym(e);
        const int a = get_edge(e, kPrevAroundOrg), b = get_edge(s, kPrevAroundOrg);
        splice(e, a);
        splice(s, b);
        set_points(e, dst(a), dst(b));
        splice(e, get_edge(a, kNextAroundLeft));
        splice(s, get_edge(b, kNextAroundLeft));
    }
    // triangleArea (:206-209), in double from the float coordinates
    static double area(double ax, double ay, double bx, double by, double cx, double cy) {
        return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    }
    int right_of(float px, float py, int e) const {  // isRightOf (:211-219)
        const Vertex& o = vtx_.at(org(e));
        const Vertex& d = vtx_.at(dst(e));
        const double a = area(px, py, d.x, d.y, o.x, o.y);
        return (a > 0) - (a < 0);
    }
    int new_edge() {  // :221-233
        if (free_qe_ <= 0) {
            qe_.push_back(QuadEdge());
            free_qe_ = (int)qe_.size() - 1;
        }
        const int e = free_qe_ * 4;
        free_qe_ = q(e).next[1];
        QuadEdge& n = q(e);
        n.next[0] = e;
        n.next[1] = e + 3;
        n.next[2] = e + 2;
        n.next[3] = e + 1;
        n.pt[0] = n.pt[1] = n.pt[2] = n.pt[3] = 0;
        return e;
    }
    void delete_edge(int e) {  // :235-247
        splice(e, get_edge(e, kPrevAroundOrg));
        const int s = sym(e);
        splice(s, get_edge(s, kPrevAroundOrg));
        QuadEdge& d = q(e);
        d.next[0] = 0;
        d.next[1] = free_qe_;
        free_qe_ = e >> 2;
    }
    int new_point(float x, float y, bool is_virtual) {  // :249-262
        if (free_pt_ == 0) {
            vtx_.push_back(Vertex());
            free_pt_ = (int)vtx_.size() - 1;
        }
        const int v = free_pt_;
        free_pt_ = vtx_[v].first;
        vtx_[v] = Vertex{x, y, 0, is_virtual ? 1 : 0};
        return v;
    }

    // Subdiv2D::locate (:272-383)
    int locate(float px, float py, int& out_edge, int& out_vertex) {
        if (qe_.size() < 4) throw MorphPlanError("Subdiv2D: subdivision is empty");
        if (px < tl_x_ || py < tl_y_ || px >= br_x_ || py >= br_y_)
            throw MorphPlanError("Subdiv2D: point outside [0,1) x [0,1)");
        int e = recent_;
        if (e <= 0) throw MorphPlanError("Subdiv2D: no current edge");
        int loc = kLocError, vertex = 0;
        int r_cur = right_of(px, py, e);
        if (r_cur > 0) {
            e = sym(e);
            r_cur = -r_cur;
        }
        const int max_edges = (int)qe_.size() * 4;
        for (int i = 0; i < max_edges; i++) {
            const int onext = next(e), dprev = get_edge(e, kPrevAroundDst);
            const int r_onext = right_of(px, py, onext), r_dprev = right_of(px, py, dprev);
            if (r_dprev > 0) {
                if (r_onext > 0 || (r_onext == 0 && r_cur == 0)) {
                    loc = kLocInside;
                    break;
                }
                r_cur = r_onext;
                e = onext;
            } else if (r_onext > 0) {
                if (r_dprev == 0 && r_cur == 0) {
                    loc = kLocInside;
                    break;
                }
                r_cur = r_dprev;
                e = dprev;
            } else if (r_cur == 0 && right_of(vtx_.at(dst(onext)).x, vtx_.at(dst(onext)).y, e) >= 0) {
                e = sym(e);
            } else {
                r_cur = r_onext;
                e = onext;
            }
        }
        recent_ = e;
        if (loc == kLocInside) {
            const Vertex& o = vtx_.at(org(e));
            const Vertex& d = vtx_.at(dst(e));
            // differences in float (Point2f arithmetic), sums in double
            double t1 = std::fabs(px - o.x);
            t1 += std::fabs(py - o.y);
            double t2 = std::fabs(px - d.x);
            t2 += std::fabs(py - d.y);
            double t3 = std::fabs(o.x - d.x);
            t3 += std::fabs(o.y - d.y);
            if (t1 < FLT_EPSILON) {
                loc = kLocVertex;
                vertex = org(e);
                e = 0;
            } else if (t2 < FLT_EPSILON) {
                loc = kLocVertex;
                vertex = dst(e);
                e = 0;
            } else if ((t1 < t3 || t2 < t3) && std::fabs(area(px, py, o.x, o.y, d.x, d.y)) < FLT_EPSILON) {
                loc = kLocOnEdge;
                vertex = 0;
            }
        }
        if (loc == kLocError) e = vertex = 0;
        out_edge = e;
        out_vertex = vertex;
        return loc;
    }

    // isPtInCircle3 (:386-397)
    static int in_circle(const Vertex& pt, const Vertex& a, const Vertex& b, const Vertex& c) {
        const double eps = FLT_EPSILON * 0.125;
        double v = ((double)a.x * a.x + (double)a.y * a.y) * area(b.x, b.y, c.x, c.y, pt.x, pt.y);
        v -= ((double)b.x * b.x + (double)b.y * b.y) * area(a.x, a.y, c.x, c.y, pt.x, pt.y);
        v += ((double)c.x * c.x + (double)c.y * c.y) * area(a.x, a.y, b.x, b.y, pt.x, pt.y);
        v -= ((double)pt.x * pt.x + (double)pt.y * pt.y) * area(a.x, a.y, b.x, b.y, c.x, c.y);
        return v > eps ? 1 : v < -eps ? -1 : 0;
    }
};

// LUImpl (core/src/matrix_decomp.cpp:50-110) as cv::solve(DECOMP_LU) runs it for n > 3; a
// singular system leaves the solution zero (lapack.cpp:1317-1318).
inline void solve_lu(double* A, double* b, int n) {
    const double eps = DBL_EPSILON * 100;
    for (int i = 0; i < n; i++) {
        int k = i;
        for (int j = i + 1; j < n; j++)
            if (std::fabs(A[j * n + i]) > std::fabs(A[k * n + i])) k = j;
        if (std::fabs(A[k * n + i]) < eps) {
            std::fill(b, b + n, 0.0);
            return;
        }
        if (k != i) {
            for (int j = i; j < n; j++) std::swap(A[i * n + j], A[k * n + j]);
            std::swap(b[i], b[k]);
        }
        const double d = -1 / A[i * n + i];
        for (int j = i + 1; j < n; j++) {
            const double alpha = A[j * n + i] * d;
            for (int c = i + 1; c < n; c++) A[j * n + c] += alpha * A[i * n + c];
            b[j] += alpha * b[i];
        }
        A[i * n + i] = -d;
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = b[i];
        for (int c = i + 1; c < n; c++) s -= A[i * n + c] * b[c];
        b[i] = s * A[i * n + i];
    }
}

// cv::getAffineTransform(src, dst) (imgproc/src/imgwarp.cpp:6340-6361), then the inversion
// warpAffine applies without WARP_INVERSE_MAP (:5655-5666): the result maps destination pixels to
// source positions.
inline void warp_matrix(const float* s, const float* d, double* M) {
    double a[36], b[6];
    for (int i = 0; i < 3; i++) {
        const int j = i * 12, k = i * 12 + 6;
        a[j] = a[k + 3] = s[2 * i];
        a[j + 1] = a[k + 4] = s[2 * i + 1];
        a[j + 2] = a[k + 5] = 1;
        a[j + 3] = a[j + 4] = a[j + 5] = 0;
        a[k] = a[k + 1] = a[k + 2] = 0;
        b[i * 2] = d[2 * i];
        b[i * 2 + 1] = d[2 * i + 1];
    }
    solve_lu(a, b, 6);
    for (int k = 0; k < 6; k++) M[k] = b[k];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11;
    M[1] *= -D;
    M[3] *= -D;
    M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1;
    M[5] = b2;
}

struct MorphPt {
    float x, y;
};

struct MorphPlan {
    std::vector<float> src_tris, dst_tris;  // 6 floats per triangle, output-normalised (octvr.hpp:60)
    std::vector<double> M;                  // 6 per triangle: ROI pixel -> source position
    std::vector<int16_t> owner;             // roi w x h: the triangle a pixel is computed from, -1 = kept as it is
    int nt() const { return (int)(src_tris.size() / 6); }
};

// The rounded ROI-local corners of a destination triangle, as fillPoly receives them (:208-214).
inline void morph_fill_points(const float* d, int* pts) {
    for (int c = 0; c < 6; c++) pts[c] = (int)std::round(d[c]);
}

// sv[j] -> dv[j]: vertex j's position before and after the morph (output-normalised).  roi: x, y, w, h of the
// camera in the W x H output.  No triangle (nt() == 0): M and owner stay empty, there is nothing to warp.
inline MorphPlan morph_plan(const std::vector<MorphPt>& sv, const std::vector<MorphPt>& dv, const int roi[4], int W,
                            int H) {
    MorphPlan P;
    if (sv.size() != dv.size()) throw MorphPlanError("morph plan: vertex lists differ in length");
    if (roi[2] <= 0 || roi[3] <= 0 || W <= 0 || H <= 0) throw MorphPlanError("morph plan: empty ROI or output");
    // getTriangleList (:22-41): Delaunay of the source vertices, triangles with a corner outside
    // [0, 1]^2 (those touching the three far initial vertices) dropped
    Subdivision sub;
    for (const MorphPt& p : sv) sub.insert(p.x, p.y);
    for (const auto& t : sub.triangles()) {
        bool inside = true;
        for (float c : t) inside = inside && c >= 0.0 && c <= 1.0;
        if (!inside) continue;
        // getTriangleListIndexes / FromIndexes (:43-67): corners by exact equality, first match
        for (int c = 0; c < 6; c++) P.src_tris.push_back(t[c]);
        for (int c = 0; c < 3; c++) {
            size_t j = 0;
            while (j < sv.size() && !(sv[j].x == t[2 * c] && sv[j].y == t[2 * c + 1])) j++;
            if (j == sv.size()) throw MorphPlanError("triangle corner is not a morph vertex");
            P.dst_tris.push_back(dv[j].x);
            P.dst_tris.push_back(dv[j].y);
        }
    }
    const int nt = P.nt();
    if (nt == 0) return P;
    if (nt >= 32767) throw MorphPlanError("too many morph triangles");

    // per triangle: warp matrix and fillPoly'd ownership (:202-231): later triangles overwrite
    const int rw = roi[2], rh = roi[3];
    auto Tx = [&](float x) { return x * (float)W - (float)roi[0]; };
    auto Ty = [&](float y) { return y * (float)H - (float)roi[1]; };
    P.M.resize((size_t)nt * 6);
    P.owner.assign((size_t)rw * rh, (int16_t)-1);
    std::vector<uint8_t> scratch((size_t)rw * rh, 0);
    for (int k = 0; k < nt; k++) {
        float s[6], d[6];
        for (int c = 0; c < 3; c++) {
            s[2 * c] = Tx(P.src_tris[6 * k + 2 * c]);
            s[2 * c + 1] = Ty(P.src_tris[6 * k + 2 * c + 1]);
            d[2 * c] = Tx(P.dst_tris[6 * k + 2 * c]);
            d[2 * c + 1] = Ty(P.dst_tris[6 * k + 2 * c + 1]);
        }
        warp_matrix(s, d, &P.M[(size_t)6 * k]);
        int pts[6];
        morph_fill_points(d, pts);
        fill_poly_u8(scratch.data(), rw, rh, pts, 3, 255);
        // the fill stays inside the corners' bounding box: only that part of the scratch is scanned and cleared
        const int x0 = std::max(0, std::min({pts[0], pts[2], pts[4]})), x1 = std::min(rw - 1, std::max({pts[0], pts[2], pts[4]}));
        const int y0 = std::max(0, std::min({pts[1], pts[3], pts[5]})), y1 = std::min(rh - 1, std::max({pts[1], pts[3], pts[5]}));
        for (int y = y0; y <= y1; y++)
            for (int x = x0; x <= x1; x++) {
                uint8_t& m = scratch[(size_t)y * rw + x];
                if (m) {
                    P.owner[(size_t)y * rw + x] = (int16_t)k;
                    m = 0;
                }
            }
    }
    return P;
}

}  // namespace octvr
