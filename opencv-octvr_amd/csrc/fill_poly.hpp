// fill_poly.hpp — cv::fillPoly(mask, {points}, color) with lineType 8, shift 0 (imgproc/src/drawing.cpp:1894-1917 ->
// CollectPolyEdges :1196-1248 -> FillEdgeCollection :1262-1405; every polygon edge is also drawn by Line :239-265 /
// LineIterator :153-236 with clipLine :80-137) on a packed 8-bit image: host arithmetic only, no HIP, so the camera masks
// (masks.cpp, rig_json.cpp), the morph plan (morph_plan.hpp) and tests/cpp/morph_plan_check.cpp share one copy.
// Internal header.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace octvr {

namespace fill_poly_detail {

constexpr int kXYShift = 16, kXYOne = 1 << kXYShift;  // drawing.cpp:46
// v << XY_SHIFT of a coordinate that may be negative (a polygon corner left of the image): the same bits, shifted
// as unsigned because C++17 leaves the signed shift of a negative value undefined
inline int to_fixed(int v) { return (int)((uint32_t)v << kXYShift); }

// clipLine(Size, pt1, pt2) (drawing.cpp:80-137): Cohen-Sutherland against [0,w-1]x[0,h-1] in int64.
inline bool clip_segment(int w, int h, int& ax, int& ay, int& bx, int& by) {
    if (w <= 0 || h <= 0) return false;
    int64_t x1 = ax, y1 = ay, x2 = bx, y2 = by;
    const int64_t right = w - 1, bottom = h - 1;
    auto code = [&](int64_t x, int64_t y) { return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8; };
    int c1 = code(x1, y1), c2 = code(x2, y2);
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        if (c1 & 12) {
            const int64_t a = c1 < 8 ? 0 : bottom;
            x1 += (a - y1) * (x2 - x1) / (y2 - y1);
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            const int64_t a = c2 < 8 ? 0 : bottom;
            x2 += (a - y2) * (x2 - x1) / (y2 - y1);
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                const int64_t a = c1 == 1 ? 0 : right;
                y1 += (a - x1) * (y2 - y1) / (x2 - x1);
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                const int64_t a = c2 == 1 ? 0 : right;
                y2 += (a - x2) * (y2 - y1) / (x2 - x1);
                x2 = a;
                c2 = 0;
            }
        }
        ax = (int)x1;
        ay = (int)y1;
        bx = (int)x2;
        by = (int)y2;
    }
    return (c1 | c2) == 0;
}

// Line(img, pt1, pt2, color, 8) through LineIterator(connectivity 8, left_to_right): Bresenham with
// a major step every pixel and the minor step added while err < 0.
inline void draw_segment(uint8_t* img, int w, int h, int ax, int ay, int bx, int by, uint8_t color) {
    if ((unsigned)ax >= (unsigned)w || (unsigned)bx >= (unsigned)w || (unsigned)ay >= (unsigned)h ||
        (unsigned)by >= (unsigned)h)
        if (!clip_segment(w, h, ax, ay, bx, by)) return;
    int dx = bx - ax, dy = by - ay;
    if (dx < 0) {  // left_to_right: start from pt2, flip both deltas
        dx = -dx;
        dy = -dy;
        ax = bx;
        ay = by;
    }
    const int ystep = dy < 0 ? -1 : 1;
    dy = dy < 0 ? -dy : dy;
    int major_x = 1, major_y = 0, minor_x = 0, minor_y = ystep;  // minusStep / plusStep
    if (dy > dx) {
        std::swap(dx, dy);
        major_x = 0;
        major_y = ystep;
        minor_x = 1;
        minor_y = 0;
    }
    int err = dx - (dy + dy);
    const int plus_delta = dx + dx, minus_delta = -(dy + dy);
    int x = ax, y = ay;
    for (int i = 0; i <= dx; i++) {
        img[(size_t)y * w + x] = color;
        const bool m = err < 0;
        err += minus_delta + (m ? plus_delta : 0);
        x += major_x + (m ? minor_x : 0);
        y += major_y + (m ? minor_y : 0);
    }
}

struct Edge {
    int y0, y1, x, dx;
    int next;  // index into the edge table, -1 = end of the active list
};

}  // namespace fill_poly_detail

// cv::fillPoly(img, {pts}, color) on a w x h CV_8U image, lineType 8, shift 0; pts = x0,y0,x1,y1,...
inline void fill_poly_u8(uint8_t* img, int w, int h, const int* pts, int npts, uint8_t color) {
    using namespace fill_poly_detail;
    if (npts <= 0) return;
    // CollectPolyEdges (shift 0, no offset): x in 16.16 fixed point, every edge also drawn as a line
    std::vector<Edge> edges;
    edges.reserve(npts + 2);
    int px0 = to_fixed(pts[2 * (npts - 1)]), py0 = pts[2 * (npts - 1) + 1];
    for (int i = 0; i < npts; i++) {
        const int px1 = to_fixed(pts[2 * i]), py1 = pts[2 * i + 1];
        draw_segment(img, w, h, (px0 + (kXYOne >> 1)) >> kXYShift, py0, (px1 + (kXYOne >> 1)) >> kXYShift, py1, color);
        if (py0 != py1) {
            Edge e;
            if (py0 < py1) {
                e.y0 = py0;
                e.y1 = py1;
                e.x = px0;
            } else {
                e.y0 = py1;
                e.y1 = py0;
                e.x = px1;
            }
            e.dx = (px1 - px0) / (py1 - py0);
            e.next = -1;
            edges.push_back(e);
        }
        px0 = px1;
        py0 = py1;
    }
    // FillEdgeCollection
    const int total = (int)edges.size();
    if (total < 2) return;
    int y_max = INT_MIN, x_max = INT_MIN, y_min = INT_MAX, x_min = INT_MAX;
    for (const Edge& e : edges) {
        const int x1 = e.x + (e.y1 - e.y0) * e.dx;
        y_min = std::min(y_min, e.y0);
        y_max = std::max(y_max, e.y1);
        x_min = std::min({x_min, e.x, x1});
        x_max = std::max({x_max, e.x, x1});
    }
    if (y_max < 0 || y_min >= h || x_max < 0 || x_min >= (w << kXYShift)) return;
    std::sort(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) {
        return a.y0 - b.y0 ? a.y0 < b.y0 : a.x - b.x ? a.x < b.x : a.dx < b.dx;
    });
    Edge sentinel{INT_MAX, 0, 0, 0, -1};
    edges.push_back(sentinel);   // [total]: stops the insertion scan
    edges.push_back(sentinel);   // [total+1]: head of the active list
    const int head = total + 1;
    edges[head].next = -1;
    int i = 0, cur = 0;
    y_max = std::min(y_max, h);
    for (int y = edges[cur].y0; y < y_max; y++) {
        int prelast = head, last = edges[head].next, keep;
        int sort_flag = 0, draw = 0;
        const bool clipline = y < 0;
        while (last >= 0 || edges[cur].y0 == y) {
            if (last >= 0 && edges[last].y1 == y) {  // edge ends on this row: unlink it
                edges[prelast].next = edges[last].next;
                last = edges[last].next;
                continue;
            }
            keep = prelast;
            if (last >= 0 && (edges[cur].y0 > y || edges[last].x < edges[cur].x)) {
                prelast = last;
                last = edges[last].next;
            } else if (i < total) {  // edge starts on this row: link it before `last`
                edges[prelast].next = cur;
                edges[cur].next = last;
                prelast = cur;
                cur = ++i;
            } else {
                break;
            }
            if (draw) {
                if (!clipline) {
                    int x1 = edges[keep].x, x2 = edges[prelast].x;
                    if (x1 > x2) std::swap(x1, x2);
                    x1 = (x1 + kXYOne - 1) >> kXYShift;
                    x2 = x2 >> kXYShift;
                    if (x1 < w && x2 >= 0) {
                        x1 = std::max(x1, 0);
                        x2 = std::min(x2, w - 1);
                        memset(img + (size_t)y * w + x1, color, (size_t)(x2 - x1 + 1));
                    }
                }
                edges[keep].x += edges[keep].dx;
                edges[prelast].x += edges[prelast].dx;
            }
            draw ^= 1;
        }
        // bubble-sort the active list by x
        keep = -1;
        do {
            prelast = head;
            last = edges[head].next;
            while (last != keep && edges[last].next >= 0) {
                const int te = edges[last].next;
                if (edges[last].x > edges[te].x) {
                    edges[prelast].next = te;
                    edges[last].next = edges[te].next;
                    edges[te].next = last;
                    prelast = te;
                    sort_flag = 1;
                } else {
                    prelast = last;
                    last = te;
                }
            }
            keep = prelast;
        } while (sort_flag && keep != edges[head].next && keep != head);
    }
}

}  // namespace octvr
