// multiband_plan.hpp — the per-rig plan of the multi-band / feather blend, on host arrays only: no HIP, no
// environment, no device pointers.  multiband_host.cpp fills an MbPlan stage by stage and uploads it;
// tests/cpp/multiband_plan_check.cpp runs the same stages on small rigs and checks each rule pixel by pixel.
//
// The stages (each indexes weights and tables by offsets kept in the plan):
//   mb_plan_rects        rectangles exactly as the reference: result ROI, align_result_roi (multiples of 2^B), per
//                        camera align_rois with the 5 * 2^B gap (blenders.cpp:595-618); per level the grid, its
//                        128 x 8 tiles and each camera's rectangle and place in the level's pyramid allocation
//   mb_seam_weights /    level-0 weights laid out over each camera's rectangle.  Levels 1..B are an input of
//   mb_feather_weights   mb_plan: the K4 pyrDown of seam / 255 in f32, one array per level
//   mb_plan              block activity and pixel owners, pyrUp tap tables, sub-tile kinds, required blocks and
//                        tiles, the work lists, down items and level-0 remap jobs
// "Required": a camera's Gaussian level is computed only on the tiles that its blend reads (its weight tiles, the
// pyrUp support of its finer level's weight tiles) and, transitively, the pyrDown support of its coarser required
// tiles.  For a rig whose seams split the panorama, this is ~1.2-1.5 cameras per pixel instead of every camera
// everywhere (the reference computes all pyramids over every align_roi).
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#define OCTVR_MB_HD __host__ __device__
#else
#define OCTVR_MB_HD
#endif

namespace octvr {

// ---- what the kernels share with the plan (kernels.hpp includes this header) -------------------------------------
// the tiled composite's and the blend's unit of work: 128 x 8 pixels
constexpr int kTileW = 128, kTileH = 8, kTilePx = kTileW * kTileH;
constexpr int kMbMaxBands = 10;
// pyrUp source patch of one 128x8 tile: <= 8 rows (4 quad rows, the row quirk, any block phase)
// by <= 72 columns (64 quad columns + borders), staged in LDS
constexpr int kUpPatchRows = 8, kUpPatchCols = 72;
struct alignas(16) UpQuad {  // one quad row (or column) of a pyrUp output; 16 B: one load per lane
    uint16_t idx[3];      // source rows (cols) of the 3 union taps, clamped, local to the coarser level
    uint16_t pad0;
    uint8_t w0[3], w1[3]; // integer weights of the quad's first / second row (col) over them
    uint8_t pad1[2];
};
static_assert(sizeof(UpQuad) == 16, "UpQuad layout");

// The same taps computed in registers instead of read from the UpQuad tables (no dependent table
// load between the camera record and the tap loads).  For the quad at even level-grid index g, local
// pixels o0 = g - off and o0 + 1 (up_taps / up_table below, pyr_up.cu:55-166):
//   o0 even (o0 = 2h):   sources h-1, h, h+1+k   w0 = 1 6 1, w1 = 0 4 4    k: rows, o0 % 8 == 6
//   o0 odd  (o0 = 2h+1): sources h, h+1, h+2+k'  w0 = 4 4 0, w1 = 1 6 1    k': rows, o0 % 8 == 5
//                                   (rows, o0 % 8 == 7: the odd pixel reads h, h+2: w0 = 4 0 4)
// A pixel outside [0, n_local) weighs 0; sources are |u| clamped to n_src - 1.  Zero-weight slots
// may hold a different (in-range) source than the table's, so the weighted sums are identical.
OCTVR_MB_HD inline int up_clamp(int u, int n_src) {
    u = u < 0 ? -u : u;
    return u < n_src - 1 ? u : n_src - 1;
}
struct UpArith {
    int idx[3];
    int w0[3], w1[3];
};
OCTVR_MB_HD inline UpArith up_arith(int g, int off, int n_local, int n_src, bool rows) {
    UpArith e;
    const int o0 = g - off;
    const int h = o0 >> 1;  // floor
    const bool odd = (o0 & 1) != 0;
    const int m8 = o0 & 7;
    const bool v0 = o0 >= 0 && o0 < n_local, v1 = o0 + 1 >= 0 && o0 + 1 < n_local;
    int u0, u2;
    if (!odd) {
        u0 = h - 1;
        u2 = h + 1 + ((rows && m8 == 6) ? 1 : 0);
        e.w0[0] = 1, e.w0[1] = 6, e.w0[2] = 1;
        e.w1[0] = 0, e.w1[1] = 4, e.w1[2] = 4;
    } else {
        u0 = h;
        u2 = h + 2 + ((rows && m8 == 5) ? 1 : 0);
        const bool q7 = rows && m8 == 7;
        e.w0[0] = 4, e.w0[1] = q7 ? 0 : 4, e.w0[2] = q7 ? 4 : 0;
        e.w1[0] = 1, e.w1[1] = 6, e.w1[2] = 1;
    }
    e.idx[0] = up_clamp(u0, n_src);
    e.idx[1] = up_clamp(u0 + 1, n_src);
    e.idx[2] = up_clamp(u2, n_src);
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int j = 0; j < 3; j++) {
        e.w0[j] = v0 ? e.w0[j] : 0;
        e.w1[j] = v1 ? e.w1[j] : 0;
    }
    return e;
}

// Sub-tiles: 32 x 8 quarters of a 128 x 8 tile (one mb_blend wave each; lane = quad).  The multi-band
// classification (owned / deep / unread / result, mb_classify below) is per sub-tile, so a seam that
// crosses a tile leaves its other quarters on the cheap paths.
constexpr int kSubW = 32, kSubs = kTileW / kSubW;
// Per-item flags of the MODE-1 remap (bits 8-23 of the item header's device word 2, see
// TiledLutDev::upload; bits 8-15 of a wide tile's camera word, for its one half): for half h and quarter q,
// bit 4h + q: that sub-tile's final result is written by the remap (its one deep camera's G0 converted),
// bit 8 + 4h + q: its G0 is written (some pyrDown or blend reads it).  Items of <= 2 halves.
OCTVR_MB_HD constexpr uint32_t item_result_bit(int h, int q) { return 1u << (4 * h + q); }
OCTVR_MB_HD constexpr uint32_t item_g0_bit(int h, int q) { return 1u << (8 + 4 * h + q); }

// ---- the plan ----------------------------------------------------------------------------------------------------
struct MbPlanError : std::invalid_argument {
    using std::invalid_argument::invalid_argument;
};
#define MB_REQUIRE(cond, msg)                              \
    do {                                                   \
        if (!(cond)) throw ::octvr::MbPlanError((msg));    \
    } while (0)

// Weight activity and required Gaussian data are kept per 8 x 8 block of a level grid; a block lies in one
// sub-tile.
constexpr int kBlkPx = 8;
static_assert(kBlkPx == kTileH && kSubW % kBlkPx == 0, "blocks tile the sub-tiles");

struct MbRect {
    int x = 0, y = 0, w = 0, h = 0;
};
struct MbItem {  // the device's uint2
    uint32_t x, y;
};
struct MbRemapJob {
    int tx, ty;  // 128 x (8 qpl) item of the level-0 grid
    int cam;
    uint32_t flags;  // item_g0_bit / item_result_bit per half and quarter
};
struct MbPlanOptions {
    bool no_deep = false;          // every owned sub-tile takes the pyrUp path (measurement / cross-check)
    bool no_remap_result = false;  // the level-0 blend writes every sub-tile (measurement / cross-check)
    int qpl = 2;                   // 128 x 8 halves per remap item
};
struct MbPlanCam {  // one camera at one level: its rectangle on the level grid and its places in the level's arrays
    int ox = 0, oy = 0, w = 0, h = 0;
    uint32_t g_pitch = 0, g_off = 0;  // bytes per row of its G, byte offset of its G in the level's allocation
    size_t w_off = 0;                 // its w x h weights in the level's weight array
    size_t up_rows = 0, up_cols = 0;  // its tap tables in MbPlanLevel::up (level < B)
    size_t up_org = 0;                // its patch origins in MbPlanLevel::up_org: ty_n of rows, then tx_n of columns
};
struct MbPlanLevel {
    int W = 0, H = 0, tx_n = 0, ty_n = 0;  // level grid, its tiles
    int bx_n = 0, by_n = 0;                // its 8 x 8 blocks
    size_t g_bytes = 0, n_weights = 0;     // all cameras' Gaussian level (u8x4), all cameras' weights
    std::vector<MbPlanCam> cams;
    std::vector<std::vector<uint8_t>> act;   // [camera][block]: some weight of the camera there is non-zero
    std::vector<uint32_t> tile_cams;         // per tile, bit n: camera n has a non-zero weight in it
    // multi-band: the owner of each level-grid pixel (the one camera with a non-zero weight, that weight exactly 1;
    // -1 otherwise); per 32 x 8 sub-tile (tile * kSubs + quarter) the cameras with a non-zero weight there and
    // its kind: 1 owned (one camera of weight exactly 1 throughout), 2 deep (R = G on every pixel), 3 read by no
    // collapse, 4 (level 0) deep with its result written by the remap
    std::vector<int8_t> owner;
    std::vector<uint32_t> sub_cams;
    std::vector<uint8_t> sub_own;
    int n_owned = 0, n_deep = 0, n_skip = 0;  // sub-tiles found owned, deep at this level (kind 2 or 4), unread
    std::vector<MbItem> work;  // multi-band: the sub-tiles mb_blend computes (kinds 0-2), MbBlendArgs::work
    int n_work = -1;           // their count, padded to a multiple of 4 (-1: every tile, no list)
    std::vector<UpQuad> up, rup;  // level < B: per camera rows then cols; the collapse's rows then cols
    int rup_rows = 0;
    std::vector<int32_t> up_org, rup_org;  // staged-patch origins per tile row, then per tile column
    std::vector<std::vector<uint8_t>> need;  // [camera][block]: the camera's G is required there
    std::vector<std::vector<uint8_t>> req;   // [camera][tile]: some block of the tile is
    size_t req_tiles = 0;                    // sum over cameras of required tiles
    std::vector<MbItem> down_items;          // level > 0: (camera, tx | ty << 16) of every required tile

    const UpQuad* cam_rows(int i) const { return up.data() + cams[i].up_rows; }
    const UpQuad* cam_cols(int i) const { return up.data() + cams[i].up_cols; }
    const UpQuad* rup_r() const { return rup.data(); }
    const UpQuad* rup_c() const { return rup.data() + rup_rows; }
    size_t sub_index(int tx, int ty, int q) const { return ((size_t)ty * tx_n + tx) * kSubs + q; }
    // the sub-tile holding 8 x 8 block (bx, by)
    size_t sub_of_block(int bx, int by) const {
        return sub_index(bx * kBlkPx / kTileW, by, (bx * kBlkPx % kTileW) / kSubW);
    }
    int kind_of_block(int bx, int by) const { return sub_own.empty() ? 0 : (int)sub_own[sub_of_block(bx, by)]; }
};
struct MbPlan {
    int n = 0, B = 0, out_w = 0, out_h = 0;
    bool feather = false;  // FeatherGPUBlender instead of MultiBandGPUBlender: one level, B = 0
    MbRect arr;            // the level-0 grid on the output frame (feather: the even rectangle around arr_ref)
    MbRect arr_ref;        // the reference's align_result_roi
    std::vector<MbRect> ar;
    int crop_w = 0, crop_h = 0;
    bool full_cover = true;
    std::vector<MbPlanLevel> lv;
    std::vector<uint8_t> seam0;  // multi-band level 0: the u8 seams over each ar[i]
    std::vector<float> w0;       // level 0 in f32: seam / 255 (the pyramid's source), or the feather weights
    std::vector<std::vector<uint8_t>> req0_sub;  // [camera][level-0 sub-tile]: the remap writes its G0 there
    std::vector<MbRemapJob> jobs;                // level-0 remap items (camera, required tile)
    int n_result = 0;                            // level-0 sub-tiles the remap writes the result of (kind 4)

    // Drop the per-pixel and per-block tables once they are uploaded: the counts and the per-tile sets stay.
    void drop_tables() {
        seam0 = {}, w0 = {}, req0_sub = {}, jobs = {};
        for (auto& L : lv)
            L.act = {}, L.owner = {}, L.work = {}, L.up = {}, L.rup = {}, L.up_org = {}, L.rup_org = {}, L.need = {},
            L.req = {}, L.down_items = {};
    }
};

// ---- rectangles (blenders.cpp:479-486, 595-618) ------------------------------------------------------------------
inline int mb_round_down(int x, int b) { return (x >> b) << b; }
inline int mb_round_up(int x, int b) {
    const int m = 1 << b;
    return x + (m - (x % m)) % m;
}

inline void mb_plan_levels(MbPlan& P) {
    const int n = P.n;
    P.lv.assign(P.B + 1, MbPlanLevel{});
    for (int l = 0; l <= P.B; l++) {
        auto& L = P.lv[l];
        L.W = P.arr.w >> l;
        L.H = P.arr.h >> l;
        L.tx_n = (L.W + kTileW - 1) / kTileW;
        L.ty_n = (L.H + kTileH - 1) / kTileH;
        L.bx_n = (L.W + kBlkPx - 1) / kBlkPx;
        L.by_n = (L.H + kBlkPx - 1) / kBlkPx;
        MB_REQUIRE((size_t)L.tx_n * L.ty_n < (1u << 24), "multi-band: level grid too large");
        L.cams.resize(n);
        size_t off = 0, wn = 0;
        for (int i = 0; i < n; i++) {
            MbPlanCam& c = L.cams[i];
            c.ox = (P.ar[i].x - P.arr.x) >> l;
            c.oy = (P.ar[i].y - P.arr.y) >> l;
            c.w = P.ar[i].w >> l;
            c.h = P.ar[i].h >> l;
            c.g_pitch = (uint32_t)c.w * 4;
            c.g_off = (uint32_t)off;
            c.w_off = wn;
            off += ((size_t)c.g_pitch * c.h + 255) & ~(size_t)255;
            wn += (size_t)c.w * c.h;
        }
        MB_REQUIRE(off < 0x7FFFFF00u, "multi-band: pyramid level larger than 2 GiB");
        L.g_bytes = off;
        L.n_weights = wn;
    }
}

// rois: each camera's x, y, w, h on the output frame.  bands is ignored for feather.
inline void mb_plan_rects(MbPlan& P, const std::vector<MbRect>& rois, int out_w, int out_h, int bands, bool feather) {
    const int n = (int)rois.size();
    const int B = feather ? 0 : bands;
    P.n = n, P.B = B, P.out_w = out_w, P.out_h = out_h, P.feather = feather;
    // tile camera sets are 32-bit masks, and the blend's f32 Laplacian sum is exact only while
    // |D| <= 255 * sum(w) stays below 2^15 (sum(w) <= n <= 32, multiband.hip)
    MB_REQUIRE(n >= 1 && n <= 32, "multi-band / feather blend: 1..32 inputs");
    MB_REQUIRE(feather || (B >= 1 && B <= kMbMaxBands), "multi-band blend: band count out of range (blend must be >= 3)");
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    for (auto& r : rois) {
        x0 = std::min(x0, r.x);
        y0 = std::min(y0, r.y);
        x1 = std::max(x1, r.x + r.w);
        y1 = std::max(y1, r.y + r.h);
    }
    const char* leaves = "multi-band: aligned result ROI leaves the output frame (blenders.cpp:727-729)";
    auto inside = [&](const MbRect& a) {
        return a.x + std::min(a.w, out_w) <= out_w && a.y + std::min(a.h, out_h) <= out_h;
    };
    P.arr = MbRect{mb_round_down(x0, B), mb_round_down(y0, B), 0, 0};
    P.arr.w = mb_round_up(x1, B) - P.arr.x;
    P.arr.h = mb_round_up(y1, B) - P.arr.y;
    P.arr_ref = P.arr;
    MB_REQUIRE(inside(P.arr_ref), leaves);
    // The level-0 grid and every camera's rectangle on it start and end on even output pixels: the remap and
    // the level-0 blend work on 2 x 2 quads that are one chroma cell of the output frame.  Multi-band
    // rectangles are multiples of 2^B (B >= 1) already.  Feather (B = 0) takes the ROIs themselves, of any
    // parity, so its rectangles grow to the enclosing even ones (A = 1) with weight 0 on the added pixels:
    // those add nothing to any sum, and where they lie outside the reference's result ROI they come out
    // black, as the reference's zeroed result image has them.
    const int A = std::max(B, 1);
    if (feather) {
        P.arr.x = mb_round_down(x0, A), P.arr.y = mb_round_down(y0, A);
        P.arr.w = mb_round_up(x1, A) - P.arr.x, P.arr.h = mb_round_up(y1, A) - P.arr.y;
    }
    const int gap = feather ? 0 : 5 * (1 << B);  // feather: the ROIs themselves
    P.ar.clear();
    for (auto& in : rois) {
        const int l = std::max(P.arr.x, mb_round_down(in.x, A) - gap);
        const int t = std::max(P.arr.y, mb_round_down(in.y, A) - gap);
        const int r = std::min(P.arr.x + P.arr.w, mb_round_up(in.x + in.w, A) + gap);
        const int b = std::min(P.arr.y + P.arr.h, mb_round_up(in.y + in.h, A) + gap);
        MB_REQUIRE(((r - l) >> B) > 0 && ((b - t) >> B) > 0, "multi-band: aligned ROI too small (blenders.cpp:614-615)");
        P.ar.push_back(MbRect{l, t, r - l, b - t});
    }
    const double max_len = std::max(P.arr.w, P.arr.h);
    MB_REQUIRE(feather || B <= (int)std::ceil(std::log(max_len) / std::log(2.0)),
               "multi-band: too many bands (blenders.cpp:621)");
    // the even grid too (an even frame holds it wherever it held the reference's rectangle; a frame of odd size
    // may not: feather's grid reaches up to one pixel further)
    MB_REQUIRE(inside(P.arr), leaves);
    P.crop_w = std::min(P.arr.w, out_w);
    P.crop_h = std::min(P.arr.h, out_h);
    P.full_cover = P.arr.x == 0 && P.arr.y == 0 && P.crop_w == out_w && P.crop_h == out_h;
    mb_plan_levels(P);
}

// ---- level-0 weights, laid out over each camera's rectangle ar[i] (0 around the ROI) -------------------------------
inline size_t mb_w0_index(const MbPlan& P, int i, const MbRect& roi, int x, int y) {
    const MbRect& a = P.ar[i];
    return P.lv[0].cams[i].w_off + (size_t)(roi.y - a.y + y) * a.w + (roi.x - a.x + x);
}

// Multi-band: level 0 = seam / 255, kept as the u8 seam (converted in-kernel bit-exactly) and in f32 for the
// pyramid.  seams[i]: roi.w x roi.h, packed.
inline void mb_seam_weights(MbPlan& P, const std::vector<MbRect>& rois, const std::vector<std::vector<uint8_t>>& seams) {
    MB_REQUIRE(seams.size() == (size_t)P.n,
               "multi-band blend needs seam masks (octvr_rig_create_masks or a .dat with seams)");
    P.seam0.assign(P.lv[0].n_weights, 0);
    P.w0.assign(P.lv[0].n_weights, 0.f);
    const float inv255 = (float)(1. / 255);
    for (int i = 0; i < P.n; i++)
        for (int y = 0; y < rois[i].h; y++)
            for (int x = 0; x < rois[i].w; x++) {
                const uint8_t v = seams[i][(size_t)y * rois[i].w + x];
                const size_t d = mb_w0_index(P, i, rois[i], x, y);
                P.seam0[d] = v;
                P.w0[d] = inv255 * (float)v;
            }
}

// Feather weights (FeatherGPUBlender ctor, blenders.cpp:531-568) from dist[i] = distanceTransform(mask_i, L2, 3)
// over the ROI: w_i = max(dist_i - border, 0); W = 1e-5f + sum_i w_i (camera order); w_i = n * w_i / W
// (DivScaleOp, div_mat.cu:82-91; plain a / b when n == 1).
inline void mb_feather_weights(MbPlan& P, const std::vector<MbRect>& rois, std::vector<std::vector<float>> dist,
                               int border) {
    const int n = P.n;
    for (auto& w : dist)
        for (float& v : w) {
            const float d = v - (float)border;
            v = d > 0.f ? d : 0.f;  // threshold(THRESH_TOZERO, 0)
        }
    std::vector<float> W((size_t)P.arr.w * P.arr.h, 1e-5f);
    auto sum_at = [&](int i, int x, int y) -> float& {
        return W[(size_t)(rois[i].y - P.arr.y + y) * P.arr.w + (rois[i].x - P.arr.x + x)];
    };
    for (int i = 0; i < n; i++)
        for (int y = 0; y < rois[i].h; y++)
            for (int x = 0; x < rois[i].w; x++) {
                float& d = sum_at(i, x, y);
                d = dist[i][(size_t)y * rois[i].w + x] + d;
            }
    P.w0.assign(P.lv[0].n_weights, 0.f);
    const float sc = (float)n;
    for (int i = 0; i < n; i++)
        for (int y = 0; y < rois[i].h; y++)
            for (int x = 0; x < rois[i].w; x++) {
                const float a = dist[i][(size_t)y * rois[i].w + x], b = sum_at(i, x, y);
                P.w0[mb_w0_index(P, i, rois[i], x, y)] = b != 0 ? (n == 1 ? a / b : sc * a / b) : 0.f;
            }
}

// The weights of every level as the later stages read them: multi-band level 0 is the u8 seam, feather's one
// level P.w0, level l >= 1 the caller's upper[l] (n_weights floats, camera i at cams[i].w_off).
struct MbWeights {
    const MbPlan& P;
    const std::vector<std::vector<float>>& upper;
    bool u8(int l) const { return l == 0 && !P.feather; }
    const float* f32(int l) const { return l == 0 ? P.w0.data() : upper[l].data(); }
    bool nonzero(int l, size_t k) const { return u8(l) ? P.seam0[k] != 0 : f32(l)[k] != 0.f; }
    bool one(int l, size_t k) const { return u8(l) ? P.seam0[k] == 255 : f32(l)[k] == 1.0f; }
};

// ---- weight activity per 8 x 8 block and tile, pixel owners, sub-tile camera sets ----------------------------------
inline void mb_plan_activity(MbPlan& P, const MbWeights& wt, int l) {
    auto& L = P.lv[l];
    L.act.assign(P.n, std::vector<uint8_t>((size_t)L.bx_n * L.by_n, 0));
    if (!P.feather) L.owner.assign((size_t)L.W * L.H, (int8_t)-2);  // -2: no weight met yet
    for (int i = 0; i < P.n; i++) {
        const auto& c = L.cams[i];
        for (int yl = 0; yl < c.h; yl++)
            for (int xl = 0; xl < c.w; xl++) {
                const size_t k = c.w_off + (size_t)yl * c.w + xl;
                if (!wt.nonzero(l, k)) continue;
                const int x = xl + c.ox, y = yl + c.oy;
                L.act[i][(size_t)(y >> 3) * L.bx_n + (x >> 3)] = 1;
                if (P.feather) continue;
                int8_t& o = L.owner[(size_t)y * L.W + x];
                o = (o == -2 && wt.one(l, k)) ? (int8_t)i : (int8_t)-1;
            }
    }
    for (int8_t& o : L.owner) o = o < 0 ? (int8_t)-1 : o;
    L.tile_cams.assign((size_t)L.tx_n * L.ty_n, 0u);
    if (!P.feather) L.sub_cams.assign((size_t)L.tx_n * L.ty_n * kSubs, 0u);
    for (int i = 0; i < P.n; i++)
        for (int by = 0; by < L.by_n; by++)
            for (int bx = 0; bx < L.bx_n; bx++) {
                if (!L.act[i][(size_t)by * L.bx_n + bx]) continue;
                L.tile_cams[(size_t)(by * kBlkPx / kTileH) * L.tx_n + bx * kBlkPx / kTileW] |= 1u << i;
                if (!P.feather) L.sub_cams[L.sub_of_block(bx, by)] |= 1u << i;
            }
}

// ---- pyrUp tap tables --------------------------------------------------------------------------------------------
// pyrUp (pyr_up.cu:55-166) source taps of one output row (col) `o` of a level of size n_out, from a
// source of size n_src: unclamped indices + weights (1,6,1 | 4,4), the 8-row block quirk for rows.
inline int up_taps(int o, bool rows, int* u, int* w) {
    if (!(o & 1)) {
        const int q = o >> 1;
        u[0] = q - 1;
        u[1] = q;
        u[2] = (rows && (o & 7) == 6) ? q + 2 : q + 1;
        w[0] = 1, w[1] = 6, w[2] = 1;
        return 3;
    }
    u[0] = (o - 1) >> 1;
    u[1] = (rows && (o & 7) == 7) ? ((o + 1) >> 1) + 1 : (o + 1) >> 1;
    w[0] = 4, w[1] = 4;
    return 2;
}

// Tap table over the level grid's quad rows (cols): grid index g -> local index g - off, valid in
// [0, n_local); sources clamped to [0, n_src) after abs (pyr_up.cu:72-79).
inline std::vector<UpQuad> up_table(int n_grid, int off, int n_local, int n_src, bool rows) {
    std::vector<UpQuad> t((n_grid + 1) / 2);
    for (size_t q = 0; q < t.size(); q++) {
        int uni[6], nu = 0;
        int us[2][3], ws[2][3], nt[2] = {0, 0};
        for (int p = 0; p < 2; p++) {
            const int o = (int)(2 * q) + p - off;
            if (o < 0 || o >= n_local) continue;
            nt[p] = up_taps(o, rows, us[p], ws[p]);
            for (int k = 0; k < nt[p]; k++) {
                bool seen = false;
                for (int j = 0; j < nu; j++) seen |= uni[j] == us[p][k];
                if (!seen) uni[nu++] = us[p][k];
            }
        }
        UpQuad& e = t[q];
        memset(&e, 0, sizeof e);
        MB_REQUIRE(nu <= 3, "pyrUp quad needs more than 3 source rows");
        std::sort(uni, uni + nu);
        for (int j = nu; j < 3; j++) uni[j] = nu ? uni[0] : 0;
        for (int j = 0; j < 3; j++) e.idx[j] = (uint16_t)std::min(n_src - 1, std::abs(uni[j]));
        for (int p = 0; p < 2; p++) {
            uint8_t* w = p ? e.w1 : e.w0;
            for (int k = 0; k < nt[p]; k++)
                for (int j = 0; j < nu; j++)
                    if (uni[j] == us[p][k]) w[j] = (uint8_t)ws[p][k];
        }
    }
    return t;
}

// mb_blend computes its taps in registers (up_arith); check once per rig that they weigh the same sources as
// the tables: per quad pixel, the summed weight of every source index.
inline void check_up_arith(const std::vector<UpQuad>& t, int off, int n_local, int n_src, bool rows) {
    for (size_t q = 0; q < t.size(); q++) {
        const UpArith e = up_arith((int)(2 * q), off, n_local, n_src, rows);
        for (int p = 0; p < 2; p++) {
            int wt[6] = {0}, we[6] = {0}, it[6], ie[6];
            for (int j = 0; j < 3; j++) {
                it[j] = t[q].idx[j], wt[j] = p ? t[q].w1[j] : t[q].w0[j];
                ie[j] = e.idx[j], we[j] = p ? e.w1[j] : e.w0[j];
                MB_REQUIRE(ie[j] >= 0 && ie[j] < n_src, "pyrUp tap outside the source");
            }
            auto weight_of = [](const int* idx, const int* w, int v) {
                int s = 0;
                for (int j = 0; j < 3; j++) s += idx[j] == v ? w[j] : 0;
                return s;
            };
            for (int j = 0; j < 3; j++)
                MB_REQUIRE(weight_of(it, wt, it[j]) == weight_of(ie, we, it[j]) &&
                               weight_of(it, wt, ie[j]) == weight_of(ie, we, ie[j]),
                           "pyrUp register taps differ from the tap table");
        }
    }
}

// The lowest and highest source index that a weighted tap of quads [q0, q1) reads (second < 0: none does).
inline std::pair<int, int> tap_span(const UpQuad* t, int q0, int q1) {
    int lo = INT32_MAX, hi = -1;
    for (int q = q0; q < q1; q++)
        for (int j = 0; j < 3; j++)
            if (t[q].w0[j] | t[q].w1[j]) lo = std::min(lo, (int)t[q].idx[j]), hi = std::max(hi, (int)t[q].idx[j]);
    return {lo, hi};
}

// Origin of each tile's staged pyrUp patch (kUpPatchRows x kUpPatchCols): the smallest source index any
// weighted tap of the tile's quads reads; the span must fit the patch.
inline std::vector<int32_t> patch_origins(const std::vector<UpQuad>& t, int quads_per_tile, int n_tiles, int limit) {
    std::vector<int32_t> o(n_tiles, 0);
    for (int k = 0; k < n_tiles; k++) {
        const auto [lo, hi] = tap_span(t.data(), k * quads_per_tile, std::min((k + 1) * quads_per_tile, (int)t.size()));
        if (hi < 0) continue;
        MB_REQUIRE(hi - lo < limit, "pyrUp patch of a tile exceeds the staged size");
        o[k] = lo;
    }
    return o;
}

// One checked table with its patch origins appended to `tables` / `origins`; returns the table's offset.
inline size_t mb_add_taps(std::vector<UpQuad>& tables, std::vector<int32_t>& origins, int n_tiles, int tile_px, int off,
                          int n_local, int n_src, bool rows) {
    // tables cover the whole tile grid: lanes of the last tile row / column past the level
    // size index them too (their weights are 0, their taps clamped in range)
    const std::vector<UpQuad> t = up_table(n_tiles * tile_px, off, n_local, n_src, rows);
    check_up_arith(t, off, n_local, n_src, rows);
    const std::vector<int32_t> o = patch_origins(t, tile_px / 2, n_tiles, rows ? kUpPatchRows : kUpPatchCols);
    const size_t at = tables.size();
    tables.insert(tables.end(), t.begin(), t.end());
    origins.insert(origins.end(), o.begin(), o.end());
    return at;
}

inline void mb_plan_taps(MbPlan& P, int l) {
    auto& L = P.lv[l];
    const auto& Ln = P.lv[l + 1];
    for (int i = 0; i < P.n; i++) {
        auto& c = L.cams[i];
        c.up_org = L.up_org.size();
        c.up_rows = mb_add_taps(L.up, L.up_org, L.ty_n, kTileH, c.oy, c.h, Ln.cams[i].h, true);
        c.up_cols = mb_add_taps(L.up, L.up_org, L.tx_n, kTileW, c.ox, c.w, Ln.cams[i].w, false);
    }
    mb_add_taps(L.rup, L.rup_org, L.ty_n, kTileH, 0, L.H, Ln.H, true);
    L.rup_rows = (int)mb_add_taps(L.rup, L.rup_org, L.tx_n, kTileW, 0, L.W, Ln.W, false);
}

// ---- classification of the sub-tiles -----------------------------------------------------------------------------
// pred(x, y) on every pixel of sub-tile (tx, ty, q) that lies inside the level grid
template <class Pred>
bool mb_sub_all(const MbPlanLevel& L, int tx, int ty, int q, Pred pred) {
    const int x0 = tx * kTileW + q * kSubW;
    for (int y = ty * kTileH; y < std::min((ty + 1) * kTileH, L.H); y++)
        for (int x = x0; x < std::min(x0 + kSubW, L.W); x++)
            if (!pred(x, y)) return false;
    return true;
}
// f(tx, ty, q, index) for every sub-tile of the level
template <class F>
void mb_each_sub(const MbPlanLevel& L, F f) {
    for (int ty = 0; ty < L.ty_n; ty++)
        for (int tx = 0; tx < L.tx_n; tx++)
            for (int q = 0; q < kSubs; q++) f(tx, ty, q, L.sub_index(tx, ty, q));
}

// Kind 1, owned: one camera with a non-zero weight in the sub-tile, and its weight is exactly 1 on every
// sub-tile pixel of the level grid (level 0: seam 255; above: the f32 pyramid's 1.0f), so each pixel's Laplacian
// is that camera's alone with weight 1 (mb_blend's fast path).  With no other camera in the sub-tile that is
// "the camera owns every pixel".
inline void mb_classify_owned(MbPlanLevel& L) {
    L.sub_own.assign(L.sub_cams.size(), 0);
    mb_each_sub(L, [&](int tx, int ty, int q, size_t s) {
        const uint32_t msk = L.sub_cams[s];
        if (__builtin_popcount(msk) != 1) return;
        const int i = __builtin_ctz(msk);
        if (L.cams[i].w < 2) return;  // the fast path reads pixel pairs
        if (!mb_sub_all(L, tx, ty, q, [&](int x, int y) { return L.owner[(size_t)y * L.W + x] == i; })) return;
        L.sub_own[s] = 1;
        L.n_owned++;
    });
}

// nonzero-weight (source, weight) pairs of grid pixel 2q + p, sources shifted by `sh`, merged and sorted by source
inline int mb_taps_of(const UpQuad& u, int p, int sh, int (&src)[3], int (&wt)[3]) {
    int k = 0;
    for (int j = 0; j < 3; j++) {
        const int w = p ? u.w1[j] : u.w0[j];
        if (!w) continue;
        const int v = (int)u.idx[j] + sh;
        int m = 0;
        while (m < k && src[m] != v) m++;
        if (m == k) src[k] = v, wt[k++] = 0;
        wt[m] += w;
    }
    for (int a = 1; a < k; a++)
        for (int b = a; b > 0 && src[b - 1] > src[b]; b--) std::swap(src[b], src[b - 1]), std::swap(wt[b], wt[b - 1]);
    return k;
}
// the camera's quad `cu` (sources local to the camera, at `sh` on the coarser grid) weighs what the collapse's `gu` does
inline bool mb_same_taps(const UpQuad& cu, int sh, const UpQuad& gu, int p) {
    int s1[3], w1[3], s2[3], w2[3];
    const int k1 = mb_taps_of(cu, p, sh, s1, w1), k2 = mb_taps_of(gu, p, 0, s2, w2);
    if (k1 != k2 || k1 == 0) return false;
    for (int j = 0; j < k1; j++)
        if (s1[j] != s2[j] || w1[j] != w2[j]) return false;
    return true;
}

// Kind 2, deep: R = G (mb_blend skips the pyrUps).
// A pixel of level l is deep for camera n when n owns it (one camera of weight exactly 1), the
// camera's pyrUp of G_{l+1} there reads the same sources with the same weights as the collapse's
// pyrUp of R_{l+1}, and every such source is deep for n at level l + 1 (at the top level: owned).
// Then R_l = G_l exactly, by induction from the top: L_l = G_l - up(G_{l+1}) (weight 1, the
// normalisation exact for |D| <= 255), R_l = L_l + up(R_{l+1}) with R_{l+1} = G_{l+1} on every tap,
// and the two pyrUps round identically (the u8 and s16 saturations are no-ops for 0..255).  A sub-tile
// whose pixels are all deep takes R = G at its level: no taps, no collapse.
inline void mb_classify_deep(MbPlan& P) {
    std::vector<int8_t> deep_next = P.lv[P.B].owner;  // per pixel of level l + 1: the camera it is deep for, or -1
    for (int l = P.B - 1; l >= 0; l--) {
        auto& L = P.lv[l];
        const auto& Ln = P.lv[l + 1];
        std::vector<std::vector<uint8_t>> rok(P.n), cok(P.n);  // the camera's row (column) taps are the collapse's
        for (int i = 0; i < P.n; i++) {
            rok[i].resize(L.H);
            cok[i].resize(L.W);
            for (int y = 0; y < L.H; y++)
                rok[i][y] = mb_same_taps(L.cam_rows(i)[y >> 1], Ln.cams[i].oy, L.rup_r()[y >> 1], y & 1);
            for (int x = 0; x < L.W; x++)
                cok[i][x] = mb_same_taps(L.cam_cols(i)[x >> 1], Ln.cams[i].ox, L.rup_c()[x >> 1], x & 1);
        }
        auto deep_px = [&](int x, int y) -> bool {
            const int c = L.owner[(size_t)y * L.W + x];
            if (c < 0 || !rok[c][y] || !cok[c][x]) return false;
            int rs[3], rw[3], cs[3], cw[3];
            const int kr = mb_taps_of(L.rup_r()[y >> 1], y & 1, 0, rs, rw), kc = mb_taps_of(L.rup_c()[x >> 1], x & 1, 0, cs, cw);
            for (int a = 0; a < kr; a++)
                for (int b = 0; b < kc; b++)
                    if (deep_next[(size_t)rs[a] * Ln.W + cs[b]] != c) return false;
            return true;
        };
        std::vector<int8_t> deep;
        if (l > 0) {  // every pixel (the finer level's test reads them)
            deep.assign((size_t)L.W * L.H, (int8_t)-1);
            for (int y = 0; y < L.H; y++)
                for (int x = 0; x < L.W; x++)
                    if (deep_px(x, y)) deep[(size_t)y * L.W + x] = L.owner[(size_t)y * L.W + x];
        }
        mb_each_sub(L, [&](int tx, int ty, int q, size_t s) {
            if (!L.sub_own[s]) return;
            if (!mb_sub_all(L, tx, ty, q, [&](int x, int y) { return l > 0 ? deep[(size_t)y * L.W + x] >= 0 : deep_px(x, y); }))
                return;
            L.sub_own[s] = 2;
            L.n_deep++;
        });
        deep_next = std::move(deep);
    }
}

// Kind 3, unread: sub-tiles of level l >= 1 that no collapse reads (every level-(l-1) sub-tile whose pyrUp taps
// reach them is deep or itself unread).  mb_blend skips them, and their Gaussian blocks are not required for them.
inline void mb_classify_unread(MbPlan& P, int l) {
    auto& L = P.lv[l];
    const auto& Lf = P.lv[l - 1];
    std::vector<uint8_t> read(L.sub_own.size(), 0);
    mb_each_sub(Lf, [&](int tx, int ty, int sq, size_t s) {
        if (Lf.sub_own[s] >= 2) return;  // deep (2, 4) or unread (3): no collapse reads level l there
        const auto [r0, r1] = tap_span(Lf.rup_r(), ty * kTileH / 2, (ty + 1) * kTileH / 2);
        const int qc = (tx * kTileW + sq * kSubW) / 2;
        const auto [c0, c1] = tap_span(Lf.rup_c(), qc, qc + kSubW / 2);
        if (r1 < 0 || c1 < 0) return;
        const int cmax = L.tx_n * kTileW - 1;
        for (int y = r0 / kTileH; y <= std::min(r1 / kTileH, L.ty_n - 1); y++)
            for (int x = c0 / kSubW; x <= std::min(c1, cmax) / kSubW; x++)
                read[(size_t)y * L.tx_n * kSubs + x] = 1;  // a tile row's sub-tiles are consecutive
    });
    for (size_t t = 0; t < read.size(); t++)
        if (!read[t]) {
            L.n_deep -= L.sub_own[t] == 2 ? 1 : 0;
            L.sub_own[t] = 3;
            L.n_skip++;
        }
}

// Kind 4: deep level-0 sub-tiles whose result the remap writes (item_result_bit).
// A deep level-0 sub-tile's result is its one camera's G0 (R = G, above), so the MODE-1 remap item of that
// camera converts it to YUV420P (or the RGBA result) right away and mb_blend skips it: its G0 is then needed
// only where a level-1 pyrDown reads it.  Only sub-tiles wholly inside the crop and the output frame qualify
// (the remap's result stores take no bounds).
inline void mb_classify_result(MbPlan& P) {
    auto& L0 = P.lv[0];
    mb_each_sub(L0, [&](int tx, int ty, int q, size_t s) {
        const int x1 = tx * kTileW + (q + 1) * kSubW, y1 = (ty + 1) * kTileH;
        if (L0.sub_own[s] != 2 || x1 > P.crop_w || y1 > P.crop_h || P.arr.x + x1 > P.out_w || P.arr.y + y1 > P.out_h)
            return;
        L0.sub_own[s] = 4;
        P.n_result++;
    });
}

inline void mb_classify(MbPlan& P, const MbPlanOptions& opt) {
    for (auto& L : P.lv) mb_classify_owned(L);
    if (opt.no_deep) return;  // every owned sub-tile stays on the pyrUp path, nothing is skipped
    mb_classify_deep(P);
    for (int l = 1; l <= P.B; l++) mb_classify_unread(P, l);
    if (!opt.no_remap_result) mb_classify_result(P);
}

// ---- required 8 x 8 blocks per camera and level, then tiles --------------------------------------------------------
// need(l) = weight blocks(l) + pyrUp support of weight blocks(l-1) + pyrDown support of need(l+1)
// (blocks of unread / remap-result sub-tiles: no blend reads G there)
inline void mb_plan_required(MbPlan& P, int l, int i) {
    auto& L = P.lv[l];
    const auto& c = L.cams[i];
    std::vector<uint8_t> need = L.act[i];
    for (int by = 0; by < L.by_n; by++)
        for (int bx = 0; bx < L.bx_n; bx++)
            if (L.kind_of_block(bx, by) >= 3) need[(size_t)by * L.bx_n + bx] = 0;
    auto mark = [&](int x0, int y0, int x1, int y1) {  // level-grid pixel rectangle, inclusive
        x0 = std::max(x0, 0), y0 = std::max(y0, 0);
        x1 = std::min(x1, L.bx_n * kBlkPx - 1), y1 = std::min(y1, L.by_n * kBlkPx - 1);
        for (int by = y0 / kBlkPx; by <= y1 / kBlkPx; by++)
            for (int bx = x0 / kBlkPx; bx <= x1 / kBlkPx; bx++) need[(size_t)by * L.bx_n + bx] = 1;
    };
    if (l >= 1) {  // pyrUp support of the finer level's weight blocks (8x8 px = 4x4 quads)
        const auto& Lf = P.lv[l - 1];
        for (int by = 0; by < Lf.by_n; by++)
            for (int bx = 0; bx < Lf.bx_n; bx++) {
                if (!Lf.act[i][(size_t)by * Lf.bx_n + bx]) continue;
                if (Lf.kind_of_block(bx, by) >= 2) continue;  // deep / unread / result: no pyrUp of G_l there
                const auto [r0, r1] = tap_span(Lf.cam_rows(i), by * kBlkPx / 2, (by + 1) * kBlkPx / 2);
                const auto [c0, c1] = tap_span(Lf.cam_cols(i), bx * kBlkPx / 2, (bx + 1) * kBlkPx / 2);
                if (r1 >= 0 && c1 >= 0) mark(c0 + c.ox, r0 + c.oy, c1 + c.ox, r1 + c.oy);
            }
    }
    if (l < P.B) {  // pyrDown support of the coarser level's required blocks
        const auto& Lc = P.lv[l + 1];
        const auto& cc = Lc.cams[i];
        for (int by = 0; by < Lc.by_n; by++)
            for (int bx = 0; bx < Lc.bx_n; bx++) {
                if (!Lc.need[i][(size_t)by * Lc.bx_n + bx]) continue;
                const int xa = std::max(bx * kBlkPx - cc.ox, 0), xb = std::min((bx + 1) * kBlkPx - 1 - cc.ox, cc.w - 1);
                const int ya = std::max(by * kBlkPx - cc.oy, 0), yb = std::min((by + 1) * kBlkPx - 1 - cc.oy, cc.h - 1);
                if (xa > xb || ya > yb) continue;
                const int sx0 = std::max(2 * xa - 2, 0), sx1 = std::min(2 * xb + 2, c.w - 1);
                const int sy0 = std::max(2 * ya - 2, 0), sy1 = std::min(2 * yb + 2, c.h - 1);
                mark(sx0 + c.ox, sy0 + c.oy, sx1 + c.ox, sy1 + c.oy);
            }
    }
    L.req[i].assign((size_t)L.tx_n * L.ty_n, 0);
    if (l == 0) P.req0_sub[i].assign((size_t)L.tx_n * L.ty_n * kSubs, 0);  // the remap writes G0 per sub-tile
    for (int by = 0; by < L.by_n; by++)
        for (int bx = 0; bx < L.bx_n; bx++) {
            uint8_t& v = need[(size_t)by * L.bx_n + bx];
            // blocks outside the camera's aligned ROI hold nothing of it
            if (!(bx * kBlkPx < c.ox + c.w && (bx + 1) * kBlkPx > c.ox && by * kBlkPx < c.oy + c.h && (by + 1) * kBlkPx > c.oy))
                v = 0;
            if (!v) continue;
            L.req[i][(size_t)(by * kBlkPx / kTileH) * L.tx_n + bx * kBlkPx / kTileW] = 1;
            if (l == 0) P.req0_sub[i][L.sub_of_block(bx, by)] = 1;
        }
    for (uint8_t v : L.req[i]) L.req_tiles += v;
    L.need[i] = std::move(need);
}

// ---- lists -------------------------------------------------------------------------------------------------------
// Per level, the sub-tiles mb_blend has work on (kinds 0-2), 4 per workgroup: it is launched over this list only,
// so sub-tiles that need nothing (unread: 3, written by the remap: 4) cost no dispatch.
inline void mb_plan_work(MbPlanLevel& L) {
    for (size_t t = 0; t < L.sub_own.size(); t++)
        if (L.sub_own[t] < 3)
            L.work.push_back(MbItem{(uint32_t)(t / kSubs) | (uint32_t)(t % kSubs) << 24 | (uint32_t)L.sub_own[t] << 27,
                                    L.sub_cams[t]});
    while (L.work.size() % 4) L.work.push_back(MbItem{3u << 27, 0u});
    L.n_work = (int)L.work.size();
}

inline void mb_plan_down(MbPlanLevel& L, int n) {
    for (int i = 0; i < n; i++)
        for (int ty = 0; ty < L.ty_n; ty++)
            for (int tx = 0; tx < L.tx_n; tx++)
                if (L.req[i][(size_t)ty * L.tx_n + tx])
                    L.down_items.push_back(MbItem{(uint32_t)i, (uint32_t)tx | ((uint32_t)ty << 16)});
}

// Level-0 remap jobs: items of qpl vertically adjacent tiles (128 x 8 qpl), kept when any of them has something to
// write.  Per half and sub-tile: G0 where required (item_g0_bit), the result where the sub-tile has kind 4 and
// this camera is its one camera (item_result_bit).
inline void mb_plan_jobs(MbPlan& P, int qpl) {
    MB_REQUIRE(qpl >= 1 && qpl <= 2, "multi-band remap: items of at most 2 tiles (item flags)");
    const auto& L0 = P.lv[0];
    for (int i = 0; i < P.n; i++)
        for (int ty = 0; ty < (L0.ty_n + qpl - 1) / qpl; ty++)
            for (int tx = 0; tx < L0.tx_n; tx++) {
                uint32_t fl = 0;
                for (int h = 0; h < qpl && ty * qpl + h < L0.ty_n; h++)
                    for (int q = 0; q < kSubs; q++) {
                        const size_t t = L0.sub_index(tx, ty * qpl + h, q);
                        if (P.req0_sub[i][t]) fl |= item_g0_bit(h, q);
                        if (!L0.sub_own.empty() && L0.sub_own[t] == 4 && L0.sub_cams[t] == 1u << i)
                            fl |= item_result_bit(h, q);
                    }
                if (fl) P.jobs.push_back(MbRemapJob{tx, ty, i, fl});
            }
}

// ---- the plan from the rectangles and the weights ------------------------------------------------------------------
// upper[l], l in 1..B: level l's f32 weights (upper[0] is not read; feather passes none).
inline void mb_plan(MbPlan& P, const std::vector<std::vector<float>>& upper, const MbPlanOptions& opt) {
    const MbWeights wt{P, upper};
    MB_REQUIRE(P.B == 0 || upper.size() == (size_t)P.B + 1, "multi-band: one weight array per level");
    for (int l = 1; l <= P.B; l++) MB_REQUIRE(upper[l].size() == P.lv[l].n_weights, "multi-band: weight level of the wrong size");
    for (int l = 0; l <= P.B; l++) mb_plan_activity(P, wt, l);
    for (int l = 0; l < P.B; l++) mb_plan_taps(P, l);
    if (!P.feather) {
        mb_classify(P, opt);
        for (auto& L : P.lv) mb_plan_work(L);
    }
    P.req0_sub.assign(P.n, {});
    for (int l = P.B; l >= 0; l--) {
        P.lv[l].need.assign(P.n, {});
        P.lv[l].req.assign(P.n, {});
        for (int i = 0; i < P.n; i++) mb_plan_required(P, l, i);
    }
    for (int l = 1; l <= P.B; l++) mb_plan_down(P.lv[l], P.n);
    mb_plan_jobs(P, opt.qpl);
}

}  // namespace octvr
