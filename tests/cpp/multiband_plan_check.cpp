// multiband_plan_check.cpp — the multi-band / feather plan (csrc/multiband_plan.hpp) on small rigs, each rule restated
// pixel by pixel from up_taps and the weights (never from the plan's tap tables or block bitmaps).  Stand-alone:
// built with -fsanitize=address,undefined, prints "multiband_plan_check ok" and exits 0 when every rule holds.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <tuple>

#include "multiband_plan.hpp"

using namespace octvr;

#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                                \
            printf("\n");                                       \
            exit(1);                                            \
        }                                                       \
    } while (0)

namespace {

struct Rig {
    std::string name;
    int out_w, out_h, bands;
    bool feather;
    std::vector<MbRect> rois;
    std::vector<std::vector<uint8_t>> seams;  // multi-band: per camera, over its ROI
};
using Upper = std::vector<std::vector<float>>;

int refl101(int v, int last) {
    if (last == 0) return 0;
    while (v < 0 || v > last) v = v < 0 ? -v : 2 * last - v;
    return v;
}
// 5 x 5 (1 4 6 4 1) / 16 pyrDown with reflect-101 borders, f32
std::vector<float> pyr_down(const float* s, int sw, int sh, int dw, int dh) {
    static const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    std::vector<float> d((size_t)dw * dh);
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            float acc = 0.f;
            for (int j = 0; j < 5; j++) {
                float row = 0.f;
                for (int i = 0; i < 5; i++)
                    row += k[i] * s[(size_t)refl101(2 * y + j - 2, sh - 1) * sw + refl101(2 * x + i - 2, sw - 1)];
                acc += k[j] * row;
            }
            d[(size_t)y * dw + x] = acc;
        }
    return d;
}

MbPlan make_plan(const Rig& r, const MbPlanOptions& opt, Upper& upper) {
    MbPlan P;
    mb_plan_rects(P, r.rois, r.out_w, r.out_h, r.bands, r.feather);
    if (r.feather) {
        std::vector<std::vector<float>> dist(r.rois.size());
        for (size_t i = 0; i < r.rois.size(); i++)  // a distance to the ROI's border (any non-negative field does)
            for (int y = 0; y < r.rois[i].h; y++)
                for (int x = 0; x < r.rois[i].w; x++)
                    dist[i].push_back((float)std::min(std::min(x + 1, y + 1), std::min(r.rois[i].w - x, r.rois[i].h - y)));
        mb_feather_weights(P, r.rois, dist, 3);
    } else {
        mb_seam_weights(P, r.rois, r.seams);
    }
    upper.assign(P.B + 1, {});
    for (int l = 1; l <= P.B; l++) {
        upper[l].resize(P.lv[l].n_weights);
        for (int i = 0; i < P.n; i++) {
            const auto &c = P.lv[l].cams[i], &p = P.lv[l - 1].cams[i];
            const float* src = (l == 1 ? P.w0.data() : upper[l - 1].data()) + p.w_off;
            const std::vector<float> d = pyr_down(src, p.w, p.h, c.w, c.h);
            std::copy(d.begin(), d.end(), upper[l].begin() + c.w_off);
        }
    }
    mb_plan(P, upper, opt);
    return P;
}

struct Seen {  // what a case met
    long kinds[5] = {0, 0, 0, 0, 0};
    long deep_or_result[kMbMaxBands + 1] = {0};
    long graded = 0, quirk_rows = 0, cut_deep = 0, off_block = 0;
};
Seen* g_seen = nullptr;

struct Taps {  // merged (source, weight) pairs, sorted by source
    int n = 0, src[3], w[3];
    bool operator==(const Taps& o) const {
        if (n != o.n) return false;
        for (int j = 0; j < n; j++)
            if (src[j] != o.src[j] || w[j] != o.w[j]) return false;
        return true;
    }
};
// pyrUp taps of local output index o from a source of n_src, sources moved by `shift`
Taps taps_of(int o, bool rows, int n_src, int shift) {
    int u[3], w[3];
    const int k = up_taps(o, rows, u, w);
    if (rows && (o & 7) >= 6) g_seen->quirk_rows++;
    std::map<int, int> m;
    for (int j = 0; j < k; j++) m[std::min(n_src - 1, std::abs(u[j])) + shift] += w[j];
    Taps t;
    for (auto& [s, wt] : m) t.src[t.n] = s, t.w[t.n++] = wt;
    return t;
}

struct Checker {
    const Rig& rig;
    const MbPlan& P;
    const Upper& upper;
    const MbPlanOptions& opt;
    std::vector<std::vector<int8_t>> deep;  // [level][pixel]: the camera the pixel is deep for, by the definition

    // camera i's weight at grid pixel (x, y) of level l: 0 none, 1 non-zero, 2 exactly one
    int weight(int l, int i, int x, int y) const {
        const auto& c = P.lv[l].cams[i];
        const int xl = x - c.ox, yl = y - c.oy;
        if (xl < 0 || yl < 0 || xl >= c.w || yl >= c.h) return 0;
        const size_t k = c.w_off + (size_t)yl * c.w + xl;
        if (l == 0 && !P.feather) return P.seam0[k] == 255 ? 2 : P.seam0[k] != 0;
        const float f = l == 0 ? P.w0[k] : upper[l][k];
        return f == 1.0f ? 2 : f != 0.f;
    }
    int owner(int l, int x, int y) const {
        int cnt = 0, who = -1, st = 0;
        for (int i = 0; i < P.n; i++)
            if (int s = weight(l, i, x, y)) cnt++, who = i, st = s;
        return cnt == 1 && st == 2 ? who : -1;
    }
    template <class F>
    void each_px(const MbPlanLevel& L, int tx, int ty, int q, F f) const {  // in-level pixels of a sub-tile
        for (int y = ty * kTileH; y < std::min((ty + 1) * kTileH, L.H); y++)
            for (int x = tx * kTileW + q * kSubW; x < std::min(tx * kTileW + (q + 1) * kSubW, L.W); x++) f(x, y);
    }
    template <class F>
    void each_sub(const MbPlanLevel& L, F f) const {
        for (int ty = 0; ty < L.ty_n; ty++)
            for (int tx = 0; tx < L.tx_n; tx++)
                for (int q = 0; q < kSubs; q++) f(tx, ty, q, ((size_t)ty * L.tx_n + tx) * kSubs + q);
    }
    int kind(int l, size_t s) const { return P.lv[l].sub_own.empty() ? 0 : P.lv[l].sub_own[s]; }
    size_t sub_at(const MbPlanLevel& L, int x, int y) const {
        return ((size_t)(y / kTileH) * L.tx_n + x / kTileW) * kSubs + (x % kTileW) / kSubW;
    }
    bool needed(int l, int i, int x, int y) const {
        const auto& L = P.lv[l];
        return L.need[i][(size_t)(y / kBlkPx) * L.bx_n + x / kBlkPx] != 0;
    }

    void level0_weights() const {
        for (int i = 0; i < P.n; i++) {
            const MbRect &a = P.ar[i], &r = rig.rois[i];
            CHECK(a.x % 2 == 0 && a.y % 2 == 0 && a.w % 2 == 0 && a.h % 2 == 0, "camera %d: odd rectangle", i);
            CHECK(a.x <= r.x && a.y <= r.y && a.x + a.w >= r.x + r.w && a.y + a.h >= r.y + r.h, "camera %d: ROI outside", i);
            for (int y = 0; y < a.h; y++)
                for (int x = 0; x < a.w; x++) {
                    const int rx = a.x + x - r.x, ry = a.y + y - r.y;
                    const bool in = rx >= 0 && ry >= 0 && rx < r.w && ry < r.h;
                    const size_t k = P.lv[0].cams[i].w_off + (size_t)y * a.w + x;
                    if (P.feather) {
                        CHECK(in ? P.w0[k] >= 0.f : P.w0[k] == 0.f, "feather weight of camera %d at %d, %d", i, x, y);
                        continue;
                    }
                    const uint8_t v = in ? rig.seams[i][(size_t)ry * r.w + rx] : 0;
                    CHECK(P.seam0[k] == v && P.w0[k] == (float)(1. / 255) * (float)v, "seam of camera %d at %d, %d", i, x, y);
                    g_seen->graded += v != 0 && v != 255;
                }
        }
    }

    void owners_and_sets() const {
        for (int l = 0; l <= P.B; l++) {
            const auto& L = P.lv[l];
            for (int i = 0; i < P.n; i++) g_seen->off_block += ((L.cams[i].ox | L.cams[i].oy) & 7) != 0;
            if (!P.feather)
                for (int y = 0; y < L.H; y++)
                    for (int x = 0; x < L.W; x++)
                        CHECK(L.owner[(size_t)y * L.W + x] == owner(l, x, y), "owner at level %d, %d, %d", l, x, y);
            std::vector<uint32_t> tiles((size_t)L.tx_n * L.ty_n, 0u);
            each_sub(L, [&](int tx, int ty, int q, size_t s) {
                uint32_t m = 0;
                each_px(L, tx, ty, q, [&](int x, int y) {
                    for (int i = 0; i < P.n; i++) m |= weight(l, i, x, y) ? 1u << i : 0u;
                });
                if (!P.feather) CHECK(L.sub_cams[s] == m, "cameras of sub-tile %zu of level %d", s, l);
                if (P.feather) g_seen->kinds[0] += m != 0;  // every tile of a feather blend is general
                tiles[s / kSubs] |= m;
            });
            CHECK(tiles == L.tile_cams, "tile camera sets of level %d", l);
        }
    }

    // the definition of mb_classify_deep's comment, by recursion from the top level
    void deep_by_definition() {
        deep.assign(P.B + 1, {});
        for (int l = P.B; l >= 0; l--) {
            const auto& L = P.lv[l];
            deep[l].assign((size_t)L.W * L.H, (int8_t)-1);
            for (int y = 0; y < L.H; y++)
                for (int x = 0; x < L.W; x++) {
                    const int c = owner(l, x, y);
                    if (c < 0) continue;
                    if (l == P.B) {
                        deep[l][(size_t)y * L.W + x] = (int8_t)c;
                        continue;
                    }
                    const MbPlanLevel& Ln = P.lv[l + 1];
                    const MbPlanCam &cc = L.cams[c], &cn = Ln.cams[c];
                    const Taps gr = taps_of(y, true, Ln.H, 0), gc = taps_of(x, false, Ln.W, 0);
                    if (!(taps_of(y - cc.oy, true, cn.h, cn.oy) == gr) || !(taps_of(x - cc.ox, false, cn.w, cn.ox) == gc)) continue;
                    bool all = true;
                    for (int a = 0; a < gr.n; a++)
                        for (int b = 0; b < gc.n; b++) all &= deep[l + 1][(size_t)gr.src[a] * Ln.W + gc.src[b]] == c;
                    if (all) deep[l][(size_t)y * L.W + x] = (int8_t)c;
                }
        }
    }

    void kinds() const {
        for (int l = 0; l <= P.B; l++) {
            const auto& L = P.lv[l];
            int n_owned = 0, n_deep = 0, n_skip = 0;
            each_sub(L, [&](int tx, int ty, int q, size_t s) {
                const int k = kind(l, s);
                g_seen->kinds[k]++;
                g_seen->deep_or_result[l] += k == 2 || k == 4;
                const uint32_t m = L.sub_cams[s];
                const int i = m ? __builtin_ctz(m) : 0;
                bool owned = __builtin_popcount(m) == 1 && L.cams[i].w >= 2, all_deep = true;
                each_px(L, tx, ty, q, [&](int x, int y) {
                    owned &= weight(l, i, x, y) == 2;
                    all_deep &= deep[l][(size_t)y * L.W + x] == i;
                });
                n_owned += owned, n_deep += k == 2 || k == 4, n_skip += k == 3;
                if (k == 1 || k == 2 || k == 4) CHECK(owned, "kind %d sub-tile %zu of level %d is not owned", k, s, l);
                // (the top level has no pyrUp to skip: its owned sub-tiles stay kind 1)
                if (k != 3) CHECK((k == 2 || k == 4) == (!opt.no_deep && l < P.B && owned && all_deep), "deep sub-tile %zu of level %d", s, l);
                if (k != 3) CHECK((k >= 1) == owned, "kind %d sub-tile %zu of level %d", k, s, l);
                const int x1 = tx * kTileW + (q + 1) * kSubW, y1 = (ty + 1) * kTileH;
                const bool inside = x1 <= P.crop_w && y1 <= P.crop_h && P.arr.x + x1 <= P.out_w && P.arr.y + y1 <= P.out_h;
                if (k == 4) CHECK(l == 0 && !opt.no_remap_result && inside, "result sub-tile %zu of level %d", s, l);
                if (k == 2 && l == 0 && !opt.no_remap_result) {
                    CHECK(!inside, "deep level-0 sub-tile %zu inside the crop is not the remap's", s);
                    g_seen->cut_deep++;
                }
                if (opt.no_deep) CHECK(k < 2, "kind %d with no_deep", k);
                if (k == 3) CHECK(l >= 1, "unread sub-tile at level 0");
            });
            CHECK(L.n_owned == n_owned && L.n_deep == n_deep && L.n_skip == n_skip, "counts of level %d", l);
        }
        // soundness of kind 3: nothing that a collapse reads is skipped
        for (int l = 1; l <= P.B; l++) {
            const auto &L = P.lv[l], &Lf = P.lv[l - 1];
            each_sub(Lf, [&](int tx, int ty, int q, size_t s) {
                if (kind(l - 1, s) >= 2) return;
                each_px(Lf, tx, ty, q, [&](int x, int y) {
                    const Taps r = taps_of(y, true, L.H, 0), c = taps_of(x, false, L.W, 0);
                    for (int a = 0; a < r.n; a++)
                        for (int b = 0; b < c.n; b++)
                            CHECK(kind(l, sub_at(L, c.src[b], r.src[a])) != 3, "level %d: a collapse of sub-tile %zu reads an unread sub-tile", l, s);
                });
            });
        }
    }

    void required() const {
        for (int l = 0; l <= P.B; l++) {
            const auto& L = P.lv[l];
            for (int i = 0; i < P.n; i++) {
                const auto& c = L.cams[i];
                // the blend's own reads, and its pyrUp's reads of the coarser level
                each_sub(L, [&](int tx, int ty, int q, size_t s) {
                    const int k = kind(l, s);
                    each_px(L, tx, ty, q, [&](int x, int y) {
                        if (!weight(l, i, x, y)) return;
                        if (k <= 2) CHECK(needed(l, i, x, y), "level %d camera %d: blend reads %d, %d", l, i, x, y);
                        if (k > 1 || l == P.B) return;
                        const auto& cn = P.lv[l + 1].cams[i];
                        const Taps r = taps_of(y - c.oy, true, cn.h, cn.oy), cc = taps_of(x - c.ox, false, cn.w, cn.ox);
                        for (int a = 0; a < r.n; a++)
                            for (int b = 0; b < cc.n; b++)
                                CHECK(needed(l + 1, i, cc.src[b], r.src[a]), "level %d camera %d: pyrUp of %d, %d", l, i, x, y);
                    });
                });
                std::vector<uint8_t> tiles((size_t)L.tx_n * L.ty_n, 0), subs(tiles.size() * kSubs, 0);
                for (int by = 0; by < L.by_n; by++)
                    for (int bx = 0; bx < L.bx_n; bx++) {
                        if (!L.need[i][(size_t)by * L.bx_n + bx]) continue;
                        tiles[(size_t)by * L.tx_n + bx * kBlkPx / kTileW] = 1;
                        subs[sub_at(L, bx * kBlkPx, by * kBlkPx)] = 1;
                        CHECK(bx * kBlkPx < c.ox + c.w && (bx + 1) * kBlkPx > c.ox && by * kBlkPx < c.oy + c.h && (by + 1) * kBlkPx > c.oy,
                              "level %d camera %d: block %d, %d required outside the rectangle", l, i, bx, by);
                        if (l == 0) continue;  // the pyrDown of this block's pixels reads 5 x 5 of the finer level
                        const auto& cf = P.lv[l - 1].cams[i];
                        for (int y = std::max(by * kBlkPx, c.oy); y < std::min((by + 1) * kBlkPx, c.oy + c.h); y++)
                            for (int x = std::max(bx * kBlkPx, c.ox); x < std::min((bx + 1) * kBlkPx, c.ox + c.w); x++)
                                for (int dy = -2; dy <= 2; dy++)
                                    for (int dx = -2; dx <= 2; dx++)
                                        CHECK(needed(l - 1, i, cf.ox + refl101(2 * (x - c.ox) + dx, cf.w - 1),
                                                     cf.oy + refl101(2 * (y - c.oy) + dy, cf.h - 1)),
                                              "level %d camera %d: pyrDown of %d, %d", l, i, x, y);
                    }
                CHECK(tiles == L.req[i], "required tiles of level %d camera %d", l, i);
                if (l == 0) CHECK(subs == P.req0_sub[i], "required level-0 sub-tiles of camera %d", i);
                // down items: exactly the required tiles of the levels above 0, in camera and raster order
                if (l == 0) continue;
                std::set<std::pair<uint32_t, uint32_t>> items;
                for (const MbItem& it : L.down_items)
                    if (it.x == (uint32_t)i) CHECK(items.insert({it.x, it.y}).second, "level %d: down item twice", l);
                size_t want = 0;
                for (size_t t = 0; t < tiles.size(); t++) {
                    if (!tiles[t]) continue;
                    want++;
                    CHECK(items.count({(uint32_t)i, (uint32_t)(t % L.tx_n) | (uint32_t)(t / L.tx_n) << 16}), "level %d: down item of tile %zu missing", l, t);
                }
                CHECK(items.size() == want, "level %d camera %d: %zu down items for %zu required tiles", l, i, items.size(), want);
            }
        }
        CHECK(P.lv[0].down_items.empty(), "down items at level 0");
    }

    void work_lists() const {
        for (int l = 0; l <= P.B; l++) {
            const auto& L = P.lv[l];
            if (P.feather) {
                CHECK(L.n_work == -1 && L.work.empty(), "feather has no work list");
                continue;
            }
            CHECK(L.n_work == (int)L.work.size() && L.work.size() % 4 == 0, "work list length of level %d", l);
            std::set<size_t> seen;
            size_t real = 0;
            for (size_t k = 0; k < L.work.size(); k++) {
                const MbItem& it = L.work[k];
                const uint32_t tile = it.x & 0xFFFFFFu, q = (it.x >> 24) & 7u, kd = it.x >> 27;
                if (kd == 3) {  // padding, at the end
                    CHECK(it.x == 3u << 27 && it.y == 0 && L.work.size() - k < 4, "padding of level %d", l);
                    continue;
                }
                CHECK(real == k, "level %d: work after padding", l);
                real++;
                CHECK(tile < (uint32_t)(L.tx_n * L.ty_n) && q < (uint32_t)kSubs, "level %d: work item %zu", l, k);
                const size_t s = (size_t)tile * kSubs + q;
                CHECK(seen.insert(s).second && kd == L.sub_own[s] && it.y == L.sub_cams[s], "level %d: work item %zu", l, k);
            }
            for (size_t s = 0; s < L.sub_own.size(); s++) CHECK((L.sub_own[s] < 3) == (seen.count(s) == 1), "level %d: sub-tile %zu and the work list", l, s);
        }
    }

    void remap_jobs() const {
        const auto& L0 = P.lv[0];
        std::map<std::tuple<int, int, int>, uint32_t> flags;
        for (const MbRemapJob& j : P.jobs) {
            CHECK(j.flags != 0, "a remap job without flags");
            CHECK(flags.emplace(std::make_tuple(j.cam, j.tx, j.ty), j.flags).second, "a remap job twice");
        }
        size_t used = 0;
        for (int i = 0; i < P.n; i++)
            for (int ty = 0; ty < (L0.ty_n + opt.qpl - 1) / opt.qpl; ty++)
                for (int tx = 0; tx < L0.tx_n; tx++) {
                    uint32_t want = 0;
                    for (int h = 0; h < opt.qpl && ty * opt.qpl + h < L0.ty_n; h++)
                        for (int q = 0; q < kSubs; q++) {
                            const size_t s = ((size_t)(ty * opt.qpl + h) * L0.tx_n + tx) * kSubs + q;
                            if (P.req0_sub[i][s]) want |= item_g0_bit(h, q);
                            if (kind(0, s) == 4 && L0.sub_cams[s] == 1u << i) want |= item_result_bit(h, q);
                        }
                    auto it = flags.find(std::make_tuple(i, tx, ty));
                    CHECK((it == flags.end() ? 0u : it->second) == want, "flags of remap job %d, %d of camera %d", tx, ty, i);
                    used += it != flags.end();
                }
        CHECK(used == P.jobs.size(), "remap jobs outside the grid");
        long results = 0;
        for (size_t s = 0; s < L0.sub_own.size(); s++) results += L0.sub_own[s] == 4;
        CHECK(results == P.n_result, "n_result");
    }

    // every weighted tap of a tile lies in the staged patch [origin, origin + limit)
    void patches() const {
        for (int l = 0; l < P.B; l++) {
            const auto &L = P.lv[l], &Ln = P.lv[l + 1];
            auto axis = [&](const int32_t* org, bool rows, int off, int n_local, int n_src) {
                const int tile = rows ? kTileH : kTileW, limit = rows ? kUpPatchRows : kUpPatchCols;
                for (int g = std::max(off, 0); g < off + n_local; g++) {
                    const Taps t = taps_of(g - off, rows, n_src, 0);
                    for (int j = 0; j < t.n; j++)
                        CHECK(t.src[j] >= org[g / tile] && t.src[j] < org[g / tile] + limit, "level %d: tap %d of %d outside the patch at %d", l, t.src[j], g, org[g / tile]);
                }
            };
            for (int i = 0; i < P.n; i++) {
                const auto& c = L.cams[i];
                axis(L.up_org.data() + c.up_org, true, c.oy, c.h, Ln.cams[i].h);
                axis(L.up_org.data() + c.up_org + L.ty_n, false, c.ox, c.w, Ln.cams[i].w);
            }
            axis(L.rup_org.data(), true, 0, L.H, Ln.H);
            axis(L.rup_org.data() + L.ty_n, false, 0, L.W, Ln.W);
        }
    }

    void all() {
        level0_weights();
        owners_and_sets();
        if (!P.feather) {
            deep_by_definition();
            kinds();
        }
        required();
        work_lists();
        remap_jobs();
        patches();
    }
};

Seen run(const Rig& rig, const MbPlanOptions& opt) {
    Seen seen;
    g_seen = &seen;
    Upper upper;
    const MbPlan P = make_plan(rig, opt, upper);
    Checker c{rig, P, upper, opt, {}};
    c.all();
    return seen;
}

// One case: the rig with no knob, with no_deep and with no_remap_result (feather: once).
Seen run_case(const Rig& rig) {
    MbPlanOptions opt;
    const Seen d = run(rig, opt);
    printf("%-28s sub-tiles general %ld owned %ld deep %ld unread %ld result %ld\n", rig.name.c_str(), d.kinds[0], d.kinds[1],
           d.kinds[2], d.kinds[3], d.kinds[4]);
    if (rig.feather) return d;
    opt.no_deep = true;
    const Seen nd = run(rig, opt);
    CHECK(nd.kinds[2] + nd.kinds[3] + nd.kinds[4] == 0 && nd.kinds[1] >= d.kinds[1], "%s with no_deep", rig.name.c_str());
    opt.no_deep = false, opt.no_remap_result = true;
    const Seen nr = run(rig, opt);
    CHECK(nr.kinds[4] == 0, "%s with no_remap_result", rig.name.c_str());
    for (int l = 0; l <= kMbMaxBands; l++)
        CHECK(nr.deep_or_result[l] == d.deep_or_result[l], "%s: deep sub-tiles of level %d with no_remap_result", rig.name.c_str(), l);
    return d;
}

// Cameras side by side, ROIs overlapping by `lap`; seam(i, X, Y) gives camera i's seam on output pixel (X, Y).
template <class F>
Rig make_rig(std::string name, int out_w, int out_h, int bands, std::vector<MbRect> rois, F seam) {
    Rig r{std::move(name), out_w, out_h, bands, false, std::move(rois), {}};
    for (size_t i = 0; i < r.rois.size(); i++) {
        const MbRect& q = r.rois[i];
        r.seams.emplace_back((size_t)q.w * q.h);
        for (int y = 0; y < q.h; y++)
            for (int x = 0; x < q.w; x++) r.seams[i][(size_t)y * q.w + x] = seam((int)i, q.x + x, q.y + y);
    }
    return r;
}

void tap_tables() {  // the register taps weigh what the tables do, at every small size and offset
    for (int n_local = 1; n_local <= 40; n_local++)
        for (int off = 0; off <= 9; off++)
            for (int rows = 0; rows < 2; rows++)
                for (int n_src : {std::max(1, n_local >> 1), (n_local + 1) >> 1}) {
                    const int n_grid = (off + n_local + 7) / 8 * 8;
                    check_up_arith(up_table(n_grid, off, n_local, n_src, rows != 0), off, n_local, n_src, rows != 0);
                }
}

}  // namespace

int main() {
    tap_tables();
    // partition seams, full cover: two cameras split the frame at x = 256
    for (int bands = 1; bands <= 3; bands++) {
        const Rig r = make_rig("partition, " + std::to_string(bands) + " band(s)", 512, 128, bands,
                               {{0, 0, 288, 128}, {224, 0, 288, 128}},
                               [](int i, int X, int) { return (uint8_t)((X < 256) == (i == 0) ? 255 : 0); });
        const Seen s = run_case(r);
        CHECK(s.kinds[0] && s.kinds[4] && s.quirk_rows, "partition: no general / result sub-tile, or no quirk row");
        if (bands >= 2) CHECK(s.kinds[3], "partition: no unread sub-tile");
    }
    {  // graded seams: three cameras, ramps across the overlaps that do not sum to 255
        const Rig r = make_rig("graded", 384, 96, 2, {{0, 0, 160, 96}, {112, 0, 160, 96}, {224, 0, 160, 96}}, [](int i, int X, int Y) {
            const int c = 80 + 112 * i, d = std::abs(X - c);  // full weight within 40 of the camera's centre
            return (uint8_t)(d <= 40 ? 255 : std::max(0, 255 - (d - 40) * 9 - (Y & 3)));
        });
        const Seen s = run_case(r);
        CHECK(s.graded && s.kinds[0] && s.kinds[1] + s.kinds[2] + s.kinds[4], "graded: no graded pixel, general or owned sub-tile");
    }
    {  // grid origin (36, 16), a 300 x 92 grid: the crop cuts the last column and row of sub-tiles
        const Rig r = make_rig("origin and crop", 512, 128, 2, {{37, 19, 170, 86}, {150, 21, 186, 84}},
                               [](int i, int X, int) { return (uint8_t)((X < 180) == (i == 0) ? 255 : 0); });
        Upper up;
        const MbPlan P = make_plan(r, MbPlanOptions{}, up);
        CHECK(P.arr.x == 36 && P.arr.y == 16 && P.arr.w == 300 && P.arr.h == 92 && !P.full_cover, "origin case: grid %d %d %d %d", P.arr.x, P.arr.y, P.arr.w, P.arr.h);
        const Seen s = run_case(r);
        CHECK(s.cut_deep && s.kinds[4], "origin: no deep sub-tile cut by the crop");
    }
    {  // camera origins off the 8-pixel block grid (B = 1: origins are multiples of 2 only)
        const Rig r = make_rig("off the block grid", 256, 64, 1, {{0, 0, 150, 64}, {100, 6, 156, 50}},
                               [](int i, int X, int) { return (uint8_t)((X < 128) == (i == 0) ? 255 : 0); });
        const Seen s = run_case(r);
        CHECK(s.off_block && s.quirk_rows, "no camera off the block grid");
    }
    {  // one camera alone
        const Rig r = make_rig("one camera", 256, 64, 2, {{0, 0, 256, 64}}, [](int, int, int) { return (uint8_t)255; });
        const Seen s = run_case(r);
        CHECK(s.kinds[0] == 0 && s.kinds[4] && s.kinds[3], "one camera: general sub-tiles, or none skipped");
    }
    {  // feather: ROIs of odd origin and size, of mixed parity
        Rig r{"feather", 256, 64, 0, true, {{3, 5, 141, 51}, {100, 2, 150, 57}, {201, 7, 54, 40}}, {}};
        const Seen s = run_case(r);
        CHECK(s.kinds[0], "feather: no tile");
    }
    printf("multiband_plan_check ok\n");
    return 0;
}
