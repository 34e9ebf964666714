// kernels.hpp — launch interface of the gfx950 kernels (internal; the public boundary is
// include/octvr_hip.h).  All launchers are stream-ordered and never synchronize.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "camera_math.hpp"
#include "frame_layout.hpp"
#include "multiband_plan.hpp"

namespace octvr {

constexpr int kMaxCams = 32;

// Composite-LUT entry (8 bytes per output pixel), built once per rig by composite_lut:
//   x = sx | sy << 16                      integer source pixel of the top-left tap, s16 each
//   y = fx | fy << 5 | cam << 10 | 1 << 15  5-bit fractions, winning camera, valid flag
// An entry with the valid bit clear produces black (no camera covers the pixel).
struct CompositeEntry {
    uint32_t xy;
    uint32_t code;
};

// Fixed-point source coordinate of a normalized map value, as RemapInvoker derives it from the
// caller's `map * W` (template.cpp:174-176): X = fl32(m * W); ix = round_half_even(X * 32), NaN and
// out-of-int-range values INT_MIN (_mm_cvtps_epi32, imgwarp.cpp:4385-4420).
__host__ __device__ inline int quantize_coord(float m, float scale) {
    float X = m * scale;
    float f = X * 32.0f;
    if (!(f >= -2147483648.f && f < 2147483648.f)) return INT32_MIN;
    return (int)rintf(f);
}

// Entry for a claimed pixel.  Template-built LUTs keep 0 <= m < 1 where the mask is set, but
// morphed or externally made ones (.dat, from_arrays) need not: the tap cell saturates to s16 like
// remap's (short) conversion and every tap outside the image reads 0 (BORDER_CONSTANT).
__host__ __device__ inline CompositeEntry make_entry(float m1, float m2, float w, float h, int cam) {
    int ix = quantize_coord(m1, w), iy = quantize_coord(m2, h);
    const int sx = min(max(ix >> 5, -32768), 32767), sy = min(max(iy >> 5, -32768), 32767);
    CompositeEntry e;
    e.xy = (uint32_t)(uint16_t)sx | ((uint32_t)(uint16_t)sy << 16);
    e.code = (uint32_t)(ix & 31) | ((uint32_t)(iy & 31) << 5) | ((uint32_t)cam << 10) | (1u << 15);
    return e;
}

// Texture-convention entry (mapper flag OCTVR_REMAP_TEXTURE): the sampling of the reference's live CUDA
// path, cv::cuda::fastRemap through a linear-filtered, clamp-addressed texture with normalized coordinates
// (cudawarping/src/cuda/fast_remap.cu:21-44, texture.hpp:124-160), as oracle/octvr_oracle.c
// orc_fast_remap_tex_rgba models NVIDIA's filter: X = fl32(u W) - 0.5, i0 = floor(X), alpha =
// floor(frac(X) 256) / 256 (8 fractional bits), taps (i0, i0 + 1) x (j0, j0 + 1) clamped to the image and
// all four used.  xy: (i0, j0) kept in [-1, size - 1] (the same taps under the clamp); code: alpha | cam <<
// 10 | valid << 15 | beta << 17 | kCodeTex.  u < 0, NaN or infinite coordinates: invalid (black).  Tiles holding
// such entries always take the gather path (tiling.cpp), whose taps and weights test kCodeTex.
constexpr uint32_t kCodeTex = 1u << 31;
__host__ __device__ inline CompositeEntry make_entry_tex(float m1, float m2, float w, float h, int cam) {
    CompositeEntry e{0u, 0u};
    const float xb = m1 * w - 0.5f, yb = m2 * h - 0.5f;
    // u < 0: fill_zero; NaN or an infinite coordinate: the model's weights are NaN and every channel
    // saturates to 0 — the same black
    if (!(m1 >= 0.f) || !(fabsf(xb) <= 3.0e38f) || !(fabsf(yb) <= 3.0e38f)) return e;
    const float fx = floorf(xb), fy = floorf(yb);
    const uint32_t a = (uint32_t)floorf((xb - fx) * 256.f), b = (uint32_t)floorf((yb - fy) * 256.f);
    const int i0 = (int)fminf(fmaxf(fx, -1.f), w - 1.f), j0 = (int)fminf(fmaxf(fy, -1.f), h - 1.f);
    e.xy = (uint32_t)(uint16_t)(int16_t)i0 | ((uint32_t)(uint16_t)(int16_t)j0 << 16);
    e.code = (a & 255u) | ((uint32_t)cam << 10) | (1u << 15) | ((b & 255u) << 17) | kCodeTex;
    return e;
}

// The 2 x 2 taps of an entry's cell (sx, sy) in a w x h image: clamped addresses and in-image flags.
struct TapCell {
    int x0, x1, y0, y1;
    bool ix0, ix1, iy0, iy1;
};
__host__ __device__ inline TapCell tap_cell(uint32_t xy, int w, int h) {
    const int sx = (int)(int16_t)(xy & 0xFFFFu), sy = (int)(int16_t)(xy >> 16);
    TapCell c;
    c.ix0 = (unsigned)sx < (unsigned)w;
    c.ix1 = (unsigned)(sx + 1) < (unsigned)w;
    c.iy0 = (unsigned)sy < (unsigned)h;
    c.iy1 = (unsigned)(sy + 1) < (unsigned)h;
    c.x0 = min(max(sx, 0), w - 1);
    c.x1 = min(max(sx + 1, 0), w - 1);
    c.y0 = min(max(sy, 0), h - 1);
    c.y1 = min(max(sy + 1, 0), h - 1);
    return c;
}

// ---- tiled composite (the per-frame hot path) -------------------------------------------------
// The output is cut into 128 x 8 pixel tiles (one 256-lane workgroup per tile, one 2x2 quad per
// lane).  Per tile the host pre-computes, once per rig, which cameras win inside it (<= 4 "slots")
// and the luma bounding box of every in-image bilinear tap of each slot.  A staged tile converts
// those boxes from YUV420P (8-byte Y + 4-byte U/V loads per 8 pixels) into packed RGBA in LDS — every source pixel
// converted once, as NPP's full-frame pass does in the reference — at a tile-uniform row stride.
// Staging work is cut into chunks of 64 eight-pixel groups, each chunk inside one slot, so a wave's
// chunk has wave-uniform slot parameters (scalar registers, no per-lane slot search).
// LDS dwords 0-3 of the tile area are zero: a black pixel's entry (0) reads its tap (x, y) there.
// Each slot's box reaches one column / row past its taps (x0 + 1, y0 + 1), including taps outside
// the source image: staging writes RGBA 0 for box pixels outside the image (BORDER_CONSTANT), so
// every tap is read from LDS at off, off + 4, off + 4 S, off + 4 S + 4 (S = row stride) unmasked.
// The LUT is tile-major (quad-major inside the tile), 4 bytes per pixel:
//   bit 0 "no gain" (RGBA mode); bits 1-2 zero; 3-12 the fraction code fx | fy << 5, so e & 0x1FF8 is
//   the byte offset of the code's two packed weight pairs in the workgroup's 8 KiB LDS weight table;
//   13-26 LDS byte offset of tap (x, y) (one v_bfe_u32); 27-29 zero; 30-31 slot (the slot's gain
//   sits at byte offset e >> 27 of a 4-slot table of f32 pairs).  Three VALU decode a pixel's entry.
// A pixel with no camera, or with every tap outside, is entry 0 and comes out black.
// (the tile, kTileW x kTileH = 128 x 8 pixels: multiband_plan.hpp)
constexpr int kTileSlots = 4;
// Items of the tiled composite: two vertically adjacent 128 x 8 tiles (128 x 16 pixels, 8 quads per lane).
constexpr int kItemHalves = 2;
// Staging LDS: 16 KiB less the composite's 176 bytes of other LDS, so its static LDS is exactly 16 KiB
// and the 8 KiB weight table starts at LDS address 0x4000 (every C2 / C4 item stages < 16 KiB; 6
// workgroups per CU by LDS)
constexpr int kTileLdsBytes = 16 * 1024 - 176;
static_assert(kTileLdsBytes <= (1 << 14), "the tiled entry's LDS byte offset field");
constexpr uint32_t kWtabBytes = 1024u * 8u;
constexpr int kTileZeroDwords = 4;
// Staging stores: 2 x 16 bytes per 8-pixel group, so a row stride is a multiple of 4 dwords.
constexpr int kStageAlignDwords = 4;
// The tiler pads an item's row stride by up to this many dwords (tiling.cpp: the stride whose tap reads
// conflict least in the LDS banks)
constexpr uint32_t kStridePadMax = 28;

struct TileSlot {
    uint16_t cam;
    uint16_t bw, bh;   // luma box size (bw a multiple of 8, bh even)
    uint16_t lds;      // dword offset of the slot's RGBA box in the tile's LDS area
    uint16_t bx0, by0; // luma box origin (bx0 multiple of 8, by0 even)
    uint16_t chunk0;   // first 64-group staging chunk of this slot (slots are chunk-aligned)
    uint16_t pad1;
};

struct TileHdr {           // one staged item
    uint32_t tile;          // item column | item row << 16 (items of 128 x 8 qpl pixels)
    uint32_t nslots;        // bits 0-7: slots used (0..4); bits 8-15: 64-group staging chunks
    uint32_t stage_groups;  // 4-pixel groups to convert into LDS (host; the device word: TiledLutDev::upload)
    uint32_t stride;        // bits 0-8: LDS row stride in dwords (max box width of the item + a bank pad); bits 9-31:
                            // the item's first chunk in the group overflow table (TiledLut::grp1)
};
constexpr int kStrideBits = 9;
static_assert(256 + kStridePadMax < (1u << kStrideBits), "a padded stride fits its field");
// Staging groups: an item stages, per slot and box row, only the 8-pixel groups between the row's leftmost
// and rightmost tap (the box layout in LDS is kept: the entries' tap offsets do not change).  One u16 per
// group: bit 15 valid, bits 8-12 the group's column in the box (x = bx0 + 8 col), bits 0-7 its row.  A
// slot's groups fill whole 64-group chunks (the last one padded with invalid groups); chunk c of an item:
// grp0[(t kGroupFirst + c) 64 + lane] for c < kGroupFirst (each wave's first chunk, loaded one iteration
// ahead by item index alone), grp1[(ovf + c - kGroupFirst) 64 + lane] after (ovf: TileHdr::stride >> 9).
constexpr int kGroupFirst = 4;
constexpr uint32_t kGroupValid = 0x8000u;

// Pixel layouts of a stitch (octvr_mapper_set_pixel_formats), a launch argument: the inputs' (all alike) and
// the output's chroma rows hold a U half and a V half ("Y over [U|V]", the default) or, with the bit set,
// U,V byte pairs (NV12).  The luma rows, the sizes and the pitch rules are the same.
constexpr int kPixInNv12 = 1, kPixOutNv12 = 2;

// One input camera as the per-frame kernels see it: a YUV420P frame in "Y over [U|V]" layout (or NV12, kPixInNv12).
struct SourceFrame {
    const uint8_t* yuv;
    int32_t w, h;
    int64_t pitch;
    const float* vig;  // vignette gain per source pixel (w x h, packed) or NULL (mapper.cpp:108-112,230-231)
};

// All camera frames of one stitch call, passed by value as a kernel argument (no per-frame H2D copy).
struct FrameSet {
    SourceFrame f[kMaxCams];
};

// The frames of one composite launch (launch_stitch, octvr_mapper_stitch_batch): 1 << nf_log2 frame sets
// (at most kMaxBatch) stitched in one pass over the tiled LUT.  The item sequence runs over (item, frame)
// pairs — unit v = item << nf_log2 | frame — so the units of one item are dealt to neighbouring workgroups
// of one XCD band at the same time: the item's entries, metadata and staging groups come from HBM (or the
// Infinity Cache) once for all the frames and from L2 for the others, while each unit stages and computes
// its own frame.  Camera c of frame f: src[(f << cam_log2) + c], cam_log2 = 5 (32 cameras) for one or two
// frames, 4 (16 cameras) for four.  The FIRST argument of the composite kernels (kernarg_frame), sized for
// its frame count (one frame: 1,040 B of kernarg, as the round-5 FrameSet + pointers).
constexpr int kMaxBatch = 4;
template <int NF>
struct FrameBatch {
    static constexpr int kCamLog2 = NF <= 2 ? 5 : 4;
    SourceFrame src[NF << kCamLog2];
    uint8_t* out[NF];        // MODE 0: the frames' YUV420P outputs (one pitch)
    const double* gains[NF]; // the frames' gains (device)
};


// One NV12 plane of a FastMapper (fastmapper.cpp / fastmapper.hip): per run {camera mask, first block},
// and per (camera, run) block either the compact entries (header + u32 offsets/fractions + u8 weights)
// or the wide uint2 entries; nblk: the blocks allocated (>= 1).
struct FastMapperPlane {
    bool compact;
    const uint2* ent;
    const uint32_t* off;
    const uint8_t* wgt;
    const uint2* hdr;
    const uint2* runs;
    uint32_t nblk;
};

// ROI-sized per-camera template data resident on the device.
struct CamTemplate {
    const float* map1;
    const float* map2;
    const uint8_t* mask;
    int32_t roi_x, roi_y, roi_w, roi_h;
    int32_t in_w, in_h;
};

// Gain-feed work description (built on the host once per rig, GainCompensatorGPU ctor
// exposure_compensate.cpp:174-221 + Mapper ctor mapper.cpp:94-114).  Every working-scale pixel of
// camera i that lies in the bitwise-AND intersection with some camera j becomes one sample: its
// 8-byte entry plus a partner mask (bit j).  Samples are sorted by (camera, source row, column); each
// camera's run is padded with invalid samples (partner mask 0) to whole runs of kGainWaveRun (one
// wave each, so a wave's frame is uniform), the whole array to chunks of kGainChunk (one workgroup,
// about one workgroup per CU on C2).
constexpr int kGainMaxCams = 16;
constexpr int kGainPer = 3;  // samples per lane of the gain feed
constexpr int kGainWaveRun = 64 * kGainPer;  // one wave's samples: contiguous, one camera
constexpr int kGainChunk = 4 * kGainWaveRun;  // one workgroup's samples (4 waves)
constexpr int kGainTotalStride = 32;  // u64 words between pair totals: one 256-B line each

// cams_dev: {output camera, input camera} in device memory (CameraParams holds the ocam polynomials).
// fragile (optional, cap + 1 words, fragile[0] zero): indices of the pixels the host must recompute
// (LutGuard, camera_math.hpp); fragile[0] receives their count (entries past cap are dropped).
hipError_t launch_lut_build(const CameraParams* cams_dev, int W, int H, float* map1, float* map2, uint8_t* mask,
                            int32_t* bbox, uint8_t* visible, uint32_t* fragile, uint32_t cap, hipStream_t s);

hipError_t launch_project_f64(const CameraParams* cams_dev, int W, int H, double* x, double* y, uint8_t* fragile,
                              hipStream_t s);

// tex: texture-convention entries (make_entry_tex) instead of cv::remap's (make_entry)
hipError_t launch_composite_lut(const CamTemplate* cams_dev, int n, int W, int H, CompositeEntry* lut,
                                hipStream_t s, int tex = 0);

// Gain feed in ONE launch (no host sync): each workgroup gathers its chunk's warped samples, takes
// the f32 RGB norm (elementNorm) and adds it per partner camera into exact u64 fixed-point totals
// (units of 2^-23, see gain_feed.hip); the last workgroup (per-XCD then global ticket) reads and
// resets the totals, assembles I(i,j), A, b and solves.  `totals` (kGainMaxCams^2) and `tickets`
// (9) must be zero before the first launch; the last workgroup leaves them zero.  tex: the samples are
// texture-convention entries (make_entry_tex).
hipError_t launch_gain_feed(const FrameSet& frames, const CompositeEntry* samples, const uint16_t* partners, int tex,
                            int n_chunks, const int32_t* N, int n,
                            unsigned long long* totals, uint32_t* tickets, double* gains, hipStream_t s,
                            bool lean = false,  // lean: <= 80 VGPRs (73 used), runs beside a composite (gain_feed.hip)
                            int pix = 0);       // kPixInNv12: the frames are NV12

// FastMapper frames of one launch (octvr_fastmapper_stitch_nv12_batch): camera c of frame f at
// src[(f << cam_log2) + c] (cam_log2 5 for up to 2 frames, 4 for 4), the frames' NV12 outputs.
template <int NF>
struct FastBatch {
    SourceFrame src[NF << (NF <= 2 ? 5 : 4)];
    uint8_t* out[NF];
};

// The feeds of nf frames (1, 2 or 4) of a batch in one launch: workgroup b feeds frame b / n_chunks into its
// own totals / tickets / gains (FeedBatch, the kernel's first argument; one frame: 536 B of kernarg).
template <int NF>
struct FeedBatch {
    SourceFrame src[NF * kGainMaxCams];  // camera c of frame f at f * kGainMaxCams + c
    unsigned long long* totals[NF];
    uint32_t* tickets[NF];
    double* gains[NF];
};
hipError_t launch_gain_feed_batch(const FrameSet* frames, int nf, const CompositeEntry* samples, const uint16_t* partners,
                                  int tex, int n_chunks, const int32_t* N, int n, unsigned long long* const* totals,
                                  uint32_t* const* tickets, double* const* gains, hipStream_t s, bool lean, int pix = 0);

hipError_t launch_set_gains(const double* host_gains, int n, double* gains_dev, hipStream_t s);

// octvr_debug_gain_solve: `count` n x n systems (device arrays, row-major) through the feed's own solver
// selection (gain_feed.hip gain_solve), the full feed's or the lean feed's; one workgroup per system.
hipError_t launch_gain_solve(const double* A, const double* b, int n, int count, bool lean, double* x, int* ok,
                             hipStream_t s);

// AsyncMultiMapper footprint upload (async.cpp): the runs of a table (frame_layout.hpp FootRun), each packed at its
// `off` by pack_run, into the cameras' device frames (pitch = width).  launch_unpack_runs: luma row 2r, luma row
// 2r + 1, then the chroma row's U and V parts, into frames "Y over [U | V]".
struct FootFrames {
    uint8_t* f[kMaxCams];
    int w[kMaxCams], h[kMaxCams];
};
hipError_t launch_unpack_runs(const uint8_t* packed, const FootRun* runs, int n_runs, const FootFrames& frames,
                              hipStream_t s);
// The same for a pipeline whose input frames are NV12 (async_kernels.hip): the run's chroma is one row of
// 8 ng bytes of U,V pairs (cut at the width) at byte column 8 g0, the frames "Y over U,V pairs"; nv12 == 0 is
// launch_unpack_runs.
hipError_t launch_unpack_runs_layout(const uint8_t* packed, const FootRun* runs, int n_runs, const FootFrames& frames,
                                     int nv12, hipStream_t s);
// octvr_async_push_device's merge (async_merge.hip): every region frame of the table (async_host.hpp
// build_merge_table) into its place in the merged device frame `out`, one launch.
struct MergeTable;
hipError_t launch_merge_regions(uint8_t* out, const MergeTable& t, hipStream_t s);
// octvr_async_set_output_format's merge (async_merge_pack.hip): every NV12 region frame of the table (async_host.hpp
// build_merge_pack_table) into its place in the merged frame `out` of the converted layout `pix`, one launch.
struct MergePackTable;
hipError_t launch_merge_pack(int pix, uint8_t* out, const MergePackTable& t, hipStream_t s);
// The converted capture layouts (the OCTVR_PIX_* values >= 16, frame_layout.hip; the arithmetic, the table and the
// layouts' descriptors in frame_layout.hpp; `pix` is the OCTVR_PIX_* value).
// launch_layout_unpack: the groups of the table's pieces (run_table: runs of at most 64 groups) from sources of the
// layout into the cameras' NV12 frames `frames` (pitch = width).  The sources are the pipeline's packed upload
// buffer (`packed`, each piece at its `off`) or, with packed NULL, one whole frame of the layout per camera at its
// pitch (>= the layout's row bytes; base and pitch even for 16-bit samples).
struct ConvSources {
    const uint8_t* packed;
    const uint8_t* f[kMaxCams];
    size_t pitch[kMaxCams];
};
hipError_t launch_layout_unpack(int pix, const FootRun* table, int n_pieces, const ConvSources& src, const FootFrames& frames,
                                hipStream_t s);
// launch_layout_pack: the whole w x h NV12 frame `src` (pitch = w) into the frame `out` of the layout at `pitch`
// (>= the layout's row bytes, any alignment; even base and pitch for 16-bit samples); bytes of a row past the
// layout's row bytes are not written.
hipError_t launch_layout_pack(int pix, const uint8_t* src, int w, int h, uint8_t* out, size_t pitch, hipStream_t s);

struct TiledLut {
    const TileHdr* meta;          // per staged item kMetaWords 16-byte words: the TileHdr, then kTileSlots TileSlots
    const uint32_t* entries;      // kTilePx per staged item, quad-major inside the tile
    int n_items;
    const uint32_t* wide_tiles;   // tile column | row << 16 of each wide tile
    const CompositeEntry* wide;   // kTilePx per wide tile
    int n_wide;
    const uint16_t* wide_cams;    // RGBA mode: output camera of each wide tile | its half's item flags << 8
    const int32_t* bands;         // kStitchBands + 1 staged-item boundaries (one band per XCD)
    uint32_t* queue;              // per band a work counter, then a done ticket, kQueueStride apart;
                                  // zero before a launch, left zero by its last workgroup
    int qpl;                      // quads per lane: an item is 128 x (8 qpl) pixels, qpl * kTilePx entries
    const uint16_t* grp0;         // staging groups of each item's first kGroupFirst chunks (kGroupFirst * 64 per item)
    const uint16_t* grp1;         // the items' further chunks
    uint32_t n_grp1;              // entries of grp1
    int tex;                      // staged entries are texture-convention ones (tiled_entry_tex)
    int e24;                      // entries packed to 24 bits (tiled_entry24): 12 bytes per lane and half
    int n_packed;                 // items held as quad records (kItemPacked); > 0 selects the instances that read them
};
constexpr int kMetaWords = 1 + kTileSlots;
constexpr int kQueueStride = 32;  // u32 words: one 128-B line per counter
// The staged items are cut into one contiguous band per XCD (locality: neighbouring tiles share
// source boxes in that XCD's L2) of equal item counts.  Measured on the C2 rig (r01 v10): equal counts
// beat every split weighted by staging chunks tried (base 16 / 8 / 4 / 2 per chunk: +2 % / +4 % / +10 % /
// +19 % stitch time) — the large pole boxes are re-read from L2 by many tiles, so staging chunks do not
// predict a tile's cost.
constexpr int kStitchBands = 8;
// 4-byte tiled entries: bit 0 = "no gain" (a pixel the gain does not touch: LUT mask 0 with an
// in-image map value; mul_scalar_with_mask, exposure_compensate.cu:15-30).  8-byte CompositeEntry
// records carry the same flag in code bit 16.  TileHdr.nslots bits 16-20: output camera (RGBA mode).
constexpr uint32_t kEntryNoGain = 1u;
constexpr int kEntrySlotShift = 30;
constexpr uint32_t kCodeNoGain = 1u << 16;

// One staged pixel's 4-byte entry (layout above): off = LDS byte offset of tap (x, y) in the item's
// staging area, fxy = fx | fy << 5.
__host__ __device__ constexpr uint32_t tiled_entry(uint32_t off, uint32_t fxy, uint32_t slot, bool nogain) {
    return (nogain ? kEntryNoGain : 0u) | (fxy & 1023u) << 3 | off << 13 | slot << kEntrySlotShift;
}

// The same entry in 24 bits, for LUTs without "no gain" pixels (TiledLutDev::upload packs them): bits 0-1
// the slot, 2-11 fxy, 12-23 the tap's LDS dword offset.  A lane's four entries of a half are packed into
// three dwords (c0 | c1 << 24, c1 >> 8 | c2 << 16, c2 >> 16 | c3 << 8): 3 instead of 4 bytes per pixel.
__host__ __device__ constexpr uint32_t tiled_entry24(uint32_t e) {
    return (e >> 30) | ((e >> 3) & 1023u) << 2 | ((e >> 15) & 4095u) << 12;
}

// Quad-packed items (blend = 0, default sampling): one 8-byte record per lane quad and half instead of four
// 4-byte entries, for items whose every quad is either black (four entries 0: record 0) or has one slot, no
// "no gain" pixel and tap origins within {0, 1} x {0, 1} of a common base (dword offsets base + dx + dy S,
// S the item's row stride) — what an output that oversamples its sources produces away from seams.  Such an
// item carries kItemPacked in TileHdr::nslots and keeps its records in the first half of its 8 KiB of
// entries (lane quad q's records of half 0 and half 1 at byte 16 q: one 16-byte load per lane); any other item
// keeps the 4-byte entries.
//   lo: bits 2-11 fxy of pixel 0, 12-21 of pixel 1, 22-31 of pixel 2 (bits 0-1 zero)
//   hi: bits 0-2 dx of pixels 0-2, 3 dy of pixel 3, 4-15 base, 16 dx of pixel 3, 17-19 dy of pixels 0-2,
//       20-21 the slot, 22-31 fxy of pixel 3
// Decode: pixel p's flags are one bit in each 16-bit half of hi & quad_flag_mask(p), so one v_dot2_u32_u16
// with the item-uniform pair quad_flag_mul(p, S) adds 4 dx + 4 S dy to the base's byte offset; a shift puts
// the pixel's fxy where wtab_read masks it (bits 3-12); the slot's gain is read once per quad.
constexpr uint32_t kItemPacked = 1u << 24;  // TileHdr::nslots
__host__ __device__ constexpr uint32_t quad_flag_mask(int p) {
    return p == 3 ? (1u << 16 | 1u << 3) : (1u << p | 1u << (17 + p));
}
// the multipliers of the low and the high half's flag bit (S a multiple of 4 dwords, so every one is whole)
__host__ __device__ constexpr uint32_t quad_flag_mul(int p, uint32_t S) {
    return p == 3 ? ((S >> 1) | 4u << 16) : ((4u >> p) | ((2u * S) >> p) << 16);
}
// the record's dword (lo for pixels 0-2, hi for pixel 3) shifted so that fxy sits at bits 3-12
__host__ __device__ constexpr uint32_t quad_fxy_view(int p, uint32_t lo, uint32_t hi) {
    return p == 0 ? lo << 1 : p == 1 ? lo >> 9 : p == 2 ? lo >> 19 : hi >> 19;
}
// LDS byte offset of the base tap and of the slot's gain pair
__host__ __device__ constexpr uint32_t quad_base4(uint32_t hi) { return (hi >> 2) & 0x3FFCu; }
__host__ __device__ constexpr uint32_t quad_gain_off(uint32_t hi) { return (hi >> 17) & 0x18u; }

// The four 4-byte entries of a record, by the arithmetic the kernel's decode runs (host model and tests).
__host__ __device__ inline void quad_unpack(uint64_t rec, uint32_t S, uint32_t e[4]) {
    const uint32_t lo = (uint32_t)rec, hi = (uint32_t)(rec >> 32);
    for (int p = 0; p < 4; p++) {
        if (!rec) {
            e[p] = 0u;
            continue;
        }
        const uint32_t a = hi & quad_flag_mask(p), m = quad_flag_mul(p, S);
        const uint32_t off = quad_base4(hi) + (a & 0xFFFFu) * (m & 0xFFFFu) + (a >> 16) * (m >> 16);
        e[p] = (quad_fxy_view(p, lo, hi) & 0x1FF8u) | off << 13 | (quad_gain_off(hi) >> 3) << 30;
    }
}

// Packs a quad's four entries of an item of row stride S (dwords); false if the quad does not qualify.
__host__ __device__ inline bool quad_pack(const uint32_t e[4], uint32_t S, uint64_t* rec) {
    *rec = 0;
    if (!(e[0] | e[1] | e[2] | e[3])) return true;  // black
    if (S < 8u || (S & 3u)) return false;
    uint32_t o[4], lo_o = 0xFFFFFFFFu;
    for (int p = 0; p < 4; p++) {
        // a black pixel beside live ones, a "no gain" pixel, a second slot
        if (!e[p] || (e[p] & 7u) || (e[p] >> 27 & 7u) || (e[p] >> 30) != (e[0] >> 30)) return false;
        if ((e[p] >> 13) & 3u) return false;
        o[p] = ((e[p] >> 13) & 0x3FFFu) >> 2;
        lo_o = o[p] < lo_o ? o[p] : lo_o;
    }
    // the base: the lowest origin, or the dword before it when the quad's leftmost and topmost origins differ
    // (origins at (1, 0) and (0, 1) of the cell)
    for (uint32_t back = 0; back < 2; back++) {
        if (lo_o < back) break;
        const uint32_t base = lo_o - back;
        uint32_t dx[4], dy[4];
        bool ok = true;
        for (int p = 0; p < 4 && ok; p++) {
            const uint32_t d = o[p] - base;
            ok = d == 0u || d == 1u || d == S || d == S + 1u;
            dx[p] = (d == 1u || d == S + 1u) ? 1u : 0u;
            dy[p] = d >= S ? 1u : 0u;
        }
        if (!ok) continue;
        const uint32_t f[4] = {(e[0] >> 3) & 1023u, (e[1] >> 3) & 1023u, (e[2] >> 3) & 1023u, (e[3] >> 3) & 1023u};
        const uint32_t lo = f[0] << 2 | f[1] << 12 | f[2] << 22;
        const uint32_t hi = dx[0] | dx[1] << 1 | dx[2] << 2 | dy[3] << 3 | base << 4 | dx[3] << 16 | dy[0] << 17 |
                            dy[1] << 18 | dy[2] << 19 | (e[0] >> 30) << 20 | f[3] << 22;
        *rec = (uint64_t)hi << 32 | lo;
        return true;
    }
    return false;
}

// A staged texture-convention pixel (make_entry_tex with all four taps inside the image): bit 0 "no gain",
// bits 1-8 alpha, 9-16 beta (8-bit fractions), 17-28 the tap's LDS dword offset, 30-31 the slot.
__host__ __device__ constexpr uint32_t tiled_entry_tex(uint32_t off, uint32_t ab, uint32_t slot, bool nogain) {
    return (nogain ? kEntryNoGain : 0u) | (ab & 0xFFFFu) << 1 | (off >> 2) << 17 | slot << kEntrySlotShift;
}

// 128 x 8 halves per item of the tiled composite (kItemHalves): the tiler's qpl.
int composite_qpl();

// ev0 / ev1 (optional): timing events around the composite (carried by the dispatch packet when it
// is a single launch).  pix: the layouts of the frames and of `out` (kPixInNv12 | kPixOutNv12)
hipError_t launch_stitch(const FrameSet& frames_dev, const TiledLut& lut, int W, int H,
                         const double* gains, int use_gain, uint8_t* out, int64_t out_pitch, hipStream_t s,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int pix = 0);
// nf frames (1, 2 or 4; frame f = frames[f], gains[f], out[f], all outputs of pitch out_pitch) in one
// composite launch (FrameBatch); more than 16 cameras need nf <= 2
hipError_t launch_stitch_batch(const FrameSet* frames, int nf, const TiledLut& lut, int W, int H,
                               const double* const* gains, int use_gain, uint8_t* const* out, int64_t out_pitch,
                               hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int pix = 0);

// ---- multi-band blend (blend > 0): MultiBandGPUBlender (blenders.cpp:589-735) ------------------
// Level l of the blend lives on the "level grid": align_result_roi >> l.  Each camera keeps its
// Gaussian pyramid G (u8x4, camera-local, dense over align_roi >> l) but only the 128x8 tiles some
// blend step reads are ever computed (tile lists built once per rig).  pyrUp is evaluated on the
// fly from 3x3 source taps per output quad through per-row / per-column tap tables (UpQuad), which
// encode pyr_up.cu's borders (abs, then clamp) and its 8-row-block quirk.
// (kMbMaxBands, the staged patch kUpPatchRows x kUpPatchCols, UpQuad and the register taps up_arith:
// multiband_plan.hpp, which also builds the tables)

struct MbCamLevel {       // one camera at one level
    uint32_t g_off;        // byte offset of the camera's G in the level's pyramid allocation
    uint32_t g_pitch;      // bytes per row of G (4 * w)
    int32_t ox, oy, w, h;  // camera's aligned ROI on the level grid: origin and size
    const void* weight;    // level 0: u8 seam mask (pitch w), else f32 Gaussian weight (pitch w)
    const UpQuad* up_rows; // pyrUp taps into this camera's next level, by level-grid quad row
    const UpQuad* up_cols; // ... by level-grid quad column
    const int32_t* up_r0;  // per tile row / column: origin of the tile's staged source patch
    const int32_t* up_c0;
};

// Level-0 pyramid images as the composite kernels' RGBA sink.
struct RgbaOut {
    uint8_t* base;
    uint32_t bytes;        // allocation size (< 2^31)
    const MbCamLevel* cams;
    // Deep level-0 tiles (multi-band, owned = 4 on the host: the result there is exactly the owner
    // camera's G0): items flagged kItemResult write their halves' final result from the remap itself,
    // so the level-0 blend skips those tiles; items flagged kItemNoG0 write no G0 for that half (nothing
    // reads it).  The result frame is addressed from the level-0 grid origin (align_result_roi's
    // top-left): `res` points there, YUV420P with the U / V planes at res_u_off / res_v_off bytes
    // (res_rgba = 0; an NV12 frame: its U,V pairs at res_u_off, res_v_off = 0, as OutFrame), or the RGBA
    // result image of a scaled output (res_rgba = 1).  Flagged tiles lie
    // wholly inside the crop and the frame (multiband_create), so the stores need no bounds.
    uint8_t* res;
    uint32_t res_bytes;    // addressable bytes from `res` (< 2^31)
    uint32_t res_pitch, res_u_off, res_v_off;
    int res_rgba;
};
// (the 32 x 8 sub-tiles kSubW / kSubs, their classification and the remap items' item_result_bit /
// item_g0_bit: multiband_plan.hpp)
constexpr uint32_t kItemAllG0 = 0xFF00u;

hipError_t launch_mb_remap(const FrameSet& frames, const TiledLut& lut, const double* gains, int use_gain,
                           const RgbaOut& out, hipStream_t s, int pix = 0);  // pix: kPixInNv12 (the result frame's
                                                                             // layout travels in RgbaOut)
// fastPyrDown<uchar4> (fast_pyr_down.cu:17-76) of every listed (camera, tile) of level l from l - 1.
hipError_t launch_mb_down(const uint2* items, int n_items, const MbCamLevel* cams_l, const MbCamLevel* cams_prev,
                          const uint8_t* g_prev, uint8_t* g_l, hipStream_t s);
struct MbBlendArgs {
    int level, bands, n_cams;
    int w_u8;                       // weights are the u8 seam mask (multi-band level 0), else f32
    int feather;                    // FeatherGPUBlender: out = sat_u8(out_scale * D), no normalisation
    float out_scale;                // (float)(1.0 / n) (convertTo alpha, blenders.cpp:579)
    int W, H;                       // level grid
    int tiles_x;
    const uint32_t* tile_cams;      // bit n: camera n has a non-zero weight in the tile
    const uint8_t* owned;           // multi-band (or NULL): the tile's one camera has weight 1 on every tile pixel
    const uint2* work;              // multi-band (or NULL): the sub-tiles to blend, 4 per workgroup (wave w of
                                    // block b takes work[4 b + w]): x = tile | quarter << 24 | owned << 27,
                                    // y = the sub-tile's cameras; padded with owned = 3 (nothing to do)
    int n_work;                     // their count, a multiple of 4 (0: nothing to launch); -1 without a list
    const MbCamLevel* cams;         // this level
    const MbCamLevel* cams_next;    // level + 1 (NULL at the top)
    const uint8_t* g;               // this level's pyramid allocation
    const uint8_t* g_next;          // level + 1 allocation
    const int16_t* r_next;          // collapsed level + 1 (s16x4, W_next x H_next)
    int W_next, H_next;
    const UpQuad* rup_rows;         // pyrUp taps of the collapse (level grid, camera independent)
    const UpQuad* rup_cols;
    const int32_t* rup_r0;          // per tile row / column: origin of the staged collapse patch
    const int32_t* rup_c0;
    int16_t* r_out;                 // level > 0: collapsed level (s16x4, pitch 4 * W shorts)
    uint8_t* out;                   // level 0: YUV420P output frame (out_nv12: NV12)
    int64_t out_pitch;
    int out_nv12;
    int out_w, out_h;
    int ax, ay, crop_w, crop_h;     // align_result_roi origin in the output frame, crop size
    uint8_t* rgba;                  // level 0, scaled output: the RGB result as RGBA (out_w x out_h) instead of YUV
    int64_t rgba_pitch;
    // level 0, multi-band: owned = 4 marks deep tiles whose result the remap wrote (kItemResult)
};
hipError_t launch_mb_blend(const MbBlendArgs& a, hipStream_t s);
// Build time: K4 pyrDown<float, BrdReflect101> with nvcc's FMA contraction (pyr_down.cu:55-192).
hipError_t launch_pyr_down_f32(const float* src, int sw, int sh, float* dst, int dw, int dh, hipStream_t s);

hipError_t launch_remap_u8(const uint8_t* src, int sw, int sh, int64_t spitch, int cn, const float* map1,
                           const float* map2, int mw, int mh, int64_t mpitch, float scale_x, float scale_y,
                           uint8_t* dst, int64_t dpitch, hipStream_t s);

// morph_controlpoints' warps (template_morph.cpp:207-231): pixel i of the w x h ROI takes the
// cv::warpAffine (INTER_LINEAR, BORDER_CONSTANT 0) of map1 / map2 / mask by triangle owner[i]'s
// matrix M[6 owner[i] ..] (already inverted as warpAffine inverts it), or is copied (owner < 0).
hipError_t launch_morph_warp(const float* map1, const float* map2, const uint8_t* mask, int w, int h,
                             const int16_t* owner, const double* M, float* out1, float* out2, uint8_t* out_mask,
                             hipStream_t s);

// cv::resize INTER_LINEAR, u8, one channel, with the CPU path's fixed-point rule
// (imgwarp.cpp:1391-1500): per output column the source column and 11-bit weights, per output row
// the two clipped source rows and weights — tables built on the host (seams.cpp), so the kernel
// does integer arithmetic only.  area2: exact 1/2 downscale, (a + b + c + d + 2) >> 2 (:2349-2400).
struct ResizeTables {
    const int32_t* xofs;  // dw
    const int16_t* ax;    // 2 * dw
    const int32_t* rows;  // 2 * dh
    const int16_t* by;    // 2 * dh
    int32_t xmax;
    int32_t area2;
};
hipError_t launch_resize_u8(const uint8_t* src, int sw, int sh, int64_t spitch, uint8_t* dst, int dw, int dh,
                            int64_t dpitch, const ResizeTables& t, hipStream_t s);

// Scaled output (mapper.cpp:290-306): cuda::resize INTER_LINEAR of the RGB(A) result (sw x sh,
// pitch spitch bytes, 4 bytes per pixel) to dw x dh (even), then RGB -> YUV420P into `out`.
hipError_t launch_resize_rgba_yuv420(const uint8_t* rgba, int sw, int sh, int64_t spitch, uint8_t* out, int dw, int dh,
                                     int64_t out_pitch, hipStream_t s, int out_nv12 = 0);

// Preview output (mapper.cpp:308-312): cuda::resize INTER_LINEAR of the RGB(A) result to a dw x dh
// CV_8UC3 image (3 bytes per pixel, pitch out_pitch).
hipError_t launch_resize_rgba_rgb(const uint8_t* rgba, int sw, int sh, int64_t spitch, uint8_t* out, int dw, int dh,
                                  int64_t out_pitch, hipStream_t s);

// ---- overlays after a blend (overlay.hip) -------------------------------------------------------
// A multi-band / feather mapper copies its overlays onto the RGBA result frame after the blend:
// result(roi_k)[mask_k != 0] = warped_k for k = 0 .. K - 1 (mapper.cpp:279-287 with the missing RGBA2RGB
// restored).  The winner among the overlays is resolved once per rig (composite_lut_kernel over the
// overlay templates), and only the 8-pixel groups (8 g <= x < 8 g + 8 of one row) that hold a covered pixel
// are kept, in row-major order: per group its position and 8 entries.  A covered pixel carries
// kCodeCovered — also where the entry is invalid (a texture-convention coordinate outside the plane), which
// is written black like any other covered pixel; entries without it are neither read nor written.
constexpr uint32_t kCodeCovered = 1u << 29;
constexpr int kOvGroupPx = 8;
constexpr int kOvBlockGroups = 256 / kOvGroupPx;  // groups of one workgroup (8 per wave)
struct OverlayList {
    const uint32_t* groups;         // x / 8 | y << 16
    const CompositeEntry* entries;  // kOvGroupPx per group; camera = the overlay's frame index N + k
    int n_groups;                   // a multiple of kOvBlockGroups (padded with uncovered groups at (0, 0))
};
// rgba: the W x H result frame, 4 bytes per pixel; every covered pixel lies inside it (overlay_list.cpp)
hipError_t launch_overlay_apply(const FrameSet& frames, const OverlayList& list, uint8_t* rgba, int64_t rgba_pitch,
                                hipStream_t s, int pix = 0);

// ---- gathered preview of a blend-0 mapper (preview.hip) -----------------------------------------
// At blend 0 a result pixel is a function of one camera's four taps and that camera's gain, so the preview
// (cuda::resize INTER_LINEAR of the result, mapper.cpp:308-312) needs no result frame: per preview pixel
// the composite's 8-byte entries of the four result pixels the resize reads, (y1, x1), (y1, x2r), (y2r, x1),
// (y2r, x2r), built once per preview size (preview_list.hpp), entry 4 pixel + tap in raster order.  An
// entry with the valid bit clear (a result pixel no camera claims, the padding) evaluates to black.
constexpr int kPvBlockEntries = 256;  // entries of one workgroup: 64 preview pixels, one tap per lane
struct PreviewList {
    const CompositeEntry* entries;
    uint32_t n_entries;  // a multiple of kPvBlockEntries (padded with zero entries)
    uint32_t n_pixels;   // dw * dh; 4 n_pixels <= n_entries
    int32_t dw, dh;      // the preview size the list was built for
    float fx, fy;        // resize_rgba_rgb_kernel's scales, (float)(1.0 / ((double)dw / W)) and the same for y
};
// out: the dw x dh CV_8UC3 preview, 3 bytes per pixel at out_pitch; gains: a frame slot's kMaxCams doubles.
// pix: kPixInNv12 (the preview stays RGB)
hipError_t launch_preview_gather(const FrameSet& frames, const PreviewList& list, const double* gains, int use_gain,
                                 uint8_t* out, int64_t out_pitch, hipStream_t s, int pix = 0);

// ---- the RGB result as a planar tensor (tensor_out.hip) -----------------------------------------
// octvr_mapper_stitch_tensor: the bytes P of a w x h preview (above) as three planes of u8, f16 or f32.
// Element (plane, y, x) is at dev + plane * plane_stride + y * row_stride + x elements and holds colour
// c = bgr ? 2 - plane : plane of pixel (x, y): P for u8, (float)P * scale[c] + bias[c] (a multiply, then an
// add) for f32, that value rounded to nearest even for f16.  Offsets are 64-bit; the host checks the strides.
constexpr int kTensorU8 = 0, kTensorF16 = 1, kTensorF32 = 2;  // OCTVR_TENSOR_*
struct TensorPlanes {
    void* dev;
    int64_t row_stride, plane_stride;  // elements
    int32_t w, h;
    int32_t dtype, bgr;
    float scale[3], bias[3];  // per colour R, G, B
};
// From the RGBA result frame (sw x sh, 4 bytes per pixel at spitch): resize_rgba_rgb_kernel's arithmetic.
hipError_t launch_tensor_resize(const uint8_t* rgba, int sw, int sh, int64_t spitch, const TensorPlanes& t, hipStream_t s);
// From the source frames through the prepared tap list (t.w x t.h = list.dw x list.dh): preview_gather_kernel's
// arithmetic.  gains: a frame slot's kMaxCams doubles.  pix: kPixInNv12.
hipError_t launch_tensor_gather(const FrameSet& frames, const PreviewList& list, const double* gains, int use_gain,
                                const TensorPlanes& t, hipStream_t s, int pix = 0);

hipError_t launch_selftest_sat(const float* in, uint8_t* out, int n, int method, hipStream_t s);

}  // namespace octvr
