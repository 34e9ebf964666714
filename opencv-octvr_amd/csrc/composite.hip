// composite.hip — the gfx950 per-frame composite: the tiled kernel's device body and its three
// __global__ wrappers, the wide-tile kernel, the launch ladder that picks an instance, the public
// launchers (launch_stitch, launch_stitch_batch, launch_mb_remap) and, because it shares the
// composite's output stores, the scaled-output resize.
//
// Built with -ffp-contract=off: every f32/f64 expression rounds exactly as written, matching the
// reference's non-FMA x86 arithmetic (the oracle, oracle/octvr_oracle.c, is compiled the same way).
// No MFMA anywhere: this is a gather + per-pixel fixed-point blend.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "device_common.hpp"
#include "kernels.hpp"

namespace octvr {

// ---------------------------------------------------------------------------------------------
// Per-frame stitch, blend = 0 (mapper.cpp:219-306 with the copy chain resolved into the tiled LUT):
// for every 2x2 output quad the winning camera of each pixel is sampled (15-bit bilinear on the
// RGBA the source converts to), gain-scaled (mul_scalar_with_mask, exposure_compensate.cu:15-30:
// saturate_cast<uchar>(px * (float)g)) and written as YUV420P (the library's own BT.601 in place of
// NPP RGBToYUV420, same sequence as oracle rgb_quad_to_yuv).
// One workgroup per 128x8 tile; staged tiles read every tap from LDS (see kernels.hpp).  Tiles are
// walked grid-stride; blocks b, b+8, ... (one XCD under round-robin dispatch) take a contiguous
// band of tiles so their source boxes share that XCD's L2.
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(TileSlot) == 16, "TileSlot layout");

// The per-call FrameBatch is the FIRST argument of the stitch kernels: index it in the kernarg
// segment directly (a wave-uniform index gives scalar loads; indexing the by-value parameter would
// copy it to scratch).  idx = (frame << cam_log2) + camera (kernels.hpp FrameBatch).
static_assert(offsetof(FrameBatch<1>, src) == 0 && offsetof(FrameBatch<4>, src) == 0, "FrameBatch layout");
__device__ __forceinline__ SourceFrame kernarg_frame(uint32_t idx) {
    const kSourceFrame* kf = (const kSourceFrame*)__builtin_amdgcn_kernarg_segment_ptr();
    SourceFrame s;
    s.yuv = kf[idx].yuv;
    s.w = kf[idx].w;
    s.h = kf[idx].h;
    s.pitch = kf[idx].pitch;
    s.vig = kf[idx].vig;
    return s;
}
template <int NF>
__device__ __forceinline__ uint8_t* kernarg_out(uint32_t f) {
    typedef __attribute__((address_space(4))) const FrameBatch<NF> kFrameBatch;
    return ((const kFrameBatch*)__builtin_amdgcn_kernarg_segment_ptr())->out[f];
}
template <int NF>
__device__ __forceinline__ const double* kernarg_gains(uint32_t f) {
    typedef __attribute__((address_space(4))) const FrameBatch<NF> kFrameBatch;
    return ((const kFrameBatch*)__builtin_amdgcn_kernarg_segment_ptr())->gains[f];
}

// One 8-pixel staging group of a tile: the YUV bytes it needs and its LDS destination.
struct StageGroup {
    uint32_t y0, y1;  // 8 Y bytes
    uint32_t uq, vq;  // 4 U bytes, 4 V bytes
    int32_t dst;      // dword index of the group's first RGBA pixel; -1 = none
    uint32_t flags;   // kStageBlack: box group outside the image; kStageNoVig: camera without vignette
    float4 g0, g1;    // VIG: vignette gains of the 8 pixels
};
// The loaded bytes are only touched in stage_store (an iteration later): a select on them right
// after the load would make the compiler wait for the load in the iteration that issues it.
constexpr uint32_t kStageBlack = 1u, kStageNoVig = 2u;
// kStageNv12 (IN = kInRuntime only): uq / vq hold the group's 8 interleaved chroma bytes (U,V pairs 0-1, 2-3)
constexpr uint32_t kStageNv12 = 4u;
// The input layout of a staging instance: known at compile time (the planar instances and the hot NV12 ones),
// or the launch's (`pix`, wave-uniform: the instances of the colder mapper kinds)
constexpr int kInPlanar = 0, kInNv12 = 1, kInRuntime = 2;

// Metadata of a staged item as the waves hold it: one 16-byte load by 5 lanes (lane 0 the TileHdr,
// lane 1 + q slot q's TileSlot), decoded with v_readlane on demand (a uniform lane index), so the
// slot descriptors never occupy scalar registers.
// Slot q, component j of lane 1 + q: 0 = cam | bw << 16, 1 = bh | lds << 16, 2 = bx0 | by0 << 16,
// 3 = chunk0.
struct TileMeta {
    int t;         // the work unit: item t >> nf_log2, frame t & (nf - 1) (FrameBatch)
    uint4 v;
    uint32_t tile, nslots, stride;
    uint32_t map;  // slot of staging chunk c < 4 in bits 2c, 2c + 1 (TiledLutDev::upload)
    uint32_t frame, fbase;  // the unit's frame and its first camera's FrameBatch index (frame << cam_log2)
};

// dword j (0-3) of slot q (wave-uniform)
__device__ __forceinline__ uint32_t slot_word(const TileMeta& m, int q, int j) {
    const uint32_t c = j == 0 ? m.v.x : j == 1 ? m.v.y : j == 2 ? m.v.z : m.v.w;
    return (uint32_t)__builtin_amdgcn_readlane((int)c, 1 + q);
}

// The slot of staging chunk c (wave-uniform) and the frame it reads, resolved with scalar work and
// scalar kernarg loads; done one phase before the vector loads that use it, so their latency hides.
struct StageSlot {
    uint32_t live;             // c is a chunk of a live item
    uint32_t cam, bw, bh, lds, bx0, by0, chunk0;
    SourceFrame f;
};

// FIRST: c < 4 (a wave's first chunk), whose slot the host stored in m.map; else searched.
template <bool FIRST = false>
__device__ __forceinline__ StageSlot stage_slot(const TileMeta& m, int t_end, int c) {
    StageSlot s;
    const uint32_t nchunks = m.t < t_end ? ((m.nslots >> 8) & 0xFFu) : 0u;
    s.live = (uint32_t)c < nchunks ? 1u : 0u;
    int q = 0;
    if constexpr (FIRST) {
        q = (int)((m.map >> (2 * c)) & 3u);
    } else {
        const int nslots = (int)(m.nslots & 0xFFu);
#pragma unroll
        for (int j = 1; j < kTileSlots; j++) q += (j < nslots && c >= (int)(slot_word(m, j, 3) & 0xFFFFu)) ? 1 : 0;
    }
    const uint32_t d0 = slot_word(m, q, 0), d1 = slot_word(m, q, 1);
    const uint32_t d2 = slot_word(m, q, 2), d3 = slot_word(m, q, 3);
    s.cam = s.live ? (d0 & 31u) : 0u;
    s.bw = d0 >> 16;
    s.bh = d1 & 0xFFFFu;
    s.lds = d1 >> 16;
    s.bx0 = d2 & 0xFFFFu;
    s.by0 = d2 >> 16;
    s.chunk0 = d3 & 0xFFFFu;
    s.f = kernarg_frame(m.fbase + s.cam);
    return s;
}

// Loads of one staging group of 8 luma pixels of a slot: g is the lane's u16 group (kernels.hpp: valid,
// column and row in the slot's box, from the item's group table), so a chunk of 64 lanes covers only the
// box rows' tap spans.  Invalid groups (a slot's last chunk, chunks past the item's) read the box origin
// and are marked dst = -1.  With box columns 8-aligned, the Y load is 8-byte and the U / V loads 4-byte
// aligned (DWORD_STAGE).  Offsets use 24-bit multiplies: rows < 256, pitch < 2^24 (checked on the host).
// NV12 frames (IN, nv12): the group's 4 U,V pairs are the 8 bytes at the group's own column of the chroma row
// (8-byte aligned where the Y load is): ONE 8-byte load, its low dword in uq (pairs 0, 1), its high in vq.
template <bool DWORD_STAGE, bool VIG, int IN = kInPlanar>
__device__ __forceinline__ void stage_load(const StageSlot& s, uint32_t stride, uint32_t g, StageGroup& sg,
                                           bool nv12 = false) {
    const bool ok = s.live && (g & kGroupValid) != 0u;
    const uint32_t row_k = ok ? (g & 255u) : 0u, col_k = ok ? (g >> 8) & 31u : 0u;
    const SourceFrame& f = s.f;
    // box groups past the image's right / bottom edge (w % 8 == 0: whole groups) stage RGBA 0:
    // they load from the box origin and are replaced by Y = 0, U = V = 128 (-> R = G = B = 0)
    const bool img = s.bx0 + col_k * 8u < (uint32_t)f.w && s.by0 + row_k < (uint32_t)f.h;
    const uint32_t row = img ? row_k : 0u, col = img ? col_k : 0u;
    const uint32_t p32 = (uint32_t)f.pitch;
    const gu8* base = (const gu8*)f.yuv;
    const gu8* Yb = base + (int64_t)s.by0 * f.pitch + s.bx0;  // by0, bx0 even: chroma rows / columns exact
    const gu8* Ub = base + (int64_t)(f.h + (int)(s.by0 >> 1)) * f.pitch + (s.bx0 >> 1);
    const gu8* Vb = Ub + (f.w >> 1);
    const uint32_t oy = __umul24(row, p32) + col * 8u, oc = __umul24(row >> 1, p32) + col * 4u;
    if (IN == kInNv12 || (IN == kInRuntime && nv12)) {
        const gu8* Cp = base + (int64_t)(f.h + (int)(s.by0 >> 1)) * f.pitch + s.bx0 + (oc + col * 4u);
        if (DWORD_STAGE) {
            const uint64_t yy = *(const gu64*)(Yb + oy);
            const uint64_t cc = *(const gu64*)Cp;
            sg.y0 = (uint32_t)yy;
            sg.y1 = (uint32_t)(yy >> 32);
            sg.uq = (uint32_t)cc;
            sg.vq = (uint32_t)(cc >> 32);
        } else {
            const gu8* Yp = Yb + oy;
            sg.y0 = (uint32_t)Yp[0] | ((uint32_t)Yp[1] << 8) | ((uint32_t)Yp[2] << 16) | ((uint32_t)Yp[3] << 24);
            sg.y1 = (uint32_t)Yp[4] | ((uint32_t)Yp[5] << 8) | ((uint32_t)Yp[6] << 16) | ((uint32_t)Yp[7] << 24);
            sg.uq = (uint32_t)Cp[0] | ((uint32_t)Cp[1] << 8) | ((uint32_t)Cp[2] << 16) | ((uint32_t)Cp[3] << 24);
            sg.vq = (uint32_t)Cp[4] | ((uint32_t)Cp[5] << 8) | ((uint32_t)Cp[6] << 16) | ((uint32_t)Cp[7] << 24);
        }
    } else if (DWORD_STAGE) {
        const uint64_t yy = *(const gu64*)(Yb + oy);
        sg.y0 = (uint32_t)yy;
        sg.y1 = (uint32_t)(yy >> 32);
        sg.uq = *(const gu32*)(Ub + oc);
        sg.vq = *(const gu32*)(Vb + oc);
    } else {
        const gu8* Yp = Yb + oy;
        const gu8* Up = Ub + oc;
        const gu8* Vp = Vb + oc;
        sg.y0 = (uint32_t)Yp[0] | ((uint32_t)Yp[1] << 8) | ((uint32_t)Yp[2] << 16) | ((uint32_t)Yp[3] << 24);
        sg.y1 = (uint32_t)Yp[4] | ((uint32_t)Yp[5] << 8) | ((uint32_t)Yp[6] << 16) | ((uint32_t)Yp[7] << 24);
        sg.uq = (uint32_t)Up[0] | ((uint32_t)Up[1] << 8) | ((uint32_t)Up[2] << 16) | ((uint32_t)Up[3] << 24);
        sg.vq = (uint32_t)Vp[0] | ((uint32_t)Vp[1] << 8) | ((uint32_t)Vp[2] << 16) | ((uint32_t)Vp[3] << 24);
    }
    sg.flags = img ? 0u : kStageBlack;
    if (IN == kInRuntime && nv12) sg.flags |= kStageNv12;
    sg.dst = ok ? (int32_t)(s.lds + __umul24(row_k, stride) + col_k * 8u) : -1;
    if (VIG) {  // 8 gains (32-byte aligned: w % 8 == 0); a camera without vignette uses 1.0 gains
        const float* gv = f.vig ? f.vig + (int64_t)(s.by0 + row) * f.w + s.bx0 + col * 8u
                                : reinterpret_cast<const float*>(f.yuv);  // any readable 32 B, unused
        sg.g0 = *reinterpret_cast<const float4*>(gv);
        sg.g1 = *reinterpret_cast<const float4*>(gv + 4);
        if (!f.vig) sg.flags |= kStageNoVig;
    }
}

// The lane's group of an item's chunk c < kGroupFirst (c = the wave: each wave's first chunk), addressed
// by the item index alone (loop-invariant voffset, scalar soffset), so it is loaded one iteration ahead
// with the item's metadata.  Carried across the loop as the u16 the load returns: as a u32 the compiler
// zero-extended it right after the load, into the loop-carried register, and that copy waited on every
// load of the iteration (vmcnt(0) before the compute); widened at the use, an iteration later, it waits
// on nothing (one frame in flight: C2 composite -1 %, C3 +1 %, `u16`).
__device__ __forceinline__ uint16_t group_issue(const __amdgpu_buffer_rsrc_t& gr, int t, int t_end, int lg) {
    const int tt = (t < t_end ? t : 0) >> lg;
    return __builtin_amdgcn_raw_buffer_load_b16(gr, (uint32_t)threadIdx.x * 2u,
                                                (uint32_t)uniform(tt) * (uint32_t)(kGroupFirst * 64 * 2), 0);
}

template <bool VIG, int IN = kInPlanar>
__device__ __forceinline__ void stage_store(const StageGroup& sg, uint32_t* s_rgb) {
    if (sg.dst < 0) return;
    const bool black = (sg.flags & kStageBlack) != 0;  // Y = 0, U = V = 128 -> RGBA 0
    const uint32_t y0 = black ? 0u : sg.y0, y1 = black ? 0u : sg.y1;
    // chroma bytes xor 0x80 read as signed bytes are u - 128: one v_cvt_f32_i32_sdwa (sext) each
    uint32_t uq = black ? 0u : sg.uq ^ 0x80808080u, vq = black ? 0u : sg.vq ^ 0x80808080u;
    auto ch = [](uint32_t w, int k) { return (float)(signed char)((w >> (8 * k)) & 255u); };
    uint4 a, b;
    if constexpr (IN == kInNv12) {  // uq = U0 V0 U1 V1, vq = U2 V2 U3 V3
        yuv2_to_rgba_c(y0 & 255u, (y0 >> 8) & 255u, ch(uq, 0), ch(uq, 1), a.x, a.y);
        yuv2_to_rgba_c((y0 >> 16) & 255u, y0 >> 24, ch(uq, 2), ch(uq, 3), a.z, a.w);
        yuv2_to_rgba_c(y1 & 255u, (y1 >> 8) & 255u, ch(vq, 0), ch(vq, 1), b.x, b.y);
        yuv2_to_rgba_c((y1 >> 16) & 255u, y1 >> 24, ch(vq, 2), ch(vq, 3), b.z, b.w);
    } else {
        if (IN == kInRuntime && (sg.flags & kStageNv12)) {  // de-interleave: two v_perm_b32
            const uint32_t lo = uq, hi = vq;
            uq = __builtin_amdgcn_perm(hi, lo, 0x06040200u);
            vq = __builtin_amdgcn_perm(hi, lo, 0x07050301u);
        }
        yuv2_to_rgba_c(y0 & 255u, (y0 >> 8) & 255u, ch(uq, 0), ch(vq, 0), a.x, a.y);
        yuv2_to_rgba_c((y0 >> 16) & 255u, y0 >> 24, ch(uq, 1), ch(vq, 1), a.z, a.w);
        yuv2_to_rgba_c(y1 & 255u, (y1 >> 8) & 255u, ch(uq, 2), ch(vq, 2), b.x, b.y);
        yuv2_to_rgba_c((y1 >> 16) & 255u, y1 >> 24, ch(uq, 3), ch(vq, 3), b.z, b.w);
    }
    if (VIG && !(sg.flags & kStageNoVig)) {
        a.x = vig_mul(a.x, sg.g0.x);
        a.y = vig_mul(a.y, sg.g0.y);
        a.z = vig_mul(a.z, sg.g0.z);
        a.w = vig_mul(a.w, sg.g0.w);
        b.x = vig_mul(b.x, sg.g1.x);
        b.y = vig_mul(b.y, sg.g1.y);
        b.z = vig_mul(b.z, sg.g1.z);
        b.w = vig_mul(b.w, sg.g1.w);
    }
    *reinterpret_cast<uint4*>(s_rgb + sg.dst) = a;
    *reinterpret_cast<uint4*>(s_rgb + sg.dst + 4) = b;
}

// Residency and register budget of the composite: 6 workgroups per CU (the grid is one resident wave
// of them), compiled with the registers of 7 (72 VGPRs, 96 SGPRs; residency of 256-thread workgroups is
// also capped by scalar registers, min(8, 800 / (sgpr16 + 16)), MI355X_MICROARCH.md, Residency), so each
// SIMD keeps 80 VGPRs / 96 SGPRs and a wave slot for one wave of the lean gain feed beside 6 composite
// waves: the next frame's feed runs under this frame's composite (frames in flight).  Set explicitly:
// with the weight table the compiler's LDS occupancy model (24 KiB per workgroup) would otherwise relax
// the budget to 5 waves' 102 VGPRs.
constexpr int kStitchBlocksPerCU = 6;
constexpr int kStitchRegBlocks = kStitchBlocksPerCU + 1;
constexpr int kStitchSgprs = 96, kStitchVgprs = 72;
// The texture-convention instance (its f32 filter holds ~20 more values per pixel): the registers of 5
// workgroups per CU instead of spilling at 72 (the composite's time does not depend on 4, 5 or 6
// workgroups per CU, §4 Round 5)
constexpr int kStitchTexRegBlocks = 5, kStitchTexVgprs = 96;

// Software pipeline over a workgroup's items (t, then the items it claims):
//   iteration of item t:  stage item t's YUV (loaded during the previous iteration) into LDS,
//                         read the next item's metadata (loaded one iteration earlier),
//                         store the previous item's output, issue the next item's entries + YUV loads and
//                         the metadata load of the item after it,
//                         then compute item t from LDS while all of those are in flight.
// No global load is waited on in the iteration that issues it, and every iteration issues the
// same vector-memory operations in the same order (clamped addresses instead of branches), so the
// compiler's wait counts stay exact across the loop.
//
// One buffer load by lanes 0..kMetaWords-1: the voffset (lane * 16) is loop-invariant, the item's
// record offset a scalar, so no per-lane 64-bit address is held across the loop.
__device__ __forceinline__ uint4 meta_issue(const __amdgpu_buffer_rsrc_t& mr, int t, int t_end, int lg) {  // t: unit
    const int lane = threadIdx.x & 63;
    const int tt = (t < t_end ? t : 0) >> lg;  // t >= 0: every item index derives from bounded claims
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    uint4 v;
    if (lane < kMetaWords) {  // exec-masked: the instruction (and its vmcnt) is the same for every wave
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(mr, (uint32_t)lane * 16u,
                                                              (uint32_t)uniform(tt) * (uint32_t)(kMetaWords * 16), 0);
        v = uint4{r.x, r.y, r.z, r.w};
    }
    return v;
}

__device__ __forceinline__ TileMeta meta_read(const uint4& v, int t, int lg, int cam_lg) {
    TileMeta m;
    m.t = t;
    m.frame = (uint32_t)t & ((1u << lg) - 1u);
    m.fbase = m.frame << cam_lg;
    m.v = v;
    m.tile = (uint32_t)__builtin_amdgcn_readlane((int)v.x, 0);
    m.nslots = (uint32_t)__builtin_amdgcn_readlane((int)v.y, 0);
    m.stride = (uint32_t)__builtin_amdgcn_readlane((int)v.w, 0);
    m.map = (uint32_t)__builtin_amdgcn_readlane((int)v.z, 0);
    return m;
}

// An item's in-flight loads: its entries (one uint4 = one quad per lane and half) and the staging
// group of the wave's first chunk.
struct TileData {
    uint4 e4[kItemHalves];
    StageGroup sg;
};

// Issue an item's entry loads and the staging loads of its first chunk per wave (sl: the slot of
// chunk `wave`, from stage_slot<true>; g: the lane's group of that chunk, from group_issue).
// er: the entries as a buffer resource — voffset = lane * 16 (loop-invariant), soffset = the item's
// scalar byte offset, so no per-lane 64-bit address is formed per item (TiledLutDev::upload checks
// that the entries fit 32-bit offsets)
// E24: the lane's four 24-bit entries of each half (tiled_entry24) as three dwords (d.e4[h].w unused)
// EP: the instance of a LUT with quad-packed items (kItemPacked, wave-uniform per item).  Only the first 16 bytes
// per lane are loaded ahead: a packed item's records of both halves (d.e4[0].x, .y and .z, .w), or half 0's
// entries of an unpacked item, whose half 1 the compute phase loads itself (stitch_tiled_body) — 4 entry
// registers in flight instead of 8, and the same instruction for either form, so no vector-memory operation
// of the issue phase sits under the per-item branch
//
// entry_issue: the load of half h of item m's entries (16 bytes per lane at the item's scalar offset)
template <bool E24, bool EP>
__device__ __forceinline__ void entry_issue(const __amdgpu_buffer_rsrc_t& er, const TileMeta& m, int t_end, int lg, int h,
                                            TileData& d) {
    const bool live = m.t < t_end;
    const int tid = threadIdx.x;
    const uint32_t so =
        (uint32_t)uniform(((live ? m.t : 0) >> lg) * kItemHalves + h) * (uint32_t)(kTilePx * (E24 ? 3 : 4));
    if constexpr (E24) {
        typedef unsigned int u32x3e __attribute__((ext_vector_type(3)));
        const u32x3e v = __builtin_amdgcn_raw_buffer_load_b96(er, (uint32_t)tid * 12u, so, 0);
        d.e4[h] = uint4{v.x, v.y, v.z, 0u};
    } else {
        typedef unsigned int u32x4e __attribute__((ext_vector_type(4)));
        const u32x4e v = __builtin_amdgcn_raw_buffer_load_b128(er, (uint32_t)tid * 16u, so, 0);
        d.e4[h] = uint4{v.x, v.y, v.z, v.w};
    }
}

template <bool DWORD_STAGE, bool VIG, bool E24, int IN = kInPlanar, bool EP = false>
__device__ __forceinline__ void data_issue(const __amdgpu_buffer_rsrc_t& er, const TileMeta& m, int t_end, int lg,
                                           const StageSlot& sl, uint32_t g, TileData& d, bool nv12 = false) {
#pragma unroll
    for (int h = 0; h < (EP ? 1 : kItemHalves); h++) entry_issue<E24, EP>(er, m, t_end, lg, h, d);
    if (!sl.live) {  // wave-uniform: no loads for a chunk the item lacks
        d.sg.dst = -1;
        return;
    }
    stage_load<DWORD_STAGE, VIG, IN>(sl, m.stride & ((1u << kStrideBits) - 1u), g, d.sg, nv12);
}

// The composite's two sinks.  MODE 0: gain + RGB -> YUV420P into the output frame (blend = 0).
// MODE 1: gain-applied RGBA into the camera's level-0 pyramid image (blend > 0; the warped image
// Mapper::stitch hands to the blender, mapper.cpp:233-262); pixels outside the camera's aligned ROI
// are dropped.  Either way a quad's result is 4 dwords.
template <int MODE>
__device__ __forceinline__ QuadOut finish_any(const float (&rgb)[4][3], const f32x2_t (&gain)[4]) {
    if constexpr (MODE == 0) {
        return finish_quad2f(rgb, gain);
    } else {
        uint32_t px[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            uint32_t v = pack_u8(rgb[p][0] * gain[p].x, 0, 0u);
            v = pack_u8(rgb[p][1] * gain[p].x, 1, v);
            px[p] = pack_u8(rgb[p][2] * gain[p].x, 2, v);
        }
        return QuadOut{px[0], px[1], px[2], px[3]};
    }
}

struct RgbaSink {
    __amdgpu_buffer_rsrc_t rsrc;
    const MbCamLevel* cams;
};

// MODE 1: the deep tiles' result frame as an OutFrame from the level-0 grid origin (RgbaOut::res), in
// the registers MODE 0's output frame takes
__device__ __forceinline__ OutFrame make_result_frame(const RgbaOut& r) {
    OutFrame o;
    o.rsrc = __builtin_amdgcn_make_buffer_rsrc(r.res, 0, (int)r.res_bytes, 0x00020000);
    o.pitch = r.res_pitch;
    o.u_off = r.res_u_off;
    o.v_off = r.res_v_off;
    return o;
}

// A deep level-0 quad's final result straight from the remap (mb_blend level 0 for owned = 4: R = G0,
// convertTo(CV_8UC3) into result(align_result_roi) and RGB -> YUV420P, or the RGBA result image of a
// scaled output).  q holds the quad's four packed RGB pixels; (x, y): the quad on the level-0 grid.
template <int OUT = kOutPlanar>
__device__ __forceinline__ void store_result(const OutFrame& o, bool rgba, const QuadOut& q, int x, int y, bool in) {
    if (rgba) {
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        const uint32_t off = in ? (uint32_t)y * o.pitch + (uint32_t)x * 4u : kDropOffset;
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{q.y01, q.y23}, o.rsrc, off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{q.u, q.v}, o.rsrc, in ? off + o.pitch : kDropOffset, 0, 0);
        return;
    }
    const uint32_t px[4] = {q.y01, q.y23, q.u, q.v};
    store_quad<OUT>(o, quad_yuv(px), x, y, in);
}

__device__ __forceinline__ void store_rgba(const RgbaSink& o, const QuadOut& q, uint32_t cam, int x, int y, bool in) {
    // the camera descriptor through the constant address space: scalar loads.  (As a plain global
    // pointer the compiler cannot rule out the kernel's own stores aliasing it and emitted per-lane
    // loads, each followed by a vmcnt(0) that drained the next item's prefetches: 34 us of C3's 94 us
    // remap.)  cam is uniform (the item's camera).
    typedef __attribute__((address_space(4))) const MbCamLevel kMbCamLevel;
    const kMbCamLevel* c = (const kMbCamLevel*)o.cams + uniform((int)cam);
    const int ox = c->ox, oy = c->oy, cw = c->w, chh = c->h;
    const uint32_t goff = c->g_off, gp = c->g_pitch;
    const int xl = x - ox, yl = y - oy;
    const bool ok = in && xl >= 0 && yl >= 0 && xl < cw && yl < chh;  // w, h even: whole quads
    const uint32_t off = ok ? goff + (uint32_t)yl * gp + (uint32_t)xl * 4u : kDropOffset;
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 r0 = {q.y01, q.y23}, r1 = {q.u, q.v};
    __builtin_amdgcn_raw_buffer_store_b64(r0, o.rsrc, off, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b64(r1, o.rsrc, ok ? off + gp : kDropOffset, 0, 0);
}

// One half of an item: MODE 0 the YUV quad into `of`; MODE 1 the G0 quad where the item's flags say some
// pyrDown or blend reads the lane's sub-tile (item_g0_bit), and the final result into `of` (the result frame)
// where they say the sub-tile is deep (item_result_bit).  The lane's sub-tile: quarter (lane & 63) >> 4.
template <int MODE, int OUT = kOutPlanar>
__device__ __forceinline__ void store_half(const OutFrame& of, const RgbaSink& ro, bool res_rgba, const QuadOut& q,
                                           uint32_t cam, uint32_t flags, int h, int x, int y, bool in) {
    if constexpr (MODE == 0) {
        store_quad<OUT>(of, q, x, y, in);
    } else {
        const int q4 = (int)((threadIdx.x & 63u) >> 4);
        if (flags & item_g0_bit(h, q4)) store_rgba(ro, q, cam, x, y, in);
        if (flags & item_result_bit(h, q4)) store_result<OUT>(of, res_rgba, q, x, y, in);
    }
}

// The composite's static LDS, one variable (so its size, exactly 16 KiB, is where the dynamic region
// starts).  The weight table is the dynamic region (kWtabBytes at launch): kept out of the static size,
// the compiler's LDS occupancy model still allows 7 workgroups per CU and keeps the 7-wave register
// budget (72 VGPRs: the lean feed's wave fits beside 6 composite waves per SIMD); the table's base is
// then the constant 0x4000 (wtab_read).
struct alignas(16) StitchLds {
    uint32_t rgb[kTileLdsBytes / 4];  // the item's staged RGBA boxes (LDS address 0)
    uint32_t spare[kMaxCams];         // (the frames' camera gains live after the weight table)
    f32x2_t slot_gain[kTileSlots];
    uint32_t claim[2];
    uint32_t pad[2];
};
static_assert(sizeof(StitchLds) == 0x4000, "the weight table at LDS 0x4000 (wtab_read)");

// LDS byte address of a tiled entry's weight pairs: the table sits at 0x4000 (the kernel's static LDS
// is exactly 16 KiB: launch_composite checks the compiled size), so one v_and_or_b32 forms it; an
// address built from an integer, so the compiler does not split off a base it cannot fold into the offset.
__device__ __forceinline__ uint2 wtab_read(uint32_t e) {
    typedef __attribute__((address_space(3))) const uint64_t lds_u64;
    const uint64_t w = *(const lds_u64*)(uintptr_t)((e & 0x1FF8u) | 0x4000u);
    return uint2{(uint32_t)w, (uint32_t)(w >> 32)};
}

// LDS byte offset of a tiled entry's tap (x, y) (kernels.hpp, entry layout): one v_bfe_u32
__device__ __forceinline__ uint32_t tap_off(uint32_t e) { return (e >> 13) & 0x3FFFu; }

// Staged items.  The staged items are split into 8 contiguous bands, one per XCD under round-robin
// dispatch (blocks b, b+8, ...), so neighbouring items' source boxes share that XCD's L2.
// TEX: texture-convention entries (tiled_entry_tex): the taps as usual, the texture filter model instead of
// the weight table.
// LG: 1 << LG frames per launch (FrameBatch; MODE 0 only)
// PF: the pixel layouts.  kPfPlanar: "Y over [U|V]" in and out.  kPfNv12: NV12 in and out, compiled in (the hot
// instances: two 8-byte loads per staging group, one 16-bit chroma store per quad).  kPfRuntime: the launch's
// `pix` (kPixInNv12 | kPixOutNv12), wave-uniform branches: mixed layouts and the colder mapper kinds.
constexpr int kPfPlanar = 0, kPfNv12 = 3, kPfRuntime = 4;
// EP: the instance of a LUT with quad-packed items (TiledLut::n_packed > 0: the blend = 0 mapper's LUT of the default
// sampling, 32-bit entries; MODE 1 reads it for that mapper's scaled output and preview)
template <bool DWORD_STAGE, int MODE, bool VIG, bool TEX, int LG, bool E24, int PF = kPfPlanar, bool EP = false>
__device__ __forceinline__ void stitch_tiled_body(const FrameBatch<1 << LG>& frames, TiledLut lut, int W, int H, int use_gain,
                                                  int64_t out_pitch, RgbaOut rgba, int pix = 0) {
    constexpr int IN = PF == kPfRuntime ? kInRuntime : PF == kPfNv12 ? kInNv12 : kInPlanar;
    constexpr int OUT = PF == kPfRuntime ? kOutRuntime : PF == kPfNv12 ? kOutNv12 : kOutPlanar;
    const bool in_nv12 = IN == kInRuntime ? (pix & kPixInNv12) != 0 : IN == kInNv12;
    const bool out_nv12 = OUT == kOutRuntime ? (pix & kPixOutNv12) != 0 : OUT == kOutNv12;
    __shared__ StitchLds L;
    extern __shared__ __attribute__((aligned(16))) uint2 s_wtab[];  // 1,024 weight pairs at LDS 0x4000
    uint32_t* const s_rgb = L.rgb;
    // per frame and camera, (frame << cam_log2) + camera: in the dynamic region after the weight table
    float* const s_gain = reinterpret_cast<float*>(s_wtab + 1024);
    constexpr int lg = LG, cam_lg = LG <= 1 ? 5 : 4;  // frames per launch 1 << lg (FrameBatch)
    static_assert(!EP || (!TEX && !E24), "quad records: the blend = 0 mapper's 32-bit LUT of the default sampling only");
    static_assert(MODE == 0 || LG == 0, "frame batches: MODE 0 only");
    // {g, g} per slot (finish_quad2f).  Written after an item's first barrier and read after its
    // second; the next write comes after the next item's first barrier, i.e. after every wave's last
    // read, so one table suffices.
    f32x2_t* const s_slot_gain = L.slot_gain;
    // per iteration parity: written before an item's staging barrier, read after it (the next write
    // to the same entry is two items later, behind the next barrier)
    uint32_t* const s_claim = L.claim;
    constexpr int kItemH = kTileH * kItemHalves;

    const int groups = kStitchBands;
    const int g = blockIdx.x % groups;
    const int step = (gridDim.x - g + groups - 1) / groups;
    const int t_begin = lut.bands[g] << lg;  // work units: (item, frame) pairs
    const int t_end = lut.bands[g + 1] << lg;
    const __amdgpu_buffer_rsrc_t ersrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint32_t*>(lut.entries), 0,
        (int)((uint32_t)max(lut.n_items, 1) * (uint32_t)(kItemHalves * kTilePx * (E24 ? 3 : 4))), 0x00020000);
    const __amdgpu_buffer_rsrc_t mrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<TileHdr*>(lut.meta), 0, (int)((uint32_t)max(lut.n_items, 1) * (uint32_t)(kMetaWords * 16)), 0x00020000);
    const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t*>(lut.grp0), 0, (int)((uint32_t)max(lut.n_items, 1) * (uint32_t)(kGroupFirst * 64 * 2)), 0x00020000);
    const __amdgpu_buffer_rsrc_t g1rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(lut.grp1), 0, (int)(lut.n_grp1 * 2u), 0x00020000);
    OutFrame of{};
    RgbaSink ro{};
    bool res_rgba = false;
    const int out_bytes = (int)((uint32_t)out_pitch * (uint32_t)(H + H / 2));
    if constexpr (MODE == 0) {
        of = make_out_frame(kernarg_out<1 << LG>(0), W, H, out_pitch, out_nv12);
    } else {
        ro = RgbaSink{__builtin_amdgcn_make_buffer_rsrc(rgba.base, 0, (int)rgba.bytes, 0x00020000), rgba.cams};
        of = make_result_frame(rgba);
        res_rgba = rgba.res_rgba != 0;
    }
    const int tid = threadIdx.x;
    const int qx = tid & 63, qy = tid >> 6;

    if (tid < (1 << (lg + cam_lg))) {
        const double* gf = kernarg_gains<1 << LG>((uint32_t)tid >> cam_lg);
        s_gain[tid] = use_gain ? (float)gf[tid & ((1 << cam_lg) - 1)] : 1.0f;
    }
    if (tid < kTileZeroDwords) s_rgb[tid] = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) s_wtab[tid + 256 * k] = bilerp_weights((uint32_t)(tid + 256 * k));
    // Item sequence of this workgroup: its first three items are static (t0, t0 + step, t0 + 2 step,
    // i.e. the band's first 3 * step items dealt round-robin), every later one is claimed from the
    // band's work counter (one returning atomic per item, issued one iteration before the item's
    // metadata load and handed to the other waves through LDS), so workgroups that drew cheap items
    // keep pulling work while expensive ones finish (static dealing left the band's workgroups
    // finishing between 31 and 80 us on C2).
    const int t0 = t_begin + (int)(blockIdx.x / groups);
    const int dyn0 = t_begin + 3 * step;  // item of claim value 0
    uint32_t* const q = lut.queue + g * kQueueStride;
    const int wave = uniform(tid >> 6);
    TileMeta cur = meta_read(meta_issue(mrsrc, t0, t_end, lg), t0, lg, cam_lg);
    const uint32_t g0 = group_issue(grsrc, t0, t_end, lg);
    __syncthreads();
    TileData d;
    data_issue<DWORD_STAGE, VIG, E24, IN, EP>(ersrc, cur, t_end, lg, stage_slot<true>(cur, t_end, wave), g0, d, in_nv12);
    int t_mv = t0 + step < t_end ? t0 + step : t_end;  // item of the metadata in flight (mv)
    int t_n2 = t_mv < t_end && t0 + 2 * step < t_end ? t0 + 2 * step : t_end;  // item after it
    uint4 mv = meta_issue(mrsrc, t_mv, t_end, lg);
    uint16_t mg = group_issue(grsrc, t_mv, t_end, lg);  // the lane's first staging group of item t_mv
    uint32_t claim = 0u;  // lane 0 of wave 0: returned value of the claim in flight
    bool claimed = false; // a claim for the item after t_n2 is in flight (uniform)
    bool first = true;
    // opaque copies of the prologue loads: the loop-header phis then merge a load with a non-load,
    // so the compiler cannot fold them into one load at the header (waited on right there)
    asm volatile("" : "+v"(mv.x), "+v"(mv.y), "+v"(mv.z), "+v"(mv.w), "+v"(mg));
#pragma unroll
    for (int h = 0; h < (EP ? 1 : kItemHalves); h++) {
        asm volatile("" : "+v"(d.e4[h].x), "+v"(d.e4[h].y), "+v"(d.e4[h].z));
        if constexpr (!E24) asm volatile("" : "+v"(d.e4[h].w));
    }
    asm volatile("" : "+v"(d.sg.y0), "+v"(d.sg.y1), "+v"(d.sg.uq), "+v"(d.sg.vq));

    // the previous item's output, stored in the next iteration: every store is then older than the
    // loads it shares the iteration with (vmcnt waits on a load that is older than a store must drain
    // everything, as loads and stores complete out of order)
    QuadOut prev[kItemHalves];
#pragma unroll
    for (int h = 0; h < kItemHalves; h++) prev[h] = QuadOut{0u, 0u, 0u, 0u};
    int px = 0, py = 0;  // the previous item's quad of this lane in its first half
    // MODE 0 stores of items wholly inside the frame: the lane's part of the byte offsets is
    // loop-invariant (voffset), the item's part a scalar (soffset) — no per-lane address arithmetic
    // (NV12: the lane's U,V pair at chroma byte 2 qx)
    const uint32_t lane_y = (uint32_t)(2 * qy) * of.pitch + (uint32_t)(2 * qx),
                   lane_c = (uint32_t)qy * of.pitch + (uint32_t)(out_nv12 ? 2 * qx : qx);
    int pox = 0, poy = 0;  // the previous item's origin (uniform)
    bool pfull = false;    // the previous item lies wholly inside W x H (uniform)
    uint32_t pcam = 0, pfl = 0;  // the previous item's RGBA-mode camera and flags (item_result_bit / item_g0_bit)
    uint32_t pfr = 0;            // the previous unit's frame (MODE 0 output)
    bool pin = false;
    uint32_t par = 0;  // iteration parity
    while (cur.t < t_end) {
        const int x = (int)(cur.tile & 0xFFFFu) * kTileW + qx * 2, y = (int)(cur.tile >> 16) * kItemH + qy * 2;
        const uint32_t S = cur.stride & ((1u << kStrideBits) - 1u);
        uint4 e4[kItemHalves];
#pragma unroll
        for (int h = 0; h < (EP ? 1 : kItemHalves); h++) e4[h] = d.e4[h];
        // every wave has read the previous item's staging area
        __syncthreads();
        if (tid < kTileZeroDwords) s_rgb[tid] = 0u;  // black pixels read offset 0 of the region
        const TileMeta nxt = meta_read(mv, t_mv, lg, cam_lg);
        {  // slot q's camera word sits in lane 1 + q of the metadata's first component
            const uint32_t cw = (uint32_t)__shfl((int)cur.v.x, 1 + (tid & 3), 64);
            // clamped to [0, FLT_MAX] (NaN -> 0) in MODE 0; no result depends on it (finish_quad2f
            // saturates with v_cvt_pk_u8_f32, which maps negative and NaN products to 0 either way)
            const float gs = s_gain[cur.fbase + (cw & 31u)];
            const float gc = MODE == 0 ? __builtin_fminf(__builtin_fmaxf(gs, 0.f), FLT_MAX) : gs;
            if (tid < kTileSlots) s_slot_gain[tid] = f32x2_t{gc, gc};
        }
        if (claimed && tid == 0) s_claim[par] = claim;  // issued one iteration ago
        stage_store<VIG, IN>(d.sg, s_rgb);
        const uint32_t nch = (cur.nslots >> 8) & 0xFFu;
        if (nch > (uint32_t)kGroupFirst) {  // large items only: the other chunks now, groups from grp1
            const uint32_t ovf = cur.stride >> kStrideBits;
            for (int c = kGroupFirst + wave; c < (int)nch; c += 4) {
                const uint32_t gk = __builtin_amdgcn_raw_buffer_load_b16(
                    g1rsrc, (uint32_t)(tid & 63) * 2u, (ovf + (uint32_t)(c - kGroupFirst)) * 128u, 0);
                StageGroup sg;
                stage_load<DWORD_STAGE, VIG, IN>(stage_slot(cur, t_end, c), S, gk, sg, in_nv12);
                stage_store<VIG, IN>(sg, s_rgb);
            }
        }
        __syncthreads();
        // the item two ahead: static on the first iteration, else the claim handed over above.
        if (!first) {
            // Global addresses derive from this LDS-handed claim (the item's header, slots and entries,
            // and through its slots the camera frames), so it is range-checked as unsigned: a value that
            // is not a claim of this band (the r02 barrier-free ablation read s_claim before wave 0 wrote
            // it, i.e. uninitialised LDS -> negative item index -> out-of-range header and entry loads and
            // a null frame pointer, hipErrorIllegalAddress) ends the sequence instead.
            // (one scalar min: dyn0 + cv then cannot wrap negative, and t_n2 below stays in [0, t_end])
            const uint32_t cv = min((uint32_t)uniform((int)s_claim[par]), 0x3FFFFFFFu);
            const int v = claimed ? dyn0 + (int)cv : t_end;
            t_n2 = v < t_end ? v : t_end;
        }
        first = false;
        if (MODE == 0 && lg) of.rsrc = __builtin_amdgcn_make_buffer_rsrc(kernarg_out<1 << LG>(pfr), 0, out_bytes, 0x00020000);
        if (MODE == 0 && pfull) {
#pragma unroll
            for (int h = 0; h < kItemHalves; h++) {
                const uint32_t sy = (uint32_t)uniform((poy + h * kTileH) * (int)of.pitch + pox);
                const uint32_t sc =
                    (uint32_t)uniform(((poy + h * kTileH) >> 1) * (int)of.pitch + (out_nv12 ? pox : pox >> 1));
                __builtin_amdgcn_raw_buffer_store_b16((uint16_t)prev[h].y01, of.rsrc, lane_y, sy, kOutPolicy);
                __builtin_amdgcn_raw_buffer_store_b16((uint16_t)prev[h].y23, of.rsrc, lane_y, sy + of.pitch, kOutPolicy);
                if (out_nv12) {  // (a constant in the compiled-in instances, else wave-uniform)
                    __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(prev[h].u | prev[h].v << 8), of.rsrc, lane_c,
                                                          sc + of.u_off, kOutPolicy);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)prev[h].u, of.rsrc, lane_c, sc + of.u_off, kOutPolicy);
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)prev[h].v, of.rsrc, lane_c, sc + of.v_off, kOutPolicy);
                }
            }
        } else {
#pragma unroll
            for (int h = 0; h < kItemHalves; h++)
                store_half<MODE, OUT>(of, ro, res_rgba, prev[h], pcam, pfl, h, px, py + h * kTileH, pin && py + h * kTileH < H);
        }
        // the next item's first staging slot resolved only now (short scalar live ranges), then its loads
        data_issue<DWORD_STAGE, VIG, E24, IN, EP>(ersrc, nxt, t_end, lg, stage_slot<true>(nxt, t_end, wave), mg, d, in_nv12);
        mv = meta_issue(mrsrc, t_n2, t_end, lg);
        mg = group_issue(grsrc, t_n2, t_end, lg);
        t_mv = t_n2;
        claimed = t_n2 < t_end;  // claim the item after it (only while the sequence is live)
        if (claimed && tid == 0) {
            // an opaque (per-lane looking) address: the atomic optimizer would otherwise rewrite the
            // single-lane claim into a wave-level one whose result it broadcasts (and waits for) at once
            int zero = tid;
            asm volatile("" : "+v"(zero));
            claim = __hip_atomic_fetch_add(q + zero, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // one half of the item from LDS: the lane's quad of 4-byte entries, or (EP, kItemPacked) its quad record;
        // each form ends in its own finish, so that only the half's four result dwords outlive the branch
        auto half_entries = [&](int h) {
            // E24: the four 24-bit entries from the three dwords (two v_alignbit_b32, one shift)
            const uint32_t ent[4] = {e4[h].x, E24 ? __builtin_amdgcn_alignbit(e4[h].y, e4[h].x, 24u) : e4[h].y,
                                     E24 ? __builtin_amdgcn_alignbit(e4[h].z, e4[h].y, 16u) : e4[h].z,
                                     E24 ? e4[h].z >> 8 : e4[h].w};
            float rgb[4][3];
            f32x2_t gain[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const uint32_t e = ent[p];
                // taps (x, y), (x+1, y) and (x, y+1), (x+1, y+1): two ds_read2_b32, no per-tap masking
                const uint8_t* r0 = reinterpret_cast<const uint8_t*>(s_rgb) +
                                    (TEX ? (e >> 15) & 0x3FFCu : E24 ? (e >> 10) & 0x3FFCu : tap_off(e));
                const uint8_t* r1 = r0 + 4u * S;
                const uint32_t c00 = reinterpret_cast<const uint32_t*>(r0)[0];
                const uint32_t c01 = reinterpret_cast<const uint32_t*>(r0)[1];
                const uint32_t c10 = reinterpret_cast<const uint32_t*>(r1)[0];
                const uint32_t c11 = reinterpret_cast<const uint32_t*>(r1)[1];
                if constexpr (TEX) {
                    tex_bilerp_f(c00, c01, c10, c11, (e >> 1) & 255u, (e >> 9) & 255u, rgb[p]);
                    gain[p] = *reinterpret_cast<const f32x2_t*>(reinterpret_cast<const uint8_t*>(s_slot_gain) + ((e >> 30) << 3));
                } else {
                    // E24: fxy at bits 2-11, so e << 1 holds it where wtab_read masks (bits 3-12)
                    bilerp_rgba_w(c00, c01, c10, c11, wtab_read(E24 ? e << 1 : e), rgb[p]);
                    // slot << 3 = e >> 27 (bits 27-29 of a tiled entry are zero; kernels.hpp); E24: bits 0-1
                    const uint32_t go = E24 ? (e << 3) & 0x18u : e >> 27;
                    gain[p] = *reinterpret_cast<const f32x2_t*>(reinterpret_cast<const uint8_t*>(s_slot_gain) + go);
                }
                if (MODE == 1 && !E24 && (e & kEntryNoGain)) gain[p] = f32x2_t{1.0f, 1.0f};
            }
            prev[h] = finish_any<MODE>(rgb, gain);
        };
        auto half_records = [&](int h, uint32_t lo, uint32_t hi) {
            float rgb[4][3];
            f32x2_t gain[4];
            const uint32_t base4 = quad_base4(hi);
            const f32x2_t gq = *reinterpret_cast<const f32x2_t*>(reinterpret_cast<const uint8_t*>(s_slot_gain) + quad_gain_off(hi));
#pragma unroll
            for (int p = 0; p < 4; p++) {
                // base + 4 dx + 4 S dy: the pixel's two flag bits, one per 16-bit half, times {4, 4 S} scaled
                const uint32_t off = __builtin_amdgcn_udot2(
                    __builtin_bit_cast(u16x2_t, hi & quad_flag_mask(p)),
                    __builtin_bit_cast(u16x2_t, (uint32_t)uniform((int)quad_flag_mul(p, S))), base4, false);
                const uint8_t* r0 = reinterpret_cast<const uint8_t*>(s_rgb) + off;
                const uint8_t* r1 = r0 + 4u * S;
                const uint32_t c00 = reinterpret_cast<const uint32_t*>(r0)[0];
                const uint32_t c01 = reinterpret_cast<const uint32_t*>(r0)[1];
                const uint32_t c10 = reinterpret_cast<const uint32_t*>(r1)[0];
                const uint32_t c11 = reinterpret_cast<const uint32_t*>(r1)[1];
                bilerp_rgba_w(c00, c01, c10, c11, wtab_read(quad_fxy_view(p, lo, hi)), rgb[p]);
                gain[p] = gq;
            }
            prev[h] = finish_any<MODE>(rgb, gain);
        };
        bool records = false;
        if constexpr (EP) records = (cur.nslots & kItemPacked) != 0u;  // wave-uniform
        if (records) {
            half_records(0, e4[0].x, e4[0].y);
            half_records(1, e4[0].z, e4[0].w);
        } else {
            half_entries(0);
            if constexpr (EP) {  // an unpacked item among packed ones: its second half is loaded (and waited for) here
                TileData dd;
                entry_issue<E24, EP>(ersrc, cur, t_end, lg, 1, dd);
                e4[1] = dd.e4[1];
            }
            half_entries(1);
        }
        px = x;
        py = y;
        pox = (int)(cur.tile & 0xFFFFu) * kTileW;
        poy = (int)(cur.tile >> 16) * kItemH;
        pfull = pox + kTileW <= W && poy + kItemH <= H;
        pcam = (cur.nslots >> 16) & 31u;
        pfr = cur.frame;
        pfl = MODE == 1 ? (cur.map >> 8) & 0xFFFFu : 0u;
        pin = x < W && y < H;
        par ^= 1u;
        cur = nxt;
    }
    // the last workgroup to finish resets the work counters for the next launch (stream order makes
    // the reset visible to it); every claim of this workgroup has returned before its ticket
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        (void)claim;
        if (__hip_atomic_fetch_add(lut.queue + kStitchBands * kQueueStride, 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
            for (int k = 0; k <= kStitchBands; k++)
                __hip_atomic_exchange(lut.queue + k * kQueueStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (MODE == 0 && lg) of.rsrc = __builtin_amdgcn_make_buffer_rsrc(kernarg_out<1 << LG>(pfr), 0, out_bytes, 0x00020000);
#pragma unroll
    for (int h = 0; h < kItemHalves; h++)
        store_half<MODE, OUT>(of, ro, res_rgba, prev[h], pcam, pfl, h, px, py + h * kTileH, pin && py + h * kTileH < H);
}

// PF: kPfPlanar or kPfNv12 (compiled in)
template <bool DWORD_STAGE, int MODE, bool VIG, int LG, bool E24, int PF = kPfPlanar, bool EP = false>
__global__ void __launch_bounds__(256, kStitchRegBlocks) __attribute__((amdgpu_num_sgpr(kStitchSgprs)))
__attribute__((amdgpu_num_vgpr(kStitchVgprs))) stitch_tiled_kernel(FrameBatch<1 << LG> frames, TiledLut lut, int W, int H,
                                                                   int use_gain, int64_t out_pitch, RgbaOut rgba) {
    stitch_tiled_body<DWORD_STAGE, MODE, VIG, false, LG, E24, PF, EP>(frames, lut, W, H, use_gain, out_pitch, rgba);
}
// The instance of every other launch with an NV12 side: the layouts from `pix` (kPfRuntime), byte-wise staging
// (any alignment) and the vignette path (cameras without one stage with kStageNoVig), at the texture
// instance's register budget.  No conversion pass either: the same kernel reads and writes the layouts itself.
template <int MODE, bool TEX, int LG, bool E24, bool EP = false>
__global__ void __launch_bounds__(256, kStitchTexRegBlocks) __attribute__((amdgpu_num_sgpr(kStitchSgprs)))
__attribute__((amdgpu_num_vgpr(kStitchTexVgprs))) stitch_tiled_pix_kernel(FrameBatch<1 << LG> frames, TiledLut lut, int W,
                                                                          int H, int use_gain, int64_t out_pitch,
                                                                          RgbaOut rgba, int pix) {
    stitch_tiled_body<false, MODE, true, TEX, LG, E24, kPfRuntime, EP>(frames, lut, W, H, use_gain, out_pitch, rgba, pix);
}
template <bool DWORD_STAGE, int MODE, bool VIG, int LG>
__global__ void __launch_bounds__(256, kStitchTexRegBlocks) __attribute__((amdgpu_num_sgpr(kStitchSgprs)))
__attribute__((amdgpu_num_vgpr(kStitchTexVgprs))) stitch_tiled_tex_kernel(FrameBatch<1 << LG> frames, TiledLut lut, int W,
                                                                          int H, int use_gain, int64_t out_pitch,
                                                                          RgbaOut rgba) {
    stitch_tiled_body<DWORD_STAGE, MODE, VIG, true, LG, false>(frames, lut, W, H, use_gain, out_pitch, rgba);
}

// Wide tiles: one workgroup per tile, 8-byte absolute entries, direct global gathers.
template <int MODE>
__global__ void __launch_bounds__(256) stitch_wide_kernel(FrameSet frames, TiledLut lut, int W, int H,
                                                          const double* gains, int use_gain, uint8_t* out,
                                                          int64_t out_pitch, RgbaOut rgba, int pix) {
    __shared__ float s_gain[kMaxCams];
    const int tid = threadIdx.x;
    if (tid < kMaxCams) s_gain[tid] = use_gain ? (float)gains[tid] : 1.0f;
    __syncthreads();
    OutFrame of{};
    RgbaSink ro{};
    if constexpr (MODE == 0) {
        of = make_out_frame(out, W, H, out_pitch, (pix & kPixOutNv12) != 0);
    } else {
        ro = RgbaSink{__builtin_amdgcn_make_buffer_rsrc(rgba.base, 0, (int)rgba.bytes, 0x00020000), rgba.cams};
        of = make_result_frame(rgba);
    }
    const uint32_t tile = (uint32_t)uniform((int)lut.wide_tiles[blockIdx.x]);
    const int x = (int)(tile & 0xFFFFu) * kTileW + (tid & 63) * 2, y = (int)(tile >> 16) * kTileH + (tid >> 6) * 2;
    const uint4* wp = reinterpret_cast<const uint4*>(lut.wide + (int64_t)blockIdx.x * kTilePx) + tid * 2;
    const uint4 e0 = wp[0], e1 = wp[1];
    const uint32_t xy[4] = {e0.x, e0.z, e1.x, e1.z};
    const uint32_t cd[4] = {e0.y, e0.w, e1.y, e1.w};
    Taps tp[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        if (pix & kPixInNv12)  // uniform
            gather_taps<true>(frames, xy[p], cd[p], tp[p]);
        else
            gather_taps<false>(frames, xy[p], cd[p], tp[p]);
    }
    uint32_t rgb[4][3];
    f32x2_t gain[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        if (cd[p] & kCodeTex)  // texture-convention entries (make_entry_tex)
            tex_bilerp(tp[p].c[0], tp[p].c[1], tp[p].c[2], tp[p].c[3], tp[p].fx, tp[p].fy, rgb[p]);
        else
            bilerp_rgba(tp[p].c[0], tp[p].c[1], tp[p].c[2], tp[p].c[3], tp[p].fx, tp[p].fy, rgb[p]);
        float gp = (MODE == 1 && (cd[p] & kCodeNoGain)) ? 1.0f : s_gain[(cd[p] >> 10) & 31u];
        gain[p] = f32x2_t{gp, gp};
    }
    const uint32_t camb = MODE == 1 ? (uint32_t)uniform((int)lut.wide_cams[blockIdx.x]) : 0u;
    float rgbf[4][3];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) rgbf[p][ch] = (float)rgb[p][ch];
    // camera word: camera | the half's quarters' result bits << 8 | G0 bits << 12 (tiling.cpp), i.e. the
    // item flags of a half 0
    const uint32_t fl = ((camb >> 8) & 15u) | ((camb >> 12) & 15u) << 8;
    store_half<MODE, kOutRuntime>(of, ro, rgba.res_rgba != 0, finish_any<MODE>(rgbf, gain), camb & 31u, fl, 0, x, y,
                                  x < W && y < H);
}

// ---------------------------------------------------------------------------------------------
// Host side: the launch ladder from the runtime selectors to the one instance they name.
// ---------------------------------------------------------------------------------------------
// One tiled launch's runtime arguments: launch_composite fills it, every level below
// reads what it needs and passes it on.
struct TiledLaunch {
    int blocks;
    const FrameSet* frames;  // 1 << lg frame sets, with their gains and outputs (out: null for MODE 1)
    const double* const* gains;
    uint8_t* const* out;
    const TiledLut& lut;
    int W, H, use_gain;
    int64_t out_pitch;
    const RgbaOut& rgba;
    hipStream_t s;
    hipEvent_t ev0, ev1;  // timing events around the launch (both null: none)
    int pix;              // kPixInNv12 | kPixOutNv12
    bool dw, vig;         // every frame 8-byte aligned (dword staging); some camera has a vignette table
    int lg;               // log2 of the frames in the batch
};

// The kernel of an instance: the choice between the three __global__ wrappers, written once.
template <bool DW, int MODE, bool V, bool TEX, int LG, bool E24, int PF, bool EP>
constexpr auto tiled_kernel() {
    if constexpr (PF == kPfRuntime)
        return &stitch_tiled_pix_kernel<MODE, TEX, LG, E24, EP>;
    else if constexpr (TEX)
        return &stitch_tiled_tex_kernel<DW, MODE, V, LG>;
    else
        return &stitch_tiled_kernel<DW, MODE, V, LG, E24, PF, EP>;
}

// The weight table's address (wtab_read) assumes the dynamic LDS starts right after StitchLds: checked
// once per kernel instance against the compiled static LDS size.
static hipError_t stitch_lds_check(const void* kernel) {
    hipFuncAttributes a;
    const hipError_t e = hipFuncGetAttributes(&a, kernel);
    if (e != hipSuccess) return e;
    return a.sharedSizeBytes == sizeof(StitchLds) ? hipSuccess : hipErrorInvalidKernelFile;
}

// dynamic LDS of the composite: the weight table, then the frames' camera gains (FrameBatch order)
constexpr uint32_t kStitchDynLds = kWtabBytes + 4u * 2u * kMaxCams;

// the frame sets as the kernel's kernarg table for 1 << LG frames
template <int LG>
static void frame_batch(const FrameSet* frames, const double* const* gains, uint8_t* const* out,
                        FrameBatch<1 << LG>& fb) {
    constexpr int cam_lg = FrameBatch<1 << LG>::kCamLog2;
    memset(&fb, 0, sizeof fb);
    for (int f = 0; f < (1 << LG); f++) {
        for (int i = 0; i < (1 << cam_lg); i++) fb.src[(f << cam_lg) + i] = frames[f].f[i];
        fb.out[f] = out ? out[f] : nullptr;
        fb.gains[f] = gains[f];
    }
}

template <bool DW, int MODE, bool V, bool TEX, int LG, bool E24, int PF, bool EP>
static hipError_t launch_tiled(const TiledLaunch& a) {
    static_assert(PF != kPfNv12 || !TEX, "compiled-in NV12: the default sampling's instances");
    constexpr auto kernel = tiled_kernel<DW, MODE, V, TEX, LG, E24, PF, EP>();
    static const hipError_t lds_ok = stitch_lds_check(reinterpret_cast<const void*>(kernel));
    if (lds_ok != hipSuccess) return lds_ok;
    FrameBatch<1 << LG> fb;
    frame_batch<LG>(a.frames, a.gains, a.out, fb);
    const dim3 grid(a.blocks), block(256);
    if constexpr (PF == kPfRuntime) {
        if (a.ev0) (void)hipEventRecord(a.ev0, a.s);
        hipLaunchKernelGGL(kernel, grid, block, kStitchDynLds, a.s, fb, a.lut, a.W, a.H, a.use_gain, a.out_pitch, a.rgba,
                           a.pix);
        if (a.ev0) (void)hipEventRecord(a.ev1, a.s);
    } else if constexpr (TEX) {
        // (no packet-carried timing events: the texture convention is not a bench line's timed kernel)
        hipLaunchKernelGGL(kernel, grid, block, kStitchDynLds, a.s, fb, a.lut, a.W, a.H, a.use_gain, a.out_pitch, a.rgba);
        if (a.ev0) (void)hipEventRecord(a.ev1, a.s);
    } else if (a.ev0) {  // the timing events carried by the dispatch packet itself
        hipExtLaunchKernelGGL(kernel, grid, block, kStitchDynLds, a.s, a.ev0, a.ev1, 0, fb, a.lut, a.W, a.H, a.use_gain,
                              a.out_pitch, a.rgba);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, kStitchDynLds, a.s, fb, a.lut, a.W, a.H, a.use_gain, a.out_pitch, a.rgba);
    }
    return hipGetLastError();
}

// the batch's frame count: 1, 2 or 4 (blend 0), 1 (MODE 1)
template <bool DW, int MODE, bool V, bool TEX, bool E24, int PF = kPfPlanar, bool EP = false>
static hipError_t launch_tiled_lg(const TiledLaunch& a) {
    if constexpr (MODE == 0) {
        if (a.lg == 1) return launch_tiled<DW, MODE, V, TEX, 1, E24, PF, EP>(a);
        if (a.lg == 2) return launch_tiled<DW, MODE, V, TEX, 2, E24, PF, EP>(a);
    }
    if (a.lg != 0) return hipErrorInvalidValue;
    return launch_tiled<DW, MODE, V, TEX, 0, E24, PF, EP>(a);
}

// the instance for the frames' staging (dword loads, vignette) and the entries' convention
template <int MODE, bool TEX, bool E24, bool EP = false>
static hipError_t launch_tiled_vd(const TiledLaunch& a) {
    if (a.pix) {
        // NV12 in and out, default sampling, aligned frames without vignette, blend 0: the compiled-in instance;
        // every other launch with an NV12 side: the instance that takes the layouts from `pix`
        if constexpr (MODE == 0 && !TEX) {
            if (a.pix == (kPixInNv12 | kPixOutNv12) && a.dw && !a.vig)
                return launch_tiled_lg<true, MODE, false, TEX, E24, kPfNv12, EP>(a);
        }
        return launch_tiled_lg<false, MODE, true, TEX, E24, kPfRuntime, EP>(a);
    }
    if (a.dw && !a.vig) return launch_tiled_lg<true, MODE, false, TEX, E24, kPfPlanar, EP>(a);
    if (a.dw) return launch_tiled_lg<true, MODE, true, TEX, E24, kPfPlanar, EP>(a);
    if (!a.vig) return launch_tiled_lg<false, MODE, false, TEX, E24, kPfPlanar, EP>(a);
    return launch_tiled_lg<false, MODE, true, TEX, E24, kPfPlanar, EP>(a);
}

// the entries' width: 24-bit (TiledLut::e24, default sampling only) or 32-bit, the latter with quad-packed
// items (TiledLut::n_packed: the blend = 0 mapper's LUT) or without
template <int MODE, bool TEX>
static hipError_t launch_tiled_for(const TiledLaunch& a) {
    if (a.lut.n_packed > 0 && (TEX || a.lut.e24)) return hipErrorInvalidValue;
    if constexpr (!TEX) {
        if (a.lut.e24) return launch_tiled_vd<MODE, TEX, true>(a);
        if (a.lut.n_packed > 0) return launch_tiled_vd<MODE, TEX, false, true>(a);
    } else {
        if (a.lut.e24) return hipErrorInvalidValue;  // texture-convention entries are never packed
    }
    return launch_tiled_vd<MODE, TEX, false>(a);
}

// nf frame sets (1, 2 or 4) in one launch of the tiled kernel (FrameBatch); wide tiles one launch per frame
template <int MODE>
static hipError_t launch_composite(const FrameSet* frames, int nf, const TiledLut& lut, int W, int H,
                                   const double* const* gains, int use_gain, uint8_t* const* out, int64_t out_pitch,
                                   const RgbaOut& rgba, hipStream_t s, hipEvent_t ev0 = nullptr,
                                   hipEvent_t ev1 = nullptr, int pix = 0) {
    if (pix & ~(kPixInNv12 | kPixOutNv12)) return hipErrorInvalidValue;
    if (lut.n_items > 0 && lut.qpl != kItemHalves) return hipErrorInvalidValue;
    const int lg = nf == 1 ? 0 : nf == 2 ? 1 : nf == 4 ? 2 : -1;
    if (lg < 0 || (MODE == 1 && nf != 1)) return hipErrorInvalidValue;
    const int cam_lg = nf <= 2 ? 5 : 4;
    for (int f = 0; f < nf; f++)
        for (int i = 1 << cam_lg; i < kMaxCams; i++)
            if (frames[f].f[i].yuv) return hipErrorInvalidValue;  // more cameras than a 4-frame batch holds
    // timing events: carried by the dispatch packet when the tiled kernel is the only launch (no marker
    // packets between the launches of the timed loop), else recorded around the launches
    const bool ext_ev = ev0 && lut.n_items > 0 && lut.n_wide == 0;
    if (ev0 && !ext_ev) {
        const hipError_t e = hipEventRecord(ev0, s);
        if (e != hipSuccess) return e;
    }
    if (lut.n_items > 0) {
        // one resident wave of workgroups (256 CUs x kStitchBlocksPerCU), each walking its XCD band's units;
        // fewer than 3 units per workgroup (C1's 4,096 items) get a third as many workgroups as units, so
        // that every workgroup has its three statically dealt units (the first 2.7 rounds of 1,536 left the
        // last round a third empty: C1 17.4 -> 15.6 us, interleaved)
        const int units = lut.n_items * nf;
        int blocks = std::min(units, 256 * kStitchBlocksPerCU);
        if (units < 3 * 256 * kStitchBlocksPerCU) blocks = (units + 2) / 3;
        blocks = std::max(8, (blocks + 7) / 8 * 8);
        // wide staging loads need 8-byte aligned Y rows (then U / V rows are 4-byte aligned)
        bool dw = true, vig = false;
        for (int f = 0; f < nf; f++)
            for (int i = 0; i < kMaxCams; i++) {
                const SourceFrame& sf = frames[f].f[i];
                if (!sf.yuv) continue;
                if ((reinterpret_cast<uintptr_t>(sf.yuv) & 7u) || (sf.pitch & 7) || (sf.w & 7)) dw = false;
                vig |= sf.vig != nullptr;
            }
        const TiledLaunch a{blocks, frames, gains, out, lut, W, H, use_gain, out_pitch, rgba, s,
                            ext_ev ? ev0 : nullptr, ext_ev ? ev1 : nullptr, pix, dw, vig, lg};
        const hipError_t e = lut.tex ? launch_tiled_for<MODE, true>(a) : launch_tiled_for<MODE, false>(a);
        if (e != hipSuccess) return e;
    }
    if (lut.n_wide > 0)
        for (int f = 0; f < nf; f++)
            hipLaunchKernelGGL(stitch_wide_kernel<MODE>, dim3(lut.n_wide), dim3(256), 0, s, frames[f], lut, W, H,
                               gains[f], use_gain, out ? out[f] : nullptr, out_pitch, rgba, pix);
    if (ev0 && !ext_ev) {
        const hipError_t e = hipEventRecord(ev1, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

int composite_qpl() { return kItemHalves; }

hipError_t launch_stitch_batch(const FrameSet* frames, int nf, const TiledLut& lut, int W, int H,
                               const double* const* gains, int use_gain, uint8_t* const* out, int64_t out_pitch,
                               hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int pix) {
    if (nf < 1 || nf > kMaxBatch) return hipErrorInvalidValue;
    return launch_composite<0>(frames, nf, lut, W, H, gains, use_gain, out, out_pitch, RgbaOut{}, s, ev0, ev1, pix);
}

hipError_t launch_stitch(const FrameSet& frames, const TiledLut& lut, int W, int H, const double* gains,
                         int use_gain, uint8_t* out, int64_t out_pitch, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1,
                         int pix) {
    return launch_composite<0>(&frames, 1, lut, W, H, &gains, use_gain, &out, out_pitch, RgbaOut{}, s, ev0, ev1, pix);
}

hipError_t launch_mb_remap(const FrameSet& frames, const TiledLut& lut, const double* gains, int use_gain,
                           const RgbaOut& out, hipStream_t s, int pix) {
    // W, H: no level-grid bound of its own (the per-camera ROI check drops what lies outside)
    // (the result frame's layout travels in `out`; a planar launch keeps the planar instances)
    const int p = (pix & kPixInNv12) | ((out.res && !out.res_rgba && out.res_v_off == 0u) ? kPixOutNv12 : 0);
    return launch_composite<1>(&frames, 1, lut, 1 << 16, 1 << 16, &gains, use_gain, nullptr, 0, out, s, nullptr, nullptr, p);
}

// ---------------------------------------------------------------------------------------------
// Scaled output (Mapper with scale_output != template size, mapper.cpp:290-306): the stitched RGB
// result is resized with cuda::resize INTER_LINEAR (the glob kernel, resize.cu:71-103, which a
// 3-channel image always takes) and converted to YUV420P.  Source: the composite's RGBA frame
// (alpha ignored).  One lane per 2x2 output quad: 4 bilinear samples, then the same RGB -> YUV420P
// quad conversion as the fused path.  nvcc contracts `out + src * w` into an FMA: explicit fmaf.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) resize_rgba_yuv420_kernel(const uint8_t* __restrict__ rgba, int sw, int sh,
                                                                 int64_t spitch, float fx, float fy, uint8_t* out,
                                                                 int dw, int dh, int64_t out_pitch, int out_nv12) {
    const OutFrame of = make_out_frame(out, dw, dh, out_pitch, out_nv12 != 0);
    const int qw = dw >> 1, qh = dh >> 1;
    const int64_t total = (int64_t)qw * qh;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int qy = (int)(q / qw), qx = (int)(q - (int64_t)qy * qw);
        uint32_t rgb[4][3];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int x = 2 * qx + (p & 1), y = 2 * qy + (p >> 1);
            const float src_x = (float)x * fx, src_y = (float)y * fy;
            const int x1 = (int)floorf(src_x), y1 = (int)floorf(src_y);
            const int x2 = x1 + 1, y2 = y1 + 1;
            const int x2r = min(x2, sw - 1), y2r = min(y2, sh - 1);
            const uint32_t* r1 = reinterpret_cast<const uint32_t*>(rgba + (int64_t)y1 * spitch);
            const uint32_t* r2 = reinterpret_cast<const uint32_t*>(rgba + (int64_t)y2r * spitch);
            const uint32_t c00 = r1[x1], c01 = r1[x2r], c10 = r2[x1], c11 = r2[x2r];
            const float w00 = ((float)x2 - src_x) * ((float)y2 - src_y);
            const float w01 = (src_x - (float)x1) * ((float)y2 - src_y);
            const float w10 = ((float)x2 - src_x) * (src_y - (float)y1);
            const float w11 = (src_x - (float)x1) * (src_y - (float)y1);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const uint32_t sh8 = 8u * ch;
                float o = 0.f;
                o = __builtin_fmaf((float)((c00 >> sh8) & 255u), w00, o);
                o = __builtin_fmaf((float)((c01 >> sh8) & 255u), w01, o);
                o = __builtin_fmaf((float)((c10 >> sh8) & 255u), w10, o);
                o = __builtin_fmaf((float)((c11 >> sh8) & 255u), w11, o);
                rgb[p][ch] = (uint32_t)sat_u8_rne(o);
            }
        }
        store_quad<kOutRuntime>(of, finish_quad_u8(rgb), 2 * qx, 2 * qy, true);  // rgb already 0..255
    }
}

hipError_t launch_resize_rgba_yuv420(const uint8_t* rgba, int sw, int sh, int64_t spitch, uint8_t* out, int dw, int dh,
                                     int64_t out_pitch, hipStream_t s, int out_nv12) {
    if (dw <= 0 || dh <= 0 || (dw & 1) || (dh & 1)) return hipErrorInvalidValue;
    // resize.cpp:82-83,105: the kernel gets (float)(1.0 / (double(dsize) / src))
    const float fx = (float)(1.0 / ((double)dw / sw)), fy = (float)(1.0 / ((double)dh / sh));
    const int64_t total = (int64_t)(dw / 2) * (dh / 2);
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(resize_rgba_yuv420_kernel, dim3(blocks), dim3(256), 0, s, rgba, sw, sh, spitch, fx, fy, out, dw,
                       dh, out_pitch, out_nv12);
    return hipGetLastError();
}

}  // namespace octvr
