/*
 * octvr_hip.h — C ABI of the MI355X-native octVR stitching path (remap + gain + seam composite).
 *
 * This is the drop-in boundary for the reference's octvr per-frame path.  Each entry point names
 * the reference interface it replaces (paths relative to the blahgeek/OpenCV-octVR root):
 *
 *   octvr_rig_*      <- vr::MapperTemplate           modules/octvr/include/octvr.hpp:47-91,
 *                                                     modules/octvr/src/template.cpp:23-322
 *   octvr_mapper_*   <- vr::Mapper                   modules/octvr/src/mapper.hpp:29-95,
 *                                                     modules/octvr/src/mapper.cpp:47-323
 *   octvr_async_*    <- vr::AsyncMultiMapper         modules/octvr/include/octvr.hpp:103-121,
 *                                                     modules/octvr/src/async.cpp:32-350
 *   octvr_fastmapper_* <- vr::FastMapper           modules/octvr/src/mapper_fast.cpp:27-195
 *   octvr_remap_*    <- cv::remap INTER_LINEAR u8    modules/imgproc/src/imgwarp.cpp:4689-4828
 *
 * Conventions: no exceptions cross the boundary; every call returns an int status
 * (OCTVR_OK = 0, negative = error, message via octvr_last_error()).  Pointers named *_dev are HIP
 * device pointers; `stream` is a hipStream_t (NULL = the legacy default stream).  A rig owns host
 * memory; a mapper owns device memory on one device and is not thread-safe.  Separate mappers on
 * separate devices are independent (the multi-GPU model: one rig per GPU).
 */
#ifndef OCTVR_HIP_H
#define OCTVR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCTVR_HIP_ABI_VERSION 1

enum {
    OCTVR_OK = 0,
    OCTVR_E_INVALID = -1,   /* bad argument / shape (reference: CV_Assert) */
    OCTVR_E_PARSE = -2,     /* bad JSON or .dat (reference: throw std::string) */
    OCTVR_E_HIP = -3,       /* HIP runtime failure */
    OCTVR_E_UNSUPPORTED = -4,
    OCTVR_E_IO = -5
};

typedef struct octvr_rig octvr_rig;
typedef struct octvr_mapper octvr_mapper;

/* One input of a MapperTemplate (octvr.hpp:55-61): ROI in output pixels, ROI-sized maps
 * (normalized x/W_in, y/H_in, or -1), ROI-sized LUT mask {0,255} and seam mask (may be NULL). */
typedef struct {
    int roi_x, roi_y, roi_w, roi_h;
    const float* map1;
    const float* map2;
    const uint8_t* mask;
    const uint8_t* seam_mask;
    const float* vignette;     /* 512x512 f32 or NULL (vignette.cpp:39-54) */
    int vignette_w, vignette_h;
} octvr_input_view;

int octvr_abi_version(void);
const char* octvr_last_error(void);
int octvr_device_count(int* count);

/* ---- device memory helpers (for C/C++ callers without their own allocator) ------------------- */
int octvr_dev_malloc(int device, size_t bytes, void** ptr);
int octvr_dev_free(void* ptr);
int octvr_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int octvr_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
int octvr_stream_sync(void* stream);

/* ---- vr::MapperTemplate -------------------------------------------------------------------- */
/* MapperTemplate(to, to_opts, w, h) + add_input(..., use_roi) for every entry of `inputs`
 * (template.cpp:23-153, apps/octvr/dump.cpp:76-93).  The projection LUT is built on `device`
 * by a gfx950 FP64 kernel.  out_w/out_h <= 0 derive from the output aspect ratio (template.cpp:32-38).
 * Seam masks are NOT built here (see octvr_rig_create_masks). */
int octvr_rig_create_json(const char* json, int out_w, int out_h, int use_roi, int device, octvr_rig** rig);
/* MapperTemplate(to, to_opts, width, height) (template.cpp:23-44): an empty template with the output
 * camera `out_type` and its options object (JSON text); width / height <= 0 derive from the output
 * aspect ratio.  flags: OCTVR_JSON_EXACT = numbers are correctly rounded (text printed from doubles with
 * 17 digits); 0 = rapidjson 1.0.2's own number rules, as the reference parses a config file. */
#define OCTVR_JSON_EXACT 1
int octvr_rig_create(const char* out_type, const char* out_opts_json, int out_w, int out_h, int device, int flags,
                     octvr_rig** rig);
/* MapperTemplate::add_input(from, from_opts, overlay, use_roi) (template.cpp:46-153): builds input (or
 * overlay) LUT on the rig's device; include masks clear earlier inputs' masks (visible_mask).  Existing
 * seam masks are dropped (create_masks again). */
int octvr_rig_add_input(octvr_rig* rig, const char* type, const char* opts_json, int overlay, int use_roi, int flags);
/* MapperTemplate(std::ifstream&) — VRv11 reader (template.cpp:258-314). */
int octvr_rig_load_dat(const char* path, octvr_rig** rig);
/* The same reader / MapperTemplate::dump writer over caller streams: read(ctx, buf, n) returns the bytes
 * read (0 = end), write(ctx, data, n) returns n on success. */
typedef size_t (*octvr_read_fn)(void* ctx, void* buf, size_t n);
typedef size_t (*octvr_write_fn)(void* ctx, const void* data, size_t n);
int octvr_rig_load_stream(octvr_read_fn read, void* ctx, octvr_rig** rig);
int octvr_rig_dump_stream(octvr_rig* rig, octvr_write_fn write, void* ctx);
/* MapperTemplate::dump — VRv11 writer, byte-compatible (template.cpp:206-256).  Like the reference,
 * creates the seam masks first when the rig has none (template.cpp:209-210). */
int octvr_rig_dump_dat(octvr_rig* rig, const char* path);
/* MapperTemplate::create_masks() without images (template.cpp:155-204): the L2 distance seam finder
 * (DistanceSeamFinder, stitching/src/seam_finders.cpp:97-133) on masks resized to <= 960 px wide,
 * seams resized back to each ROI.  Resizes run on `device`; replaces existing seam masks. */
int octvr_rig_create_masks(octvr_rig* rig, int device);
/* Build a rig from caller arrays (ROI-sized maps/masks, row-major, tightly packed). */
int octvr_rig_create_from_arrays(int out_w, int out_h, int n_inputs, const int* rois, const float* const* map1,
                                 const float* const* map2, const uint8_t* const* masks,
                                 const uint8_t* const* seam_masks_or_null, octvr_rig** rig);
/* inputs[i].vignette (overlay = 0) or overlay_inputs[i].vignette: a w x h f32 gain map, or none
 * (map NULL, w = h = 0).  Overlay i of a rig made from arrays: */
int octvr_rig_set_vignette(octvr_rig* rig, int i, int overlay, const float* map, int w, int h);
int octvr_rig_add_overlay_arrays(octvr_rig* rig, const int* roi, const float* map1, const float* map2,
                                 const uint8_t* mask);
int octvr_rig_num_inputs(const octvr_rig* rig, int* n);
int octvr_rig_out_size(const octvr_rig* rig, int* w, int* h);
int octvr_rig_get_input(const octvr_rig* rig, int i, octvr_input_view* view);

/* Overlay inputs of the rig (MapperTemplate::overlay_inputs, octvr.hpp:62; built like the inputs by
 * add_input(..., overlay = true), template.cpp:46-153, written to .dat at template.cpp:248-255). */
int octvr_rig_num_overlays(const octvr_rig* rig, int* n);
/* ROI, maps, mask (and vignette) of overlay i; seam_mask is NULL (overlays have none). */
int octvr_rig_get_overlay(const octvr_rig* rig, int i, octvr_input_view* view);
/* MapperTemplate::morph_controlpoints(control_points) (modules/octvr/src/template_morph.cpp:69-237,
 * called by octvr_dump -c, apps/octvr/dump.cpp:98-99): control_points_json is the rig JSON's
 * "control_points" array, [[n0, n1, x0, y0, x1, y1], ...] (n0 < n1, normalized input coordinates).
 * Warps every input's map1 / map2 / mask piecewise-affinely (Delaunay triangles of the control
 * points' output positions -> their distance-weighted midpoints); seam masks are left as they are.
 * Needs a rig built by octvr_rig_create_json (camera models): OCTVR_E_UNSUPPORTED otherwise, and for
 * fisheye / pinhole control-point cameras (no image_to_obj in the reference).  Points that the
 * reference would index out of bounds (NaN projection, outside the camera's ROI) give
 * OCTVR_E_INVALID.  n_used (optional): control points kept after the 0.1 distance filter. */
int octvr_rig_morph_controlpoints(octvr_rig* rig, const char* control_points_json, int* n_used);
/* inputs[i].src_triangles / dst_triangles (octvr.hpp:60) of the last morph: 6 floats (x0 y0 x1 y1 x2
 * y2, normalized output coordinates) per triangle.  *n = count; src / dst may be NULL (count only). */
int octvr_rig_get_triangles(const octvr_rig* rig, int i, float* src, float* dst, int cap, int* n);
void octvr_rig_destroy(octvr_rig* rig);
/* An independent deep copy of a rig (camera models, LUTs, seams, include-mask visibility state): what
 * copying a vr::MapperTemplate copies (its Input vectors, octvr.hpp:56-64), so add_input / morph on
 * one copy leave the other unchanged. */
int octvr_rig_clone(const octvr_rig* rig, octvr_rig** out);

/* ---- vr::Mapper ---------------------------------------------------------------------------- */
/* Mapper(mt, in_sizes, blend, enable_gain, scale_output) (mapper.cpp:47-191).
 * blend: 0 = no blend (composite by LUT mask, later input wins; mapper.cpp:268-277), > 0 multi-band
 * with ceil(log2(blend)) - 1 bands (MultiBandGPUBlender), < 0 feather with border -blend
 * (FeatherGPUBlender); blend != 0 needs seam masks (octvr_rig_create_masks or a .dat).
 * scale_w/scale_h: 0 = output at template size, else the output is resized (mapper.cpp:290-306).
 * Overlays: a rig with N inputs and K overlays takes n_inputs = N + K sizes (inputs, then overlays; anything
 * else is OCTVR_E_INVALID), N + K <= 32, and every in_dev / in_pitch array of the stitch calls below holds N + K
 * entries per frame: camera N + k is overlay k's live frame, of its own even size, in the same layout and under
 * the same pitch rules as the inputs (octvr_mapper_set_pixel_formats covers it).  An overlay goes through the
 * inputs' per-pixel path (YUV -> RGB, vignette, remap in the mapper's sampling convention) but is never gained
 * and stays out of the gain estimation and the blenders: after the blend over the N inputs, for k = 0 .. K - 1,
 * result(roi_k)[mask_k != 0] = warped_k (a later overlay wins), and the scaled output, the RGB -> YUV420
 * conversion and the preview are taken from the patched result (mapper.cpp:279-312).  Parity unpinned: the
 * reference omits the overlays' RGBA -> RGB conversion before copyTo (mapper.cpp:147-151, 270) and fails there;
 * this is its behaviour with that conversion restored.  Gains stay one per input (N): n_gains, octvr_mapper_gains.
 * A single input disables gain and blend whatever overlays it has (mapper.cpp:78-82).  With blend 0 the overlays
 * are the last cameras of the composite LUT (no extra pass; frames in flight and batches as usual, a batch of 4
 * needs N + K <= 16).  With blend != 0 the mapper stitches through its one RGBA result frame, overlay_apply_kernel
 * patches it, and the identity resize converts it: more than one frame in flight is OCTVR_E_UNSUPPORTED. */
int octvr_mapper_create(const octvr_rig* rig, int device, int n_inputs, const int* in_w, const int* in_h, int blend,
                        int enable_gain, int scale_w, int scale_h, octvr_mapper** mapper);
/* The same with creation flags (no reference counterpart; 0 = octvr_mapper_create).
 * OCTVR_REMAP_TEXTURE: sample the camera frames as the reference's live CUDA path does —
 * cv::cuda::fastRemap through a linear-filtered, clamp-addressed texture (cudawarping/src/cuda/
 * fast_remap.cu:21-44): x = u W - 0.5, 8-bit fractions, taps clamped to the image, u < 0 -> 0 — instead
 * of cv::remap's fixed point (imgwarp.cpp; the default, which the CPU and OpenCL paths share).  The
 * texture filter is NVIDIA hardware behaviour; this mode follows the oracle's model of it
 * (oracle/octvr_oracle.c orc_fast_remap_tex_rgba) bit for bit, gain samples included.  Tiles whose taps
 * all lie inside their camera's image are staged in LDS like the default's (stitch_tiled_tex_kernel, a
 * 16-bit fraction code per pixel); tiles with a tap the clamp moves take the gather kernel.  The f32
 * filter model costs about twice the default's VALU per pixel, so the mode is slower.  Other bits:
 * OCTVR_E_INVALID. */
#define OCTVR_REMAP_TEXTURE 1
int octvr_mapper_create_ex(const octvr_rig* rig, int device, int n_inputs, const int* in_w, const int* in_h, int blend,
                           int enable_gain, int scale_w, int scale_h, int flags, octvr_mapper** mapper);
/* Mapper::stitch (mapper.cpp:193-323) on device-resident YUV420P frames in the "Y over [U|V]"
 * layout of mapper.hpp:75-83: rows [0,H) = Y (W bytes), rows [H, 3H/2) = U in bytes [0, W/2) and
 * V in bytes [W/2, W) of each row; `pitch` = bytes per row (>= W).  gains: NULL = estimate
 * (GainCompensatorGPU::feed), else set_gains (n_gains == the rig's inputs N, overlays aside).  Stream-ordered,
 * no host sync. */
int octvr_mapper_stitch_yuv420p(octvr_mapper* mapper, const uint8_t* const* in_dev, const size_t* in_pitch,
                                uint8_t* out_dev, size_t out_pitch, const double* gains, int n_gains, void* stream);
/* n_frames (1, 2 or 4) consecutive frames of the same rig in one call (no reference counterpart; the
 * reference stitches a frame per Mapper::stitch): frame f's inputs are in_dev[f * n_inputs + i] /
 * in_pitch[...], its output out_dev[f] (all outputs of pitch out_pitch); gains NULL = estimate every frame's
 * own gains, else n_frames * N values (N: the rig's inputs without its overlays).  Each frame gets its own gain feed into its own frame slot, then
 * ONE composite launch stitches all of them: its work runs over (item, frame) pairs, so an item's LUT entries,
 * metadata and staging groups are fetched once for the batch.  Every output equals a separate stitch of its
 * frame, bit for bit.  Needs n_frames frames in flight (octvr_mapper_set_frames_in_flight) and, for 4, at
 * most 16 inputs and overlays together; scaled-output and multi-band / feather mappers stitch the frames one
 * by one. */
int octvr_mapper_stitch_batch(octvr_mapper* mapper, int n_frames, const uint8_t* const* in_dev, const size_t* in_pitch,
                              uint8_t* const* out_dev, size_t out_pitch, const double* gains, void* stream);
/* The same with Mapper::stitch's preview_output (mapper.cpp:308-312): the RGB result resized
 * (cuda::resize INTER_LINEAR) into a preview_w x preview_h CV_8UC3 device image (3 bytes per pixel,
 * row pitch preview_pitch); preview_dev NULL = none.  Needs one frame in flight, unless preview_w x preview_h is
 * the size octvr_mapper_prepare_preview prepared: then the stitch is the one without a preview and the preview
 * is gathered after it (below). */
int octvr_mapper_stitch_preview(octvr_mapper* mapper, const uint8_t* const* in_dev, const size_t* in_pitch,
                                uint8_t* out_dev, size_t out_pitch, uint8_t* preview_dev, int preview_w, int preview_h,
                                size_t preview_pitch, const double* gains, int n_gains, void* stream);
/* A preview without the result frame (no reference counterpart), for a blend-0 mapper with the output at
 * template size.  There a result pixel is a function of one camera's four taps and that camera's gain, so the
 * preview's pixels can be computed from the source frames: this call builds, for exactly preview_w x preview_h,
 * the list of the result pixels cuda::resize INTER_LINEAR reads (four per preview pixel, 32 bytes of device memory
 * per preview pixel) from `rig`.  Afterwards octvr_mapper_stitch_preview with a preview of that size runs the
 * launches of a stitch without a preview plus one gather kernel on the same stream: the same bytes as the
 * result-frame path, the result frame never allocated, any number of frames in flight, the timed interval
 * (octvr_mapper_set_timing) covering the composite and the gather.  A preview of any other size takes the
 * result-frame path as before, with its one frame in flight.  One prepared size per mapper: a second call
 * replaces it, 0, 0 drops it.  `rig` must be the rig the mapper was created from (the mapper keeps no maps): a rig
 * whose output size, input count, overlay count or ROIs differ is OCTVR_E_INVALID; the same maps are the
 * caller's contract.  Overlays of a blend-0 mapper are cameras of the same LUT and are covered.
 * OCTVR_E_UNSUPPORTED (the reason in octvr_last_error) for a multi-band / feather mapper, whose result is not
 * a per-pixel function of the sources, and for a scaled output, which needs the result frame anyway.
 * Synchronizes the mapper, as octvr_mapper_set_frames_in_flight does.  octvr_mapper_info reports
 * "preview_prepared": [w, h] ([0, 0]: none) and "preview_entries"; octvr_mapper_traffic models the stitch and
 * does not change.  preview_w * preview_h <= OCTVR_MAX_PREPARED_PREVIEW_PIXELS (OCTVR_E_INVALID above). */
#define OCTVR_MAX_PREPARED_PREVIEW_PIXELS (1 << 26)
int octvr_mapper_prepare_preview(octvr_mapper* mapper, const octvr_rig* rig, int preview_w, int preview_h);
/* The RGB result as a planar tensor (no reference counterpart): what a model takes, with no packed-RGB or 4:2:0
 * detour.  Let P[y][x][c] be the bytes octvr_mapper_stitch_preview writes for a w x h preview of the same
 * stitch (at template size: the RGB result itself).  Element (plane, y, x) is stored at
 * dev + plane * plane_stride + y * row_stride + x elements and holds colour c of pixel (x, y), c = plane for
 * bgr = 0 and 2 - plane for bgr = 1:
 *   OCTVR_TENSOR_U8   P
 *   OCTVR_TENSOR_F32  (float)P * scale[c] + bias[c], a multiply and then an add in f32 (two roundings)
 *   OCTVR_TENSOR_F16  that f32 value rounded to nearest even; overflow gives inf, subnormal halves are kept
 * scale and bias are indexed by colour R, G, B whatever `bgr` says, and ignored for U8.  A float tensor at a
 * resized size goes through the preview's u8 rounding.  Elements between w and row_stride, and between planes,
 * are never written.  dev needs the element size's alignment only; rows at wider alignments get wider stores.
 * out_dev non-NULL: the YUV frame of octvr_mapper_stitch_yuv420p as well, the same bytes and gains, in the
 * mapper's output format.  out_dev NULL: no YUV frame is written and out_pitch is ignored.
 * The tensor takes one of the preview's two paths.  Of the size octvr_mapper_prepare_preview prepared it is
 * gathered from the source frames: any number of frames in flight, and with out_dev NULL no composite is launched
 * at all (the gain feed or set_gains, then the gather).  Of any other size it is resized from the result frame,
 * which serves every mapper (blends, scaled output, overlays, texture mode, any input format), needs one frame in
 * flight as the preview does (OCTVR_E_INVALID otherwise), and with out_dev NULL skips the conversion to YUV.
 * OCTVR_E_INVALID before any launch, the mapper left usable: tensor or dev NULL, a dtype outside the enum, bgr
 * outside {0, 1}, w or h <= 0, row_stride < w, plane_stride < row_stride * (h - 1) + w, dev not a multiple of the
 * element size.  The kernels address with 64 bits: a tensor may reach 2 GiB and more from dev.
 * octvr_mapper_info counts "tensor_resized", "tensor_gathered" and "tensor_no_composite" (gathered tensors whose
 * stitch launched no composite); the timed interval (octvr_mapper_set_timing) covers the stitch and the tensor
 * kernel. */
enum { OCTVR_TENSOR_U8 = 0, OCTVR_TENSOR_F16 = 1, OCTVR_TENSOR_F32 = 2 };
typedef struct octvr_tensor_out {
    void* dev;            /* device memory of the mapper's device */
    int w, h;             /* picture size: any size a preview may have */
    int dtype;            /* OCTVR_TENSOR_* */
    int bgr;              /* 0: planes R, G, B;  1: planes B, G, R */
    size_t row_stride;    /* in elements, >= w */
    size_t plane_stride;  /* in elements, >= row_stride * (h - 1) + w (planes do not overlap) */
    float scale[3], bias[3]; /* per colour R, G, B whatever `bgr` says; ignored for U8 */
} octvr_tensor_out;
int octvr_mapper_stitch_tensor(octvr_mapper* mapper, const uint8_t* const* in_dev, const size_t* in_pitch,
                               uint8_t* out_dev /* may be NULL */, size_t out_pitch, const octvr_tensor_out* tensor,
                               const double* gains, int n_gains, void* stream);
/* Mapper::gains() (mapper.hpp:88-90): gains used by the last stitch, one per input (n >= N; overlays have
 * none) (synchronizes the stream). */
int octvr_mapper_gains(octvr_mapper* mapper, double* gains, int n);
/* Frames in flight (no reference counterpart: vr::Mapper is not re-entrant, and AsyncMultiMapper
 * serialises its stitches on one compute stream, async.cpp:78-92).  k slots of per-frame device state
 * (gains, gain-feed totals, composite work queue); consecutive stitches take the slots in turn, so
 * stitches issued on different streams overlap (frame k+1's gain feed under frame k's composite).
 * A stitch waits (through an event) only for its slot's previous stitch.
 * k > 1 needs the output at template size (no scaled output; OCTVR_E_UNSUPPORTED otherwise) and, on a
 * multi-band / feather mapper, no overlays (they are copied onto the one result frame; OCTVR_E_UNSUPPORTED);
 * multi-band / feather mappers get per-slot pyramids.  Synchronizes. */
#define OCTVR_MAX_FRAMES_IN_FLIGHT 16
int octvr_mapper_set_frames_in_flight(octvr_mapper* mapper, int k);
/* Pixel layouts of the frames (no reference counterpart: the reference's frames come from ffmpeg through
 * NPP in its own planar layout; hardware video decoders and encoders speak NV12).  Both layouts are
 * W x 3H/2 bytes with rows [0,H) = Y:
 *   OCTVR_PIX_YUV420P  rows [H, 3H/2): U in bytes [0, W/2), V in bytes [W/2, W)  ("Y over [U|V]", the default)
 *   OCTVR_PIX_NV12     rows [H, 3H/2): W/2 byte pairs U,V (U first: true NV12; the FastMapper's NV12 keeps
 *                      the reference's V,U order)
 * in_format holds for every in_dev[i], out_format for out_dev, of every later octvr_mapper_stitch_yuv420p,
 * octvr_mapper_stitch_batch and octvr_mapper_stitch_preview (the preview image stays RGB).  The two are
 * independent; `pitch` rules are unchanged (>= W, any alignment).  The kernels read and write the layouts
 * themselves (no conversion pass, no intermediate frame): the result is the planar stitch of the same
 * pixels, bit for bit, with the chroma bytes rearranged.  Any other value: OCTVR_E_INVALID.  Synchronizes.
 * The octvr_async_* pipeline has its own setter, octvr_async_set_pixel_formats, which sets its mappers' formats
 * through this one; the FastMapper is not affected.
 *
 *   OCTVR_PIX_UYVY422  packed 4:2:2, what uncompressed capture and playout cards move: a frame is H rows of 2 W
 *                      bytes, U0 Y0 V0 Y1 per pixel pair (W, H even); `pitch` >= 2 W, any alignment, any base
 *                      address.  Valid for either side, independently of the other.
 * The stitch itself is a 4:2:0 one, and the chroma rules of the two conversions are this project's definitions
 * (parity unpinned, as the BT.601 conversions are):
 *   in  (4:2:2 -> 4:2:0): chroma row r of the 4:2:0 frame is, for U and V and per byte,
 *                         (c[2r] + c[2r + 1] + 1) >> 1 of the packed rows 2r and 2r + 1; luma is copied;
 *   out (4:2:0 -> 4:2:2): packed rows 2r and 2r + 1 both carry chroma row r; luma is copied.
 * So out-then-in is the identity, and a UYVY stitch is the planar stitch of the converted frames, bit for bit.
 * Unlike NV12 these are conversion passes: every frame slot owns one 4:2:0 frame per camera, which one launch
 * fills from the packed frames inside the mapper's source footprint (only the bytes some kernel reads are
 * converted), and one 4:2:0 output frame, which one launch packs into out_dev; bytes of a row of out_dev between
 * 2 W and the pitch are not written.  The frames are allocated when the format is set and freed when it is
 * unset.  OCTVR_E_INVALID from a stitch whose UYVY pitch is below 2 W, before any launch.  octvr_mapper_info
 * reports "uyvy_runs", "uyvy_in_bytes" (packed bytes read per frame) and "uyvy_out_bytes" (written).
 *
 * The other 8-bit 4:2:2 capture layouts, each valid for either side independently of the other side's format,
 * with the same two chroma rules, the same per-slot frames and footprint conversion (W, H even; any pitch
 * alignment and any base address):
 *   OCTVR_PIX_YUYV422  packed, H rows of 2 W bytes, Y0 U0 Y1 V0 per pixel pair (YUY2: V4L2 / UVC devices, HDMI
 *                      grabbers, DirectShow); `pitch` >= 2 W
 *   OCTVR_PIX_YUV422P  planar (ffmpeg yuv422p), W x 2H bytes: rows [0, H) are Y; row H + j holds chroma row j, U in
 *                      bytes [0, W/2) and V in bytes [W/2, W) ("Y over [U|V]" with H chroma rows); `pitch` >= W
 *   OCTVR_PIX_NV16     semi-planar (hardware 4:2:2 decoders, capture SDKs), W x 2H bytes: rows [0, H) are Y; row
 *                      H + j holds chroma row j as W/2 byte pairs U,V; `pitch` >= W
 *   in  (4:2:2 -> 4:2:0): chroma row r = (c[2r] + c[2r + 1] + 1) >> 1 per byte, for U and V; luma is copied;
 *   out (4:2:0 -> 4:2:2): chroma rows 2r and 2r + 1 both carry chroma row r; luma is copied; bytes between a
 *                         row's width and its pitch are never written.
 * Out-then-in is the identity, and a stitch in any of them is the planar stitch of the converted frames, bit for
 * bit.  A pitch below the row's width is OCTVR_E_INVALID before any launch.  octvr_mapper_info reports
 * "yuv422_runs", "yuv422_in_bytes" and "yuv422_out_bytes" for a side in one of these three layouts (the "uyvy_*"
 * keys stay UYVY's alone).
 *
 * 10-bit frames, each valid for either side independently of the other side's format, through the same per-slot
 * NV12 frames and footprint conversion (the stitch stays the 8-bit one).  Every sample is a 16-bit little-endian
 * word, so a row is 2 W bytes; W, H even; `pitch` >= 2 W in bytes; the base address and the pitch are multiples
 * of 2 (else OCTVR_E_INVALID before any launch), no other alignment is needed:
 *   OCTVR_PIX_P010       4:2:0 semi-planar (HEVC Main10 from hardware decoders, what encoders take), W x 3H/2
 *                        words: rows [0, H) are Y; row H + j is chroma row j as W/2 U,V word pairs.  The sample
 *                        is in bits 15..6; the low 6 bits are ignored on input and written as 0
 *   OCTVR_PIX_YUV420P10  4:2:0 planar (ffmpeg yuv420p10le), "Y over [U|V]" in words: row H + j holds U in words
 *                        [0, W/2) and V in [W/2, W).  The sample is in bits 9..0; the high 6 bits are ignored on
 *                        input (word & 0x3FF) and written as 0
 *   OCTVR_PIX_P210       4:2:2 semi-planar, W x 2H words: H rows of Y, then H chroma rows of U,V word pairs; the
 *                        sample in bits 15..6 as P010's
 *   OCTVR_PIX_YUV422P10  4:2:2 planar (ffmpeg yuv422p10le), W x 2H words: row H + j holds U in words [0, W/2) and V
 *                        in [W/2, W); the sample in bits 9..0 as YUV420P10's
 *   in  v8 = min(255, (v10 + 2) >> 2) per sample (for P010 / P210 min(255, (word + 128) >> 8)); the 4:2:2 layouts
 *       narrow each chroma sample first and then average the 8-bit rows, (c8[2r] + c8[2r + 1] + 1) >> 1 (10-bit
 *       3 and 6 give 1 and 2, so 2);
 *   out v10 = v8 << 2 (the word v8 << 8 for P010 / P210, v8 << 2 for the planar two); the 4:2:2 layouts write
 *       chroma row r to rows 2r and 2r + 1; bytes between a row's 2 W bytes and its pitch are never written.
 * Out-then-in is the identity, and a stitch in any of them is the planar 8-bit stitch of the frames converted by
 * the in rule, stored by the out rule, bit for bit.  octvr_mapper_info reports "yuv10_runs", "yuv10_in_bytes" and
 * "yuv10_out_bytes" for a side in one of these four (the "uyvy_*" and "yuv422_*" keys are then 0).
 *
 * OCTVR_PIX_V210: 10-bit 4:2:2 as uncompressed SDI / HDMI capture and playout cards hand it over (DeckLink, AJA,
 * Bluefish) and as ffmpeg's and QuickTime's `v210` codec stores it; valid for either side independently of the other
 * side's format, through the same per-slot NV12 frames and footprint conversion.  A W x H frame (W, H even) is H
 * rows of 16-byte blocks of four little-endian 32-bit words; a word carries three 10-bit components in bits 9..0,
 * 19..10 and 29..20 (bits 31..30 are ignored on input and written as 0).  Block b of a row holds its pixels
 * 6 b .. 6 b + 5:
 *   word 0 = Cb0 | Y0 << 10 | Cr0 << 20      word 1 = Y1 | Cb1 << 10 | Y2 << 20
 *   word 2 = Cr1 | Y3 << 10 | Cb2 << 20      word 3 = Y4 | Cr2 << 10 | Y5 << 20
 * with Cb_k, Cr_k the chroma of the pixel pair 6 b + 2 k, 6 b + 2 k + 1.  A row is 128 * ceil(W / 48) bytes (padded
 * to 48 pixels): on input the components of pixels >= W and the blocks past the last pixel are ignored; on output
 * every byte of the row is written, those components and blocks as 0; bytes between the row and the pitch are never
 * written.  `pitch` >= the row's bytes; the base address and the pitch are multiples of 4 (else OCTVR_E_INVALID
 * before any launch, the output untouched), no other alignment is needed.  The two rules are P210's: in
 * v8 = min(255, (v10 + 2) >> 2) per component, each chroma row narrowed first, then (c8[2r] + c8[2r + 1] + 1) >> 1;
 * out v10 = v8 << 2 with chroma row r on rows 2r and 2r + 1.  Out-then-in is the identity, and a v210 stitch is the
 * planar 8-bit stitch of the frames converted by the in rule, stored by the out rule, bit for bit.
 * octvr_mapper_info reports "v210_runs", "v210_in_bytes" (the 16-byte blocks the conversion reads per frame: the
 * blocks that hold a footprint run's pixels, in its two rows, each counted once) and "v210_out_bytes" (the row's
 * bytes times H at the output size); the "uyvy_*", "yuv422_*" and "yuv10_*" keys are then 0.  Y210, v216 and 12-bit
 * samples are not taken. */
enum {
    OCTVR_PIX_YUV420P = 0,
    OCTVR_PIX_NV12 = 1,
    OCTVR_PIX_UYVY422 = 16,
    OCTVR_PIX_YUYV422 = 17,
    OCTVR_PIX_YUV422P = 18,
    OCTVR_PIX_NV16 = 19,
    OCTVR_PIX_P010 = 32,
    OCTVR_PIX_YUV420P10 = 33,
    OCTVR_PIX_P210 = 34,
    OCTVR_PIX_YUV422P10 = 35,
    OCTVR_PIX_V210 = 48
};
int octvr_mapper_set_pixel_formats(octvr_mapper* mapper, int in_format, int out_format);
int octvr_mapper_pixel_formats(const octvr_mapper* mapper, int* in_format, int* out_format);
/* Algorithmic device bytes read+written by one launch of the composite (stitch) kernel: 4 B tiled
 * LUT entry (8 B in wide tiles) + 1.5 B YUV420 out per output pixel + 1.5 B per input pixel (each
 * source frame read once) + the per-item headers (multi-band / feather: the whole blend sequence; with
 * overlays also the result frame's read-back, overlay_apply_kernel's work list, the source bytes under its taps
 * and the pixels it writes). */
int octvr_mapper_traffic(const octvr_mapper* mapper, double* bytes_per_frame);
/* The same split into the rig constants the composite reads once per launch (tiled-LUT entries, item headers,
 * wide-tile entries: read once for a whole frame batch, octvr_mapper_stitch_batch) and the per-frame bytes
 * (output, source); lut + frame = octvr_mapper_traffic.  Multi-band / feather: lut 0. */
int octvr_mapper_traffic_parts(const octvr_mapper* mapper, double* lut_bytes, double* frame_bytes);
/* Live per-kernel timing for roofline accounting: with enable = k > 0, every k-th stitch brackets
 * its main (composite) kernel with HIP events on the caller's stream (0 = off).  kernel_time
 * synchronizes on the recorded events, returns the summed device time and launch count, and resets
 * the log. */
int octvr_mapper_set_timing(octvr_mapper* mapper, int enable);
int octvr_mapper_kernel_time(octvr_mapper* mapper, double* total_ms, int* launches);
/* The same log with frames in flight (launches on several streams overlap): span_ms = summed
 * start-to-end times, busy_ms = length of the union of the launches' intervals (the wall time some
 * composite was running).  Synchronizes and resets the log. */
int octvr_mapper_kernel_busy(octvr_mapper* mapper, double* span_ms, double* busy_ms, int* launches);
/* The logged launches themselves: [start_ms[k], end_ms[k]] relative to the first launch's start, in issue
 * order, at most `cap` of them (*n: how many were logged); the log is then cleared as by kernel_busy. */
int octvr_mapper_kernel_intervals(octvr_mapper* mapper, double* start_ms, double* end_ms, int cap, int* n);
/* The arithmetic behind kernel_busy, on host arrays: span = sum of (end - start), busy = length of the
 * union of the n intervals [start[k], end[k]] (overlapping, nested, touching or disjoint, any order). */
int octvr_interval_union(const double* start, const double* end, int n, double* span, double* busy);
/* Build-time statistics of a mapper as a JSON object (tiles, wide tiles, staged bytes, gain samples;
 * "inputs": N, "overlays": K, and for a multi-band / feather mapper overlay_apply_kernel's "overlay_groups" and
 * "overlay_px"). */
int octvr_mapper_info(const octvr_mapper* mapper, char* buf, size_t len);
void octvr_mapper_destroy(octvr_mapper* mapper);

/* ---- vr::AsyncMultiMapper -------------------------------------------------------------------- */
/* AsyncMultiMapper::New(mts, in_sizes, out_size, blend_modes, gain_modes, output_regions, preview)
 * (modules/octvr/src/async.cpp:195-350, octvr.hpp:103-121): one vr::Mapper per rig, all fed the same
 * n_inputs camera frames, each writing the region output_regions[4*i .. 4*i+3] = (x, y, w, h) (fractions
 * of out_w x out_h, async.cpp:20-30) of one merged YUV420P output.  gain_modes[i]: -1 = no gain, i = estimate,
 * j in [0, i) = use mapper j's gains of the same frame (async.cpp:78-86; rigs i and j then have the same number
 * of inputs, else OCTVR_E_INVALID).  n_inputs = N_i + K_i for every rig i (inputs, then overlays, as each
 * reference Mapper asserts against the shared frames); the split may differ per rig.  A 3-deep pipeline of pinned host
 * and device buffers overlaps the host copies, the H2D upload, the stitch and the D2H download of
 * consecutive frames (async.cpp:32-172).  No preview: octvr_async_create_preview adds it. */
typedef struct octvr_async octvr_async;
int octvr_async_create(const octvr_rig* const* rigs, int n_rigs, int device, int n_inputs, const int* in_w,
                       const int* in_h, int out_w, int out_h, const int* blend_modes, const int* gain_modes,
                       const double* output_regions, octvr_async** async);
/* The same with mapper creation flags for every mapper (octvr_mapper_create_ex; OCTVR_REMAP_TEXTURE keeps
 * the reference's CUDA sampling, which its AsyncMultiMapper runs through vr::Mapper). */
int octvr_async_create_ex(const octvr_rig* const* rigs, int n_rigs, int device, int n_inputs, const int* in_w,
                          const int* in_h, int out_w, int out_h, const int* blend_modes, const int* gain_modes,
                          const double* output_regions, int flags, octvr_async** async);
/* The same with AsyncMultiMapper::New's preview_size (async.cpp:73-110, 141-171): every frame, each mapper
 * also writes Mapper::stitch's preview_output (its RGB result resized, cuda::resize INTER_LINEAR,
 * mapper.cpp:308-312) into its region _rect_mul_size(output_regions[i], preview) of one preview_w x
 * preview_h RGB image (CV_8UC3, black where no region writes; a region whose rectangle is empty writes
 * none), which is downloaded with the outputs and published when the frame's outputs are written:
 * octvr_async_pop_preview reads the latest, a sink receives every one.  preview_w = preview_h = 0: none
 * (= octvr_async_create_ex).  Mappers with a preview stitch through their RGB result frame
 * (mapper.cpp:266-312 order: composite, then RGB -> YUV420P and the preview resize), except a blend-0 mapper
 * whose region is at its template's size: that one is prepared for its preview rectangle's size
 * (octvr_mapper_prepare_preview) and gathers the same bytes after its plain composite. */
int octvr_async_create_preview(const octvr_rig* const* rigs, int n_rigs, int device, int n_inputs, const int* in_w,
                               const int* in_h, int out_w, int out_h, const int* blend_modes, const int* gain_modes,
                               const double* output_regions, int flags, int preview_w, int preview_h,
                               octvr_async** async);
/* vr::PreviewDataHeader (octvr.hpp:97-101): what the reference writes in front of the RGB bytes of each
 * Qt shared-memory zone (async.cpp:163-167): width, height, step = 0, fps = 1 / (mean frame interval over
 * the last completed block of 10 frames, in s), 0 until 10 frames have completed (async.cpp:141-147). */
typedef struct octvr_preview_header {
    int width, height;
    int step;
    double fps;
} octvr_preview_header;
/* The latest published preview: rgb (host, preview_h rows of preview_w * 3 bytes, row pitch `pitch`) and
 * its header.  Before the first frame completes, hdr->width = hdr->height = 0 and rgb is untouched (the
 * reference's zones start with a zeroed header, preview_video.cpp:62-66).  OCTVR_E_INVALID without a
 * preview.  After pop() of frame k with no later frame pushed, this is frame k's preview. */
int octvr_async_pop_preview(octvr_async* async, uint8_t* rgb, size_t pitch, octvr_preview_header* hdr);
/* Called on the pipeline's copy-out thread for every frame's preview, after that frame's outputs are written
 * and before its pop() returns (the reference's Qt shared-memory write, async.cpp:149-171): rgb = the
 * downloaded preview (host, valid during the call only), pitch = preview_w * 3.  A Qt caller writes it into
 * zone *meta of its two QSharedMemory zones.  NULL removes the sink.  The sink runs with no
 * lock of the pipeline held: it may call octvr_async_pop_preview or octvr_async_set_preview_sink.  Called from
 * any other thread, octvr_async_set_preview_sink returns after a running sink call has returned. */
typedef void (*octvr_preview_sink)(void* user, const uint8_t* rgb, size_t pitch, const octvr_preview_header* hdr);
int octvr_async_set_preview_sink(octvr_async* async, octvr_preview_sink sink, void* user);
/* Build-time facts of the pipeline as a JSON object: packed_bytes (the footprint bytes uploaded per frame,
 * run gaps included), runs, frame bytes, preview size, the mappers' creation flags, and "pixel_formats":
 * [in, out], the current OCTVR_PIX_* pair; "device_frames", the frames octvr_async_push_device has queued so
 * far, and "merge_launches", the merge kernel's launches for them (0 or 1 per device frame);
 * "merge_pack_launches", merge_pack_kernel's launches (octvr_async_set_output_format: 1 per frame of a converted
 * output layout, host and device frames alike, else 0);
 * "preview_prepared": per mapper the [w, h] of the preview it gathers from the source frames ([0, 0]: none). */
int octvr_async_info(const octvr_async* async, char* buf, size_t len);
/* Pixel layouts of the pipeline's host planes (no reference counterpart: the reference's planes are planar;
 * decoders, capture cards and encoders speak NV12): OCTVR_PIX_YUV420P (the default) or OCTVR_PIX_NV12, for the
 * inputs (all alike) and for the merged output independently — all four pairs are valid.  The array shapes of
 * push and register_output do not change; with NV12
 *   inputs:  in_planes[3*i] = Y (W x H), in_planes[3*i+1] = the interleaved U,V plane (W bytes x H/2 rows, U
 *            first, pitch >= W), in_planes[3*i+2] is ignored and may be NULL;
 *   output:  out_planes[0] = Y, out_planes[1] = the U,V plane (out_w bytes x out_h/2 rows, pitch >= out_w),
 *            out_planes[2] is ignored and may be NULL;
 * and push, register_output, unregister_output and the registered-set match compare only the planes the format
 * uses.  The formats are forwarded to every mapper (octvr_mapper_set_pixel_formats: the kernels read and write
 * NV12 themselves), the copy-in packs a run's U,V row in place of its U and V rows (same bytes per run: the
 * footprint runs are not rebuilt), a kernel of its own unpacks them into NV12 device frames, and the
 * download / copy-out move a region's Y and U,V rows.  The merged NV12 output is the merged planar output of
 * the same pixels, bit for bit, with the chroma bytes rearranged: region k's chroma lands at its chroma
 * rectangle c read in pair units, bytes [2 c.x, 2 c.x + 2 c.w) of the U,V plane's rows [c.y, c.y + c.h); bytes
 * outside every region, and between a plane's width and its pitch, are never written.  The preview stays RGB.
 * OCTVR_E_INVALID: any other value; frames pending; a change of the output format while output plane sets are
 * registered (their plane count and geometry depend on it).  A pipeline on which this was never called behaves
 * exactly as before.  Synchronizes.
 * OCTVR_PIX_UYVY422 (octvr_mapper_set_pixel_formats) is valid as the input format: in_planes[3*i] is camera i's
 * packed plane (2 W bytes x H rows, pitch >= 2 W), the other two entries are ignored; octvr_async_push_device
 * takes one packed device frame per camera (pitch >= 2 W).  The copy-in packs the footprint runs of the packed
 * rows at 2 B per pixel, and one kernel converts them — a device frame's straight from the caller's frames,
 * after ready_event — into NV12 device frames that all mappers read (they stay on NV12 input: one conversion
 * per frame, not one per mapper).  As the output format of this call it is OCTVR_E_UNSUPPORTED: the merge, the
 * copy-out and the registered planes it sets up are per-plane tables of a 4:2:0 frame; the merged frame in a
 * converted layout is octvr_async_set_output_format's.
 * OCTVR_PIX_YUYV422, OCTVR_PIX_YUV422P and OCTVR_PIX_NV16 are valid as the input format in the same way (one
 * conversion per frame for all mappers), and OCTVR_E_UNSUPPORTED as the output format here for the same reason.  Host
 * planes of a push: YUYV in_planes[3*i] only (2 W bytes x H rows); YUV422P Y (W x H), U and V (W/2 bytes x H rows
 * each); NV16 Y and the U,V plane (W bytes x H rows each), the third entry is ignored.  The copy-in packs a
 * footprint run at 4 bytes per pixel of the run: its two luma rows, then its two chroma rows in the format's
 * layout.  octvr_async_push_device takes one device frame per camera in the Mapper's layout of the format.
 * OCTVR_PIX_P010, OCTVR_PIX_YUV420P10, OCTVR_PIX_P210 and OCTVR_PIX_YUV422P10 likewise: the input format only here (as
 * the output format OCTVR_E_UNSUPPORTED, nothing changed; octvr_async_set_output_format sets them).  Host planes of a push, rows of 16-bit words with even pitches and
 * addresses: P010 / P210 Y (2 W bytes x H rows) and the U,V plane (2 W bytes x H/2 or H rows), the third entry is
 * ignored; the planar two Y, U and V (U and V W bytes x H/2 or H rows each).  The copy-in packs a footprint run as
 * its two luma rows, then its chroma row(s) in the format's layout: 6 bytes per pixel of the run for 4:2:0, 8 for
 * 4:2:2.  octvr_async_push_device takes one device frame per camera in the Mapper's layout of the format.
 * OCTVR_PIX_V210 is an input format as well: in_planes[3*i] is camera i's one plane (H rows of 128 * ceil(W / 48)
 * bytes; address and pitch multiples of 4), octvr_async_push_device takes one such device frame per camera.  The
 * copy-in packs a footprint run as the 16-byte blocks that hold its pixels, those of its first row, then those of its
 * second.  As the output format, here and in octvr_async_set_output_format, it is OCTVR_E_UNSUPPORTED with nothing
 * changed: v210 out of the pipeline is not built (merge_pack_kernel's regions would have to start at a multiple of
 * 6 pixels). */
int octvr_async_set_pixel_formats(octvr_async* async, int in_format, int out_format);
int octvr_async_pixel_formats(const octvr_async* async, int* in_format, int* out_format);
/* The layout of the merged frame, any of the ten OCTVR_PIX_* values (no reference counterpart: a playout card
 * takes UYVY or YUYV, a Main10 encoder P010).  For OCTVR_PIX_YUV420P and OCTVR_PIX_NV12 this is
 * octvr_async_set_pixel_formats(current input format, out_format).  For a converted layout D (UYVY422, YUYV422,
 * YUV422P, NV16, P010, YUV420P10, P210, YUV422P10) the input format stays as it is, every mapper is put on NV12
 * output, and one kernel per frame (merge_pack_kernel) reads the mappers' NV12 region frames and writes the merged
 * frame in layout D: the merge and the out rule of octvr_mapper_set_pixel_formats in one pass, with no merged
 * 4:2:0 intermediate.  octvr_async_pixel_formats and octvr_async_info's "pixel_formats" then report D as the output
 * format; "merge_pack_launches" counts the kernel's launches, one per frame, host and device frames alike (a device
 * frame's single whole-frame region is not stitched in place with a converted output).
 *   Region rule: a region must be a whole sub-picture of the layout.  With r and c the luma and chroma rectangles
 *     octvr_async_create computed, r.x and r.y are even, c.x == r.x / 2 and c.y == r.y / 2 for every region;
 *     otherwise OCTVR_E_INVALID, naming the region, with nothing changed.  (Creation keeps its looser rule: the
 *     planar outputs place luma and chroma independently, a pixel pair of a packed row cannot.)
 *   The merged frame is D's row bytes of out_w wide and D's rows of out_h high (the table under
 *     octvr_mapper_set_pixel_formats); the pitch is at least a row; for 16-bit layouts bases and pitches are even;
 *     a device frame is below 2 GiB.  octvr_async_push and octvr_async_register_output take D's host planes as the
 *     input side lays them out: one packed plane (2 out_w bytes x out_h rows); Y and the U,V plane; or Y, U and V
 *     (each half a row's bytes wide), chroma planes of out_h / 2 rows (4:2:0) or out_h rows (4:2:2); entries past the
 *     layout's planes are ignored.  octvr_async_push_device takes out_dev / out_pitch as one device frame in the
 *     Mapper's layout of D.
 *   Where region k lands (S = bytes per sample, cr = chroma rows per row pair, 1 or 2):
 *     packed   rows [r.y, r.y + r.h), bytes [2 r.x, 2 r.x + 2 r.w);
 *     pairs    luma rows [r.y, r.y + r.h), bytes [S r.x, S (r.x + r.w)); chroma rows out_h + cr r.y / 2 +
 *              [0, cr r.h / 2) of a frame (rows cr r.y / 2 + [0, cr r.h / 2) of the U,V plane), the same bytes;
 *     halves   luma as pairs; the same chroma rows, U at bytes [S r.x / 2, S (r.x + r.w) / 2) and V at
 *              S out_w / 2 plus the same in a frame (at the same bytes of the V plane).
 *   The bytes are the out rule applied to the bytes the same pipeline writes there with NV12 output, bit for bit:
 *     10-bit samples are v8 << 8 (bits 15..6) or v8 << 2 (bits 9..0), the other bits 0; with 4:2:2 each chroma row
 *     is written twice.  Bytes outside every region, and between a row's width and its pitch, are never written, in
 *     device frames, host planes and registered planes.  Preview, gain chaining, overlays and pop order are
 *     untouched.
 *   A host frame: each slot owns one device frame of layout D, which the same launch fills; each region's plane
 *     rectangles are downloaded by one 2-D copy each, straight into registered planes or into pinned staging, whose
 *     rows the copy-out then copies.  These buffers are allocated by this call and freed when a later
 *     octvr_async_set_pixel_formats(in, native out) leaves converted output — which is also how the input format is
 *     changed while the output is converted: set the pair, then call this again.
 * OCTVR_E_INVALID, nothing changed: an unknown value; frames pending; a change of the output format while output
 * plane sets are registered; the region rule; more than 32 regions.  Synchronizes. */
int octvr_async_set_output_format(octvr_async* async, int out_format);
/* push(inputs, output) (async.cpp:174-189): in_planes[3*i+0/1/2] = Y, U, V host planes of input i
 * (W x H, W/2 x H/2, W/2 x H/2) with row pitches in_pitches[3*i+k]; out_planes[0/1/2] / out_pitches: the
 * merged output's Y (out_w x out_h), U and V (out_w/2 x out_h/2) planes (NV12 sides: Y, U,V, unused — see
 * octvr_async_set_pixel_formats).  Returns once the frame is queued; all planes must stay valid until the
 * matching pop. */
int octvr_async_push(octvr_async* async, const uint8_t* const* in_planes, const size_t* in_pitches,
                     uint8_t* const* out_planes, const size_t* out_pitches);
/* push for frames that already live on the device (no reference counterpart: a decoder, a capture DMA, a
 * tensor or another kernel wrote them, and an encoder or a model reads the result there).
 *   in_dev[i] / in_pitch[i], i < n_inputs: one device frame per input, then per overlay, in the layout
 *     octvr_mapper_stitch_yuv420p takes: W x 3H/2 bytes, pitch >= W, any alignment; "Y over [U|V]" or NV12 as
 *     the pipeline's input format says (octvr_async_set_pixel_formats).
 *   out_dev / out_pitch: the merged device frame, out_w x 3 out_h / 2 bytes, pitch >= out_w, in the
 *     pipeline's output format.  Region k's bytes land where push puts them in the host planes: Y at its
 *     rectangle r; planar chroma at its chroma rectangle c of the U half (columns [0, out_w / 2) of the rows
 *     from out_h) and of the V half (columns from out_w / 2); NV12 chroma at bytes [2 c.x, 2 c.x + 2 c.w) of
 *     rows out_h + [c.y, c.y + c.h).  Bytes outside every region, and between out_w and the pitch, are never
 *     written.
 *   ready_event: a hipEvent_t the pipeline's compute stream waits for before any kernel reads the inputs;
 *     NULL: the inputs are complete already.
 * No host staging, no upload and no download for such a frame: the mappers read the caller's frames in
 * place and stitch into the pipeline's region frames, gains chained and the preview written as for push, then
 * one kernel places every region into the merged frame (a single region covering the whole output is
 * stitched straight into out_dev).  The preview, a small host image, is still downloaded and published.
 * Returns once the frame is queued.  octvr_async_pop returns its status once the merged frame is complete on
 * the device, the compute stream synchronised: the caller may then read it from any stream.  The frames must
 * stay allocated and untouched until that pop.  push and push_device may be mixed; pop order is push order
 * and octvr_async_pending counts both.
 * OCTVR_E_INVALID, with nothing queued or launched: a NULL pointer; a pitch below the width; an output frame
 * of 2 GiB or more or an input frame beyond the mappers' limits; in_dev[i] or out_dev that
 * hipPointerGetAttributes does not report as device memory of the pipeline's device (host memory, pinned
 * memory included); more than 32 regions (one merge launch's table). */
int octvr_async_push_device(octvr_async* async, const uint8_t* const* in_dev, const size_t* in_pitch,
                            uint8_t* out_dev, size_t out_pitch, void* ready_event);
/* pop() (async.cpp:191-193): blocks until the oldest pushed frame has been written to its output planes
 * (octvr_async_push_device: to its merged device frame); returns that frame's status (OCTVR_E_INVALID if
 * nothing is pending). */
int octvr_async_pop(octvr_async* async);
/* Register an output plane set (Y, U, V of out_w x out_h, out_w/2 x out_h/2, ...) that the caller reuses
 * (a ring of output frames, as the reference reuses its output Mats, async.cpp:113-138): the planes are
 * page-locked (hipHostRegister) and every later push with exactly these pointers and pitches is downloaded
 * straight into them — no pinned staging, no host copy-out.  The planes must stay allocated until
 * octvr_async_unregister_output or octvr_async_destroy.  OCTVR_E_HIP if the memory cannot be locked (the
 * planes then keep the staging path).  Planes whose page-rounded byte ranges touch or overlap — one contiguous
 * NV12 frame registered as (Y = its first out_h rows, U,V = the rows after), or U and V as the two column
 * halves of one array — are locked once, as one merged range; planes in separate allocations each get their
 * own hipHostRegister, as before. */
int octvr_async_register_output(octvr_async* async, uint8_t* const* planes, const size_t* pitches);
/* Undo octvr_async_register_output (no frame may be pending). */
int octvr_async_unregister_output(octvr_async* async, uint8_t* const* planes);
/* Frames pushed and not yet popped. */
int octvr_async_pending(const octvr_async* async, int* n);
/* Drains the frames in flight and joins the pipeline's worker threads (the reference leaves its five
 * threads running forever, async.cpp:337-349). */
void octvr_async_destroy(octvr_async* async);

/* ---- vr::FastMapper ------------------------------------------------------------------------- */
/* FastMapper(mt, in_sizes) (modules/octvr/src/mapper_fast.cpp:27-109): feather-weighted NV12 stitch
 * (weights 255 * max(DT_i - 5, 0) / (1e-5 + sum), half-size chroma maps); the rig's inputs must cover
 * the whole output (no ROI, mapper_fast.cpp:50-51) and have no overlays. */
typedef struct octvr_fastmapper octvr_fastmapper;
int octvr_fastmapper_create(const octvr_rig* rig, int device, int n_inputs, const int* in_w, const int* in_h,
                            octvr_fastmapper** fastmapper);
/* FastMapper::stitch_nv12 (mapper_fast.cpp:153-195) on device NV12 frames (H rows of Y, then H/2 rows
 * of interleaved U,V).  Output: W x 3H/2, chroma rows interleaved V,U — the reference's
 * channel order (merge of the V-then-U accumulators).  Stream-ordered; the FastMapper keeps no per-call
 * device state, so calls with their own outputs may run concurrently on different streams.
 * Frames, as for the Mapper: an input of width w and height h at any base address (no alignment) and any
 * pitch with w <= pitch < 2^24, no pitch alignment; pitch * 3h/2 bytes must be readable from the base (the
 * kernels read the padding of a row, never past that size) and be at least 8 (a contiguous 2 x 2 frame is
 * refused: "input frame below 8 bytes").  The output at any base address and any out_pitch >= W; bytes of
 * a row past W are not written, and every byte of the W x 3H/2 window is (0 where no input has weight).
 * A frame that breaks these is refused with OCTVR_E_INVALID before anything is launched
 * (tests/test_gpu_fastmapper_layouts.py pins all of this on the GPU). */
int octvr_fastmapper_stitch_nv12(octvr_fastmapper* fastmapper, const uint8_t* const* in_dev, const size_t* in_pitch,
                                 uint8_t* out_dev, size_t out_pitch, void* stream);
/* Algorithmic bytes one stitch_nv12 moves (entries read, output written, source bytes its weighted taps
 * reach): the roofline basis of bench.py --config F2. */
/* n_frames (1, 2 or 4) frames in one launch per plane (no reference counterpart): frame f's inputs are
 * in_dev[f * n_inputs + i], its output out_dev[f] (one pitch); each run's entries and feather weights are
 * loaded once and applied to every frame.  Every output equals stitch_nv12 of its frame, bit for bit.  4
 * frames hold at most 16 inputs. */
int octvr_fastmapper_stitch_nv12_batch(octvr_fastmapper* fastmapper, int n_frames, const uint8_t* const* in_dev,
                                       const size_t* in_pitch, uint8_t* const* out_dev, size_t out_pitch, void* stream);
int octvr_fastmapper_traffic(const octvr_fastmapper* fastmapper, double* bytes);
/* The same split into entries / weights / block headers (once per launch) and per-frame bytes (taps, output). */
int octvr_fastmapper_traffic_parts(const octvr_fastmapper* fastmapper, double* lut_bytes, double* frame_bytes);
void octvr_fastmapper_destroy(octvr_fastmapper* fastmapper);

/* ---- standalone kernels --------------------------------------------------------------------- */
/* cv::remap(src, dst, map1*sx, map2*sy, INTER_LINEAR, BORDER_CONSTANT) on u8 with cn in {1,3,4}
 * channels: 5-bit coordinates, 15-bit weights (imgwarp.cpp:211-280, 3812-4030, 4246-4497). */
int octvr_remap_u8(const uint8_t* src_dev, int sw, int sh, size_t spitch, int cn, const float* map1_dev,
                   const float* map2_dev, int mw, int mh, size_t mpitch_elems, float scale_x, float scale_y,
                   uint8_t* dst_dev, size_t dpitch, void* stream);

/* ---- camera mask rasterisation (host; what octvr_rig_create_json uses for `selection`,
 *      `exclude_masks`, `include_masks`, camera.cpp:96-187) ------------------------------------ */
/* cv::fillPoly(img, {pts}, color), lineType 8, shift 0, on a w x h u8 image (row pitch w);
 * pts = x0,y0,x1,y1,... (imgproc/src/drawing.cpp:1196-1405, 1894-1917). */
int octvr_fill_poly_u8(uint8_t* img, int w, int h, const int* pts, int npts, uint8_t color);
/* cv::imdecode(png, IMREAD_COLOR) for PNG data (imgcodecs/src/grfmt_png.cpp:240-286), written as
 * R,G,B bytes into rgb (capacity rgb_cap bytes); *w, *h receive the size.  rgb may be NULL to query. */
int octvr_png_decode_rgb(const uint8_t* png, size_t n, uint8_t* rgb, size_t rgb_cap, int* w, int* h);

/* ---- self-test hooks (used by tests/, not by the stitching path) ---------------------------------- */
/* LUT-build bookkeeping of a JSON rig: the number of input i's output pixels whose projection the GPU
 * build left to the host because a last-ulp device / glibc libm difference could change them
 * (LutGuard, camera_math.hpp); 0 for rigs from .dat / arrays. */
int octvr_rig_lut_recomputed(const octvr_rig* rig, int i, uint64_t* n);
/* The FP64 projection (MapperTemplate::add_input's (x, y) before the f32 rounding, template.cpp:70-95)
 * of every pixel of an out_w x out_h output for input `input` of a JSON rig, on `device` (where = 0;
 * fragile[k] = 1 where the guard defers the pixel to the host) or on the host with glibc (where = 1,
 * fragile unused).  x, y, fragile: host arrays of out_w * out_h.  Include masks are not evaluated. */
int octvr_debug_project_f64(const char* json, int out_w, int out_h, int input, int device, int where, double* x,
                            double* y, uint8_t* fragile);
/* FastMapper index audit (host only, no GPU): builds the FastMapper plan of `rig` for these input sizes
 * (8-byte entries when force_wide) exactly as octvr_fastmapper_create does, and replays on the host every
 * index fast_y_kernel / fast_uv_kernel derive for every run, camera group, slot and lane — block, entry,
 * weight and header indices against the uploaded arrays, camera against the frame set, each 8-byte tap-row
 * load against an NV12 frame of pitch w + pitch_pad, the in-image taps' bytes inside the loaded 8, the
 * output bytes.  Writes per-plane counts as JSON; returns OCTVR_E_INVALID if any access is out of range.
 * Addresses are replayed relative to the frame's base: the kernels form the same offsets whatever the base,
 * so a base off 4-byte alignment (unaligned 8-byte loads) is covered by the GPU tests only. */
int octvr_debug_fastmapper_audit(const octvr_rig* rig, int n_inputs, const int* in_w, const int* in_h, int force_wide,
                                 int pitch_pad, char* json, size_t len);
/* The blend = 0 composite's tiling on the host only (no GPU): the copy chain's winner per output pixel,
 * then the tiled LUT exactly as octvr_mapper_create builds it — including its check that every tap of
 * every pixel lies in a staged group of its slot (OCTVR_E_INVALID otherwise) — reported as JSON (items,
 * wide tiles, staged pixels against the boxes' pixels, bytes, chunk histogram).  flags: the mapper's
 * creation flags (OCTVR_REMAP_TEXTURE: texture-convention entries, interior ones staged, border tiles wide). */
int octvr_debug_tiled_lut_info(const octvr_rig* rig, int n_inputs, const int* in_w, const int* in_h, int flags,
                               char* json, size_t len);
/* The blend = 0 composite's 8-byte quad records (host only, no GPU): for each of n_quads quads of four 4-byte tiled
 * entries of an item of LDS row stride `stride` (dwords), ok[q] = 1 and records[q] = its record where the quad
 * qualifies (all black, or one slot and tap origins within {0, 1} x {0, 1} of a base), else ok[q] = 0 and
 * records[q] = 0; unpacked[4 q ..] = the record decoded back by the kernel's arithmetic. */
int octvr_debug_entry_pack(const uint32_t* entries, int n_quads, uint32_t stride, uint64_t* records, uint8_t* ok,
                           uint32_t* unpacked);
/* The gain feed's samples as octvr_mapper_create lays them out (host only, no GPU): per sample its entry
 * (samples[2k] = xy, samples[2k+1] = code, kernels.hpp CompositeEntry) and partner mask, in the order the
 * feed's waves take them (padding included).  count receives the number of samples; samples / partners
 * NULL = count only. */
int octvr_debug_gain_plan(const octvr_rig* rig, int n_inputs, const int* in_w, const int* in_h, int flags,
                          uint32_t* samples, uint16_t* partners, size_t cap, size_t* count);
/* The rig-config JSON reader on one document: the first number of `json` (a number, or the first element
 * of an array), parsed with rapidjson's rules (flags 0, as the reference reads its configs) or correctly
 * rounded (OCTVR_JSON_EXACT; out-of-range literals give +-HUGE_VAL / the subnormal / 0 as strtod). */
int octvr_debug_json_number(const char* json, int flags, double* value);
/* The AsyncMultiMapper copy-in's packing on caller-given runs (host only, no GPU): run k = runs[4k .. 4k+3] =
 * (camera, row pair, first 8-pixel group, groups) of cameras of in_w x in_h pixels, packed back to back into
 * `packed` (capacity cap) by the function the pipeline's copy-in stage calls, from planes / pitches laid out as
 * octvr_async_push's in_planes / in_pitches for `format` (OCTVR_PIX_*).  sizes[k] (optional) receives run k's
 * packed bytes, *bytes the total.  OCTVR_E_INVALID for a run outside its frame, a bad plane or a short buffer. */
/* (For OCTVR_PIX_UYVY422 planes[3*cam] is the camera's packed plane and a run packs its two packed rows.  For
 * OCTVR_PIX_YUYV422, _YUV422P and _NV16 the planes are octvr_async_push's for the format and a run is its two luma
 * rows, then its two chroma rows; for the four 10-bit formats its two luma rows, then its one or two chroma rows.) */
int octvr_debug_pack_runs(int n_inputs, const int* in_w, const int* in_h, const uint32_t* runs, int n_runs,
                          const uint8_t* const* planes, const size_t* pitches, int format, uint8_t* packed, size_t cap,
                          size_t* sizes, size_t* bytes);
/* The footprint runs a UYVY-input mapper's unpack launch converts, as (camera, row pair, first group, groups)
 * quadruples in `runs` (capacity cap runs; NULL: count only).  OCTVR_E_INVALID when the input format is not
 * OCTVR_PIX_UYVY422. */
int octvr_debug_mapper_uyvy_runs(const octvr_mapper* mapper, uint32_t* runs, size_t cap, size_t* count);
/* The host build's worker threads (tiler, seam finder, blender weights, audits) on n_threads threads of
 * which thread `failing` raises an error (test hook, no GPU): the error reaches the caller as a status
 * (OCTVR_E_INVALID + octvr_last_error) instead of terminating the process; failing < 0 = none fails. */
int octvr_debug_worker_failure(int n_threads, int failing);
/* The gain feed's device solver (cv::solve on the GPU) on caller-given systems: `count` host systems of the
 * same n (1..16), A row-major with row stride n (count * n * n doubles), b count * n doubles, one 256-thread
 * workgroup per system running the function the feed kernels end in.  lean = 0: the full feed's choice (closed
 * forms for n <= 3, the register LU for 4..8, the workgroup LU for 9..16); lean = 1: the lean feed's (closed
 * forms for n <= 3, the workgroup LU for 4..16).  ok[k] = 1 and x[k * n ..] = the solution where system k
 * solves, else ok[k] = 0 (x zeroed; the feed's "gains = 1 on failure" rule is the feed's own). */
int octvr_debug_gain_solve(const double* A, const double* b, int n, int count, int lean, double* x, int* ok);
/* Saturating float -> u8 conversion as the kernels implement it (method 0: rint + clamp in VALU,
 * method 1: v_cvt_pk_u8_f32), for a known-answer test of round-half-even and clamping on device. */
int octvr_selftest_sat_u8(const float* in_dev, uint8_t* out_dev, int n, int method, void* stream);

#ifdef __cplusplus
}
#endif
#endif
