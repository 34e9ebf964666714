// mapper.hpp — the mapper (vr::Mapper) behind the C ABI and the functions of its translation units that
// cross files (internal): mapper.cpp, gain_plan.cpp, and their callers octvr_hip.cpp, debug_abi.cpp, async.cpp.
#pragma once

#include <memory>
#include <utility>
#include <vector>

#include "frame_layout.hpp"
#include "host_common.hpp"

// =================================================================================================
// Mapper (vr::Mapper)
// =================================================================================================
struct octvr_mapper {
    template <class T>
    using DevBuf = octvr::DevBuf<T>;
    int device = 0;
    int n = 0;   // inputs N: what the gain estimation and the blenders see
    int nc = 0;  // cameras N + K: the frames of a stitch call, the K overlays at the tail (camera N + k)
    int W = 0, H = 0;
    int use_gain = 0;
    std::vector<int> in_w, in_h;
    // tiled composite LUT (kernels.hpp), blend = 0; tiles.queue is only the size of a slot's work queue
    octvr::TiledLutDev tiles;
    int n_tiles = 0;
    // multi-band blend state, blend > 0 (multiband_host.cpp)
    std::unique_ptr<octvr::MultiBand, octvr::MultiBandDeleter> mb;
    int blend = 0;
    // gain feed
    DevBuf<octvr::CompositeEntry> samples;  // working-scale samples that lie in some pair intersection
    DevBuf<uint16_t> partners;       // per sample: bit j = the sample is in the (camera, j) intersection
    DevBuf<int32_t> N;
    int n_chunks = 0, n_samples = 0;
    size_t n_entries = 0;
    std::vector<double> last_gains;
    std::vector<DevBuf<float>> vig;  // per camera: vignette map resized to the input size, or empty
    octvr::SourceFootprint foot;     // the input bytes this mapper's kernels read (host_common.hpp)
    int tex = 0;                     // OCTVR_REMAP_TEXTURE: texture-convention entries (make_entry_tex)
    // scaled output (scaled_output_size != stitch size, mapper.cpp:69,153-155,290-306): the RGB result
    // as an RGBA frame, resized + converted to YUV420P by a second kernel
    int SW = 0, SH = 0;
    bool scaled = false;
    DevBuf<uint8_t> result;
    DevBuf<octvr::MbCamLevel> result_view;  // the result frame as a one-entry RGBA sink of the composite
    // Overlays of a multi-band / feather mapper: the work list of overlay_apply_kernel (overlay.hip), which
    // copies the overlays onto the result frame after the blend.  A blend-0 mapper has none: its overlays
    // are cameras of the composite LUT.
    octvr::OverlayListDev ov;
    // The prepared preview (octvr_mapper_prepare_preview): preview_gather_kernel's tap list for one preview
    // size, blend 0 and unscaled output only.  A stitch whose preview has that size gathers it from the source
    // frames after the composite, on the frame slot's gains, and needs no result frame.
    octvr::PreviewListDev pv;
    std::vector<int> rois;  // x, y, w, h per camera: what prepare_preview checks its rig against
    // octvr_mapper_stitch_tensor so far: tensors resized from the result frame, tensors gathered through the
    // prepared list, and the gathered ones whose stitch launched no composite (no YUV frame asked for)
    uint64_t tensor_resized = 0, tensor_gathered = 0, tensor_no_composite = 0;
    // Per-frame device state that consecutive stitches would otherwise share: the gains, the feed's
    // pair totals and tickets, the composite's work queue.  A mapper is created with one slot;
    // octvr_mapper_set_frames_in_flight adds slots so that stitches issued on different streams overlap
    // (frame k+1's gain feed runs under frame k's composite).  A stitch takes the next slot in turn and
    // waits only for that slot's previous stitch when it was issued on another stream.
    struct FrameSlot {
        double* gains = nullptr;
        unsigned long long* totals = nullptr;  // [kGainMaxCams][kGainMaxCams] exact pair sums, units of 2^-23
        uint32_t* tickets = nullptr;           // 8 per-XCD + 1 global last-workgroup-done counters
        uint32_t* queue = nullptr;
        hipEvent_t done = nullptr;  // recorded after the slot's last stitch (its stream may since be gone)
        const octvr::FootFrames* conv_in = nullptr;  // converted input: the slot's NV12 frame per camera (SlotBufs)
        uint8_t* conv_out = nullptr;                 // converted output: the slot's NV12 output frame
    };
    struct SlotBufs {
        DevBuf<double> gains;
        DevBuf<unsigned long long> totals;
        DevBuf<uint32_t> tickets, queue;
        // Converted sides (octvr_mapper_set_pixel_formats): one NV12 frame per camera (pitch = width) that the
        // slot's unpack launch fills inside the footprint and every stage of the stitch reads, and one NV12
        // output frame (SW x 3 SH / 2) the stitch writes and the pack launch reads
        std::vector<DevBuf<uint8_t>> conv_in;
        octvr::FootFrames conv_frames{};
        DevBuf<uint8_t> conv_out;
    };
    std::vector<FrameSlot> slots;
    std::vector<std::unique_ptr<SlotBufs>> slot_bufs;  // owners of the slots' buffers, slot by slot
    int cur_slot = 0;                                  // slot of the last stitch
    int timing = 0;             // event-timing period in stitches (0 = off)
    uint64_t timed_calls = 0;
    int pix = 0;                // layouts of the inputs and the output (octvr_mapper_set_pixel_formats): kPixInNv12 | kPixOutNv12
    // A converted capture layout on either side (mapper_set_conv; frame_layout.hpp): the stitch itself then runs
    // on the frame slot's NV12 frames (`pix` carries NV12 for that side).  conv_fmt_in / conv_fmt_out: the side's
    // OCTVR_PIX_* value (0: the side is 8-bit 4:2:0, conv_in / conv_out false); conv_table: the unpack kernel's
    // pieces over this mapper's footprint, the same for every layout (the sources are frames: no piece's `off` is
    // read); conv_in_px: the pixels of the pieces' rows, run_bpp() packed bytes each; conv_in_v210: the bytes of the
    // v210 blocks that hold the runs' pixels (LayoutDesc::run_bytes of every run).
    bool conv_in = false, conv_out = false;
    int conv_fmt_in = 0, conv_fmt_out = 0;
    DevBuf<octvr::FootRun> conv_table;
    size_t conv_runs = 0, conv_in_px = 0, conv_in_v210 = 0;
    std::vector<octvr::FootRun> conv_foot_runs;  // the runs the table was cut from (octvr_debug_mapper_uyvy_runs)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events, free_events;  // recorded / reusable
    ~octvr_mapper() {
        for (auto& sl : slots)
            if (sl.done) (void)hipEventDestroy(sl.done);
        for (auto* v : {&events, &free_events})
            for (auto& e : *v) {
                (void)hipEventDestroy(e.first);
                (void)hipEventDestroy(e.second);
            }
    }
};

namespace octvr {

// ---- mapper.cpp ------------------------------------------------------------------------------------
// Mapper(mt, in_sizes, blend, enable_gain, scale_output) (mapper.cpp:60-191); flags: OCTVR_REMAP_TEXTURE
std::unique_ptr<octvr_mapper> mapper_create(const octvr_rig* rig, int device, int n_inputs, const int* in_w,
                                            const int* in_h, int blend, int enable_gain, int scale_w, int scale_h,
                                            int flags);
// preview_output of Mapper::stitch (mapper.cpp:308-312): a CV_8UC3 device image
struct PreviewOut {
    uint8_t* dev;
    int w, h;
    size_t pitch;
};
// tensor (octvr_mapper_stitch_tensor; not together with a preview): the RGB result as planes.  Only then may
// out_dev be NULL: no YUV frame is written, and a tensor of the prepared preview size launches no composite.
void mapper_stitch(octvr_mapper* m, const uint8_t* const* in_dev, const size_t* in_pitch, uint8_t* out_dev,
                   size_t out_pitch, const double* gains, int n_gains, const double* gains_dev, hipStream_t s,
                   const PreviewOut* preview = nullptr, const octvr_tensor_out* tensor = nullptr);
void mapper_stitch_batch(octvr_mapper* m, int nb, const uint8_t* const* in_dev, const size_t* in_pitch,
                         uint8_t* const* out_dev, size_t out_pitch, const double* gains, hipStream_t s);
// octvr_mapper_prepare_preview: the tap list of a w x h preview from `rig` (the rig the mapper was created
// from: its size, counts and ROIs are checked, its maps are the caller's contract); 0, 0 drops the list.
// Synchronizes the mapper.  OCTVR_E_UNSUPPORTED for a blended or scaled mapper.
void mapper_prepare_preview(octvr_mapper* m, const octvr_rig* rig, int w, int h);
// The converted sides (octvr_mapper_set_pixel_formats): allocates or frees every frame slot's NV12 frames and
// builds the unpack table from the mapper's footprint.  The mapper is synchronized by the caller.
// in / out: the side's converted format (frame_layout.hpp converted_format) or 0 for an 8-bit 4:2:0 side.
void mapper_set_conv(octvr_mapper* m, int in, int out);
// Consecutive set groups of a footprint as runs, gaps of up to `gap` groups bridged; bytes: their 4:2:0 size.
constexpr int kRunGap = 2;
std::vector<FootRun> footprint_runs(const SourceFootprint& f, size_t& bytes, int gap = kRunGap);
// Waits for the last stitch of every frame slot.
void mapper_sync(octvr_mapper& m);
// k frame slots; the last frame's gains survive into slot 0 (octvr_mapper_set_frames_in_flight)
void mapper_set_frames_in_flight(octvr_mapper* m, int k);
void mapper_set_timing(octvr_mapper* m, int enable);
// Reads back the recorded timing events: waits for them, hands each launch's [start, end] in ms after the
// first launch's start to f, and returns the event pairs to the free list.  Returns the launches.
int mapper_drain_timing(octvr_mapper* m, const std::function<void(double start_ms, double end_ms)>& f);
// Algorithmic bytes of one frame, and the part of them a batch reads once (the tiled LUT).
double mapper_traffic(const octvr_mapper* m);
double tiled_lut_bytes(const TiledLut& t, int n_packed = 0);
// The per-frame composite's tiled LUT of a W x H winner LUT: items of 128 x (8 composite_qpl()) pixels,
// black outside the frame.  n_jobs: the items of the grid, empty ones included.
TiledLutBuild build_frame_tiles(const std::vector<CompositeEntry>& lut, int W, int H, const std::vector<int>& in_w,
                                const std::vector<int>& in_h, int* n_jobs = nullptr);
int mapper_num_inputs(const octvr_mapper* m);
bool mapper_has_gain(const octvr_mapper* m);
const double* mapper_gains_dev(const octvr_mapper* m);
void mapper_out_size(const octvr_mapper* m, int* w, int* h);
const SourceFootprint& mapper_footprint(const octvr_mapper* m);

// ---- gain_plan.cpp ---------------------------------------------------------------------------------
struct GainPlan {
    std::vector<CompositeEntry> samples;
    std::vector<uint16_t> partners;
    std::vector<int32_t> N;
    int n_chunks = 0;
    size_t pairs_px = 0;
};
GainPlan plan_gain(const octvr_rig& rig, int n, const std::vector<int>& in_w, const std::vector<int>& in_h, int tex);
void setup_gain(octvr_mapper& m, const octvr_rig& rig);
std::vector<float> resize_linear_f32(const float* src, int sw, int sh, int dw, int dh);

}  // namespace octvr
