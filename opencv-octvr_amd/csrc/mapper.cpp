// mapper.cpp — vr::Mapper on the device: creation, frame slots, the stitch of one frame and of a batch,
// timing read-back and the traffic model.  Host orchestration only; the kernels are in the *.hip files.
#include "mapper.hpp"
#include "overlay_list.hpp"
#include "preview_list.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace octvr {

namespace {

// The RGB(A) result frame of the scaled-output and preview paths (allocated on first use).
void ensure_result(octvr_mapper& m) {
    if (m.result.p) return;
    REQUIRE((uint64_t)m.W * m.H * 4 < 0x7FFFFF80ull, "stitch frame larger than 2 GiB as RGBA");
    DeviceGuard dg(m.device);
    // result = 0 (mapper.cpp:156): pixels no camera writes stay black in every frame
    m.result.alloc((size_t)m.W * m.H * 4);
    HIP_CHECK(hipMemset(m.result.p, 0, m.result.n));
    MbCamLevel v{};
    v.g_off = 0;
    v.g_pitch = (uint32_t)m.W * 4;
    v.w = m.W;
    v.h = m.H;
    m.result_view.upload(&v, 1);
}

// The copy chain over cameras [first, last) resolved per output pixel (composite_lut_kernel): the last one
// whose mask is set wins.  The cameras before `first` take part with an empty ROI, so an entry's camera is
// the frame index.  Per-camera templates -> device, the LUT back, the per-camera maps dropped.
template <class Camera>
std::vector<CompositeEntry> winner_lut(const octvr_mapper& m, const Camera& camera, int first, int last) {
    std::vector<DevBuf<float>> m1(last), m2(last);
    std::vector<DevBuf<uint8_t>> mk(last);
    std::vector<CamTemplate> ct(last, CamTemplate{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0});
    for (int i = first; i < last; i++) {
        const RigInput& in = camera(i);
        m1[i].upload(in.map1.data(), in.map1.size());
        m2[i].upload(in.map2.data(), in.map2.size());
        mk[i].upload(in.mask.data(), in.mask.size());
        ct[i] = CamTemplate{m1[i].p, m2[i].p, mk[i].p, in.roi[0], in.roi[1], in.roi[2], in.roi[3], m.in_w[i], m.in_h[i]};
    }
    DevBuf<CamTemplate> ctd;
    ctd.upload(ct.data(), ct.size());
    DevBuf<CompositeEntry> lut;
    lut.alloc((size_t)m.W * m.H);
    HIP_CHECK(launch_composite_lut(ctd.p, last, m.W, m.H, lut.p, nullptr, m.tex));
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<CompositeEntry> lut8((size_t)m.W * m.H);
    HIP_CHECK(hipMemcpy(lut8.data(), lut.p, lut8.size() * sizeof(CompositeEntry), hipMemcpyDeviceToHost));
    return lut8;
}

// The overlays of a multi-band / feather mapper (cameras N .. N + K - 1): their winner LUT, the pixels some
// overlay's mask covers marked (a covered pixel whose entry is invalid is still written, black), cut down to
// overlay_apply_kernel's work list; the taps it reads join the mapper's footprint.
template <class Camera>
void setup_overlays(octvr_mapper& m, const Camera& camera) {
    std::vector<CompositeEntry> lut = winner_lut(m, camera, m.n, m.nc);
    for (int i = m.n; i < m.nc; i++) {
        const RigInput& in = camera(i);
        for (int ry = 0; ry < in.roi[3]; ry++)
            for (int rx = 0; rx < in.roi[2]; rx++) {
                const int x = in.roi[0] + rx, y = in.roi[1] + ry;
                if (x < 0 || y < 0 || x >= m.W || y >= m.H || !in.mask[(size_t)ry * in.roi[2] + rx]) continue;
                lut[(size_t)y * m.W + x].code |= kCodeCovered;
            }
    }
    const OverlayListBuild<CompositeEntry> b = build_overlay_list(lut, m.W, m.H, kCodeCovered, kOvBlockGroups);
    SourceFootprint taps;
    taps.init(m.in_w, m.in_h);
    for (const CompositeEntry& e : b.entries) taps.mark_taps(e);
    m.foot.merge(taps);
    m.ov.covered = b.covered;
    m.ov.source_bytes = taps.bytes();
    m.ov.groups.upload(b.groups.data(), b.groups.size());
    m.ov.entries.upload(b.entries.data(), b.entries.size());
    m.ov.view = OverlayList{m.ov.groups.p, m.ov.entries.p, (int)b.groups.size()};
}

// The caller's output frame: a whole frame of the converted layout (the stitch then writes the slot's own NV12
// frame), else of either 4:2:0 layout, which the stitch kernel addresses through a buffer resource with 32-bit
// offsets.
void check_out_frame(const octvr_mapper* m, const uint8_t* out_dev, size_t out_pitch) {
    const LayoutDesc d = layout_of(m->conv_out ? m->conv_fmt_out : OCTVR_PIX_YUV420P);
    const char* why = frame_fault(d, out_dev, out_pitch, m->SW, m->SH, 0x7FFFFF80ull);
    REQUIRE(!why, std::string("output ") + why);
}

// The caller's tensor (octvr_hip.h octvr_tensor_out), checked before anything is put on the stream, as the
// kernels' view of it.  The kernels form 64-bit element offsets, so a tensor may reach any distance from dev;
// the strides are bounded so that no offset of a row overflows.
TensorPlanes check_tensor(const octvr_tensor_out* t) {
    REQUIRE(t && t->dev, "NULL tensor");
    REQUIRE(t->dtype == OCTVR_TENSOR_U8 || t->dtype == OCTVR_TENSOR_F16 || t->dtype == OCTVR_TENSOR_F32,
            "tensor dtype must be OCTVR_TENSOR_U8, OCTVR_TENSOR_F16 or OCTVR_TENSOR_F32");
    REQUIRE(t->bgr == 0 || t->bgr == 1, "tensor bgr must be 0 or 1");
    REQUIRE(t->w > 0 && t->h > 0, "bad tensor size");
    REQUIRE(t->row_stride >= (size_t)t->w && t->row_stride < ((size_t)1 << 31),
            "tensor row stride below its width (or 2^31 elements and more)");
    REQUIRE(t->plane_stride >= t->row_stride * (size_t)(t->h - 1) + (size_t)t->w && t->plane_stride < ((size_t)1 << 58),
            "tensor planes overlap (or a plane stride of 2^58 elements and more)");
    const size_t es = t->dtype == OCTVR_TENSOR_U8 ? 1 : t->dtype == OCTVR_TENSOR_F16 ? 2 : 4;
    REQUIRE(reinterpret_cast<uintptr_t>(t->dev) % es == 0, "tensor not aligned to its element size");
    // one workgroup per row segment of at least 64 pixels (tensor_out.hip)
    REQUIRE(((uint64_t)t->w + 63) / 64 * (uint64_t)t->h < 0x7FFFFFFFull, "tensor too large");
    TensorPlanes p;
    memset(&p, 0, sizeof p);
    p.dev = t->dev;
    p.row_stride = (int64_t)t->row_stride;
    p.plane_stride = (int64_t)t->plane_stride;
    p.w = t->w;
    p.h = t->h;
    p.dtype = t->dtype;
    p.bgr = t->bgr;
    for (int c = 0; c < 3; c++) {
        p.scale[c] = t->scale[c];
        p.bias[c] = t->bias[c];
    }
    return p;
}

// The kernels' view of one frame's inputs.
FrameSet frame_set(const octvr_mapper* m, const uint8_t* const* in_dev, const size_t* in_pitch) {
    FrameSet fs;
    memset(&fs, 0, sizeof fs);
    for (int i = 0; i < m->nc; i++) fs.f[i] = checked_source_frame(in_dev[i], in_pitch[i], m->in_w[i], m->in_h[i], m->vig[i].p);
    return fs;
}

// The caller's frames of a converted input side, checked before anything is put on the stream.
ConvSources conv_sources(const octvr_mapper* m, const uint8_t* const* in_dev, const size_t* in_pitch) {
    ConvSources cs;
    memset(&cs, 0, sizeof cs);
    const LayoutDesc d = layout_of(m->conv_fmt_in);
    for (int i = 0; i < m->nc; i++) {
        const char* why = frame_fault(d, in_dev[i], in_pitch[i], m->in_w[i], m->in_h[i], 0x7FFFFFFFull);
        REQUIRE(!why, std::string("input ") + why);
        cs.f[i] = in_dev[i];
        cs.pitch[i] = in_pitch[i];
    }
    return cs;
}

// The pack launch of a converted output side: the slot's NV12 output frame into the caller's frame.
void conv_pack(const octvr_mapper* m, const uint8_t* src, uint8_t* out, size_t pitch, hipStream_t s) {
    HIP_CHECK(launch_layout_pack(m->conv_fmt_out, src, m->SW, m->SH, out, pitch, s));
}

// The slot's unpack launch over the mapper's footprint, and the NV12 frames every later stage reads.
FrameSet conv_unpack_slot(const octvr_mapper* m, const octvr_mapper::FrameSlot& sl, const ConvSources& cs, hipStream_t s) {
    HIP_CHECK(launch_layout_unpack(m->conv_fmt_in, m->conv_table.p, (int)m->conv_table.n, cs, *sl.conv_in, s));
    FrameSet fs;
    memset(&fs, 0, sizeof fs);
    for (int i = 0; i < m->nc; i++)
        fs.f[i] = checked_source_frame(sl.conv_in->f[i], (size_t)m->in_w[i], m->in_w[i], m->in_h[i], m->vig[i].p);
    return fs;
}

// ---- frame slots -------------------------------------------------------------------------------------
// The slot's NV12 frames of the converted sides, as the mapper's formats say (allocated or freed).  The
// input frames hold the fixed pattern of the AsyncMultiMapper's slots outside the footprint: nothing reads it.
void slot_conv(const octvr_mapper& m, octvr_mapper::SlotBufs& b, octvr_mapper::FrameSlot& sl) {
    b.conv_in.clear();
    b.conv_frames = FootFrames{};
    b.conv_out.reset();
    sl.conv_in = nullptr;
    sl.conv_out = nullptr;
    if (m.conv_in) {
        b.conv_in.resize(m.nc);
        for (int i = 0; i < m.nc; i++) {
            const size_t bytes = (size_t)m.in_w[i] * (size_t)(m.in_h[i] / 2 * 3);
            b.conv_in[i].alloc(bytes);
            HIP_CHECK(hipMemset(b.conv_in[i].p, 0x5A, bytes));
            b.conv_frames.f[i] = b.conv_in[i].p;
            b.conv_frames.w[i] = m.in_w[i];
            b.conv_frames.h[i] = m.in_h[i];
        }
        sl.conv_in = &b.conv_frames;
    }
    if (m.conv_out) {
        b.conv_out.alloc((size_t)m.SW * (size_t)(m.SH / 2 * 3));
        sl.conv_out = b.conv_out.p;
    }
}

// One more slot: gains of 1, the feed's totals and tickets and the composite's work queue zeroed.  The
// caller synchronises the device before a stream uses the slot.
octvr_mapper::FrameSlot make_slot(octvr_mapper& m) {
    auto b = std::make_unique<octvr_mapper::SlotBufs>();
    const std::vector<double> ones(kMaxCams, 1.0);
    b->gains.upload(ones.data(), ones.size());
    if (m.use_gain) {
        b->totals.alloc((size_t)kGainMaxCams * kGainMaxCams * kGainTotalStride);
        HIP_CHECK(hipMemset(b->totals.p, 0, b->totals.n * sizeof(unsigned long long)));
        b->tickets.alloc(9);
        HIP_CHECK(hipMemset(b->tickets.p, 0, b->tickets.n * sizeof(uint32_t)));
    }
    if (m.tiles.queue.n) {
        b->queue.alloc(m.tiles.queue.n);
        HIP_CHECK(hipMemset(b->queue.p, 0, b->queue.n * sizeof(uint32_t)));
    }
    octvr_mapper::FrameSlot sl;
    sl.gains = b->gains.p;
    sl.totals = b->totals.p;
    sl.tickets = b->tickets.p;
    sl.queue = b->queue.p;
    slot_conv(m, *b, sl);
    m.slot_bufs.push_back(std::move(b));
    return sl;
}

// The next slot in turn.  Stitches sharing a frame slot (gains, feed totals, work counters) are ordered:
// each waits for the slot's previous stitch (with one slot: for the previous stitch, as vr::Mapper is not
// re-entrant either).  Always through the event, never by comparing stream handles: a destroyed stream's
// handle value can come back as a new stream that is not ordered after the old one.
octvr_mapper::FrameSlot& take_slot(octvr_mapper* m, hipStream_t s) {
    m->cur_slot = (m->cur_slot + 1) % (int)m->slots.size();
    octvr_mapper::FrameSlot& sl = m->slots[m->cur_slot];
    if (sl.done) HIP_CHECK(hipStreamWaitEvent(s, sl.done, 0));
    return sl;
}

// The slot's stitch has been issued on s.
void finish_slot(octvr_mapper::FrameSlot& sl, hipStream_t s) {
    if (!sl.done) HIP_CHECK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(sl.done, s));
}

// The frame's gains into its slot: copied from another mapper (gains_dev), set (gains, one per input), or
// estimated by the gain feed (GainCompensatorGPU::feed, exposure_compensate.cpp:223-297).
void stitch_gains(octvr_mapper* m, octvr_mapper::FrameSlot& sl, const FrameSet& fs, const double* gains,
                  const double* gains_dev, hipStream_t s) {
    if (!m->use_gain) return;
    if (gains_dev) {
        HIP_CHECK(hipMemcpyAsync(sl.gains, gains_dev, sizeof(double) * m->n, hipMemcpyDeviceToDevice, s));
    } else if (gains) {
        HIP_CHECK(launch_set_gains(gains, m->n, sl.gains, s));
    } else if (m->n_chunks == 0) {  // no intersections: A = diag(b), every gain is 1
        const std::vector<double> ones(m->n, 1.0);
        HIP_CHECK(launch_set_gains(ones.data(), m->n, sl.gains, s));
    } else {
        // with frames in flight the feed runs beside the previous frame's composite: the lean
        // variant fits next to it (the wide-prefetch one waits for its workgroups to drain)
        const bool lean = m->slots.size() > 1;
        HIP_CHECK(launch_gain_feed(fs, m->samples.p, m->partners.p, m->tex, m->n_chunks, m->N.p, m->n, sl.totals,
                                   sl.tickets, sl.gains, s, lean, m->pix));
    }
}

// The timing events of this stitch, or none (octvr_mapper_set_timing: every `timing`-th stitch)
std::pair<hipEvent_t, hipEvent_t> stitch_events(octvr_mapper* m) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timed = m->timing > 0 && (m->timed_calls++ % (uint64_t)m->timing) == 0;
    if (!timed) return {e0, e1};
    if (m->free_events.empty()) {
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
    } else {
        e0 = m->free_events.back().first;
        e1 = m->free_events.back().second;
        m->free_events.pop_back();
    }
    return {e0, e1};
}

// The event pair of one stitch: kept with the recorded ones once the launch is issued, else (an exception
// on the way) returned to the reusable ones.
struct TimedPair {
    octvr_mapper* m;
    hipEvent_t e0, e1;
    bool kept = false;
    explicit TimedPair(octvr_mapper* mapper) : m(mapper) {
        const auto ev = stitch_events(mapper);
        e0 = ev.first;
        e1 = ev.second;
    }
    TimedPair(const TimedPair&) = delete;
    void keep() {
        if (e0) m->events.emplace_back(e0, e1);
        kept = true;
    }
    ~TimedPair() {
        if (!e0 || kept) return;
        try {
            m->free_events.emplace_back(e0, e1);
        } catch (...) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
        }
    }
};

}  // namespace

// Runs of a footprint: per camera and row pair, consecutive set groups, gaps of up to `gap` groups bridged
// (a few more bytes for fewer, longer copies: the AsyncMultiMapper's host copies bridge kRunGap).  A cell (row
// pair r, group g) is the same pixels in every input layout, and with an even width a run's NV12 chroma row (yb
// bytes at byte 8 g0) is as long as its planar U and V rows together (2 cb): offsets and sizes hold for both
// 4:2:0 layouts (a converted layout has its own offsets, frame_layout.hpp run_table).
std::vector<FootRun> footprint_runs(const SourceFootprint& f, size_t& bytes, int gap) {
    std::vector<FootRun> runs;
    bytes = 0;
    for (int i = 0; i < (int)f.w.size(); i++)
        for (int r = 0; r < f.row_pairs(i); r++) {
            int g = 0;
            const int G = f.groups(i);
            while (g < G) {
                if (!f.test(i, r, g)) {
                    g++;
                    continue;
                }
                int e = g + 1, last = g;  // last set group of the run
                while (e < G && e - last <= gap + 1) {
                    if (f.test(i, r, e)) last = e;
                    e++;
                }
                const int ng = last - g + 1;
                const int yb = std::min(8 * (g + ng), f.w[i]) - 8 * g;
                const int cb = std::max(0, std::min(4 * (g + ng), f.w[i] / 2) - 4 * g);
                runs.push_back(FootRun{(uint32_t)i | (uint32_t)r << 8, (uint32_t)g, (uint32_t)ng, (uint32_t)bytes});
                bytes += (size_t)(2 * yb + 2 * cb);
                g = last + 1;
            }
        }
    return runs;
}

// The stitch of a converted side runs on NV12 frames of the frame slot: NV12 because a packed or U,V group's
// chroma is already U,V pairs (one 8-byte chroma store per group in, one 8-byte chroma load per chunk out, no
// split into a U and a V half), and because every layout in and out then takes the composite's compiled-in NV12
// instance.  The layouts share the frames, the table and the runs; only the two launches' format differs.
void mapper_set_conv(octvr_mapper* m, int in_fmt, int out_fmt) {
    const bool in = in_fmt != 0, out = out_fmt != 0;
    m->conv_fmt_in = in_fmt;  // the slot frames depend on the sides being converted only, not on the layout
    m->conv_fmt_out = out_fmt;
    if (in == m->conv_in && out == m->conv_out) return;
    DeviceGuard dg(m->device);
    if (in && !m->conv_table.p) {
        // every source read of the mapper lies in its footprint (host_common.hpp SourceFootprint: the staged
        // groups, the wide tiles', the multi-band remap's, the overlays' and the gain samples' taps, in either
        // sampling convention; the gathered preview's taps are the composite's) — what the AsyncMultiMapper's
        // footprint upload already relies on — so the unpack converts exactly these runs
        size_t bytes420 = 0;
        // no gaps bridged: a lane converts one group, a bridged group would only be more bytes
        const std::vector<FootRun> runs = footprint_runs(m->foot, bytes420, 0);
        m->conv_foot_runs = runs;
        // the pieces are the same in every layout; the offsets (4 bytes per pixel here) are not read
        size_t bytes4 = 0;
        const std::vector<FootRun> table = run_table(LayoutUyvy::desc, runs, m->in_w, bytes4);
        REQUIRE(bytes4 < ((size_t)1 << 32) && table.size() < 0x7FFFFFFFu, "input footprint exceeds 4 GiB");
        m->conv_in_px = bytes4 / 4;
        m->conv_in_v210 = 0;
        for (const FootRun& r : runs) m->conv_in_v210 += kLayoutV210.run_bytes(m->in_w[r.cam & 31u], (int)r.g0, (int)r.ng);
        m->conv_runs = runs.size();
        m->conv_table.upload(table.data(), table.size());
    }
    m->conv_in = in;
    m->conv_out = out;
    for (size_t k = 0; k < m->slots.size(); k++) slot_conv(*m, *m->slot_bufs[k], m->slots[k]);
    HIP_CHECK(hipDeviceSynchronize());  // the memsets complete before any stream uses the frames
}

// Mapper::stitch (mapper.cpp:193-323).  gains_dev (device, n doubles): gains of another mapper of the
// same inputs, copied stream-ordered (AsyncMultiMapper's gain_modes chaining, async.cpp:78-86).
void mapper_stitch(octvr_mapper* m, const uint8_t* const* in_dev, const size_t* in_pitch, uint8_t* out_dev,
                   size_t out_pitch, const double* gains, int n_gains, const double* gains_dev, hipStream_t s,
                   const PreviewOut* preview, const octvr_tensor_out* tensor) {
    REQUIRE(m && in_dev && in_pitch && (out_dev || tensor) && !(preview && tensor), "NULL argument");
    // a preview of the prepared size is gathered from the source frames after the composite (preview.hip):
    // the stitch itself is the one without a preview
    const bool gathered = preview && m->pv.view.dw > 0 && preview->w == m->pv.view.dw && preview->h == m->pv.view.dh;
    if (preview) {
        REQUIRE(preview->dev && preview->w > 0 && preview->h > 0 && preview->pitch >= (size_t)preview->w * 3,
                "bad preview output");
        if (!gathered) {
            // the preview resizes the whole-frame RGB result, which one frame slot owns
            REQUIRE(m->slots.size() == 1, "preview output needs one frame in flight");
            ensure_result(*m);
        }
    }
    // a tensor is chosen as a preview is: of the prepared size it is gathered from the source frames
    // (tensor_out.hip), of any other it is resized from the result frame
    TensorPlanes tp;
    const bool tensor_gathered = tensor && m->pv.view.dw > 0 && tensor->w == m->pv.view.dw && tensor->h == m->pv.view.dh;
    if (tensor) {
        tp = check_tensor(tensor);
        if (!tensor_gathered) {
            REQUIRE(m->slots.size() == 1, "tensor output needs one frame in flight");
            ensure_result(*m);
        }
    }
    if (out_dev) check_out_frame(m, out_dev, out_pitch);
    DeviceGuard dg(m->device);
    // converted sides: the slot's unpack launch fills its NV12 input frames, which every stage below reads,
    // and the stitch writes the slot's NV12 output frame, which the pack launch converts at the end
    ConvSources us;
    FrameSet fs;
    if (m->conv_in)
        us = conv_sources(m, in_dev, in_pitch);
    else
        fs = frame_set(m, in_dev, in_pitch);
    REQUIRE(!m->use_gain || gains_dev || !gains || n_gains == m->n, "gains must have one entry per input");
    octvr_mapper::FrameSlot& sl = take_slot(m, s);
    TimedPair ev(m);
    hipEvent_t e0 = ev.e0, e1 = ev.e1;
    const bool timed = e0 != nullptr;
    // the events bracket the conversions too
    const bool outer = m->scaled || m->mb || preview || tensor || m->conv_in || m->conv_out;
    if (m->conv_in) {
        if (timed) HIP_CHECK(hipEventRecord(e0, s));
        fs = conv_unpack_slot(m, sl, us, s);
    }
    stitch_gains(m, sl, fs, gains, gains_dev, s);
    uint8_t* const caller_out = out_dev;
    const size_t caller_pitch = out_pitch;
    const bool pack = m->conv_out && out_dev;
    if (pack) {
        out_dev = sl.conv_out;
        out_pitch = (size_t)m->SW;
    }
    // overlays after a blend are copied onto the RGB(A) result too (mapper.cpp:279-287)
    const bool overlays = m->ov.view.n_groups > 0;
    if (timed && outer && !m->conv_in) HIP_CHECK(hipEventRecord(e0, s));  // else the composite records its own
    if (m->scaled || (preview && !gathered) || (tensor && !tensor_gathered) || overlays) {
        // stitch at template size into the RGB(A) result, then resize + RGB -> YUV420P (mapper.cpp:290-306)
        // (one frame slot only: the result frame is shared); without scaling the resize is the identity
        if (m->mb)
            multiband_run(*m->mb, 0, fs, sl.gains, m->use_gain, nullptr, 0, s, m->result.p, (int64_t)m->W * 4, m->pix);
        else
            HIP_CHECK(launch_mb_remap(fs, m->tiles.view, sl.gains, m->use_gain,
                                      RgbaOut{m->result.p, (uint32_t)m->result.n, m->result_view.p}, s, m->pix));
        if (overlays) HIP_CHECK(launch_overlay_apply(fs, m->ov.view, m->result.p, (int64_t)m->W * 4, s, m->pix));
        if (out_dev)
            HIP_CHECK(launch_resize_rgba_yuv420(m->result.p, m->W, m->H, (int64_t)m->W * 4, out_dev, m->SW, m->SH,
                                                (int64_t)out_pitch, s, (m->pix & kPixOutNv12) != 0));
        if (tensor) {  // never the gathered one: a prepared size needs blend 0, no scaling and no overlay pass
            HIP_CHECK(launch_tensor_resize(m->result.p, m->W, m->H, (int64_t)m->W * 4, tp, s));
            m->tensor_resized++;
        }
        if (preview)  // cuda::resize(result, preview_output, ...) (mapper.cpp:308-312)
            HIP_CHECK(launch_resize_rgba_rgb(m->result.p, m->W, m->H, (int64_t)m->W * 4, preview->dev, preview->w,
                                             preview->h, (int64_t)preview->pitch, s));
    } else if (m->mb) {
        multiband_run(*m->mb, m->cur_slot, fs, sl.gains, m->use_gain, out_dev, (int64_t)out_pitch, s, nullptr, 0, m->pix);
    } else {
        TiledLut view = m->tiles.view;
        view.queue = sl.queue;
        // with a gathered preview the events above and below bracket the composite and the preview kernel
        if (out_dev)  // a gathered tensor alone reads the source frames itself: no composite
            HIP_CHECK(launch_stitch(fs, view, m->W, m->H, sl.gains, m->use_gain, out_dev, (int64_t)out_pitch, s,
                                    outer ? nullptr : e0, outer ? nullptr : e1, m->pix));
        if (tensor_gathered) {
            HIP_CHECK(launch_tensor_gather(fs, m->pv.view, sl.gains, m->use_gain, tp, s, m->pix));
            m->tensor_gathered++;
            if (!out_dev) m->tensor_no_composite++;
        }
        if (gathered)
            HIP_CHECK(launch_preview_gather(fs, m->pv.view, sl.gains, m->use_gain, preview->dev, (int64_t)preview->pitch, s,
                                            m->pix));
    }
    if (pack) conv_pack(m, sl.conv_out, caller_out, caller_pitch, s);
    if (timed && outer) HIP_CHECK(hipEventRecord(e1, s));
    ev.keep();
    finish_slot(sl, s);
}

// nb frames (1, 2 or 4) of the same rig in one composite launch (FrameBatch, kernels.hpp): each frame's
// gains into its own frame slot (nb consecutive slots, each waited for as mapper_stitch waits for one),
// then one pass over the tiled LUT for all of them.  Scaled-output and multi-band / feather mappers have no
// batched kernel: their frames are stitched one by one.
void mapper_stitch_batch(octvr_mapper* m, int nb, const uint8_t* const* in_dev, const size_t* in_pitch,
                         uint8_t* const* out_dev, size_t out_pitch, const double* gains, hipStream_t s) {
    REQUIRE(m && in_dev && in_pitch && out_dev, "NULL argument");
    REQUIRE(nb == 1 || nb == 2 || nb == 4, "a batch holds 1, 2 or 4 frames");
    for (int f = 0; f < nb; f++) REQUIRE(out_dev[f], "NULL output");
    if (nb == 1 || m->scaled || m->mb) {
        for (int f = 0; f < nb; f++)
            mapper_stitch(m, in_dev + (size_t)f * m->nc, in_pitch + (size_t)f * m->nc, out_dev[f], out_pitch,
                          gains ? gains + (size_t)f * m->n : nullptr, gains ? m->n : 0, nullptr, s);
        return;
    }
    REQUIRE((int)m->slots.size() >= nb, "a batch of n frames needs n frames in flight (octvr_mapper_set_frames_in_flight)");
    REQUIRE(nb <= 2 || m->nc <= 16, "a batch of 4 frames holds 16 cameras per frame (inputs and overlays)");
    for (int f = 0; f < nb; f++) check_out_frame(m, out_dev[f], out_pitch);
    DeviceGuard dg(m->device);
    FrameSet fs[kMaxBatch];  // every frame checked before any of them puts work on the stream
    ConvSources us[kMaxBatch];
    for (int f = 0; f < nb; f++) {
        if (m->conv_in)
            us[f] = conv_sources(m, in_dev + (size_t)f * m->nc, in_pitch + (size_t)f * m->nc);
        else
            fs[f] = frame_set(m, in_dev + (size_t)f * m->nc, in_pitch + (size_t)f * m->nc);
    }
    const double* g[kMaxBatch];
    octvr_mapper::FrameSlot* sl[kMaxBatch];
    const bool feed = m->use_gain && !gains && m->n_chunks > 0;  // every frame's gains estimated: one feed launch
    unsigned long long* tot[kMaxBatch];
    uint32_t* tick[kMaxBatch];
    double* gd[kMaxBatch];
    TimedPair ev(m);
    const bool outer = ev.e0 && (m->conv_in || m->conv_out);  // the events bracket the conversions too
    uint8_t* out[kMaxBatch];
    for (int f = 0; f < nb; f++) {
        sl[f] = &take_slot(m, s);
        if (f == 0 && outer) HIP_CHECK(hipEventRecord(ev.e0, s));
        if (m->conv_in) fs[f] = conv_unpack_slot(m, *sl[f], us[f], s);  // each frame converted in its own slot
        out[f] = m->conv_out ? sl[f]->conv_out : out_dev[f];
        if (!feed) stitch_gains(m, *sl[f], fs[f], gains ? gains + (size_t)f * m->n : nullptr, nullptr, s);
        g[f] = sl[f]->gains;
        tot[f] = sl[f]->totals;
        tick[f] = sl[f]->tickets;
        gd[f] = sl[f]->gains;
    }
    if (feed)  // GainCompensatorGPU::feed of each frame (exposure_compensate.cpp:223-297), all in one launch
        HIP_CHECK(launch_gain_feed_batch(fs, nb, m->samples.p, m->partners.p, m->tex, m->n_chunks, m->N.p, m->n, tot, tick,
                                         gd, s, true, m->pix));
    TiledLut view = m->tiles.view;
    view.queue = sl[0]->queue;  // this launch's work counters (the first frame's slot)
    HIP_CHECK(launch_stitch_batch(fs, nb, view, m->W, m->H, g, m->use_gain, out, (int64_t)(m->conv_out ? (size_t)m->SW : out_pitch),
                                  s, outer ? nullptr : ev.e0, outer ? nullptr : ev.e1, m->pix));
    for (int f = 0; f < nb && m->conv_out; f++) conv_pack(m, sl[f]->conv_out, out_dev[f], out_pitch, s);
    if (outer) HIP_CHECK(hipEventRecord(ev.e1, s));
    ev.keep();
    for (int f = 0; f < nb; f++) finish_slot(*sl[f], s);
}

int mapper_num_inputs(const octvr_mapper* m) { return m->n; }
bool mapper_has_gain(const octvr_mapper* m) { return m->use_gain != 0; }
const double* mapper_gains_dev(const octvr_mapper* m) { return m->slots[m->cur_slot].gains; }
const SourceFootprint& mapper_footprint(const octvr_mapper* m) { return m->foot; }
void mapper_out_size(const octvr_mapper* m, int* w, int* h) {
    *w = m->SW;
    *h = m->SH;
}

SourceFrame checked_source_frame(const uint8_t* ptr, size_t pitch, int w, int h, const float* vig) {
    REQUIRE(ptr && pitch >= (size_t)w, "bad input frame");
    // the staging loads form row offsets with 24-bit multiplies (composite.hip stage_load)
    REQUIRE(pitch < ((size_t)1 << 24), "input pitch must be below 16 MiB");
    // the gain feed reads frames through 32-bit buffer resources
    REQUIRE((uint64_t)pitch * (uint64_t)(h + h / 2) < 0x7FFFFFFFull, "input frame larger than 2 GiB");
    // ... in 8-byte segments (gain_feed.hip feed_taps_issue)
    REQUIRE((uint64_t)pitch * (uint64_t)(h + h / 2) >= 8, "input frame below 8 bytes");
    return SourceFrame{ptr, w, h, (int64_t)pitch, vig};
}

TiledLutBuild build_frame_tiles(const std::vector<CompositeEntry>& lut, int W, int H, const std::vector<int>& in_w,
                                const std::vector<int>& in_h, int* n_jobs) {
    // items of 128 x 16 (two quads per lane, OCTVR_QPL) for the per-frame composite
    const int qpl = composite_qpl();
    const int tx_n = (W + kTileW - 1) / kTileW, ty_n = (H + kTileH * qpl - 1) / (kTileH * qpl);
    std::vector<TileJob> jobs;
    jobs.reserve((size_t)tx_n * ty_n);
    for (int ty = 0; ty < ty_n; ty++)
        for (int tx = 0; tx < tx_n; tx++) jobs.push_back(TileJob{tx, ty, 0});
    if (n_jobs) *n_jobs = tx_n * ty_n;
    // build_tiled_lut checks that every tap of every pixel lies in a staged group of its slot
    return build_tiled_lut(jobs, [&](int, int x, int y) {
        return (x < W && y < H) ? lut[(size_t)y * W + x] : CompositeEntry{0u, 0u};
    }, in_w, in_h, qpl);
}

std::unique_ptr<octvr_mapper> mapper_create(const octvr_rig* rig, int device, int n_inputs, const int* in_w,
                                            const int* in_h, int blend, int enable_gain, int scale_w, int scale_h,
                                            int flags) {
    REQUIRE(rig && in_w && in_h, "NULL argument");
    REQUIRE((flags & ~OCTVR_REMAP_TEXTURE) == 0, "unknown mapper flags");
    // the frames of a stitch: every input, then every overlay (mapper.cpp:208, inputs.size() == masks.size())
    const int n_in = (int)rig->inputs.size(), n_ov = (int)rig->overlays.size();
    REQUIRE(n_in + n_ov <= kMaxCams, "too many inputs and overlays");
    REQUIRE(n_inputs == n_in + n_ov, n_ov ? "in_sizes must cover every input and every overlay (N + K)"
                                          : "in_sizes must cover every input");
    REQUIRE(scale_w >= 0 && scale_h >= 0 && (scale_w == 0) == (scale_h == 0), "bad scaled output size");
    REQUIRE(rig->out_w % 2 == 0 && rig->out_h % 2 == 0, "YUV420 output needs even width/height");
    auto m = std::make_unique<octvr_mapper>();
    m->device = device;
    m->tex = (flags & OCTVR_REMAP_TEXTURE) ? 1 : 0;
    m->n = n_in;
    m->nc = n_in + n_ov;
    m->W = rig->out_w;
    m->H = rig->out_h;
    // scaled_output_size = scale_output.area() == 0 ? mt.out_size : scale_output (mapper.cpp:69)
    m->SW = scale_w ? scale_w : m->W;
    m->SH = scale_h ? scale_h : m->H;
    REQUIRE(m->SW % 2 == 0 && m->SH % 2 == 0, "YUV420 output needs even width/height");
    m->scaled = m->SW != m->W || m->SH != m->H;
    REQUIRE(!m->scaled || (uint64_t)m->W * m->H * 4 < 0x7FFFFF80ull, "stitch frame larger than 2 GiB as RGBA");
    m->in_w.assign(in_w, in_w + n_inputs);
    m->in_h.assign(in_h, in_h + n_inputs);
    for (int i = 0; i < m->nc; i++)
        REQUIRE(m->in_w[i] > 0 && m->in_h[i] > 0 && m->in_w[i] % 2 == 0 && m->in_h[i] % 2 == 0 &&
                    m->in_w[i] <= 65535 && m->in_h[i] <= 65535,
                "input and overlay sizes must be even and < 65536");
    // mapper.cpp:78-82: a single input disables gain (and blend), whatever overlays it has
    m->use_gain = (enable_gain && m->n > 1) ? 1 : 0;
    m->blend = m->n > 1 ? blend : 0;
    REQUIRE(!m->use_gain || m->n <= 16, "gain estimation supports at most 16 inputs");
    DeviceGuard dg(device);
    // camera i of the stitch: input i, or overlay i - N
    auto camera = [&](int i) -> const RigInput& { return i < n_in ? rig->inputs[i] : rig->overlays[i - n_in]; };
    // vignette: cv::cuda::resize(vignette, vignette_maps[i], in_size) (mapper.cpp:108-112), applied to
    // every source pixel before the remap (mapper.cpp:230-231), overlays included
    m->vig.resize(m->nc);
    for (int i = 0; i < m->nc; i++) {
        const RigInput& in = camera(i);
        m->rois.insert(m->rois.end(), in.roi, in.roi + 4);
        if (in.vignette.empty()) continue;
        const std::vector<float> v = resize_linear_f32(in.vignette.data(), in.vig_w, in.vig_h, m->in_w[i], m->in_h[i]);
        m->vig[i].upload(v.data(), v.size());
    }
    m->foot.init(m->in_w, m->in_h);
    if (m->blend > 0) {
        // MultiBandGPUBlender(seam_masks, rois, bands), bands = ceil(log2(blend)) - 1 (mapper.cpp:171-176)
        const int bands = (int)(std::ceil(std::log((double)m->blend) / std::log(2.)) - 1.);
        m->mb.reset(multiband_create(*rig, device, bands, m->in_w, m->in_h, 0, &m->foot, m->tex));
    } else if (m->blend < 0) {
        // FeatherGPUBlender(masks, rois, border = -blend) (mapper.cpp:177-182)
        m->mb.reset(multiband_create(*rig, device, 0, m->in_w, m->in_h, -m->blend, &m->foot, m->tex));
    } else {
        // per-camera templates -> device, composite LUT, then drop the per-camera maps.  The overlays are the
        // last cameras of the copy chain (mapper.cpp:279-287 after :268-277), so they win their pixels in the
        // same LUT and the stitch does no extra work for them; their gain stays the slot's constant 1
        // (make_slot), and sat_u8(px * 1.0f) = px.
        const std::vector<CompositeEntry> lut8 = winner_lut(*m, camera, 0, m->nc);
        const TiledLutBuild tb = build_frame_tiles(lut8, m->W, m->H, m->in_w, m->in_h, &m->n_tiles);
        footprint_add_tiles(m->foot, tb);
        m->tiles.upload(tb, false, true);  // quad records for the items that qualify
    }
    if (m->mb && n_ov) setup_overlays(*m, camera);
    if (m->scaled || m->ov.view.n_groups) ensure_result(*m);
    m->last_gains.assign(m->n, 1.0);
    if (m->use_gain) setup_gain(*m, *rig);
    m->slots.push_back(make_slot(*m));
    HIP_CHECK(hipDeviceSynchronize());  // the slot's memsets complete before any stream uses it
    return m;
}

void mapper_sync(octvr_mapper& m) {
    for (auto& sl : m.slots)
        if (sl.done) HIP_CHECK(hipEventSynchronize(sl.done));
}

void mapper_set_frames_in_flight(octvr_mapper* m, int k) {
    REQUIRE(m && k >= 1 && k <= OCTVR_MAX_FRAMES_IN_FLIGHT, "frames in flight must be 1..OCTVR_MAX_FRAMES_IN_FLIGHT");
    if (k > 1 && m->scaled)
        throw OctvrError(OCTVR_E_UNSUPPORTED, "frames in flight > 1 need the output at template size (no scaled output)");
    if (k > 1 && m->ov.view.n_groups)  // the overlays are copied onto the one result frame
        throw OctvrError(OCTVR_E_UNSUPPORTED, "frames in flight > 1 with overlays need blend 0 (no multi-band or feather)");
    DeviceGuard dg(m->device);
    mapper_sync(*m);
    if (m->cur_slot != 0) {  // keep the last frame's gains for gains() / chaining
        HIP_CHECK(hipMemcpy(m->slots[0].gains, m->slots[m->cur_slot].gains, sizeof(double) * m->n,
                            hipMemcpyDeviceToDevice));
        m->cur_slot = 0;
    }
    for (size_t i = 1; i < m->slots.size(); i++)
        if (m->slots[i].done) (void)hipEventDestroy(m->slots[i].done);
    m->slots.resize(1);
    m->slot_bufs.resize(1);
    for (int i = 1; i < k; i++) m->slots.push_back(make_slot(*m));
    if (m->mb) multiband_set_slots(*m->mb, k);
    HIP_CHECK(hipDeviceSynchronize());  // the memsets complete before any stream uses the slots
}

void mapper_prepare_preview(octvr_mapper* m, const octvr_rig* rig, int w, int h) {
    REQUIRE(m && w >= 0 && h >= 0 && (w == 0) == (h == 0), "bad arguments");
    // the blender's result is not a function of one camera's taps, and a scaled mapper stitches through the
    // result frame whatever its preview
    if (m->mb)
        throw OctvrError(OCTVR_E_UNSUPPORTED, "a prepared preview needs blend 0: a blended pixel is not a function of one "
                                              "camera's taps (multi-band / feather mappers preview from the result frame)");
    if (m->scaled)
        throw OctvrError(OCTVR_E_UNSUPPORTED, "a prepared preview needs the output at template size: a scaled mapper "
                                              "stitches through the result frame anyway");
    DeviceGuard dg(m->device);
    mapper_sync(*m);  // stitches in flight read the list they were issued with
    if (w == 0) {
        m->pv.entries.reset();
        m->pv.view = PreviewList{};
        return;
    }
    // 4 entries per pixel: the entry index stays below 2^28 and the list below 2 GiB
    REQUIRE((uint64_t)w * (uint64_t)h <= (uint64_t)OCTVR_MAX_PREPARED_PREVIEW_PIXELS,
            "preview larger than OCTVR_MAX_PREPARED_PREVIEW_PIXELS");
    REQUIRE(rig, "NULL rig");
    const int n_in = (int)rig->inputs.size(), n_ov = (int)rig->overlays.size();
    REQUIRE(rig->out_w == m->W && rig->out_h == m->H && n_in == m->n && n_in + n_ov == m->nc,
            "the rig is not the one the mapper was created from (output size, inputs or overlays differ)");
    auto camera = [&](int i) -> const RigInput& { return i < n_in ? rig->inputs[i] : rig->overlays[i - n_in]; };
    for (int i = 0; i < m->nc; i++) {
        const RigInput& in = camera(i);
        REQUIRE(std::equal(in.roi, in.roi + 4, m->rois.begin() + 4 * i),
                "the rig is not the one the mapper was created from (an ROI differs)");
        const size_t k = (size_t)in.roi[2] * in.roi[3];
        REQUIRE(in.map1.size() == k && in.map2.size() == k && in.mask.size() == k, "rig maps do not match their ROI");
    }
    // the composite's own winner LUT again (the mapper dropped its per-camera maps), cut down to the result
    // pixels the resize reads: every tap of the list is a tap of the composite's entry for that pixel, so
    // the footprint stays as it is (tests/cpp/preview_list_check.cpp)
    const std::vector<CompositeEntry> lut8 = winner_lut(*m, camera, 0, m->nc);
    const PreviewListBuild<CompositeEntry> b = build_preview_list(lut8, m->W, m->H, w, h, kPvBlockEntries);
    REQUIRE(b.pixels == (size_t)w * h && !b.entries.empty(), "preview size not representable");
    m->pv.view = PreviewList{};
    m->pv.entries.upload(b.entries.data(), b.entries.size());
    m->pv.view = PreviewList{m->pv.entries.p, (uint32_t)b.entries.size(), (uint32_t)b.pixels, w, h, b.fx, b.fy};
}

void mapper_set_timing(octvr_mapper* m, int enable) {
    REQUIRE(m && enable >= 0, "bad arguments");
    m->timing = enable;
    m->timed_calls = 0;
    if (enable) {
        // the event pairs of the next timed stitches created now, not inside the caller's timed region
        // (hipEventCreate there cost the 20-step bench region ~20 us of host time per step)
        DeviceGuard dg(m->device);
        constexpr size_t kEventReserve = 1024;
        while (m->free_events.size() + m->events.size() < kEventReserve) {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            HIP_CHECK(hipEventCreate(&e0));
            const hipError_t e = hipEventCreate(&e1);
            if (e != hipSuccess) (void)hipEventDestroy(e0);
            HIP_CHECK(e);
            m->free_events.emplace_back(e0, e1);
        }
    }
}

int mapper_drain_timing(octvr_mapper* m, const std::function<void(double, double)>& f) {
    DeviceGuard dg(m->device);
    for (auto& e : m->events) {
        HIP_CHECK(hipEventSynchronize(e.second));
        float start = 0, len = 0;
        HIP_CHECK(hipEventElapsedTime(&start, m->events[0].first, e.first));
        HIP_CHECK(hipEventElapsedTime(&len, e.first, e.second));
        f((double)start, (double)start + (double)len);
    }
    const int launches = (int)m->events.size();
    m->free_events.insert(m->free_events.end(), m->events.begin(), m->events.end());
    m->events.clear();
    return launches;
}

// The bytes of the tiled LUT one pass of the composite reads: 4 B entries (3 B packed, 2 B in the n_packed
// items of quad records, 8 B in wide tiles), tile headers / slots.
double tiled_lut_bytes(const TiledLut& t, int n_packed) {
    return (t.e24 ? 3.0 : 4.0) * t.n_items * kTilePx * t.qpl - 2.0 * n_packed * kTilePx * t.qpl + 8.0 * t.n_wide * kTilePx +
           (double)t.n_items * (sizeof(TileHdr) + kTileSlots * sizeof(TileSlot)) + 4.0 * t.n_wide;
}

double mapper_traffic(const octvr_mapper* m) {
    // composite kernel: 4 B tiled-LUT entry (8 B in wide tiles) + 1.5 B YUV420 output per output
    // pixel, the unique source bytes its staged boxes cover (YUV420P, 1.5 B per luma pixel: the
    // circular crops leave the rest of each frame unread), tile headers / slots.  Multi-band: the
    // sum over the sequence's launches (multiband_traffic_parts).
    // Overlays after a blend: the blend's result as RGBA written (by the blend, counted there as its YUV
    // output) and read back by the identity resize, the work list (4 B per group + 8 B per entry), the
    // unique source bytes under the overlays' taps and 4 B per covered pixel written.
    if (m->mb && m->ov.view.n_groups)
        return multiband_traffic(*m->mb) + 4.0 * m->W * m->H + 1.5 * m->SW * m->SH +
               (double)m->ov.view.n_groups * (4.0 + 8.0 * kOvGroupPx) + m->ov.source_bytes + 4.0 * (double)m->ov.covered;
    if (m->mb) return multiband_traffic(*m->mb);
    return tiled_lut_bytes(m->tiles.view, m->tiles.n_packed) + 1.5 * m->W * m->H + m->tiles.source_bytes;
}

}  // namespace octvr
