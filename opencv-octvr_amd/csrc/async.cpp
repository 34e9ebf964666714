// async.cpp — vr::AsyncMultiMapper (modules/octvr/src/async.cpp:32-350) on one device.
//
// Same five-stage pipeline as the reference — host planes -> pinned staging -> device upload ->
// stitch of every mapper -> device download -> pinned -> host output planes — over a ring of
// kSlots buffer sets, so consecutive frames overlap (frame k+2 is copied in while k+1 uploads and
// k is stitched).  Differences from the reference, all deliberate:
//   * one HIP stream per stage (upload, compute, download), never the legacy default stream;
//   * gain chaining (gain_modes[i] = j < i) copies mapper j's device gains on the compute stream
//     instead of round-tripping them through the host (async.cpp:78-86);
//   * worker threads are joinable and exit when the object is destroyed (the reference's five
//     threads loop forever and its destructor clears joinable std::threads, async.cpp:87-90,337-349);
//   * a failing frame carries its status to pop() instead of asserting;
//   * the two host-copy stages split their rows over a few helper threads (RowPool): one thread's
//     memcpy from pageable memory (~15 GB/s) otherwise bounds the whole pipeline (scripts/async_trace.py);
//   * only the input bytes some kernel of some mapper reads are copied and uploaded (the union of the
//     mappers' source footprints, host_common.hpp SourceFootprint), packed, and put in place on the
//     device by one kernel: with the copy chain each output pixel comes from one camera, so a C2 frame
//     needs ~18 MB of its 75 MB of YUV (the composite's staged groups plus the gain samples' row pairs,
//     DESIGN.md §6);
//   * output planes the caller registers once (octvr_async_register_output: a ring it reuses, as the
//     reference's own output Mats are reused, async.cpp:113-138) are page-locked and written by the D2H
//     copies directly, region by region (2-D copies at the caller's pitch): no pinned staging and no
//     copy-out for them; other planes take the staging path;
//   * the preview (async.cpp:73-110, 141-171) is published to a caller-read buffer and an optional sink
//     (octvr_async_pop_preview / octvr_async_set_preview_sink) instead of Qt shared memory, which stays
//     the caller's;
//   * the host planes may be NV12 on either side (octvr_async_set_pixel_formats): the mappers read and write
//     that layout themselves, and every stage here moves a Y plane and one U,V plane instead of three planes;
//   * frames that already live on the device skip the host stages (octvr_async_push_device): the mappers read
//     the caller's device frames in place and one kernel (async_merge.hip) places the region frames into the
//     caller's merged device frame; such frames travel the same queues, so pop order is push order;
//   * the inputs may be in a converted capture layout (frame_layout.hpp: packed UYVY 4:2:2, what capture cards
//     deliver, YUYV, YUV422P, NV16 and the 10-bit P010, YUV420P10, P210, YUV422P10): one kernel (frame_layout.hip)
//     converts the uploaded runs into the slot's NV12 device frames — once for all mappers, which stay on NV12
//     input; device frames are converted the same way from the caller's frames;
//   * the merged frame may be in a converted layout too (octvr_async_set_output_format): the mappers write NV12
//     region frames and one kernel (async_merge_pack.hip) merges and converts them in one pass, into the caller's
//     device frame or into the slot's own frame of that layout, whose region rectangles are then downloaded.
// Every input layout takes the same host path: a table of footprint runs with their places in the packed buffer
// (RunPlan: the native layouts' at 3 B per pixel of a run's row, a converted layout's run_table at 4, 6 or 8), one
// pack_run per run, one upload, one unpack launch.  Every output path places a region's pieces by one table
// (async_host.hpp region_pieces; a converted output layout's by region_rects).
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "abi_guard.hpp"
#include "async_host.hpp"
#include "frame_layout.hpp"
#include "mapper.hpp"

using namespace octvr;

namespace {

constexpr int kSlots = 3;  // BUF_SIZE (async.cpp:261)

template <class T>
class Channel {  // blocking FIFO; close() wakes every waiter, pop() then drains what is left
public:
    void push(T v) {
        {
            std::lock_guard<std::mutex> g(mu_);
            q_.push_back(std::move(v));
        }
        cv_.notify_one();
    }
    bool pop(T& out) {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        return true;
    }
    void close() {
        {
            std::lock_guard<std::mutex> g(mu_);
            closed_ = true;
        }
        cv_.notify_all();
    }

private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<T> q_;
    bool closed_ = false;
};

using Rect = PlaneRect;

// _rect_mul_size (async.cpp:20-30)
Rect rect_mul_size(const double* r, int W, int H) {
    Rect o{(int)std::round(r[0] * W), (int)std::round(r[1] * H), (int)std::round(r[2] * W), (int)std::round(r[3] * H)};
    if (o.x + o.w >= W) o.w = W - o.x;
    if (o.y + o.h >= H) o.h = H - o.y;
    return o;
}

struct PinnedBuf {
    uint8_t* p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    void alloc(size_t bytes) {
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault));
        n = bytes;
    }
};

struct Slot {  // one frame's buffers: the packed footprint runs, the device frames ("Y over [U|V]", or with NV12
              // "Y over U,V pairs"; pitch = width)
    std::unique_ptr<PinnedBuf> packed_host;
    DevBuf<uint8_t> packed_dev;
    DevBuf<uint8_t> preview_dev;  // preview_w x preview_h RGB, black outside the regions (async.cpp:314-316)
    std::unique_ptr<PinnedBuf> preview_host;
    std::vector<std::unique_ptr<PinnedBuf>> out_host;
    std::vector<DevBuf<uint8_t>> in_dev, out_dev;
    FootFrames frames{};
    // with a converted output layout (octvr_async_set_output_format): the merged frame of that layout, pitch = its
    // row bytes, which merge_pack_kernel fills for a host frame, and the pinned staging of its region rectangles
    std::unique_ptr<DevBuf<uint8_t>> conv_out_dev;
    std::unique_ptr<PinnedBuf> conv_out_host;
};

struct Job {
    std::vector<const uint8_t*> in_planes;
    std::vector<size_t> in_pitches;
    uint8_t* out_planes[3] = {nullptr, nullptr, nullptr};
    size_t out_pitches[3] = {0, 0, 0};
    bool direct = false;  // the output planes are registered: the D2H writes them, no copy-out
    // octvr_async_push_device: in_planes / in_pitches hold one device frame per input, the merged frame is
    // written on the device (no copy-in, upload, download or copy-out; the preview still comes down)
    bool device = false;
    uint8_t* out_dev = nullptr;
    size_t out_pitch = 0;
    hipEvent_t ready = nullptr;  // the compute stream waits for it before the first kernel (NULL: nothing)
    int slot = -1;
    int status = OCTVR_OK;
    std::string error;
};

// Helper threads of one host-copy stage: run(n, f) calls f(lo, hi) over n rows split into contiguous
// ranges, the calling thread taking the last one, and returns when all are done.  One run at a time
// (each stage owns its pool); f must not throw (memcpy only).
class RowPool {
public:
    explicit RowPool(int helpers) {
        for (int i = 0; i < helpers; i++) th_.emplace_back([this, i] { loop(i); });
    }
    ~RowPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    template <class F>
    void run(size_t n, F f) {
        const size_t T = th_.size() + 1;
        std::function<void(size_t, size_t)> fn = f;
        {
            std::lock_guard<std::mutex> g(mu_);
            job_ = &fn;
            n_ = n;
            left_ = th_.size();
            gen_++;
        }
        cv_.notify_all();
        fn(n * (T - 1) / T, n);
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [&] { return left_ == 0; });
        job_ = nullptr;
    }

private:
    void loop(int i) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(size_t, size_t)>* f;
            size_t n, T;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return quit_ || gen_ != seen; });
                if (quit_) return;
                seen = gen_;
                f = job_;
                n = n_;
                T = th_.size() + 1;
            }
            (*f)(n * (size_t)i / T, n * (size_t)(i + 1) / T);
            {
                std::lock_guard<std::mutex> g(mu_);
                if (--left_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t, size_t)>* job_ = nullptr;
    size_t n_ = 0, left_ = 0;
    uint64_t gen_ = 0;
    bool quit_ = false;
};
constexpr int kCopyHelpers = 5;  // per host-copy stage (the GPU box grants ~16 host threads per GPU)

template <class F>
void stage(Job& j, F&& f) {  // run a stage unless the frame already failed; record the first failure
    if (j.status != OCTVR_OK) return;
    try {
        f();
    } catch (const OctvrError& e) {
        j.status = e.code;
        j.error = e.what();
    } catch (const std::exception& e) {
        j.status = OCTVR_E_HIP;
        j.error = e.what();
    }
}

}  // namespace

struct octvr_async {
    int device = 0;
    int n_in = 0;
    int out_w = 0, out_h = 0;
    std::vector<int> in_w, in_h;
    std::vector<octvr_mapper*> mappers;
    std::vector<int> gain_modes;
    std::vector<Rect> regions, regions_uv;  // per mapper: its rectangle in the Y and in the U / V planes
    int flags = 0;
    // layouts of the host planes (octvr_async_set_pixel_formats); the mappers carry the same pair.  Written by
    // the caller's thread with no frame pending, read by the stages while a frame is
    int in_fmt = OCTVR_PIX_YUV420P, out_fmt = OCTVR_PIX_YUV420P;
    int out_planes_used() const { return layout_of(out_fmt).planes(); }
    // preview (async.cpp:73-76): preview_w x preview_h RGB; per mapper its rectangle (w or h <= 0: none)
    int preview_w = 0, preview_h = 0;
    std::vector<Rect> preview_rects;
    std::mutex pub_mu;  // the published preview, its header and the sink
    std::vector<uint8_t> pub;
    octvr_preview_header pub_hdr{0, 0, 0, 0.0};
    octvr_preview_sink sink = nullptr;
    void* sink_user = nullptr;
    // the sink runs outside pub_mu (it may call back into the preview API); a thread that replaces the sink
    // waits for a running call to return, unless it is that call itself
    bool sink_busy = false;
    std::thread::id sink_thread;
    std::condition_variable sink_idle;
    // fps over blocks of 10 frames, as the reference's copy-out thread keeps it (async.cpp:141-147): the
    // frame interval is measured from the previous frame's copy-out (the first from creation, fps_timer)
    std::chrono::steady_clock::time_point fps_t = std::chrono::steady_clock::now();
    int64_t frame_count = 0;
    double frame_total_ms = 0, frame_fps = 0;
    // What a frame uploads: the runs with their places in the packed buffers, the same table on the device for the
    // unpack launch, and the packed bytes.  native: what the mappers read of the inputs (footprint_runs), for both
    // 4:2:0 layouts; conv: the unpack kernel's pieces over the same runs (run_table), built when a converted format is
    // first set and again when conv_bpp changes.
    struct RunPlan {
        std::vector<FootRun> runs;
        DevBuf<FootRun> dev;
        size_t bytes = 0;
    };
    RunPlan native, conv;
    int conv_bpp = 0;  // LayoutDesc::run_key conv's offsets were built with: packed bytes per pixel of a piece's row (0: no table)
    bool in_conv() const { return converted_format(in_fmt); }
    const RunPlan& plan() const { return in_conv() ? conv : native; }
    // the unpack launch of a converted input format over its table, from the packed buffer or the caller's frames
    void conv_unpack(const ConvSources& src, const FootFrames& frames, hipStream_t s) {
        HIP_CHECK(launch_layout_unpack(in_fmt, conv.dev.p, (int)conv.runs.size(), src, frames, s));
    }
    // the input format's launch that puts a slot's uploaded runs in place in its device frames
    void unpack_packed(const Slot& sl, hipStream_t s) {
        if (!in_conv()) {
            HIP_CHECK(launch_unpack_runs_layout(sl.packed_dev.p, native.dev.p, (int)native.runs.size(), sl.frames,
                                                in_fmt == OCTVR_PIX_NV12, s));
            return;
        }
        ConvSources src;
        memset(&src, 0, sizeof src);
        src.packed = sl.packed_dev.p;
        conv_unpack(src, sl.frames, s);
    }
    Slot slots[kSlots];
    // output plane sets the caller registered (octvr_async_register_output): page-locked, downloaded into
    struct RegOut {
        uint8_t* p[3];
        size_t pitch[3];
        std::vector<PinRange> pinned;  // what hipHostRegister locked: the planes' ranges, merged (merge_pin_ranges)
        bool same(int np, uint8_t* const* planes, const size_t* pitches) const {  // pitches NULL: any
            for (int k = 0; k < np; k++)
                if (p[k] != planes[k] || (pitches && pitch[k] != pitches[k])) return false;
            return true;
        }
    };
    static void unpin(const RegOut& r) {
        for (const PinRange& g : r.pinned) (void)hipHostUnregister(reinterpret_cast<void*>(g.begin));
    }
    std::vector<RegOut> reg_out;  // caller thread only (register / push / destroy)
    hipStream_t up = nullptr, comp = nullptr, down = nullptr;
    Channel<std::shared_ptr<Job>> q_in, q_up, q_map, q_down, q_out, q_done;
    Channel<int> free_slots;
    std::vector<std::thread> threads;
    RowPool copy_in_pool{kCopyHelpers}, copy_out_pool{kCopyHelpers};
    int pending = 0;  // pushed, not popped (caller thread only)
    int64_t device_frames = 0;               // octvr_async_push_device calls that queued a frame (caller thread only)
    std::atomic<int64_t> merge_launches{0};  // merge_regions_kernel launches (compute thread)
    std::atomic<int64_t> merge_pack_launches{0};  // merge_pack_kernel launches (compute thread)
    // a converted output layout (octvr_async_set_output_format): out_fmt is that layout, the mappers write NV12
    bool out_conv() const { return converted_format(out_fmt); }
    size_t conv_out_pitch() const { return (size_t)layout_of(out_fmt).row_bytes(out_w); }
    LayoutRects rects(size_t k) const { return region_rects(layout_of(out_fmt), regions[k], out_w, out_h); }
    void free_conv_out() {
        for (auto& sl : slots) {
            sl.conv_out_dev.reset();
            sl.conv_out_host.reset();
        }
    }
    RegionPieces pieces(size_t k) const { return region_pieces(regions[k], regions_uv[k], out_fmt == OCTVR_PIX_NV12); }
    bool whole_frame_region() const {
        return regions.size() == 1 && regions[0].x == 0 && regions[0].y == 0 && regions[0].w == out_w && regions[0].h == out_h;
    }

    ~octvr_async() {
        q_in.close();
        for (auto& t : threads)
            if (t.joinable()) t.join();
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        for (const RegOut& r : reg_out) unpin(r);
        for (hipStream_t s : {up, comp, down})
            if (s) (void)hipStreamDestroy(s);
        for (auto& sl : slots) {
            sl.in_dev.clear();
            sl.out_dev.clear();
            sl.packed_dev.reset();
            sl.packed_host.reset();
            sl.preview_dev.reset();
            sl.preview_host.reset();
            sl.out_host.clear();
            sl.conv_out_dev.reset();
            sl.conv_out_host.reset();
        }
        for (auto* m : mappers) octvr_mapper_destroy(m);
        if (prev >= 0) (void)hipSetDevice(prev);
    }

    // run_copy_inputs_mat_to_hostmem (async.cpp:32-56), restricted to the mappers' source footprint: the
    // rows and columns no kernel of any mapper reads are neither copied nor uploaded
    void copy_in(Job& j) {
        int s = -1;
        if (!free_slots.pop(s)) throw OctvrError(OCTVR_E_INVALID, "pipeline closed");
        j.slot = s;
        if (j.device) return;  // the mappers read the caller's frames in place
        stage(j, [&] {
            uint8_t* const dst = slots[s].packed_host->p;
            const std::vector<FootRun>& runs = plan().runs;
            const LayoutDesc d = layout_of(in_fmt);
            copy_in_pool.run(runs.size(), [&](size_t lo, size_t hi) {
                for (size_t k = lo; k < hi; k++) {
                    const FootRun& r = runs[k];
                    const int i = (int)(r.cam & 31u);
                    pack_run(d, dst + r.off, in_w[i], (int)(r.cam >> 8), (int)r.g0, (int)r.ng, &j.in_planes[3 * i],
                             &j.in_pitches[3 * i]);
                }
            });
        });
    }

    // run_upload_inputs_hostmem_to_gpumat (async.cpp:58-68): the packed runs, then one kernel puts them in
    // place in the device frames (bytes outside the footprint keep whatever they held: nothing reads them)
    void upload(Job& j) {
        if (j.device) return;
        stage(j, [&] {
            DeviceGuard dg(device);
            Slot& sl = slots[j.slot];
            if (const size_t bytes = plan().bytes) {
                HIP_CHECK(hipMemcpyAsync(sl.packed_dev.p, sl.packed_host->p, bytes, hipMemcpyHostToDevice, up));
                unpack_packed(sl, up);
            }
            HIP_CHECK(hipStreamSynchronize(up));
        });
    }

    // run_do_mapping (async.cpp:70-91)
    void map(Job& j) {
        stage(j, [&] {
            DeviceGuard dg(device);
            Slot& sl = slots[j.slot];
            std::vector<const uint8_t*> in(n_in);
            std::vector<size_t> pitch(n_in);
            // device frames of a converted layout are converted into the slot's frames first, once for all mappers
            const bool own = !j.device || in_conv();
            for (int i = 0; i < n_in; i++) {
                in[i] = own ? sl.in_dev[i].p : j.in_planes[i];
                pitch[i] = own ? (size_t)in_w[i] : j.in_pitches[i];
            }
            if (j.device && j.ready) HIP_CHECK(hipStreamWaitEvent(comp, j.ready, 0));
            if (j.device && in_conv()) {
                ConvSources src;
                memset(&src, 0, sizeof src);
                for (int i = 0; i < n_in; i++) {
                    src.f[i] = j.in_planes[i];
                    src.pitch[i] = j.in_pitches[i];
                }
                conv_unpack(src, sl.frames, comp);
            }
            // a device frame's single region covering the whole output is stitched where it belongs
            const bool in_place = j.device && !out_conv() && whole_frame_region();
            for (size_t k = 0; k < mappers.size(); k++) {
                const int gm = gain_modes[k];
                const double* chained = nullptr;
                if (gm >= 0 && gm < (int)k && mapper_has_gain(mappers[gm])) chained = mapper_gains_dev(mappers[gm]);
                // preview_output(_rect_mul_size(output_regions[i], preview_output.size())) (async.cpp:75-76): the
                // region's view of the preview image (an empty view is no preview, mapper.cpp:308)
                PreviewOut pv{};
                const bool with_pv = preview_w > 0 && preview_rects[k].w > 0 && preview_rects[k].h > 0;
                if (with_pv) {
                    const Rect& r = preview_rects[k];
                    const size_t pp = (size_t)preview_w * 3;
                    pv = PreviewOut{sl.preview_dev.p + (size_t)r.y * pp + (size_t)r.x * 3, r.w, r.h, pp};
                }
                mapper_stitch(mappers[k], in.data(), pitch.data(), in_place ? j.out_dev : sl.out_dev[k].p,
                              in_place ? j.out_pitch : (size_t)regions[k].w, nullptr, 0, chained, comp,
                              with_pv ? &pv : nullptr);
            }
            if (out_conv()) {  // every NV12 region frame into the merged frame of the output layout, one launch
                std::vector<const uint8_t*> src;
                for (auto& b : sl.out_dev) src.push_back(b.p);
                MergePackTable t;
                REQUIRE(build_merge_pack_table(layout_of(out_fmt), regions.data(), regions_uv.data(), src.data(), (int)src.size(),
                                               out_w, out_h, j.device ? j.out_pitch : conv_out_pitch(), t),
                        "regions do not fit a merge launch");
                HIP_CHECK(launch_merge_pack(out_fmt, j.device ? j.out_dev : sl.conv_out_dev->p, t, comp));
                merge_pack_launches++;
            } else if (j.device && !in_place) {  // every region frame into its place in the merged frame, one launch
                std::vector<const uint8_t*> src;
                for (auto& b : sl.out_dev) src.push_back(b.p);
                MergeTable t;
                REQUIRE(build_merge_table(regions.data(), regions_uv.data(), src.data(), (int)src.size(), out_w, out_h,
                                          j.out_pitch, out_fmt == OCTVR_PIX_NV12, t),
                        "regions do not fit a merge launch");
                HIP_CHECK(launch_merge_regions(j.out_dev, t, comp));
                merge_launches++;
            }
            HIP_CHECK(hipStreamSynchronize(comp));
        });
    }

    // run_download_outputs_gpumat_to_hostmem (async.cpp:93-111)
    void download(Job& j) {
        stage(j, [&] {
            DeviceGuard dg(device);
            Slot& sl = slots[j.slot];
            for (size_t k = 0; k < mappers.size() && !j.device; k++) {
                if (out_conv()) {
                    // the region's rectangles of the slot's merged frame: into the caller's registered planes, or
                    // to the same place in the pinned staging
                    const size_t fp = conv_out_pitch();
                    const LayoutRects rc = rects(k);
                    for (int i = 0; i < rc.n; i++) {
                        const LayoutRect& p = rc.p[i];
                        const size_t at = p.fy * fp + p.fx;
                        uint8_t* const dst = j.direct ? j.out_planes[p.plane] + p.y * j.out_pitches[p.plane] + p.x
                                                      : sl.conv_out_host->p + at;
                        HIP_CHECK(hipMemcpy2DAsync(dst, j.direct ? j.out_pitches[p.plane] : fp, sl.conv_out_dev->p + at, fp, p.bytes,
                                                   p.rows, hipMemcpyDeviceToHost, down));
                    }
                    continue;
                }
                if (!j.direct) {
                    HIP_CHECK(hipMemcpyAsync(sl.out_host[k]->p, sl.out_dev[k].p, sl.out_host[k]->n, hipMemcpyDeviceToHost,
                                             down));
                    continue;
                }
                // straight into the caller's registered planes: the pieces of the device region frame, whose
                // pitch is the region's width
                const RegionPieces pc = pieces(k);
                for (int i = 0; i < pc.n; i++) {
                    const RegionPiece& p = pc.p[i];
                    HIP_CHECK(hipMemcpy2DAsync(j.out_planes[p.plane] + p.y * j.out_pitches[p.plane] + p.x, j.out_pitches[p.plane],
                                               sl.out_dev[k].p + p.src, (size_t)regions[k].w, p.bytes, p.rows,
                                               hipMemcpyDeviceToHost, down));
                }
            }
            if (preview_w > 0)  // async.cpp:102-103
                HIP_CHECK(hipMemcpyAsync(sl.preview_host->p, sl.preview_dev.p, sl.preview_host->n, hipMemcpyDeviceToHost,
                                         down));
            HIP_CHECK(hipStreamSynchronize(down));
        });
    }

    // run_copy_outputs_hostmem_to_mat (async.cpp:113-172)
    void copy_out(Job& j) {
        stage(j, [&] {
            if (j.direct || j.device) return;  // the D2H wrote the caller's planes / the frame stays on the device
            Slot& sl = slots[j.slot];
            for (size_t k = 0; k < mappers.size() && out_conv(); k++) {
                // the rows of the region's rectangles, plane after plane, split over the pool
                const size_t fp = conv_out_pitch();
                const LayoutRects rc = rects(k);
                size_t first[4] = {0, 0, 0, 0};
                for (int i = 0; i < rc.n; i++) first[i + 1] = first[i] + rc.p[i].rows;
                copy_out_pool.run(first[rc.n], [&](size_t lo, size_t hi) {
                    for (int i = 0; i < rc.n; i++) {
                        const LayoutRect& p = rc.p[i];
                        for (size_t y = std::max(lo, first[i]); y < std::min(hi, first[i + 1]); y++)
                            memcpy(j.out_planes[p.plane] + (p.y + y - first[i]) * j.out_pitches[p.plane] + p.x,
                                   sl.conv_out_host->p + (p.fy + y - first[i]) * fp + p.fx, p.bytes);
                    }
                });
            }
            for (size_t k = 0; k < mappers.size() && !out_conv(); k++) {
                const RegionPieces pc = pieces(k);
                const size_t w = (size_t)regions[k].w, luma_rows = pc.p[0].rows;
                const uint8_t* src = sl.out_host[k]->p;
                // the region's rows, luma then chroma, split over the pool: a chroma row is all chroma pieces' row
                copy_out_pool.run(luma_rows + pc.p[1].rows, [&](size_t lo, size_t hi) {
                    for (int i = 0; i < pc.n; i++) {
                        const RegionPiece& p = pc.p[i];
                        const size_t first = i ? luma_rows : 0;
                        for (size_t y = std::max(lo, first); y < std::min(hi, first + p.rows); y++)
                            memcpy(j.out_planes[p.plane] + (p.y + y - first) * j.out_pitches[p.plane] + p.x,
                                   src + p.src + (y - first) * w, p.bytes);
                    }
                });
            }
        });
        // frame_total_time += fps_timer.tick(); fps over every block of 10 frames (async.cpp:141-147)
        const auto now = std::chrono::steady_clock::now();
        frame_total_ms += std::chrono::duration<double, std::milli>(now - fps_t).count();
        fps_t = now;
        if (++frame_count == 10) {
            frame_fps = 1.0 / (frame_total_ms / (double)frame_count / 1000);
            frame_count = 0;
            frame_total_ms = 0;
        }
        // the preview with its PreviewDataHeader (async.cpp:149-171): published, then handed to the sink
        if (preview_w > 0 && j.status == OCTVR_OK) {
            const Slot& sl = slots[j.slot];
            const octvr_preview_header h{preview_w, preview_h, 0, frame_fps};
            octvr_preview_sink call = nullptr;
            void* user = nullptr;
            {
                std::lock_guard<std::mutex> g(pub_mu);
                memcpy(pub.data(), sl.preview_host->p, pub.size());
                pub_hdr = h;
                call = sink;
                user = sink_user;
                sink_busy = call != nullptr;
                sink_thread = std::this_thread::get_id();
            }
            // outside the lock: the sink may read the preview (octvr_async_pop_preview) or replace itself
            if (call) {
                call(user, sl.preview_host->p, (size_t)preview_w * 3, &h);
                {
                    std::lock_guard<std::mutex> g(pub_mu);
                    sink_busy = false;
                }
                sink_idle.notify_all();
            }
        }
    }

    template <class F>
    void worker(Channel<std::shared_ptr<Job>>& in, Channel<std::shared_ptr<Job>>& out, F f) {
        std::shared_ptr<Job> j;
        while (in.pop(j)) {
            f(*j);
            out.push(std::move(j));
        }
        out.close();
    }

    void start() {
        threads.emplace_back([this] {
            std::shared_ptr<Job> j;
            while (q_in.pop(j)) {
                try {
                    copy_in(*j);
                } catch (const OctvrError& e) {
                    j->status = e.code;
                    j->error = e.what();
                }
                q_up.push(std::move(j));
            }
            q_up.close();
        });
        threads.emplace_back([this] { worker(q_up, q_map, [this](Job& j) { upload(j); }); });
        threads.emplace_back([this] { worker(q_map, q_down, [this](Job& j) { map(j); }); });
        threads.emplace_back([this] { worker(q_down, q_out, [this](Job& j) { download(j); }); });
        threads.emplace_back([this] {
            std::shared_ptr<Job> j;
            while (q_out.pop(j)) {
                copy_out(*j);
                if (j->slot >= 0) free_slots.push(j->slot);
                q_done.push(std::move(j));
            }
            free_slots.close();
            q_done.close();
        });
    }
};

namespace {

// The host planes of a w-wide frame of the layout (frame_layout.hpp: planes(), plane_row_bytes) are there, wide
// enough and, for 16-bit samples, at even addresses and pitches; entries past the layout's planes are ignored.
template <class P>
bool planes_ok(const LayoutDesc& d, int w, P* const* planes, const size_t* pitches) {
    for (int k = 0; k < d.planes(); k++)
        if (!planes[k] || pitches[k] < (size_t)d.plane_row_bytes(k, w) || !d.aligned(planes[k], pitches[k])) return false;
    return true;
}
bool output_planes_ok(const octvr_async* a, uint8_t* const* planes, const size_t* pitches) {
    return planes_ok(layout_of(a->out_fmt), a->out_w, planes, pitches);
}

}  // namespace

extern "C" {

int octvr_async_create(const octvr_rig* const* rigs, int n_rigs, int device, int n_inputs, const int* in_w,
                       const int* in_h, int out_w, int out_h, const int* blend_modes, const int* gain_modes,
                       const double* output_regions, octvr_async** out) {
    return octvr_async_create_ex(rigs, n_rigs, device, n_inputs, in_w, in_h, out_w, out_h, blend_modes, gain_modes,
                                 output_regions, 0, out);
}

int octvr_async_create_ex(const octvr_rig* const* rigs, int n_rigs, int device, int n_inputs, const int* in_w,
                          const int* in_h, int out_w, int out_h, const int* blend_modes, const int* gain_modes,
                          const double* output_regions, int flags, octvr_async** out) {
    return octvr_async_create_preview(rigs, n_rigs, device, n_inputs, in_w, in_h, out_w, out_h, blend_modes, gain_modes,
                                      output_regions, flags, 0, 0, out);
}

int octvr_async_create_preview(const octvr_rig* const* rigs, int n_rigs, int device, int n_inputs, const int* in_w,
                               const int* in_h, int out_w, int out_h, const int* blend_modes, const int* gain_modes,
                               const double* output_regions, int flags, int preview_w, int preview_h,
                               octvr_async** out) {
    return guarded([&] {
        REQUIRE(rigs && n_rigs > 0 && in_w && in_h && blend_modes && gain_modes && output_regions && out,
                "NULL argument");
        REQUIRE(n_inputs > 0 && n_inputs <= kMaxCams && out_w > 0 && out_h > 0 && out_w % 2 == 0 && out_h % 2 == 0, "bad sizes");
        REQUIRE(preview_w >= 0 && preview_h >= 0 && (uint64_t)preview_w * (uint64_t)preview_h * 3 < 0x7FFFFF80ull,
                "bad preview size");
        auto a = std::make_unique<octvr_async>();
        a->device = device;
        a->flags = flags;
        // preview_size.area() > 0 enables the preview (async.cpp:99, 299)
        if ((int64_t)preview_w * preview_h > 0) {
            a->preview_w = preview_w;
            a->preview_h = preview_h;
            a->pub.assign((size_t)preview_w * preview_h * 3, 0);
        }
        a->n_in = n_inputs;
        a->out_w = out_w;
        a->out_h = out_h;
        a->in_w.assign(in_w, in_w + n_inputs);
        a->in_h.assign(in_h, in_h + n_inputs);
        a->gain_modes.assign(gain_modes, gain_modes + n_rigs);
        for (int i = 0; i < n_inputs; i++)
            REQUIRE(in_w[i] > 0 && in_h[i] > 0 && in_w[i] % 2 == 0 && in_h[i] % 2 == 0, "input sizes must be even");
        for (int k = 0; k < n_rigs; k++) {
            REQUIRE(rigs[k], "NULL rig");
            const Rect r = rect_mul_size(output_regions + 4 * k, out_w, out_h);
            const Rect c = rect_mul_size(output_regions + 4 * k, out_w / 2, out_h / 2);
            REQUIRE(r.x >= 0 && r.y >= 0 && r.w > 0 && r.h > 0 && r.w % 2 == 0 && r.h % 2 == 0,
                    "output region must be a non-empty even-sized rectangle inside the output");
            // the reference copies the mapper's U / V planes into the region of the output's U / V planes
            // (async.cpp:133-135); a size mismatch would reallocate the destination instead
            REQUIRE(c.w == r.w / 2 && c.h == r.h / 2, "output region's chroma rectangle is not half its luma rectangle");
            a->regions.push_back(r);
            a->regions_uv.push_back(c);
            a->preview_rects.push_back(a->preview_w ? rect_mul_size(output_regions + 4 * k, a->preview_w, a->preview_h)
                                                    : Rect{0, 0, 0, 0});
            octvr_mapper* m = nullptr;
            // Mapper(mts[i], in_sizes, blend_modes[i], gain_modes[i] >= 0, r.size()) (async.cpp:250-255)
            const int rc = octvr_mapper_create_ex(rigs[k], device, n_inputs, in_w, in_h, blend_modes[k],
                                                  gain_modes[k] >= 0 ? 1 : 0, r.w, r.h, flags, &m);
            if (rc != OCTVR_OK) throw OctvrError(rc, std::string("mapper ") + std::to_string(k) + ": " + octvr_last_error());
            a->mappers.push_back(m);
            // a blend-0 mapper whose region is at template size gathers its preview rectangle from the source
            // frames (octvr_mapper_prepare_preview); every other mapper previews from its result frame
            const Rect& pr = a->preview_rects.back();
            if (pr.w > 0 && pr.h > 0 && !m->mb && !m->scaled &&
                (uint64_t)pr.w * (uint64_t)pr.h <= (uint64_t)OCTVR_MAX_PREPARED_PREVIEW_PIXELS)
                mapper_prepare_preview(m, rigs[k], pr.w, pr.h);
            // n_inputs = N_k + K_k held for this rig (mapper_create); the split may differ per rig, but a
            // chained mapper takes the other's N gains
            const int gm = gain_modes[k];
            REQUIRE(gm < 0 || gm >= k || mapper_num_inputs(a->mappers[gm]) == mapper_num_inputs(m),
                    "gain_modes chains rigs with different numbers of inputs (overlays aside)");
        }
        DeviceGuard dg(device);
        HIP_CHECK(hipStreamCreateWithFlags(&a->up, hipStreamNonBlocking));
        HIP_CHECK(hipStreamCreateWithFlags(&a->comp, hipStreamNonBlocking));
        HIP_CHECK(hipStreamCreateWithFlags(&a->down, hipStreamNonBlocking));
        // what the mappers read of the inputs: one packed upload of those bytes per frame
        SourceFootprint foot;
        foot.init(a->in_w, a->in_h);
        for (auto* m : a->mappers) foot.merge(mapper_footprint(m));
        a->native.runs = footprint_runs(foot, a->native.bytes);
        REQUIRE(a->native.bytes < ((size_t)1 << 32), "input footprint exceeds 4 GiB");
        if (!a->native.runs.empty()) a->native.dev.upload(a->native.runs.data(), a->native.runs.size());
        for (auto& sl : a->slots) {
            sl.packed_host.reset(new PinnedBuf());
            sl.packed_host->alloc(std::max<size_t>(a->native.bytes, 1));
            sl.packed_dev.alloc(std::max<size_t>(a->native.bytes, 1));
            for (int i = 0; i < n_inputs; i++) {
                const size_t bytes = (size_t)in_w[i] * (in_h[i] / 2 * 3);
                sl.in_dev.emplace_back();
                sl.in_dev.back().alloc(bytes);
                // bytes outside the footprint are never read; a fixed pattern rather than stale memory
                HIP_CHECK(hipMemset(sl.in_dev.back().p, 0x5A, bytes));
                sl.frames.f[i] = sl.in_dev.back().p;
                sl.frames.w[i] = in_w[i];
                sl.frames.h[i] = in_h[i];
            }
            if (a->preview_w) {  // GpuMat(preview_size, CV_8UC3).setTo(0) + HostMem (async.cpp:299-305)
                const size_t pb = (size_t)a->preview_w * a->preview_h * 3;
                sl.preview_dev.alloc(pb);
                HIP_CHECK(hipMemset(sl.preview_dev.p, 0, pb));
                sl.preview_host.reset(new PinnedBuf());
                sl.preview_host->alloc(pb);
            }
            for (int k = 0; k < n_rigs; k++) {
                const size_t bytes = (size_t)a->regions[k].w * (a->regions[k].h / 2 * 3);
                sl.out_host.emplace_back(new PinnedBuf());
                sl.out_host.back()->alloc(bytes);
                sl.out_dev.emplace_back();
                sl.out_dev.back().alloc(bytes);
            }
        }
        for (int s = 0; s < kSlots; s++) a->free_slots.push(s);
        a->start();
        *out = a.release();
    }, OCTVR_E_HIP);
}

int octvr_async_push(octvr_async* a, const uint8_t* const* in_planes, const size_t* in_pitches,
                     uint8_t* const* out_planes, const size_t* out_pitches) {
    if (!a || !in_planes || !in_pitches || !out_planes || !out_pitches) {
        set_last_error("NULL argument");
        return OCTVR_E_INVALID;
    }
    auto j = std::make_shared<Job>();
    j->in_planes.assign(in_planes, in_planes + 3 * a->n_in);
    j->in_pitches.assign(in_pitches, in_pitches + 3 * a->n_in);
    for (int i = 0; i < a->n_in; i++)
        if (!planes_ok(layout_of(a->in_fmt), a->in_w[i], in_planes + 3 * i, in_pitches + 3 * i)) {
            set_last_error("bad input plane");
            return OCTVR_E_INVALID;
        }
    if (!output_planes_ok(a, out_planes, out_pitches)) {
        set_last_error("bad output plane");
        return OCTVR_E_INVALID;
    }
    const int np = a->out_planes_used();
    for (int k = 0; k < np; k++) {
        j->out_planes[k] = out_planes[k];
        j->out_pitches[k] = out_pitches[k];
    }
    for (const octvr_async::RegOut& r : a->reg_out) j->direct |= r.same(np, out_planes, out_pitches);
    a->q_in.push(std::move(j));
    a->pending++;
    return OCTVR_OK;
}

int octvr_async_push_device(octvr_async* a, const uint8_t* const* in_dev, const size_t* in_pitch, uint8_t* out_dev,
                            size_t out_pitch, void* ready_event) {
    return guarded([&] {
        REQUIRE(a && in_dev && in_pitch && out_dev, "NULL argument");
        // the mappers' own limit (mapper.cpp check_out_frame), and the merge's 32-bit offsets
        const char* why = frame_fault(layout_of(a->out_fmt), out_dev, out_pitch, a->out_w, a->out_h, 0x7FFFFF80ull);
        REQUIRE(!why, std::string("output ") + why);
        REQUIRE(a->whole_frame_region() || (int)a->regions.size() <= kMergeMaxRegions,
                "more regions than one merge launch takes");
        for (int i = 0; i < a->n_in; i++) {
            // the limits mapper_stitch sets (mapper.cpp conv_sources, checked_source_frame), refused here before
            // anything is queued
            why = frame_fault(layout_of(a->in_fmt), in_dev[i], in_pitch[i], a->in_w[i], a->in_h[i], 0x7FFFFFFFull);
            REQUIRE(!why, std::string("input ") + why);
            REQUIRE(a->in_conv() || in_pitch[i] < ((size_t)1 << 24), "input pitch must be below 16 MiB");
        }
        // a host pointer (pinned memory included: the kernels could read it, slowly) is refused before any launch
        DeviceGuard dg(a->device);
        auto on_device = [&](const void* p) {
            hipPointerAttribute_t at;
            memset(&at, 0, sizeof at);
            if (hipPointerGetAttributes(&at, p) != hipSuccess) {
                (void)hipGetLastError();
                return false;
            }
            return at.type == hipMemoryTypeDevice && at.device == a->device;
        };
        for (int i = 0; i < a->n_in; i++) REQUIRE(on_device(in_dev[i]), "input frame is not device memory of the pipeline's device");
        REQUIRE(on_device(out_dev), "output frame is not device memory of the pipeline's device");
        auto j = std::make_shared<Job>();
        j->device = true;
        j->in_planes.assign(in_dev, in_dev + a->n_in);
        j->in_pitches.assign(in_pitch, in_pitch + a->n_in);
        j->out_dev = out_dev;
        j->out_pitch = out_pitch;
        j->ready = static_cast<hipEvent_t>(ready_event);
        a->q_in.push(std::move(j));
        a->pending++;
        a->device_frames++;
    }, OCTVR_E_HIP);
}

int octvr_async_pop(octvr_async* a) {
    if (!a || a->pending <= 0) {
        set_last_error("no frame pending");
        return OCTVR_E_INVALID;
    }
    std::shared_ptr<Job> j;
    if (!a->q_done.pop(j)) {
        set_last_error("pipeline closed");
        return OCTVR_E_INVALID;
    }
    a->pending--;
    if (j->status != OCTVR_OK) set_last_error(j->error);
    return j->status;
}

int octvr_async_pending(const octvr_async* a, int* n) {
    if (!a || !n) {
        set_last_error("NULL argument");
        return OCTVR_E_INVALID;
    }
    *n = a->pending;
    return OCTVR_OK;
}

int octvr_async_register_output(octvr_async* a, uint8_t* const* planes, const size_t* pitches) {
    if (!a || !planes || !pitches) {
        set_last_error("NULL argument");
        return OCTVR_E_INVALID;
    }
    if (!output_planes_ok(a, planes, pitches)) {
        set_last_error("bad output plane");
        return OCTVR_E_INVALID;
    }
    const int np = a->out_planes_used();
    for (const octvr_async::RegOut& r : a->reg_out)
        if (r.same(np, planes, pitches)) return OCTVR_OK;  // already registered
    return guarded([&] {
        DeviceGuard dg(a->device);
        octvr_async::RegOut r{};
        // Planes of one allocation (a contiguous NV12 frame's Y and U,V; U and V as column halves of one
        // array) share pages or overlap: each page is locked once, through the merged range that holds it
        std::vector<PinRange> ranges;
        const LayoutDesc d = layout_of(a->out_fmt);
        for (int k = 0; k < np; k++) {
            const size_t rows = (size_t)d.plane_rows(k, a->out_h), w = (size_t)d.plane_row_bytes(k, a->out_w);
            const uintptr_t b = reinterpret_cast<uintptr_t>(planes[k]);
            ranges.push_back(PinRange{b, b + pitches[k] * (rows - 1) + w});
            r.p[k] = planes[k];
            r.pitch[k] = pitches[k];
        }
        const long page = sysconf(_SC_PAGESIZE);
        for (const PinRange& g : merge_pin_ranges(ranges, (uintptr_t)(page > 0 ? page : 4096))) {
            const hipError_t e = hipHostRegister(reinterpret_cast<void*>(g.begin), g.end - g.begin, hipHostRegisterDefault);
            if (e != hipSuccess) {
                octvr_async::unpin(r);
                (void)hipGetLastError();
                throw OctvrError(OCTVR_E_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e));
            }
            r.pinned.push_back(g);
        }
        a->reg_out.push_back(r);
    }, OCTVR_E_HIP);
}

int octvr_async_unregister_output(octvr_async* a, uint8_t* const* planes) {
    if (!a || !planes) {
        set_last_error("NULL argument");
        return OCTVR_E_INVALID;
    }
    if (a->pending > 0) {  // a queued frame may still be written into them
        set_last_error("frames pending: pop them before unregistering their planes");
        return OCTVR_E_INVALID;
    }
    for (size_t i = 0; i < a->reg_out.size(); i++) {
        const octvr_async::RegOut& r = a->reg_out[i];
        if (!r.same(a->out_planes_used(), planes, nullptr)) continue;
        DeviceGuard dg(a->device);
        octvr_async::unpin(r);
        a->reg_out.erase(a->reg_out.begin() + (long)i);
        return OCTVR_OK;
    }
    set_last_error("planes not registered");
    return OCTVR_E_INVALID;
}

int octvr_async_set_pixel_formats(octvr_async* a, int in_format, int out_format) {
    return guarded([&] {
        REQUIRE(a, "NULL argument");
        auto known = [](int f) {
            return f == OCTVR_PIX_YUV420P || f == OCTVR_PIX_NV12 || converted_format(f);
        };
        REQUIRE(known(in_format) && known(out_format), "pixel format must be an OCTVR_PIX_* value");
        if (out_format == OCTVR_PIX_V210)
            throw OctvrError(OCTVR_E_UNSUPPORTED,
                             "v210 out of the pipeline is not built: OCTVR_PIX_V210 is an input format here (a Mapper writes "
                             "it: octvr_mapper_set_pixel_formats)");
        if (converted_format(out_format))
            throw OctvrError(OCTVR_E_UNSUPPORTED,
                             "the converted layouts (4:2:2, 10-bit) are input formats of the pipeline only: its merge, copy-out "
                             "and registered output planes are per-plane tables of an 8-bit 4:2:0 frame (a Mapper writes them: "
                             "octvr_mapper_set_pixel_formats; the pipeline's merged frame in such a layout is "
                             "octvr_async_set_output_format's)");
        REQUIRE(a->pending == 0, "frames pending: pop them before changing the pixel formats");
        REQUIRE(out_format == a->out_fmt || a->reg_out.empty(),
                "output planes are registered: unregister them before changing the output format");
        // the footprint runs are shared by both layouts because a run's NV12 chroma row is as long as its
        // U and V rows together, which needs even widths (they are, since creation)
        for (int w : a->in_w) REQUIRE(w % 2 == 0, "input widths must be even");
        DeviceGuard dg0(a->device);
        const LayoutDesc in_layout = layout_of(in_format);
        const bool in_conv = in_layout.converted();
        // the pieces' places in the packed buffer are the format's own: 4, 6 or 8 bytes per pixel of a piece's row, or
        // v210's covering blocks (run_key); a switch between them rebuilds the table
        if (in_conv && a->conv_bpp != in_layout.run_key() && !a->native.runs.empty()) {
            size_t bytes = 0;
            std::vector<FootRun> t = run_table(in_layout, a->native.runs, a->in_w, bytes);
            REQUIRE(bytes < ((size_t)1 << 32) && t.size() < 0x7FFFFFFFu, "input footprint exceeds 4 GiB");
            a->conv.dev.upload(t.data(), t.size());
            for (auto& sl : a->slots)  // 4 to 8 bytes per pixel of a row pair against 3: larger packed buffers
                if (sl.packed_host->n < bytes) {
                    sl.packed_host.reset(new PinnedBuf());
                    sl.packed_host->alloc(bytes);
                    sl.packed_dev.alloc(bytes);
                }
            a->conv.runs = std::move(t);
            a->conv.bytes = bytes;
            a->conv_bpp = in_layout.run_key();
        }
        // a pipeline with a converted input converts once for all its mappers, which read its NV12 frames
        const int mapper_in = in_conv ? OCTVR_PIX_NV12 : in_format;
        for (octvr_mapper* m : a->mappers) {
            const int rc = octvr_mapper_set_pixel_formats(m, mapper_in, out_format);
            if (rc != OCTVR_OK) throw OctvrError(rc, octvr_last_error());
        }
        if (in_format != a->in_fmt) {  // the other layout's chroma cells are elsewhere: back to the pattern
            for (auto& sl : a->slots)
                for (int i = 0; i < a->n_in; i++)
                    HIP_CHECK(hipMemset(sl.in_dev[i].p, 0x5A, (size_t)a->in_w[i] * (a->in_h[i] / 2 * 3)));
        }
        a->in_fmt = in_format;
        a->out_fmt = out_format;
        a->free_conv_out();  // a native output format leaves converted output
    }, OCTVR_E_HIP);
}

int octvr_async_set_output_format(octvr_async* a, int out_format) {
    if (!a) {
        set_last_error("NULL argument");
        return OCTVR_E_INVALID;
    }
    if (out_format == OCTVR_PIX_YUV420P || out_format == OCTVR_PIX_NV12)
        return octvr_async_set_pixel_formats(a, a->in_fmt, out_format);
    return guarded([&] {
        const LayoutDesc d = layout_of(out_format);
        REQUIRE(d.converted(), "pixel format must be an OCTVR_PIX_* value");
        if (d.v210())
            throw OctvrError(OCTVR_E_UNSUPPORTED,
                             "v210 out of the pipeline is not built: merge_pack_kernel places regions by 16-byte chunks of "
                             "samples, v210's would have to start at a multiple of 6 pixels");
        REQUIRE(a->pending == 0, "frames pending: pop them before changing the output format");
        REQUIRE(out_format == a->out_fmt || a->reg_out.empty(),
                "output planes are registered: unregister them before changing the output format");
        REQUIRE((int)a->regions.size() <= kMergeMaxRegions, "more regions than one merge launch takes");
        for (size_t k = 0; k < a->regions.size(); k++)
            if (!region_is_subpicture(a->regions[k], a->regions_uv[k]))
                throw OctvrError(OCTVR_E_INVALID, "output region " + std::to_string(k) +
                                                      " is no whole sub-picture of a converted layout: its x and y must be even "
                                                      "and its chroma rectangle must start at their halves");
        const size_t pitch = (size_t)d.row_bytes(a->out_w), bytes = pitch * (size_t)d.rows(a->out_h);
        {
            std::vector<const uint8_t*> src(a->regions.size(), nullptr);
            MergePackTable t;
            REQUIRE(build_merge_pack_table(d, a->regions.data(), a->regions_uv.data(), src.data(), (int)src.size(), a->out_w,
                                           a->out_h, pitch, t),
                    "the merged frame of this layout does not fit a merge launch (2 GiB, 2^31 work items)");
        }
        DeviceGuard dg(a->device);
        // the slots' merged frame and its staging first: a failed allocation leaves the formats as they were
        std::vector<std::unique_ptr<DevBuf<uint8_t>>> dev(kSlots);
        std::vector<std::unique_ptr<PinnedBuf>> host(kSlots);
        for (int s = 0; s < kSlots; s++) {
            dev[s].reset(new DevBuf<uint8_t>());
            dev[s]->alloc(bytes);
            host[s].reset(new PinnedBuf());
            host[s]->alloc(bytes);
        }
        // the mappers keep their input format and write NV12 region frames, the frame pack_lane reads
        const int mapper_in = a->in_conv() ? OCTVR_PIX_NV12 : a->in_fmt;
        for (octvr_mapper* m : a->mappers) {
            const int rc = octvr_mapper_set_pixel_formats(m, mapper_in, OCTVR_PIX_NV12);
            if (rc != OCTVR_OK) throw OctvrError(rc, octvr_last_error());
        }
        for (int s = 0; s < kSlots; s++) {
            a->slots[s].conv_out_dev = std::move(dev[s]);
            a->slots[s].conv_out_host = std::move(host[s]);
        }
        a->out_fmt = out_format;
    }, OCTVR_E_HIP);
}

int octvr_async_pixel_formats(const octvr_async* a, int* in_format, int* out_format) {
    if (!a || !in_format || !out_format) {
        set_last_error("NULL argument");
        return OCTVR_E_INVALID;
    }
    *in_format = a->in_fmt;
    *out_format = a->out_fmt;
    return OCTVR_OK;
}

int octvr_async_pop_preview(octvr_async* a, uint8_t* rgb, size_t pitch, octvr_preview_header* hdr) {
    if (!a || !hdr || (a->preview_w > 0 && (!rgb || pitch < (size_t)a->preview_w * 3))) {
        set_last_error("bad arguments");
        return OCTVR_E_INVALID;
    }
    if (a->preview_w == 0) {
        set_last_error("the pipeline has no preview (preview size 0)");
        return OCTVR_E_INVALID;
    }
    std::lock_guard<std::mutex> g(a->pub_mu);
    *hdr = a->pub_hdr;
    if (a->pub_hdr.width == 0) return OCTVR_OK;  // nothing published yet
    const size_t rb = (size_t)a->preview_w * 3;
    for (int y = 0; y < a->preview_h; y++) memcpy(rgb + (size_t)y * pitch, a->pub.data() + (size_t)y * rb, rb);
    return OCTVR_OK;
}

int octvr_async_set_preview_sink(octvr_async* a, octvr_preview_sink sink, void* user) {
    if (!a) {
        set_last_error("NULL argument");
        return OCTVR_E_INVALID;
    }
    std::unique_lock<std::mutex> g(a->pub_mu);
    a->sink_idle.wait(g, [&] { return !a->sink_busy || a->sink_thread == std::this_thread::get_id(); });
    a->sink = sink;
    a->sink_user = user;
    return OCTVR_OK;
}

int octvr_async_info(const octvr_async* a, char* buf, size_t len) {
    if (!a || !buf || len == 0) {
        set_last_error("bad arguments");
        return OCTVR_E_INVALID;
    }
    size_t in_bytes = 0, out_bytes = 0;
    for (int i = 0; i < a->n_in; i++) in_bytes += (size_t)a->in_w[i] * (a->in_h[i] / 2 * 3);
    for (const Rect& r : a->regions) out_bytes += (size_t)r.w * (r.h / 2 * 3);
    char tmp[1024];
    snprintf(tmp, sizeof tmp,
             "{\"mappers\": %d, \"inputs\": %d, \"packed_bytes\": %zu, \"runs\": %zu, \"input_frame_bytes\": %zu, "
             "\"output_bytes\": %zu, \"preview\": [%d, %d], \"flags\": %d, \"slots\": %d, \"pixel_formats\": [%d, %d], "
             "\"device_frames\": %lld, \"merge_launches\": %lld, \"merge_pack_launches\": %lld",
             (int)a->mappers.size(), a->n_in, a->native.bytes, a->native.runs.size(), in_bytes, out_bytes, a->preview_w,
             a->preview_h, a->flags, kSlots, a->in_fmt, a->out_fmt, (long long)a->device_frames,
             (long long)a->merge_launches.load(), (long long)a->merge_pack_launches.load());
    // per mapper the preview size it gathers from the source frames ([0, 0]: it previews from its result frame,
    // or has no preview)
    std::string js = tmp;
    js += ", \"preview_prepared\": [";
    for (size_t k = 0; k < a->mappers.size(); k++)
        js += std::string(k ? ", [" : "[") + std::to_string(a->mappers[k]->pv.view.dw) + ", " +
              std::to_string(a->mappers[k]->pv.view.dh) + "]";
    js += "]}";
    if (js.size() >= len) {
        set_last_error("buffer too small");
        return OCTVR_E_INVALID;
    }
    memcpy(buf, js.c_str(), js.size() + 1);
    return OCTVR_OK;
}

void octvr_async_destroy(octvr_async* a) { delete a; }

}  // extern "C"
