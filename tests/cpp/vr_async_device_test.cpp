// vr_async_device_test — vr::AsyncMultiMapper::push_device (include/octvr.hpp) with frames in device memory
// from octvr_dev_malloc, built by build() and run by tests/test_gpu_cpp_async_device.py.  It reads the case
// directory vr_api_test reads (case.txt, out_opts.json, in<i>.txt, in<i>_opts.json) and, per frame f of
// `frames`, frame<i>_<f>.yuv ("Y over [U|V]").  Two mappers of the same template write the top and the bottom
// half of a W x 2H merged frame, the second with the first one's gains.  The input frames are uploaded at a
// pitch of width + 64, the merged frames live at a pitch of W + 32 and start as 0x5A; all frames are pushed,
// then popped, and each merged frame goes to out_async_device_<f>.yuv with its pitch (3H rows of W + 32 bytes).
// Usage: vr_async_device_test DIR FRAMES
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "octvr.hpp"

static std::string slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) throw std::runtime_error("cannot read " + p);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

static void ok(int rc, const char* what) {
    if (rc != OCTVR_OK) throw std::runtime_error(std::string(what) + ": " + octvr_last_error());
}

struct DevFrame {  // rows x pitch bytes from octvr_dev_malloc
    uint8_t* p = nullptr;
    size_t pitch = 0, rows = 0;
    DevFrame(size_t rows_, size_t pitch_) : pitch(pitch_), rows(rows_) {
        void* v = nullptr;
        ok(octvr_dev_malloc(0, rows * pitch, &v), "octvr_dev_malloc");
        p = static_cast<uint8_t*>(v);
    }
    DevFrame(const DevFrame&) = delete;
    ~DevFrame() { octvr_dev_free(p); }
};

template <class F>
static bool throws(F f) {
    try {
        f();
    } catch (const cv::Exception&) {
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s DIR FRAMES\n", argv[0]);
        return 2;
    }
    const std::string d = std::string(argv[1]) + "/";
    const int nf = atoi(argv[2]);
    try {
        std::istringstream head(slurp(d + "case.txt"));
        std::string out_type;
        int W = 0, H = 0, n = 0, blend = 0, pw = 0, ph = 0, use_roi = 1;
        head >> out_type >> W >> H >> n >> blend >> pw >> ph >> use_roi;
        vr::MapperTemplate mt(out_type, slurp(d + "out_opts.json"), W, H);
        std::vector<cv::Size> sizes(n);
        for (int i = 0; i < n; i++) {
            std::string type;
            std::istringstream c(slurp(d + "in" + std::to_string(i) + ".txt"));
            c >> type >> sizes[i].width >> sizes[i].height;
            mt.add_input(type, slurp(d + "in" + std::to_string(i) + "_opts.json"), false, use_roi != 0);
        }
        std::unique_ptr<vr::AsyncMultiMapper> am(vr::AsyncMultiMapper::New(
            {mt, mt}, sizes, cv::Size(W, 2 * H), {blend, blend}, {0, 0},
            {cv::Rect_<double>(0, 0, 1, .5), cv::Rect_<double>(0, .5, 1, .5)}, cv::Size(0, 0)));

        const size_t out_pitch = (size_t)W + 32, out_rows = (size_t)H * 3;
        std::vector<std::vector<std::unique_ptr<DevFrame>>> frames(nf);
        std::vector<std::unique_ptr<DevFrame>> outs;
        for (int f = 0; f < nf; f++) {
            std::vector<const uint8_t*> in;
            std::vector<size_t> pitch;
            for (int i = 0; i < n; i++) {
                const size_t w = sizes[i].width, rows = (size_t)sizes[i].height * 3 / 2, p = w + 64;
                const std::string raw = slurp(d + "frame" + std::to_string(i) + "_" + std::to_string(f) + ".yuv");
                if (raw.size() != w * rows) throw std::runtime_error("bad frame size");
                std::vector<uint8_t> host(rows * p, 0xEE);
                for (size_t r = 0; r < rows; r++) memcpy(&host[r * p], raw.data() + r * w, w);
                frames[f].emplace_back(new DevFrame(rows, p));
                ok(octvr_memcpy_h2d(frames[f].back()->p, host.data(), host.size()), "octvr_memcpy_h2d");
                in.push_back(frames[f].back()->p);
                pitch.push_back(p);
            }
            outs.emplace_back(new DevFrame(out_rows, out_pitch));
            const std::vector<uint8_t> fill(out_rows * out_pitch, 0x5A);
            ok(octvr_memcpy_h2d(outs.back()->p, fill.data(), fill.size()), "octvr_memcpy_h2d");
            if (f == 0) {  // refused before anything is queued: a frame count, a pitch, a host pointer
                std::vector<uint8_t> host_frame(out_rows * out_pitch);
                std::vector<const uint8_t*> few(in.begin(), in.end() - 1);
                std::vector<size_t> few_pitch(pitch.begin(), pitch.end() - 1);
                if (!throws([&] { am->push_device(few, few_pitch, outs.back()->p, out_pitch); }))
                    throw std::runtime_error("a missing input frame should throw");
                if (!throws([&] { am->push_device(in, pitch, outs.back()->p, (size_t)W - 2); }))
                    throw std::runtime_error("an output pitch below the width should throw");
                if (!throws([&] { am->push_device(in, pitch, host_frame.data(), out_pitch); }))
                    throw std::runtime_error("a host output frame should throw");
            }
            am->push_device(in, pitch, outs.back()->p, out_pitch);
        }
        for (int f = 0; f < nf; f++) {
            am->pop();
            std::vector<uint8_t> host(out_rows * out_pitch);
            ok(octvr_memcpy_d2h(host.data(), outs[f]->p, host.size()), "octvr_memcpy_d2h");
            std::ofstream o(d + "out_async_device_" + std::to_string(f) + ".yuv", std::ios::binary);
            o.write(reinterpret_cast<const char*>(host.data()), (std::streamsize)host.size());
        }
        if (!throws([&] { am->pop(); })) throw std::runtime_error("pop with nothing pending should throw");
        am.reset();
        std::ofstream(d + "ok_async_device") << "ok";
        return 0;
    } catch (const std::string& e) {
        std::cerr << "error (std::string): " << e << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
    }
    return 1;
}
