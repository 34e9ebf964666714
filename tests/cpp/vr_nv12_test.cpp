// vr_nv12_test — vr::Mapper with NV12 frames in and out (include/octvr.hpp set_pixel_formats), built by
// build() and run by tests/test_gpu_cpp_nv12.py.  It reads the case directory vr_api_test reads (case.txt,
// out_opts.json, in<i>.txt, in<i>_opts.json, frame<i>.yuv — the frames here already NV12), stitches once and
// writes out_nv12.yuv and gains_nv12.txt next to it.
// Usage: vr_nv12_test DIR
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
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

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s DIR\n", argv[0]);
        return 2;
    }
    const std::string d = std::string(argv[1]) + "/";
    try {
        std::istringstream head(slurp(d + "case.txt"));
        std::string out_type;
        int W = 0, H = 0, n = 0, blend = 0, pw = 0, ph = 0, use_roi = 1;
        head >> out_type >> W >> H >> n >> blend >> pw >> ph >> use_roi;
        vr::MapperTemplate mt(out_type, slurp(d + "out_opts.json"), W, H);
        std::vector<cv::Size> sizes(n);
        std::vector<cv::cuda::GpuMat> gin(n);
        for (int i = 0; i < n; i++) {
            std::string type;
            std::istringstream c(slurp(d + "in" + std::to_string(i) + ".txt"));
            c >> type >> sizes[i].width >> sizes[i].height;
            mt.add_input(type, slurp(d + "in" + std::to_string(i) + "_opts.json"), false, use_roi != 0);
            cv::Mat frame(sizes[i].height * 3 / 2, sizes[i].width, CV_8UC1);
            const std::string raw = slurp(d + "frame" + std::to_string(i) + ".yuv");
            if (raw.size() != frame.total()) throw std::runtime_error("bad frame size");
            memcpy(frame.data, raw.data(), raw.size());
            gin[i].upload(frame);
        }
        vr::Mapper mapper(mt, sizes, blend, true);
        int fi = -1, fo = -1;
        mapper.pixel_formats(fi, fo);
        if (fi != OCTVR_PIX_YUV420P || fo != OCTVR_PIX_YUV420P) throw std::runtime_error("the default is YUV420P");
        mapper.set_pixel_formats(OCTVR_PIX_NV12, OCTVR_PIX_NV12);
        mapper.pixel_formats(fi, fo);
        if (fi != OCTVR_PIX_NV12 || fo != OCTVR_PIX_NV12) throw std::runtime_error("pixel_formats after set");
        bool threw = false;
        try {
            mapper.set_pixel_formats(2, OCTVR_PIX_NV12);
        } catch (const cv::Exception&) {
            threw = true;
        }
        if (!threw) throw std::runtime_error("an unknown pixel format should throw");
        cv::cuda::GpuMat gout, no_preview;
        mapper.stitch(gin, gout, no_preview);
        cv::Mat out;
        gout.download(out);
        {
            std::ofstream f(d + "out_nv12.yuv", std::ios::binary);
            for (int r = 0; r < out.rows; r++) f.write(reinterpret_cast<const char*>(out.ptr(r)), out.cols);
        }
        {
            std::ofstream g(d + "gains_nv12.txt");
            g.precision(17);
            for (double v : mapper.gains()) g << v << "\n";
        }
        std::ofstream(d + "ok_nv12") << "ok";
        return 0;
    } catch (const std::string& e) {
        std::cerr << "error (std::string): " << e << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
    }
    return 1;
}
