// vr_async_nv12_test — vr::AsyncMultiMapper with NV12 planes in and out (include/octvr.hpp
// set_pixel_formats), built by build() and run by tests/test_gpu_cpp_async_nv12.py.  It reads the case
// directory vr_api_test reads (case.txt, out_opts.json, in<i>.txt, in<i>_opts.json) and, per frame f of
// `frames`, frame<i>_<f>.yuv (already NV12); one mapper writes the whole output.  All frames are pushed, then
// popped; each merged output goes to out_async_nv12_<f>.yuv as one NV12 frame.  The U,V planes are handed over
// as CV_8UC2 Mats of W/2 x H/2, the third Mat of every tuple is empty.
// Usage: vr_async_nv12_test DIR FRAMES
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "octvr.hpp"

static std::string slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) throw std::runtime_error("cannot read " + p);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

typedef std::tuple<cv::Mat, cv::Mat, cv::Mat> Planes;

// (Y, U,V as CV_8UC2, empty) views of one contiguous NV12 frame
static Planes nv12_planes(cv::Mat& frame, int w, int h) {
    return Planes(frame(cv::Rect(0, 0, w, h)), cv::Mat(h / 2, w / 2, CV_8UC2, frame.ptr(h), frame.step), cv::Mat());
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
            {mt}, sizes, cv::Size(W, H), {blend}, {0}, {cv::Rect_<double>(0, 0, 1, 1)}, cv::Size(0, 0)));
        int fi = -1, fo = -1;
        am->pixel_formats(fi, fo);
        if (fi != OCTVR_PIX_YUV420P || fo != OCTVR_PIX_YUV420P) throw std::runtime_error("the default is YUV420P");
        bool threw = false;
        try {
            am->set_pixel_formats(OCTVR_PIX_NV12, 7);
        } catch (const cv::Exception&) {
            threw = true;
        }
        if (!threw) throw std::runtime_error("an unknown pixel format should throw");
        am->set_pixel_formats(OCTVR_PIX_NV12, OCTVR_PIX_NV12);
        am->pixel_formats(fi, fo);
        if (fi != OCTVR_PIX_NV12 || fo != OCTVR_PIX_NV12) throw std::runtime_error("pixel_formats after set");

        std::vector<std::vector<cv::Mat>> frames(nf);
        std::vector<cv::Mat> outs(nf);
        for (int f = 0; f < nf; f++) {
            std::vector<Planes> in;
            for (int i = 0; i < n; i++) {
                cv::Mat frame(sizes[i].height * 3 / 2, sizes[i].width, CV_8UC1);
                const std::string raw = slurp(d + "frame" + std::to_string(i) + "_" + std::to_string(f) + ".yuv");
                if (raw.size() != frame.total()) throw std::runtime_error("bad frame size");
                memcpy(frame.data, raw.data(), raw.size());
                frames[f].push_back(frame);
                in.push_back(nv12_planes(frames[f].back(), sizes[i].width, sizes[i].height));
            }
            outs[f].create(H * 3 / 2, W, CV_8UC1);
            memset(outs[f].data, 0x5A, outs[f].total());
            Planes out = nv12_planes(outs[f], W, H);
            if (f == 0) {  // a U,V plane of the wrong shape is refused before anything is queued
                Planes bad(std::get<0>(out), cv::Mat(H / 2, W / 2, CV_8UC1, outs[f].ptr(H), outs[f].step), cv::Mat());
                threw = false;
                try {
                    am->push(in, bad);
                } catch (const cv::Exception&) {
                    threw = true;
                }
                if (!threw) throw std::runtime_error("a W/2 x H/2 CV_8UC1 U,V plane should throw");
            }
            am->push(in, out);
        }
        for (int f = 0; f < nf; f++) {
            am->pop();
            std::ofstream o(d + "out_async_nv12_" + std::to_string(f) + ".yuv", std::ios::binary);
            for (int r = 0; r < outs[f].rows; r++) o.write(reinterpret_cast<const char*>(outs[f].ptr(r)), outs[f].cols);
        }
        am.reset();
        std::ofstream(d + "ok_async_nv12") << "ok";
        return 0;
    } catch (const std::string& e) {
        std::cerr << "error (std::string): " << e << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
    }
    return 1;
}
