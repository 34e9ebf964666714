// vr_async_out_test — vr::AsyncMultiMapper::set_output_format (include/octvr.hpp), built by build() and run by
// tests/test_gpu_cpp_async_out.py.  It reads the case directory vr_api_test reads (case.txt, out_opts.json,
// in<i>.txt, in<i>_opts.json) and frame<i>_<f>.yuv for f = 0, 1 (planar "Y over [U|V]" frames); one mapper writes the
// whole output.  Frame 0 is merged as UYVY (one packed plane of 2W x H bytes), frame 1 as P010 (Y of 2W x H bytes
// and the U,V plane of 2W x H/2 bytes), each into planes of pitch = row + 8 filled with 0x5A; the rows go to
// out_async_uyvy.bin and out_async_p010.bin without the padding, which must still hold the fill.
// Usage: vr_async_out_test DIR
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

// rows x bytes inside a Mat of bytes + 8 columns full of 0x5A
static cv::Mat padded(cv::Mat& backing, int rows, int bytes) {
    backing.create(rows, bytes + 8, CV_8UC1);
    memset(backing.data, 0x5A, backing.total());
    return backing(cv::Rect(0, 0, bytes, rows));
}

static void write_rows(std::ofstream& o, const cv::Mat& backing, int bytes) {
    for (int r = 0; r < backing.rows; r++) {
        o.write(reinterpret_cast<const char*>(backing.ptr(r)), bytes);
        for (int b = bytes; b < backing.cols; b++)
            if (backing.ptr(r)[b] != 0x5A) throw std::runtime_error("bytes past a row's width were written");
    }
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
        for (int i = 0; i < n; i++) {
            std::string type;
            std::istringstream c(slurp(d + "in" + std::to_string(i) + ".txt"));
            c >> type >> sizes[i].width >> sizes[i].height;
            mt.add_input(type, slurp(d + "in" + std::to_string(i) + "_opts.json"), false, use_roi != 0);
        }
        std::unique_ptr<vr::AsyncMultiMapper> am(vr::AsyncMultiMapper::New(
            {mt}, sizes, cv::Size(W, H), {blend}, {0}, {cv::Rect_<double>(0, 0, 1, 1)}, cv::Size(0, 0)));
        bool threw = false;
        try {
            am->set_output_format(7);
        } catch (const cv::Exception&) {
            threw = true;
        }
        if (!threw) throw std::runtime_error("an unknown output format should throw");
        threw = false;
        try {
            am->set_pixel_formats(OCTVR_PIX_YUV420P, OCTVR_PIX_UYVY422);
        } catch (const cv::Exception&) {
            threw = true;
        }
        if (!threw) throw std::runtime_error("set_pixel_formats still refuses a converted output format");

        std::vector<std::vector<cv::Mat>> frames(2);
        cv::Mat back[3];
        for (int f = 0; f < 2; f++) {
            am->set_output_format(f == 0 ? OCTVR_PIX_UYVY422 : OCTVR_PIX_P010);
            int fi = -1, fo = -1;
            am->pixel_formats(fi, fo);
            if (fi != OCTVR_PIX_YUV420P || fo != (f == 0 ? OCTVR_PIX_UYVY422 : OCTVR_PIX_P010))
                throw std::runtime_error("pixel_formats after set_output_format");
            std::vector<Planes> in;
            for (int i = 0; i < n; i++) {
                const int w = sizes[i].width, h = sizes[i].height;
                cv::Mat frame(h * 3 / 2, w, CV_8UC1);
                const std::string raw = slurp(d + "frame" + std::to_string(i) + "_" + std::to_string(f) + ".yuv");
                if (raw.size() != frame.total()) throw std::runtime_error("bad frame size");
                memcpy(frame.data, raw.data(), raw.size());
                frames[f].push_back(frame);
                cv::Mat& m = frames[f].back();
                in.push_back(Planes(m(cv::Rect(0, 0, w, h)), m(cv::Rect(0, h, w / 2, h / 2)), m(cv::Rect(w / 2, h, w / 2, h / 2))));
            }
            Planes out = f == 0 ? Planes(padded(back[0], H, 2 * W), cv::Mat(), cv::Mat())
                                : Planes(padded(back[1], H, 2 * W), padded(back[2], H / 2, 2 * W), cv::Mat());
            am->push(in, out);
            am->pop();
        }
        {
            std::ofstream o(d + "out_async_uyvy.bin", std::ios::binary);
            write_rows(o, back[0], 2 * W);
        }
        {
            std::ofstream o(d + "out_async_p010.bin", std::ios::binary);
            write_rows(o, back[1], 2 * W);
            write_rows(o, back[2], 2 * W);
        }
        am.reset();
        std::ofstream(d + "ok_async_out") << "ok";
        return 0;
    } catch (const std::string& e) {
        std::cerr << "error (std::string): " << e << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
    }
    return 1;
}
