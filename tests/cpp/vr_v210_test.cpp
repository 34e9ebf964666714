// vr_v210_test — vr::Mapper with v210 frames in and out (include/octvr.hpp set_pixel_formats with OCTVR_PIX_V210),
// built by build() and run by tests/test_gpu_cpp_v210.py.  It reads the case directory vr_api_test reads (case.txt,
// out_opts.json, in<i>.txt, in<i>_opts.json, frame<i>.v210 — H rows of 128 ceil(W / 48) bytes), stitches once into
// an output it lets the mapper create and writes out.v210 and gains_v210.txt next to it.
// Usage: vr_v210_test DIR
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
            cv::Mat frame(sizes[i].height, 128 * ((sizes[i].width + 47) / 48), CV_8UC1);
            const std::string raw = slurp(d + "frame" + std::to_string(i) + ".v210");
            if (raw.size() != frame.total()) throw std::runtime_error("bad frame size");
            memcpy(frame.data, raw.data(), raw.size());
            gin[i].upload(frame);
        }
        vr::Mapper mapper(mt, sizes, blend, true);
        mapper.set_pixel_formats(OCTVR_PIX_V210, OCTVR_PIX_V210);
        int fi = -1, fo = -1;
        mapper.pixel_formats(fi, fo);
        if (fi != OCTVR_PIX_V210 || fo != OCTVR_PIX_V210 || OCTVR_PIX_V210 != 48) throw std::runtime_error("pixel_formats after set");
        for (int bad : {47, 49}) {
            bool threw = false;
            try {
                mapper.set_pixel_formats(bad, OCTVR_PIX_V210);
            } catch (const cv::Exception&) {
                threw = true;
            }
            if (!threw) throw std::runtime_error("an unknown pixel format should throw");
        }
        cv::cuda::GpuMat gout, no_preview;
        mapper.stitch(gin, gout, no_preview);
        if (gout.rows != H || gout.cols != 128 * ((W + 47) / 48) || gout.type() != CV_8UC1)
            throw std::runtime_error("the created output is no v210 frame of the output size");
        cv::Mat out;
        gout.download(out);
        {
            std::ofstream f(d + "out.v210", std::ios::binary);
            for (int r = 0; r < out.rows; r++) f.write(reinterpret_cast<const char*>(out.ptr(r)), out.cols);
        }
        {
            std::ofstream g(d + "gains_v210.txt");
            g.precision(17);
            for (double v : mapper.gains()) g << v << "\n";
        }
        std::ofstream(d + "ok_v210") << "ok";
        return 0;
    } catch (const std::string& e) {
        std::cerr << "error (std::string): " << e << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
    }
    return 1;
}
