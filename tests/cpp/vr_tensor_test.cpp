// vr_tensor_test — vr::Mapper::stitch_tensor (include/octvr.hpp) from a C++ caller, built by build() and run by
// tests/test_gpu_cpp_tensor.py.  It reads the case directory vr_api_test reads (case.txt, out_opts.json,
// in<i>.txt, in<i>_opts.json, frame<i>.yuv; the preview size of case.txt is the tensor's) and tensor.txt (scale
// R G B, then bias R G B), stitches once into an f32 BGR tensor with the YUV frame beside it, and writes
// tensor_bgr.f32 (3 planes of h x w floats), out_tensor.yuv and gains_tensor.txt next to them.
// Usage: vr_tensor_test DIR
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
        int W = 0, H = 0, n = 0, blend = 0, tw = 0, th = 0, use_roi = 1;
        head >> out_type >> W >> H >> n >> blend >> tw >> th >> use_roi;
        vr::MapperTemplate mt(out_type, slurp(d + "out_opts.json"), W, H);
        std::vector<cv::Size> sizes(n);
        std::vector<cv::cuda::GpuMat> gin(n);
        std::vector<const uint8_t*> ptrs;
        std::vector<size_t> pitches;
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
            ptrs.push_back(gin[i].data);
            pitches.push_back(gin[i].step);
        }
        vr::Mapper mapper(mt, sizes, blend, true);
        cv::cuda::GpuMat planes, gout;
        planes.create(3 * th, tw, CV_32FC1);  // plane p: rows [p th, (p + 1) th)
        gout.create(H * 3 / 2, W, CV_8UC1);
        vr::TensorOut t(planes.data, cv::Size(tw, th), OCTVR_TENSOR_F32, true);
        if (t.scale[0] != 1.f || t.bias[2] != 0.f) throw std::runtime_error("TensorOut defaults to scale 1, bias 0");
        t.row_stride = planes.step / sizeof(float);
        t.plane_stride = t.row_stride * (size_t)th;
        std::istringstream tv(slurp(d + "tensor.txt"));
        for (int c = 0; c < 3; c++) tv >> t.scale[c];
        for (int c = 0; c < 3; c++) tv >> t.bias[c];
        bool threw = false;
        try {
            vr::TensorOut bad = t;
            bad.dtype = 3;
            mapper.stitch_tensor(ptrs, pitches, gout.data, gout.step, bad);
        } catch (const cv::Exception&) {
            threw = true;
        }
        if (!threw) throw std::runtime_error("an unknown tensor dtype should throw");
        mapper.stitch_tensor(ptrs, pitches, gout.data, gout.step, t);
        cv::Mat host, out;
        planes.download(host);
        gout.download(out);
        {
            std::ofstream f(d + "tensor_bgr.f32", std::ios::binary);
            for (int r = 0; r < host.rows; r++) f.write(reinterpret_cast<const char*>(host.ptr(r)), (size_t)host.cols * sizeof(float));
        }
        {
            std::ofstream f(d + "out_tensor.yuv", std::ios::binary);
            for (int r = 0; r < out.rows; r++) f.write(reinterpret_cast<const char*>(out.ptr(r)), out.cols);
        }
        {
            std::ofstream g(d + "gains_tensor.txt");
            g.precision(17);
            for (double v : mapper.gains()) g << v << "\n";
        }
        std::ofstream(d + "ok_tensor") << "ok";
        return 0;
    } catch (const std::string& e) {
        std::cerr << "error (std::string): " << e << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
    }
    return 1;
}
