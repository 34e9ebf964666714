// vr_overlay_test — a reference-style caller of a template with overlays (include/octvr.hpp), built by build()
// and run by tests/test_gpu_cpp_overlay.py.  It follows apps/octvr/dump.cpp:84-93: every input, then every
// overlay through add_input, create_masks, dump to a .dat; then it loads the .dat back and stitches once with
// vr::Mapper over the N + K frames (inputs, then overlays).  The case directory holds case.txt ("out_type W H N K
// blend use_roi"), out_opts.json, cam<i>.txt ("type width height") and cam<i>_opts.json for the N inputs and
// then the K overlays, and frame<i>.yuv; it writes out_overlay.yuv and gains_overlay.txt next to them.
// Usage: vr_overlay_test DIR
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
        int W = 0, H = 0, n = 0, k = 0, blend = 0, use_roi = 1;
        head >> out_type >> W >> H >> n >> k >> blend >> use_roi;
        std::vector<cv::Size> sizes(n + k);
        std::vector<cv::cuda::GpuMat> gin(n + k);
        {
            vr::MapperTemplate mt(out_type, slurp(d + "out_opts.json"), W, H);
            for (int i = 0; i < n + k; i++) {
                std::string type;
                std::istringstream c(slurp(d + "cam" + std::to_string(i) + ".txt"));
                c >> type >> sizes[i].width >> sizes[i].height;
                mt.add_input(type, slurp(d + "cam" + std::to_string(i) + "_opts.json"), i >= n, use_roi != 0);
                cv::Mat frame(sizes[i].height * 3 / 2, sizes[i].width, CV_8UC1);
                const std::string raw = slurp(d + "frame" + std::to_string(i) + ".yuv");
                if (raw.size() != frame.total()) throw std::runtime_error("bad frame size");
                memcpy(frame.data, raw.data(), raw.size());
                gin[i].upload(frame);
            }
            if ((int)mt.inputs.size() != n || (int)mt.overlay_inputs.size() != k)
                throw std::runtime_error("add_input(overlay) did not split inputs and overlays");
            mt.create_masks();
            std::ofstream f(d + "t.dat", std::ios::binary);
            mt.dump(f);
        }
        std::ifstream f(d + "t.dat", std::ios::binary);
        vr::MapperTemplate mt(f);
        if ((int)mt.inputs.size() != n || (int)mt.overlay_inputs.size() != k)
            throw std::runtime_error("the .dat lost inputs or overlays");
        bool threw = false;
        try {  // N sizes for an N + K rig
            vr::Mapper bad(mt, std::vector<cv::Size>(sizes.begin(), sizes.begin() + n), blend, true);
        } catch (const cv::Exception&) {
            threw = true;
        }
        if (k > 0 && !threw) throw std::runtime_error("N sizes for a rig with overlays should throw");
        vr::Mapper mapper(mt, sizes, blend, true);
        cv::cuda::GpuMat gout, no_preview;
        std::vector<cv::cuda::GpuMat> few(gin.begin(), gin.begin() + n);
        threw = false;
        try {  // N frames for an N + K mapper
            mapper.stitch(few, gout, no_preview);
        } catch (const cv::Exception&) {
            threw = true;
        }
        if (k > 0 && !threw) throw std::runtime_error("N frames for a mapper with overlays should throw");
        mapper.stitch(gin, gout, no_preview);
        cv::Mat out;
        gout.download(out);
        {
            std::ofstream o(d + "out_overlay.yuv", std::ios::binary);
            for (int r = 0; r < out.rows; r++) o.write(reinterpret_cast<const char*>(out.ptr(r)), out.cols);
        }
        const std::vector<double> gains = mapper.gains();
        if ((int)gains.size() != n) throw std::runtime_error("gains() must have one entry per input");
        {
            std::ofstream g(d + "gains_overlay.txt");
            g.precision(17);
            for (double v : gains) g << v << "\n";
        }
        std::ofstream(d + "ok_overlay") << "ok";
        return 0;
    } catch (const std::string& e) {
        std::cerr << "error (std::string): " << e << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
    }
    return 1;
}
