// rig_dat.cpp — the rig's VRv11 .dat form (template.cpp:206-314): reader, writer and the stream adapters
// over the C ABI's read / write callbacks.  Pure host code.
#include <cstring>
#include <istream>
#include <memory>
#include <ostream>
#include <streambuf>
#include <vector>

#include "host_common.hpp"

namespace octvr {

namespace {

constexpr const char* kDatMagic = "VRv11";
constexpr int CV_8UC1 = 0, CV_32FC1 = 5;

struct DatWriter {
    std::ostream& f;
    void i64(int64_t v) { f.write(reinterpret_cast<const char*>(&v), 8); }
    void mat(int type, int rows, int cols, const void* data, size_t elem) {
        i64(type);
        i64(rows);
        i64(cols);
        if (rows * cols == 0 || !data) return;
        f.write(reinterpret_cast<const char*>(data), (std::streamsize)((size_t)rows * cols * elem));
    }
    void input(const RigInput& in) {
        for (int k = 0; k < 4; k++) i64(in.roi[k]);
        mat(CV_32FC1, in.roi[3], in.roi[2], in.map1.data(), 4);
        mat(CV_32FC1, in.roi[3], in.roi[2], in.map2.data(), 4);
        mat(CV_8UC1, in.roi[3], in.roi[2], in.mask.data(), 1);
        if (in.vignette.empty())
            mat(0, 0, 0, nullptr, 1);  // empty cv::Mat: type 0, 0x0 (Mat() header)
        else
            mat(CV_32FC1, in.vig_h, in.vig_w, in.vignette.data(), 4);
    }
};

struct DatReader {
    std::istream& f;
    int64_t i64() {
        int64_t v = 0;
        f.read(reinterpret_cast<char*>(&v), 8);
        if (!f) throw OctvrError(OCTVR_E_PARSE, "truncated .dat file");
        return v;
    }
    // Rmat: returns rows, cols, type; data appended to `out` (bytes)
    void mat(int want_type, int& rows, int& cols, std::vector<uint8_t>& out) {
        const int64_t type = i64(), r64 = i64(), c64 = i64();
        out.clear();
        // cv::Mat dimensions are non-negative ints; bound the element count before allocating
        if (r64 < 0 || c64 < 0 || r64 > INT32_MAX || c64 > INT32_MAX)
            throw OctvrError(OCTVR_E_PARSE, ".dat: bad Mat dimensions");
        rows = (int)r64;
        cols = (int)c64;
        if ((int64_t)rows * cols == 0) {
            rows = cols = 0;
            return;
        }
        if ((uint64_t)rows * (uint64_t)cols > ((uint64_t)1 << 34))
            throw OctvrError(OCTVR_E_PARSE, ".dat: Mat too large");
        if (want_type >= 0 && type != want_type) throw OctvrError(OCTVR_E_PARSE, "unexpected Mat type in .dat");
        size_t elem = type == CV_32FC1 ? 4 : type == CV_8UC1 ? 1 : 0;
        if (!elem) throw OctvrError(OCTVR_E_PARSE, "unsupported Mat type in .dat");
        out.resize((size_t)rows * cols * elem);
        f.read(reinterpret_cast<char*>(out.data()), (std::streamsize)out.size());
        if (!f) throw OctvrError(OCTVR_E_PARSE, "truncated .dat file");
    }
    // ROI x, y >= 0, w, h > 0 and inside the out_w x out_h frame (as octvr_rig_create_from_arrays)
    void input(RigInput& in, int out_w, int out_h) {
        int64_t roi[4];
        for (int k = 0; k < 4; k++) roi[k] = i64();
        // no sums of untrusted int64 fields: each bound is checked against the frame before the next
        // one is derived from it (roi[0] = INT64_MAX, w = 1 must not wrap into range)
        if (roi[0] < 0 || roi[1] < 0 || roi[0] > out_w || roi[1] > out_h || roi[2] <= 0 || roi[3] <= 0 ||
            roi[2] > out_w - roi[0] || roi[3] > out_h - roi[1])
            throw OctvrError(OCTVR_E_PARSE, ".dat: ROI outside the output frame");
        for (int k = 0; k < 4; k++) in.roi[k] = (int)roi[k];
        std::vector<uint8_t> b;
        int r, c;
        mat(CV_32FC1, r, c, b);
        in.map1.resize((size_t)r * c);
        memcpy(in.map1.data(), b.data(), b.size());
        mat(CV_32FC1, r, c, b);
        in.map2.resize((size_t)r * c);
        memcpy(in.map2.data(), b.data(), b.size());
        mat(CV_8UC1, r, c, b);
        in.mask = b;
        const size_t roi_px = (size_t)in.roi[2] * (size_t)in.roi[3];
        if (in.map1.size() != roi_px || in.map2.size() != roi_px || in.mask.size() != roi_px)
            throw OctvrError(OCTVR_E_PARSE, ".dat: map / mask size does not match ROI");
        mat(-1, r, c, b);
        in.vignette.resize(b.size() / 4);
        if (!b.empty()) memcpy(in.vignette.data(), b.data(), b.size());
        in.vig_w = c;
        in.vig_h = r;
    }
};

// std::streambuf over the C ABI's read / write callbacks (octvr_rig_load_stream / dump_stream).
struct CbOutBuf : std::streambuf {
    octvr_write_fn fn;
    void* ctx;
    char buf[1 << 16];
    CbOutBuf(octvr_write_fn f, void* c) : fn(f), ctx(c) { setp(buf, buf + sizeof buf); }
    bool flush_buf() {
        const size_t n = (size_t)(pptr() - pbase());
        if (n && fn(ctx, pbase(), n) != n) return false;
        setp(buf, buf + sizeof buf);
        return true;
    }
    int overflow(int c) override {
        if (!flush_buf()) return traits_type::eof();
        if (c != traits_type::eof()) {
            *pptr() = (char)c;
            pbump(1);
        }
        return traits_type::not_eof(c);
    }
    int sync() override { return flush_buf() ? 0 : -1; }
};
struct CbInBuf : std::streambuf {
    octvr_read_fn fn;
    void* ctx;
    char buf[1 << 16];
    CbInBuf(octvr_read_fn f, void* c) : fn(f), ctx(c) { setg(buf, buf, buf); }
    int underflow() override {
        const size_t n = fn(ctx, buf, sizeof buf);
        if (n == 0) return traits_type::eof();
        setg(buf, buf, buf + n);
        return traits_type::to_int_type(buf[0]);
    }
};

}  // namespace

// MapperTemplate::dump body (template.cpp:206-256)
void dat_write(octvr_rig& rig, std::ostream& os) {
    if (rig.seam_masks.empty()) rig_create_masks(rig);  // MapperTemplate::dump (template.cpp:209-210)
    REQUIRE(rig.seam_masks.size() == rig.inputs.size(), "seam mask count does not match the inputs");
    DatWriter w{os};
    w.f.write(kDatMagic, 5);
    w.i64(rig.out_w);
    w.i64(rig.out_h);
    w.i64((int64_t)rig.inputs.size());
    for (auto& in : rig.inputs) w.input(in);
    for (size_t i = 0; i < rig.seam_masks.size(); i++) {
        const RigInput& in = rig.inputs[i];
        w.mat(CV_8UC1, in.roi[3], in.roi[2], rig.seam_masks[i].data(), 1);
    }
    w.i64((int64_t)rig.overlays.size());
    for (auto& in : rig.overlays) w.input(in);
    w.f.flush();
    if (!w.f) throw OctvrError(OCTVR_E_IO, "write failed");
}

// MapperTemplate(std::ifstream&) body (template.cpp:258-314)
std::unique_ptr<octvr_rig> dat_read(std::istream& is) {
    DatReader r{is};
    char magic[5];
    r.f.read(magic, 5);
    if (!r.f || strncmp(magic, kDatMagic, 5) != 0)
        throw OctvrError(OCTVR_E_PARSE, "Invalid data file (version does not match)");
    auto rig = std::make_unique<octvr_rig>();
    const int64_t ow = r.i64(), oh = r.i64();
    if (ow <= 0 || oh <= 0 || ow > 65535 || oh > 65535) throw OctvrError(OCTVR_E_PARSE, ".dat: bad output size");
    rig->out_w = (int)ow;
    rig->out_h = (int)oh;
    int64_t n = r.i64();
    if (n < 0 || n > kMaxCams) throw OctvrError(OCTVR_E_PARSE, ".dat: bad input count");
    rig->inputs.resize(n);
    for (auto& in : rig->inputs) r.input(in, rig->out_w, rig->out_h);
    rig->seam_masks.resize(n);
    for (int64_t i = 0; i < n; i++) {
        int rr, cc;
        r.mat(CV_8UC1, rr, cc, rig->seam_masks[i]);
        // MapperTemplate::dump writes one ROI-sized seam mask per input (template.cpp:245-246)
        if (rig->seam_masks[i].size() != (size_t)rig->inputs[i].roi[2] * (size_t)rig->inputs[i].roi[3])
            throw OctvrError(OCTVR_E_PARSE, ".dat: seam mask size does not match ROI");
    }
    int64_t no = r.i64();
    if (no < 0 || no > kMaxCams) throw OctvrError(OCTVR_E_PARSE, ".dat: bad overlay count");
    rig->overlays.resize(no);
    for (auto& in : rig->overlays) r.input(in, rig->out_w, rig->out_h);
    return rig;
}

void dat_write(octvr_rig& rig, octvr_write_fn write, void* ctx) {
    CbOutBuf buf(write, ctx);
    std::ostream os(&buf);
    dat_write(rig, os);
}

std::unique_ptr<octvr_rig> dat_read(octvr_read_fn read, void* ctx) {
    CbInBuf buf(read, ctx);
    std::istream is(&buf);
    return dat_read(is);
}

}  // namespace octvr
