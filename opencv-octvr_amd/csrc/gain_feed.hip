// gain_feed.hip — gfx950 kernels of the gain compensation: cv::solve's LU on the device, the
// one-launch gain feed (full and lean), set_gains, and the footprint-run unpack.
//
// Built with -ffp-contract=off: every f32/f64 expression rounds exactly as written, matching the
// reference's non-FMA x86 arithmetic (the oracle, oracle/octvr_oracle.c, is compiled the same way).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "device_common.hpp"
#include "kernels.hpp"

namespace octvr {

constexpr int kLuBlockMin = 9;  // smallest n solved by the workgroup-parallel LU (below: one lane, registers)

// cv::solve (lapack.cpp:1050-1275) with the matrix in registers: closed forms for n <= 3, LUImpl
// (matrix_decomp.cpp:50-110) above, instantiated per n so every index is static.
template <int N>
__device__ bool lu_solve(double (&A)[N * N], double (&b)[N]) {
    const double eps = DBL_EPSILON * 100;
#pragma unroll
    for (int i = 0; i < N; i++) {
        int k = i;
        double best = fabs(A[i * N + i]);
#pragma unroll
        for (int j = i + 1; j < N; j++) {
            const double v = fabs(A[j * N + i]);
            if (v > best) {
                best = v;
                k = j;
            }
        }
        if (best < eps) return false;
        if (k != i) {  // rare (A is diagonally dominant here): the select-based swap only when needed
#pragma unroll
            for (int j = i + 1; j < N; j++) {  // row swap i <-> k as selects (static indices only)
                const bool sw = (j == k);
#pragma unroll
                for (int c = i; c < N; c++) {
                    const double ai = A[i * N + c], aj = A[j * N + c];
                    A[i * N + c] = sw ? aj : ai;
                    A[j * N + c] = sw ? ai : aj;
                }
                const double bi = b[i], bj = b[j];
                b[i] = sw ? bj : bi;
                b[j] = sw ? bi : bj;
            }
        }
        const double d = -1 / A[i * N + i];
#pragma unroll
        for (int j = i + 1; j < N; j++) {
            const double alpha = A[j * N + i] * d;
#pragma unroll
            for (int c = i + 1; c < N; c++) A[j * N + c] += alpha * A[i * N + c];
            b[j] += alpha * b[i];
        }
        A[i * N + i] = -d;
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double s = b[i];
#pragma unroll
        for (int c = i + 1; c < N; c++) s -= A[i * N + c] * b[c];
        b[i] = s * A[i * N + i];
    }
    return true;
}

template <int N>
__device__ bool solve_fixed(const double* Ain, const double* bin, double* x) {
    double A[N * N], b[N];
#pragma unroll
    for (int k = 0; k < N * N; k++) A[k] = Ain[k];
#pragma unroll
    for (int k = 0; k < N; k++) b[k] = bin[k];
#define Sd(y, xx) A[(y) * N + (xx)]
    if constexpr (N == 1) {
        const double d = Sd(0, 0);
        if (d == 0.) return false;
        x[0] = b[0] / d;
        return true;
    } else if constexpr (N == 2) {
        double d = (double)Sd(0, 0) * Sd(1, 1) - (double)Sd(0, 1) * Sd(1, 0);
        if (d == 0.) return false;
        d = 1. / d;
        const double t = (b[0] * Sd(1, 1) - b[1] * Sd(0, 1)) * d;
        x[1] = (b[1] * Sd(0, 0) - b[0] * Sd(1, 0)) * d;
        x[0] = t;
        return true;
    } else if constexpr (N == 3) {
        double d = Sd(0, 0) * ((double)Sd(1, 1) * Sd(2, 2) - (double)Sd(1, 2) * Sd(2, 1)) -
                   Sd(0, 1) * ((double)Sd(1, 0) * Sd(2, 2) - (double)Sd(1, 2) * Sd(2, 0)) +
                   Sd(0, 2) * ((double)Sd(1, 0) * Sd(2, 1) - (double)Sd(1, 1) * Sd(2, 0));
        if (d == 0.) return false;
        d = 1. / d;
        x[0] = ((Sd(1, 1) * Sd(2, 2) - Sd(1, 2) * Sd(2, 1)) * b[0] + (Sd(0, 2) * Sd(2, 1) - Sd(0, 1) * Sd(2, 2)) * b[1] +
                (Sd(0, 1) * Sd(1, 2) - Sd(0, 2) * Sd(1, 1)) * b[2]) * d;
        x[1] = ((Sd(1, 2) * Sd(2, 0) - Sd(1, 0) * Sd(2, 2)) * b[0] + (Sd(0, 0) * Sd(2, 2) - Sd(0, 2) * Sd(2, 0)) * b[1] +
                (Sd(0, 2) * Sd(1, 0) - Sd(0, 0) * Sd(1, 2)) * b[2]) * d;
        x[2] = ((Sd(1, 0) * Sd(2, 1) - Sd(1, 1) * Sd(2, 0)) * b[0] + (Sd(0, 1) * Sd(2, 0) - Sd(0, 0) * Sd(2, 1)) * b[1] +
                (Sd(0, 0) * Sd(1, 1) - Sd(0, 1) * Sd(1, 0)) * b[2]) * d;
        return true;
    } else {
        if (!lu_solve<N>(A, b)) return false;
#pragma unroll
        for (int k = 0; k < N; k++) x[k] = b[k];
        return true;
    }
#undef Sd
}


// The same LUImpl with the whole workgroup: per pivot every thread finds the pivot row (same scan
// order), one thread per column swaps, one thread per (row, column) eliminates; every element sees
// exactly the serial operation sequence of LUImpl (matrix_decomp.cpp:50-110), so the result is
// bit-identical to lu_solve<N>.  Used for n = 9..16 (too large for one lane's registers).
// Call with all threads of the workgroup; returns the same flag everywhere.
__device__ bool lu_solve_block(double* A, double* b, int n, double* x) {
    const double eps = DBL_EPSILON * 100;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = 0; i < n; i++) {
        int k = i;
        for (int j = i + 1; j < n; j++)
            if (fabs(A[j * n + i]) > fabs(A[k * n + i])) k = j;
        if (fabs(A[k * n + i]) < eps) return false;  // uniform: every thread read the same values
        __syncthreads();
        if (k != i) {
            for (int c = i + tid; c <= n; c += nt) {  // column n is b
                double* ri = (c < n) ? &A[i * n + c] : &b[i];
                double* rk = (c < n) ? &A[k * n + c] : &b[k];
                const double t = *ri;
                *ri = *rk;
                *rk = t;
            }
            __syncthreads();
        }
        const double d = -1 / A[i * n + i];
        const int w = n - i;  // columns i+1 .. n (n = b)
        for (int q = tid; q < (n - 1 - i) * w; q += nt) {
            const int j = i + 1 + q / w, c = i + 1 + q % w;
            const double alpha = A[j * n + i] * d;
            if (c < n)
                A[j * n + c] += alpha * A[i * n + c];
            else
                b[j] += alpha * b[i];
        }
        __syncthreads();
        if (tid == 0) A[i * n + i] = -d;
        __syncthreads();
    }
    if (tid == 0) {
        for (int i = n - 1; i >= 0; i--) {
            double s = b[i];
            for (int c = i + 1; c < n; c++) s -= A[i * n + c] * b[c];
            b[i] = s * A[i * n + i];
        }
        for (int i = 0; i < n; i++) x[i] = b[i];
    }
    __syncthreads();
    return true;
}

// inlined into its one call site per feed instance (as a called function — the three frame-count instances
// made the inliner stop — the one-in-flight C2 feed's serial tail grew from 16.4 to 20.0 us)
__device__ __forceinline__ bool solve_dispatch(double* A, double* b, int n, double* x) {
    switch (n) {
#define CASE(K) \
    case K:     \
        return solve_fixed<K>(A, b, x);
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
        default:
            return false;
    }
}

// n <= 3 only: the closed forms (few registers)
__device__ bool solve_small(double* A, double* b, int n, double* x) {
    switch (n) {
        case 1: return solve_fixed<1>(A, b, x);
        case 2: return solve_fixed<2>(A, b, x);
        case 3: return solve_fixed<3>(A, b, x);
        default: return false;
    }
}

// cv::solve (lapack.cpp:1050-1275) on A, b in LDS, x to LDS, with the whole workgroup: the feed's choice of
// solver.  Full feed (LEAN = false): one lane with the matrix in registers for n <= 8 (closed forms n <= 3),
// the LU across the workgroup for 9..16.  Lean feed: the closed forms for n <= 3, the workgroup LU above (the
// register LU would set the lean kernel's VGPR budget).  flag: one LDS int for the single lane's verdict.
// Call with A and b visible to every thread (a barrier after they were written); returns the same flag
// everywhere, x is written and visible where it is true.
template <bool LEAN>
__device__ __forceinline__ bool gain_solve(double* A, double* b, int n, double* x, int* flag) {
    bool ok;
    if (LEAN && n > 3) {
        ok = lu_solve_block(A, b, n, x);
    } else if (LEAN || n < kLuBlockMin || n <= 3) {
        if (threadIdx.x == 0) *flag = (LEAN ? solve_small(A, b, n, x) : solve_dispatch(A, b, n, x)) ? 1 : 0;
        __syncthreads();
        ok = *flag != 0;
    } else {
        ok = lu_solve_block(A, b, n, x);
    }
    return ok;
}

// ---------------------------------------------------------------------------------------------
// Gain feed (GainCompensatorGPU::feed, exposure_compensate.cpp:223-297) — one launch.
// Sample s of camera i (a working-scale pixel, nearest resize of the warped ROI, mapper.cpp:234-237)
// contributes its f32 norm (core/src/cuda/gpu_mat.cu:443-449) to the masked sum of every pair
// (i, j) whose intersection contains it: I(i,j) = sum / N(i,j).
//
// Exact, order-free sums: a norm is sqrtf of an integer, so it is 0 or lies in [1, 442] and is a
// whole multiple of 2^-23; a pair sum of fewer than 2^21 of them (the working scale holds ~1e5
// pixels, checked on the host) is an integer below 2^53 in units of 2^-23.  Every partial sum is
// therefore exact in f64, and the per-pair totals are kept as u64 fixed point (units of 2^-23)
// added with device-scope integer atomics: the result equals the sequential f64 sum bit for bit,
// whatever order the workgroups finish in.
//
// Completion: per-XCD tickets (blockIdx % 8), then one global ticket; the last workgroup reads the
// totals with returning atomics (executed at the memory side, so no L2 staleness across XCDs),
// resets them, assembles A, b and solves.
// ---------------------------------------------------------------------------------------------
// Wave sum of an f64 through DPP moves (quad perms, row rotations, row broadcasts 15 / 31; the
// total lands in lane 63) instead of LDS-routed shuffles.  The gain-feed sums are exact (see below),
// so the summation order does not change the result.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_f64<0xb1>(v);   // quad_perm [1,0,3,2]
    v += dpp_f64<0x4e>(v);   // quad_perm [2,3,0,1]
    v += dpp_f64<0x124>(v);  // row_ror 4
    v += dpp_f64<0x128>(v);  // row_ror 8
    v += dpp_f64<0x142>(v);  // row_bcast 15
    v += dpp_f64<0x143>(v);  // row_bcast 31
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                            __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// Row i of GainCompensatorGPU::feed's system (exposure_compensate.cpp:279-296) from I(i,j) and
// N(i,j) (both n x n), in the reference's j order: A(i,i) = sum_j beta N + (j != i) 2 alpha I^2 N,
// A(i,j) = -2 alpha I(i,j) I(j,i) N, b(i) = sum_j beta N.  A has row stride n.
__device__ __forceinline__ void gain_system_row(const double* I, const int32_t* Nm, int n, int i, double* A, double* b) {
    const double alpha = 0.01, beta = 100;
    double bi = 0.0, aii = 0.0;
    for (int j = 0; j < n; j++) {
        const int Nij = Nm[i * n + j];
        bi += beta * Nij;
        aii += beta * Nij;
        if (j == i) continue;
        aii += 2 * alpha * I[i * n + j] * I[i * n + j] * Nij;
        A[i * n + j] = 0.0 - 2 * alpha * I[i * n + j] * I[j * n + i] * Nij;
    }
    A[i * n + i] = aii;
    b[i] = bi;
}

// Gain-feed gathers: per sample the 2 luma, 2 U and 2 V row segments of its 2x2 taps as 8-byte buffer
// loads from 4-byte aligned starts (6 loads instead of 12 byte loads).  The frame-sized buffer resource
// range-checks whole dwords, so a load may not reach past the frame's last byte: only a V row segment of
// the last chroma row can (Y rows are followed by the chroma rows, U halves by V halves), and its start
// is clamped to size - 8, the bytes taken relative to the clamped start.  Everything the extraction
// needs — the tap bytes' positions in the 8 loaded bytes as v_perm selectors, the taps' in-image flags,
// the fractions — is derived once at issue and carried to feed_taps_finish, after every sample's loads
// are in flight.
//
// NV12 frames: a tap pair's chroma is the U,V pairs at bytes c0 * 2 and c1 * 2 of ONE interleaved row, so a
// sample takes 2 luma and 2 chroma row segments (4 loads).  The segment starts at the 4-byte aligned
// (c0 * 2) & ~3, i.e. at an even chroma sample, so that the pair's 4 bytes lie at bytes 0-5 of it (aligned to
// four samples as the planar segments are, a pair at samples 3 and 4 would need bytes 6-9).  Every chroma
// row can be the frame's last row, so both starts are clamped to size - 8 (u0 / u1 hold the two segments,
// the shifts travel in the V row shifts' bits; v0 / v1 are unused).
struct FeedRaw {
    uint2 y0, y1, u0, u1, v0, v1;
    uint32_t sel;   // bytes of taps x0, x1: luma (bits 0-15), chroma (16-31), as v_perm selectors
    uint32_t meta;  // code bits 0-15 (fx, fy, valid), in-image ix0 ix1 iy0 iy1 at 16-19, V row shifts at 20-22 / 23-25
};

template <bool NV12 = false>
__device__ __forceinline__ void feed_taps_issue(__amdgpu_buffer_rsrc_t rs, const SourceFrame& f, uint32_t xy,
                                                uint32_t code, FeedRaw& r) {
    const TapCell tc = tap_cell(xy, f.w, f.h);
    const uint32_t p = (uint32_t)f.pitch;
    const uint32_t lim = (uint32_t)f.pitch * (uint32_t)(f.h + f.h / 2) - 8u;  // frames >= 8 B (host check)
    const uint32_t uo = (uint32_t)f.h * p, vo = uo + (uint32_t)(f.w >> 1);
    const uint32_t x0 = (uint32_t)tc.x0, x1 = (uint32_t)tc.x1, c0 = x0 >> 1, c1 = x1 >> 1;
    const uint32_t xa = x0 & ~3u, ca = c0 & ~3u;
    const uint32_t ry0 = (uint32_t)tc.y0 * p, ry1 = (uint32_t)tc.y1 * p;
    const uint32_t rc0 = (uint32_t)(tc.y0 >> 1) * p, rc1 = (uint32_t)(tc.y1 >> 1) * p;
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    u32x2 t;
    if constexpr (NV12) {
        const uint32_t cb = (c0 * 2u) & ~3u;  // <= w - 2: inside the row
        const uint32_t sc0 = uo + rc0 + cb, sc1 = uo + rc1 + cb;
        const uint32_t lc0 = min(sc0, lim), lc1 = min(sc1, lim);  // the pair's bytes stay inside the 8 loaded
        t = __builtin_amdgcn_raw_buffer_load_b64(rs, ry0 + xa, 0, 0);
        r.y0 = make_uint2(t.x, t.y);
        t = __builtin_amdgcn_raw_buffer_load_b64(rs, ry1 + xa, 0, 0);
        r.y1 = make_uint2(t.x, t.y);
        t = __builtin_amdgcn_raw_buffer_load_b64(rs, lc0, 0, 0);
        r.u0 = make_uint2(t.x, t.y);
        t = __builtin_amdgcn_raw_buffer_load_b64(rs, lc1, 0, 0);
        r.u1 = make_uint2(t.x, t.y);
        const uint32_t iy = x0 & 3u, ic = (c0 * 2u) & 3u;  // U bytes of the two taps: ic, ic + 2 (c1 - c0)
        r.sel = iy | (iy + (x1 - x0)) << 8 | ic << 16 | (ic + 2u * (c1 - c0)) << 24;
        r.meta = (code & 0xFFFFu) | (tc.ix0 ? 1u << 16 : 0u) | (tc.ix1 ? 1u << 17 : 0u) | (tc.iy0 ? 1u << 18 : 0u) |
                 (tc.iy1 ? 1u << 19 : 0u) | (sc0 - lc0) << 20 | (sc1 - lc1) << 23;
        return;
    }
    const uint32_t sv0 = vo + rc0 + ca, sv1 = vo + rc1 + ca;
    const uint32_t lv0 = min(sv0, lim), lv1 = min(sv1, lim);
    t = __builtin_amdgcn_raw_buffer_load_b64(rs, ry0 + xa, 0, 0);
    r.y0 = make_uint2(t.x, t.y);
    t = __builtin_amdgcn_raw_buffer_load_b64(rs, ry1 + xa, 0, 0);
    r.y1 = make_uint2(t.x, t.y);
    t = __builtin_amdgcn_raw_buffer_load_b64(rs, uo + rc0 + ca, 0, 0);
    r.u0 = make_uint2(t.x, t.y);
    t = __builtin_amdgcn_raw_buffer_load_b64(rs, uo + rc1 + ca, 0, 0);
    r.u1 = make_uint2(t.x, t.y);
    t = __builtin_amdgcn_raw_buffer_load_b64(rs, lv0, 0, 0);
    r.v0 = make_uint2(t.x, t.y);
    t = __builtin_amdgcn_raw_buffer_load_b64(rs, lv1, 0, 0);
    r.v1 = make_uint2(t.x, t.y);
    const uint32_t iy = x0 & 3u, ic = c0 & 3u;  // x1 - x0, c1 - c0 in {0, 1}
    r.sel = iy | (iy + (x1 - x0)) << 8 | ic << 16 | (ic + (c1 - c0)) << 24;
    r.meta = (code & 0xFFFFu) | (tc.ix0 ? 1u << 16 : 0u) | (tc.ix1 ? 1u << 17 : 0u) | (tc.iy0 ? 1u << 18 : 0u) |
             (tc.iy1 ? 1u << 19 : 0u) | (sv0 - lv0) << 20 | (sv1 - lv1) << 23;
}

// Same taps, validity and conversions as gather_taps_frame (device_common.hpp), without vignette.
template <bool NV12 = false>
__device__ __forceinline__ void feed_taps_finish(const FeedRaw& r, Taps& t) {
    const uint32_t m = r.meta;
    const uint32_t sy = (r.sel & 0xFFFFu) | 0x0C0C0000u, sc = (r.sel >> 16) | 0x0C0C0000u;
    const uint32_t sv0 = sc + ((m >> 20) & 7u) * 0x0101u, sv1 = sc + ((m >> 23) & 7u) * 0x0101u;
    // two tap bytes of each row segment in bytes 0, 1
    const uint32_t Y0 = __builtin_amdgcn_perm(r.y0.y, r.y0.x, sy), Y1 = __builtin_amdgcn_perm(r.y1.y, r.y1.x, sy);
    uint32_t U0, U1, V0, V1;
    if constexpr (NV12) {  // sv0 / sv1: the U bytes in the (clamped) interleaved segments; V is the next byte
        U0 = __builtin_amdgcn_perm(r.u0.y, r.u0.x, sv0), U1 = __builtin_amdgcn_perm(r.u1.y, r.u1.x, sv1);
        V0 = __builtin_amdgcn_perm(r.u0.y, r.u0.x, sv0 + 0x0101u), V1 = __builtin_amdgcn_perm(r.u1.y, r.u1.x, sv1 + 0x0101u);
    } else {
        U0 = __builtin_amdgcn_perm(r.u0.y, r.u0.x, sc), U1 = __builtin_amdgcn_perm(r.u1.y, r.u1.x, sc);
        V0 = __builtin_amdgcn_perm(r.v0.y, r.v0.x, sv0), V1 = __builtin_amdgcn_perm(r.v1.y, r.v1.x, sv1);
    }
    uint32_t ca, cb, cc, cd;
    yuv_pair_to_rgba(Y0, U0, V0, ca, cb);
    yuv_pair_to_rgba(Y1, U1, V1, cc, cd);
    const bool valid = (m & 0x8000u) != 0;
    const bool ix0 = (m >> 16) & 1u, ix1 = (m >> 17) & 1u, iy0 = (m >> 18) & 1u, iy1 = (m >> 19) & 1u;
    t.c[0] = (valid && ix0 && iy0) ? ca : 0u;
    t.c[1] = (valid && ix1 && iy0) ? cb : 0u;
    t.c[2] = (valid && ix0 && iy1) ? cc : 0u;
    t.c[3] = (valid && ix1 && iy1) ? cd : 0u;
    t.fx = m & 31u;
    t.fy = (m >> 5) & 31u;
}

// LEAN = false: every sample's gathers in flight at once (kGainPer samples per lane) and the register
// LU (163 VGPRs: the shortest feed on an idle GPU).  LEAN = true: kLeanBatch samples per lane per
// round, partner sums in LDS, the workgroup LU above n = 3 (<= 80 VGPRs), so the feed of frame k+1
// fits beside frame k's composite (6 workgroups per CU at 72 VGPRs / 96 SGPRs / 20.7 KiB LDS) and runs
// under it.  Both sum the same exact values: identical gains.
constexpr int kLeanBatch = 3;  // lean feed: samples per lane in flight per round
// The sample's warped pixel (RGB) from its taps: cv::remap's fixed-point bilinear, or the texture filter of
// the texture-convention mode (tex, uniform)
__device__ __forceinline__ void sample_rgb(const Taps& t, int tex, uint32_t (&rgb)[3]) {
    if (tex)
        tex_bilerp(t.c[0], t.c[1], t.c[2], t.c[3], t.fx, t.fy, rgb);
    else
        bilerp_rgba(t.c[0], t.c[1], t.c[2], t.c[3], t.fx, t.fy, rgb);
}

// The feed's FIRST argument (FeedBatch): camera c of frame f read from the kernarg segment (scalar loads,
// kSourceFrame)
static_assert(offsetof(FeedBatch<1>, src) == 0 && offsetof(FeedBatch<4>, src) == 0, "FeedBatch layout");

template <bool LEAN, int NF, bool NV12>
__device__ __forceinline__ void gain_feed_body(const CompositeEntry* samples, const uint16_t* partners, int tex,
                                               int n_chunks, const int32_t* N, int n) {
    typedef __attribute__((address_space(4))) const FeedBatch<NF> kFeedBatch;
    __shared__ int s_last;
    __shared__ double s_I[kGainMaxCams * kGainMaxCams];
    __shared__ double s_A[kGainMaxCams * kGainMaxCams];
    __shared__ double s_b[kGainMaxCams];
    __shared__ double s_x[kGainMaxCams];
    const int tid = threadIdx.x, lane = tid & 63;
    // Wave w of workgroup b takes the kGainWaveRun contiguous samples from (4 b + w) kGainWaveRun: one
    // camera's (runs padded on the host with invalid samples, partner mask 0), named in every entry's
    // code.  Every norm is 0 or a multiple of 2^-23 in [1, 2^9), so the f64 sums below are exact in any order.
    constexpr int kPer = kGainPer;
    const int wave = tid >> 6;
    __shared__ double s_wsum[4][kGainMaxCams];
    __shared__ int s_wcam[4];
    // workgroup b: frame b / n_chunks of the batch (FeedBatch), chunk cb of it
    const kFeedBatch* kb = (const kFeedBatch*)__builtin_amdgcn_kernarg_segment_ptr();
    const int frame = uniform((int)(blockIdx.x / (uint32_t)n_chunks)), cb = (int)blockIdx.x - frame * n_chunks;
    unsigned long long* const totals = kb->totals[frame];
    uint32_t* const tickets = kb->tickets[frame];
    double* const gains = kb->gains[frame];
    const int k0 = (cb * 4 + wave) * kGainWaveRun + lane;
    const int cam = uniform((int)((samples[(cb * 4 + wave) * kGainWaveRun].code >> 10) & 15u));
    SourceFrame fr;  // one camera per wave: uniform frame
    {
        const kSourceFrame& kf = kb->src[frame * kGainMaxCams + cam];
        fr.yuv = kf.yuv;
        fr.w = kf.w;
        fr.h = kf.h;
        fr.pitch = kf.pitch;
        fr.vig = kf.vig;
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(fr.yuv), 0, (int)((uint32_t)fr.pitch * (uint32_t)(fr.h + fr.h / 2)), 0x00020000);
    if constexpr (LEAN) {
        // one sample per lane at a time; per partner a wave sum added into the wave's LDS row
        // (kLeanBatch samples per lane in flight per round)
        if (lane < kGainMaxCams) s_wsum[wave][lane] = 0.0;
        static_assert(kPer % kLeanBatch == 0, "lean feed batches");
#pragma unroll 1
        for (int u0 = 0; u0 < kPer; u0 += kLeanBatch) {
            CompositeEntry e[kLeanBatch];
            uint32_t pm[kLeanBatch];
#pragma unroll
            for (int u = 0; u < kLeanBatch; u++) {
                e[u] = samples[k0 + (u0 + u) * 64];
                pm[u] = partners[k0 + (u0 + u) * 64];
            }
            Taps t[kLeanBatch];
            if (fr.vig || tex) {  // vignette / clamped texture taps: per-tap byte gathers
#pragma unroll
                for (int u = 0; u < kLeanBatch; u++) gather_taps_frame<NV12>(fr, e[u].xy, e[u].code, t[u]);
            } else {
                FeedRaw raw[kLeanBatch];
#pragma unroll
                for (int u = 0; u < kLeanBatch; u++) feed_taps_issue<NV12>(rs, fr, e[u].xy, e[u].code, raw[u]);
#pragma unroll
                for (int u = 0; u < kLeanBatch; u++) feed_taps_finish<NV12>(raw[u], t[u]);
            }
            double nv[kLeanBatch];
            uint32_t pm_any = 0u;
#pragma unroll
            for (int u = 0; u < kLeanBatch; u++) {
                uint32_t rgb[3];
                sample_rgb(t[u], tex, rgb);
                nv[u] = (double)sqrtf((float)(rgb[0] * rgb[0] + rgb[1] * rgb[1] + rgb[2] * rgb[2]));
                pm_any |= pm[u];
            }
            // partners present in this wave's batch (wave-uniform): one wave sum each
            uint32_t jm = 0u;
            for (int j = 0; j < n; j++) jm |= __ballot((pm_any >> j) & 1u) ? 1u << j : 0u;
#pragma unroll 1
            while (jm) {
                const int j = __builtin_ctz(jm);
                jm &= jm - 1;
                double v = 0.0;
#pragma unroll
                for (int u = 0; u < kLeanBatch; u++) v += ((pm[u] >> j) & 1u) ? nv[u] : 0.0;
                v = wave_sum(v);
                if (lane == 0) s_wsum[wave][j] += v;
            }
        }
    } else {
        // kGainPer samples per lane, all gathers issued before any arithmetic
        double acc[kGainMaxCams];
#pragma unroll
        for (int j = 0; j < kGainMaxCams; j++) acc[j] = 0.0;
        uint32_t pm[kPer];
        Taps t[kPer];
        CompositeEntry es[kPer];
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            es[u] = samples[k0 + u * 64];
            pm[u] = partners[k0 + u * 64];
        }
        if (fr.vig || tex) {  // vignette / clamped texture taps: per-tap byte gathers
#pragma unroll
            for (int u = 0; u < kPer; u++) gather_taps_frame<NV12>(fr, es[u].xy, es[u].code, t[u]);
        } else {
            FeedRaw raw[kPer];
#pragma unroll
            for (int u = 0; u < kPer; u++) feed_taps_issue<NV12>(rs, fr, es[u].xy, es[u].code, raw[u]);
#pragma unroll
            for (int u = 0; u < kPer; u++) feed_taps_finish<NV12>(raw[u], t[u]);
        }
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            uint32_t rgb[3];
            sample_rgb(t[u], tex, rgb);
            const double nv = (double)sqrtf((float)(rgb[0] * rgb[0] + rgb[1] * rgb[1] + rgb[2] * rgb[2]));
#pragma unroll
            for (int j = 0; j < kGainMaxCams; j++)
                if (pm[u] & (1u << j)) acc[j] += nv;
        }
        // exact sums: per wave (DPP)
#pragma unroll
        for (int j = 0; j < kGainMaxCams; j++) {  // unrolled: the n reductions' DPP chains interleave
            if (j < n) {
                const double v = wave_sum(acc[j]);
                if (lane == 0) s_wsum[wave][j] = v;
            }
        }
    }
    // then per (camera, partner) over the workgroup's waves, then one u64 atomic per pair
    if (lane == 0) s_wcam[wave] = cam;
    __syncthreads();
    if (tid < 4 * n) {  // (wave w, partner j); the first wave of each camera adds for all its waves
        const int w = tid / n, j = tid - w * n, c = s_wcam[w];
        bool first = true;
        for (int x = 0; x < w; x++) first &= s_wcam[x] != c;
        if (first) {
            double v = 0.0;
            for (int x = w; x < 4; x++)
                if (s_wcam[x] == c) v += s_wsum[x][j];
            if (v != 0.0)
                __hip_atomic_fetch_add(&totals[(c * kGainMaxCams + j) * kGainTotalStride],
                                       (unsigned long long)(v * 8388608.0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // every wave's adds have completed before the workgroup takes its ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        // the frame's tickets sharded by chunk (cb & 7: mostly one shard per XCD under round-robin dispatch)
        const int xcd = cb & 7;
        const uint32_t in_xcd = (uint32_t)((n_chunks - xcd + 7) >> 3);
        int last = 0;
        if (__hip_atomic_fetch_add(&tickets[xcd], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_xcd - 1) {
            const uint32_t groups = (uint32_t)min(n_chunks, 8);
            last = __hip_atomic_fetch_add(&tickets[8], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    // ---- the last workgroup ------------------------------------------------------------------
    __shared__ int32_t s_N[kGainMaxCams * kGainMaxCams];
    if (tid < n * n) {
        const int i = tid / n, j = tid - i * n;
        const int32_t Nij = N[tid];
        s_N[tid] = Nij;
        const unsigned long long raw =
            __hip_atomic_exchange(&totals[(i * kGainMaxCams + j) * kGainTotalStride], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_I[tid] = (i != j) ? ((double)raw * 0x1p-23) / Nij : 0.0;
    }
    if (tid < 9) __hip_atomic_exchange(&tickets[tid], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid < n) gain_system_row(s_I, s_N, n, tid, s_A, s_b);
    __syncthreads();
    const bool ok = gain_solve<LEAN>(s_A, s_b, n, s_x, &s_last);
    if (tid < n) gains[tid] = ok ? s_x[tid] : 1.0;  // cv::solve failure leaves gains_ unspecified; 1 as the oracle
}

// octvr_debug_gain_solve: workgroup k solves system k of `count` n x n systems (row-major, row stride n) with
// gain_solve, the feed's own tail, on LDS copies as the feed holds them.  x[k * n ..] is written where ok[k] = 1.
template <bool LEAN>
__device__ __forceinline__ void gain_solve_body(const double* A, const double* b, int n, double* x, int* ok) {
    __shared__ int s_flag;
    __shared__ double s_A[kGainMaxCams * kGainMaxCams];
    __shared__ double s_b[kGainMaxCams];
    __shared__ double s_x[kGainMaxCams];
    const int tid = threadIdx.x;
    const size_t sys = blockIdx.x;
    if (tid < n * n) s_A[tid] = A[sys * (size_t)(n * n) + tid];
    if (tid < n) {
        s_b[tid] = b[sys * (size_t)n + tid];
        s_x[tid] = 0.0;
    }
    __syncthreads();
    const bool good = gain_solve<LEAN>(s_A, s_b, n, s_x, &s_flag);
    if (tid < n) x[sys * (size_t)n + tid] = good ? s_x[tid] : 0.0;
    if (tid == 0) ok[sys] = good ? 1 : 0;
}
__global__ void __launch_bounds__(256) gain_solve_kernel(const double* A, const double* b, int n, double* x, int* ok) {
    gain_solve_body<false>(A, b, n, x, ok);
}
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(80)))
gain_solve_lean_kernel(const double* A, const double* b, int n, double* x, int* ok) {
    gain_solve_body<true>(A, b, n, x, ok);
}

hipError_t launch_gain_solve(const double* A, const double* b, int n, int count, bool lean, double* x, int* ok,
                             hipStream_t s) {
    if (n < 1 || n > kGainMaxCams || count < 1) return hipErrorInvalidValue;
    if (lean)
        hipLaunchKernelGGL(gain_solve_lean_kernel, dim3(count), dim3(256), 0, s, A, b, n, x, ok);
    else
        hipLaunchKernelGGL(gain_solve_kernel, dim3(count), dim3(256), 0, s, A, b, n, x, ok);
    return hipGetLastError();
}

// NV12: the frames' chroma rows are U,V pairs (kPixInNv12)
template <int NF, bool NV12 = false>
__global__ void __launch_bounds__(256) gain_feed_kernel(FeedBatch<NF> batch, const CompositeEntry* samples,
                                                        const uint16_t* partners, int tex, int n_chunks, const int32_t* N,
                                                        int n) {
    (void)batch;  // read through the kernarg segment (kFeedBatch)
    gain_feed_body<false, NF, NV12>(samples, partners, tex, n_chunks, N, n);
}
template <int NF, bool NV12 = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(80)))
gain_feed_lean_kernel(FeedBatch<NF> batch, const CompositeEntry* samples, const uint16_t* partners, int tex, int n_chunks,
                      const int32_t* N, int n) {
    (void)batch;
    gain_feed_body<true, NF, NV12>(samples, partners, tex, n_chunks, N, n);
}

// One feed launch's runtime arguments (launch_gain_feed_batch's own, without the two it dispatches on)
struct FeedLaunch {
    const FrameSet* frames;
    const CompositeEntry* samples;
    const uint16_t* partners;
    int tex, n_chunks;
    const int32_t* N;
    int n;
    unsigned long long* const* totals;
    uint32_t* const* tickets;
    double* const* gains;
    hipStream_t s;
    bool lean;
};

template <int NF, bool NV12>
static void launch_feed_nf(const FeedLaunch& a) {
    FeedBatch<NF> fb;
    memset(&fb, 0, sizeof fb);
    for (int f = 0; f < NF; f++) {
        for (int i = 0; i < kGainMaxCams; i++) fb.src[f * kGainMaxCams + i] = a.frames[f].f[i];
        fb.totals[f] = a.totals[f];
        fb.tickets[f] = a.tickets[f];
        fb.gains[f] = a.gains[f];
    }
    if (a.lean)
        hipLaunchKernelGGL((gain_feed_lean_kernel<NF, NV12>), dim3(a.n_chunks * NF), dim3(256), 0, a.s, fb, a.samples,
                           a.partners, a.tex, a.n_chunks, a.N, a.n);
    else
        hipLaunchKernelGGL((gain_feed_kernel<NF, NV12>), dim3(a.n_chunks * NF), dim3(256), 0, a.s, fb, a.samples,
                           a.partners, a.tex, a.n_chunks, a.N, a.n);
}

template <bool NV12>
static void launch_feed(int nf, const FeedLaunch& a) {
    if (nf == 1)
        launch_feed_nf<1, NV12>(a);
    else if (nf == 2)
        launch_feed_nf<2, NV12>(a);
    else
        launch_feed_nf<4, NV12>(a);
}

hipError_t launch_gain_feed_batch(const FrameSet* frames, int nf, const CompositeEntry* samples, const uint16_t* partners,
                                  int tex, int n_chunks, const int32_t* N, int n, unsigned long long* const* totals,
                                  uint32_t* const* tickets, double* const* gains, hipStream_t s, bool lean, int pix) {
    if (n_chunks <= 0 || n > kGainMaxCams) return hipErrorInvalidValue;
    if (nf != 1 && nf != 2 && nf != 4) return hipErrorInvalidValue;
    const FeedLaunch a{frames, samples, partners, tex, n_chunks, N, n, totals, tickets, gains, s, lean};
    if (pix & kPixInNv12)
        launch_feed<true>(nf, a);
    else
        launch_feed<false>(nf, a);
    return hipGetLastError();
}

hipError_t launch_gain_feed(const FrameSet& frames, const CompositeEntry* samples, const uint16_t* partners, int tex,
                            int n_chunks, const int32_t* N, int n,
                            unsigned long long* totals, uint32_t* tickets, double* gains, hipStream_t s, bool lean, int pix) {
    return launch_gain_feed_batch(&frames, 1, samples, partners, tex, n_chunks, N, n, &totals, &tickets, &gains, s, lean,
                                  pix);
}

struct GainArgs {
    double g[kMaxCams];
};
__global__ void set_gains_kernel(GainArgs a, int n, double* gains) {
    if ((int)threadIdx.x < n) gains[threadIdx.x] = a.g[threadIdx.x];
}

hipError_t launch_set_gains(const double* host_gains, int n, double* gains_dev, hipStream_t s) {
    GainArgs a;
    for (int i = 0; i < kMaxCams; i++) a.g[i] = i < n ? host_gains[i] : 1.0;
    hipLaunchKernelGGL(set_gains_kernel, dim3(1), dim3(64), 0, s, a, n, gains_dev);
    return hipGetLastError();
}

// One workgroup per footprint run: its packed bytes into the camera's frame (byte stores of consecutive
// lanes: whole-line writes per wave).
__global__ void __launch_bounds__(256) unpack_runs_kernel(const uint8_t* packed, const FootRun* runs, FootFrames fr) {
    const FootRun r = runs[blockIdx.x];
    const int cam = (int)(r.cam & 31u), rp = (int)(r.cam >> 8);
    const int w = fr.w[cam], h = fr.h[cam];
    const int x0 = 8 * (int)r.g0, yb = min(8 * (int)(r.g0 + r.ng), w) - x0;
    const int c0 = 4 * (int)r.g0, cb = max(0, min(4 * (int)(r.g0 + r.ng), w / 2) - c0);
    const uint8_t* src = packed + r.off;
    uint8_t* const f = fr.f[cam];
    uint8_t* const d0 = f + (size_t)(2 * rp) * (size_t)w + x0;
    uint8_t* const d1 = d0 + w;
    uint8_t* const du = f + (size_t)(h + rp) * (size_t)w + c0;
    uint8_t* const dv = du + w / 2;
    const int tot = 2 * yb + 2 * cb;
    for (int k = threadIdx.x; k < tot; k += 256) {
        uint8_t* d = k < yb ? d0 + k : k < 2 * yb ? d1 + (k - yb) : k < 2 * yb + cb ? du + (k - 2 * yb) : dv + (k - 2 * yb - cb);
        *d = src[k];
    }
}

hipError_t launch_unpack_runs(const uint8_t* packed, const FootRun* runs, int n_runs, const FootFrames& frames,
                              hipStream_t s) {
    if (n_runs <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_runs_kernel, dim3(n_runs), dim3(256), 0, s, packed, runs, frames);
    return hipGetLastError();
}

}  // namespace octvr
