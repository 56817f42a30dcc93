// dcvc_metrics.hip - distortion metrics of a decoded frame on the device (the reference computes them on the host:
// test_video.py:94-127 get_distortion, src/utils/metrics.py:9-96): the unrounded planes the metrics compare, the sum of
// squared errors behind the PSNR, and the per-scale SSIM / contrast means behind MS-SSIM.
// All metric arithmetic is fp64 (var = E[a^2] - mu^2 cancels at values up to 65025) without contraction, reductions run
// in a fixed order (per-thread strided sums, a block tree, partials summed by index): the same input gives the same bits.
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr int MB = 256;          // threads per block
constexpr int kF64 = -1;         // internal element type: the fp64 planes of the coarser MS-SSIM scales

inline int mblocks(int64_t n) { return (int)((n + MB - 1) / MB); }
inline bool plane_type_ok(int t) { return t == DCVC_F16 || t == DCVC_F32 || t == DCVC_U8 || t == DCVC_U16; }

__device__ __forceinline__ double ldd(const void* p, int type, int64_t i)
{
    switch (type) {
    case DCVC_F16: return (double)static_cast<const _Float16*>(p)[i];
    case DCVC_F32: return (double)static_cast<const float*>(p)[i];
    case DCVC_U8: return (double)static_cast<const uint8_t*>(p)[i];
    case DCVC_U16: return (double)static_cast<const uint16_t*>(p)[i];
    default: return static_cast<const double*>(p)[i];
    }
}

// ------------------------------------------------------------------ metric planes
template <typename T>
__global__ void metric_planes_kernel(const T* x, int HP, int WP, int H, int W, T* yp, T* up, T* vp)
{
    const int64_t ny = (int64_t)H * W, nc = (int64_t)(H >> 1) * (W >> 1);
    const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (i >= ny + 2 * nc) return;
    if (i < ny) {
        st(yp, i, yuv420_luma<T>(x, WP, (int)(i / W), (int)(i % W)));
        return;
    }
    const int64_t j = i - ny;
    const int c = j < nc ? 1 : 2;
    const int64_t k = c == 1 ? j : j - nc;
    const int w2 = W >> 1;
    st(c == 1 ? up : vp, k, yuv420_chroma<T>(x + (int64_t)c * HP * WP, WP, (int)(k / w2), (int)(k % w2)));
}

// ------------------------------------------------------------------ squared error
__global__ __launch_bounds__(MB) void sse_partial_kernel(int ta, const void* a, int tb, const void* b, int64_t n, double* partial)
{
    __shared__ double red[MB];
    const int64_t stride = (int64_t)gridDim.x * MB;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x; i < n; i += stride) {
        const double d = ldd(a, ta, i) - ldd(b, tb, i);
        s = s + d * d;
    }
    s = block_sum<MB>(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[e] = (partial[off[e]] + ... + partial[off[e] + cnt[e] - 1]) / div[e], block e; `out` may be pinned host memory
constexpr int kMaxSums = 10;
struct SumArgs {
    int off[kMaxSums], cnt[kMaxSums];
    double div[kMaxSums];
};

__global__ __launch_bounds__(MB) void sum_partials_kernel(const double* partial, SumArgs a, double* out)
{
    __shared__ double red[MB];
    const int e = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < a.cnt[e]; i += MB) s = s + partial[a.off[e] + i];
    s = block_sum<MB>(s, red);
    if (threadIdx.x == 0) out[e] = s / a.div[e];
}

// ------------------------------------------------------------------ MS-SSIM
constexpr int MS_WIN = 11, MS_HALO = MS_WIN - 1;
constexpr int MS_TW = 32, MS_TH = 16;                          // outputs per block
constexpr int MS_SW = MS_TW + MS_HALO, MS_SH = MS_TH + MS_HALO; // staged input tile
constexpr int MS_MAX_LEVELS = 5;

struct Gauss {
    double g[MS_WIN];
};

// the next scale: ndimage.convolve(x, ones(2, 2) / 4, mode='reflect')[::2, ::2] (metrics.py:52-66) - the 2x2 box at
// even positions, the last row / column paired with itself at odd sizes
__global__ void msssim_down_kernel(int ta, const void* a, int tb, const void* b, int h, int w, double* oa, double* ob)
{
    const int h2 = (h + 1) >> 1, w2 = (w + 1) >> 1;
    const int i = blockIdx.x * MB + threadIdx.x;
    if (i >= h2 * w2) return;
    const int y = i / w2, x = i - y * w2;
    const int64_t r0 = (int64_t)(2 * y) * w, r1 = (int64_t)min(2 * y + 1, h - 1) * w;
    const int c0 = 2 * x, c1 = min(2 * x + 1, w - 1);
    oa[i] = 0.25 * (((ldd(a, ta, r0 + c0) + ldd(a, ta, r0 + c1)) + ldd(a, ta, r1 + c0)) + ldd(a, ta, r1 + c1));
    ob[i] = 0.25 * (((ldd(b, tb, r0 + c0) + ldd(b, tb, r0 + c1)) + ldd(b, tb, r1 + c0)) + ldd(b, tb, r1 + c1));
}

// One scale (calc_ssim, metrics.py:15-36, with the 11x11 Gaussian applied as a row pass and a column pass instead of by
// FFT): a block owns MS_TW x MS_TH positions of the 'valid' (h - 10) x (w - 10) maps, stages its input tile of both
// planes in LDS as fp64, forms the row sums of a, b, a*a, b*b, a*b in LDS, then per position the five windowed means,
// the ssim and cs values, and writes the block's two sums to partial[block] (ssim) and partial[blocks + block] (cs).
__global__ __launch_bounds__(MB) void msssim_level_kernel(int ta, const void* a, int tb, const void* b, int h, int w, Gauss gw,
                                                          double c1, double c2, double* partial)
{
    __shared__ double sa[MS_SH][MS_SW], sb[MS_SH][MS_SW];
    __shared__ double rp[5][MS_SH][MS_TW];
    __shared__ double red[MB];
    const int x0 = blockIdx.x * MS_TW, y0 = blockIdx.y * MS_TH;
    const int oh = h - MS_HALO, ow = w - MS_HALO;
    for (int it = threadIdx.x; it < MS_SH * MS_SW; it += MB) {
        const int r = it / MS_SW, c = it - r * MS_SW;
        const int y = y0 + r, x = x0 + c;
        const bool in = y < h && x < w;                      // (positions past the plane feed masked outputs only)
        const int64_t idx = (int64_t)y * w + x;
        sa[r][c] = in ? ldd(a, ta, idx) : 0.0;
        sb[r][c] = in ? ldd(b, tb, idx) : 0.0;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < MS_SH * MS_TW; it += MB) {
        const int r = it / MS_TW, c = it - r * MS_TW;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
        for (int k = 0; k < MS_WIN; ++k) {
            const double av = sa[r][c + k], bv = sb[r][c + k], g = gw.g[k];
            s0 = s0 + g * av;
            s1 = s1 + g * bv;
            s2 = s2 + g * (av * av);
            s3 = s3 + g * (bv * bv);
            s4 = s4 + g * (av * bv);
        }
        rp[0][r][c] = s0;
        rp[1][r][c] = s1;
        rp[2][r][c] = s2;
        rp[3][r][c] = s3;
        rp[4][r][c] = s4;
    }
    __syncthreads();
    double ssim = 0.0, cs = 0.0;
    for (int it = threadIdx.x; it < MS_TH * MS_TW; it += MB) {
        const int r = it / MS_TW, c = it - r * MS_TW;
        if (y0 + r >= oh || x0 + c >= ow) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < MS_WIN; ++k) {
            const double g = gw.g[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = m[q] + g * rp[q][r + k][c];
        }
        const double mu_a = m[0], mu_b = m[1];
        const double var_a = m[2] - mu_a * mu_a, var_b = m[3] - mu_b * mu_b, cov = m[4] - mu_a * mu_b;
        const double cs_num = 2.0 * cov + c2, cs_den = var_a + var_b + c2;
        cs = cs + cs_num / cs_den;
        ssim = ssim + ((2.0 * mu_a * mu_b + c1) * cs_num) / ((mu_a * mu_a + mu_b * mu_b + c1) * cs_den);
    }
    ssim = block_sum<MB>(ssim, red);
    cs = block_sum<MB>(cs, red);
    if (threadIdx.x == 0) {
        const int nb = gridDim.x * gridDim.y, bid = blockIdx.y * gridDim.x + blockIdx.x;
        partial[bid] = ssim;
        partial[nb + bid] = cs;
    }
}

// sizes of every scale and the layout of the workspace: the fp64 planes of scales 1.., then the per-block partial sums
struct MsPlan {
    int levels;
    int h[MS_MAX_LEVELS], w[MS_MAX_LEVELS], bx[MS_MAX_LEVELS], by[MS_MAX_LEVELS];
    int64_t off_a[MS_MAX_LEVELS], off_b[MS_MAX_LEVELS];   // in doubles (scale 0 reads the caller's planes)
    int64_t off_part;                                      // in doubles
    int part[MS_MAX_LEVELS];                               // offset of the scale's partials inside the partial area
    int64_t total;                                         // bytes
};

bool ms_plan(int H, int W, MsPlan& p)
{
    if (H < 88 || W < 88 || (int64_t)H * W > (1ll << 30)) return false;
    p.levels = (H >= 176 && W >= 176) ? 5 : 4;
    int64_t off = 0;
    int part = 0;
    for (int l = 0, h = H, w = W; l < p.levels; ++l, h = (h + 1) >> 1, w = (w + 1) >> 1) {
        p.h[l] = h;
        p.w[l] = w;
        p.bx[l] = (w - MS_HALO + MS_TW - 1) / MS_TW;
        p.by[l] = (h - MS_HALO + MS_TH - 1) / MS_TH;
        p.off_a[l] = p.off_b[l] = 0;
        if (l > 0) {
            p.off_a[l] = off;
            p.off_b[l] = off + (int64_t)h * w;
            off += 2 * (int64_t)h * w;
        }
        p.part[l] = part;
        part += 2 * p.bx[l] * p.by[l];
    }
    p.off_part = off;
    p.total = (off + part) * (int64_t)sizeof(double);
    return true;
}

}  // namespace

extern "C" {

int dcvc_frame_to_yuv420_planes(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* y, void* u, void* v,
                                void* stream)
{
    const char* who = "dcvc_frame_to_yuv420_planes";
    if (int rc = dcvc::check_frame(who, "the frame", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    const uintptr_t planes = (uintptr_t)y | (uintptr_t)u | (uintptr_t)v;
    DCVC_REQUIRE(y && u && v && planes % dcvc::elem_size(dtype) == 0 && H % 2 == 0 && W % 2 == 0,
                 "%s: a null or misaligned plane or an odd size (%d x %d)", who, H, W);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        metric_planes_kernel<T><<<mblocks((int64_t)H * W * 3 / 2), MB, 0, (hipStream_t)stream>>>(
            (const T*)x_nchw, Hp, Wp, H, W, (T*)y, (T*)u, (T*)v);
    });
}

int dcvc_sse(int a_type, const void* a, int b_type, const void* b, int64_t n, void* workspace, double* out_host, void* stream)
{
    DCVC_REQUIRE(a && b && workspace && out_host, "dcvc_sse: null pointer");
    DCVC_REQUIRE(plane_type_ok(a_type) && plane_type_ok(b_type), "dcvc_sse: bad element types %d, %d", a_type, b_type);
    DCVC_REQUIRE(n > 0 && n <= (1ll << 40), "dcvc_sse: bad size %lld", (long long)n);
    double* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, out_host, 0));
    const int nb = (int)std::min<int64_t>(DCVC_SSE_BLOCKS, (n + 4 * MB - 1) / (4 * MB));
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(sse_partial_kernel, dim3(nb), dim3(MB), 0, st, a_type, a, b_type, b, n, partial);
    DCVC_LAUNCH_CHECK();
    SumArgs sa = {};
    sa.cnt[0] = nb;
    sa.div[0] = 1.0;
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(MB), 0, st, (const double*)partial, sa, out_dev);
    DCVC_LAUNCH_CHECK();
    return 0;
}

int64_t dcvc_msssim_ws_bytes(int H, int W)
{
    MsPlan p;
    if (!ms_plan(H, W, p)) {
        dcvc::set_error("dcvc_msssim_ws_bytes: MS-SSIM needs planes of at least 88 x 88 (got %d x %d)", H, W);
        return dcvc::E_ARG;
    }
    return p.total;
}

int dcvc_msssim_stats(int a_type, const void* a, int b_type, const void* b, int H, int W, double data_range, void* workspace,
                      double* out_host, int* levels_out, void* stream)
{
    DCVC_REQUIRE(a && b && workspace && out_host, "dcvc_msssim_stats: null pointer");
    DCVC_REQUIRE(plane_type_ok(a_type) && plane_type_ok(b_type), "dcvc_msssim_stats: bad element types %d, %d", a_type, b_type);
    DCVC_REQUIRE(((uintptr_t)workspace & 7) == 0, "dcvc_msssim_stats: workspace not 8-byte aligned");
    MsPlan p;
    DCVC_REQUIRE(ms_plan(H, W, p), "dcvc_msssim_stats: MS-SSIM needs planes of at least 88 x 88 (got %d x %d)", H, W);
    double* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, out_host, 0));
    // 11-tap Gaussian, sigma 1.5, normalised: the 2-D window of fspecial_gauss (metrics.py:9-12) is its outer product
    Gauss gw;
    double gsum = 0.0;
    for (int k = 0; k < MS_WIN; ++k) {
        gw.g[k] = std::exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
        gsum += gw.g[k];
    }
    for (int k = 0; k < MS_WIN; ++k) gw.g[k] /= gsum;
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    double* partial = ws + p.off_part;
    SumArgs sa = {};
    const void *pa = a, *pb = b;
    int ta = a_type, tb = b_type;
    for (int l = 0; l < p.levels; ++l) {
        if (l > 0) {
            double *na = ws + p.off_a[l], *nb = ws + p.off_b[l];
            hipLaunchKernelGGL(msssim_down_kernel, dim3(mblocks((int64_t)p.h[l] * p.w[l])), dim3(MB), 0, st, ta, pa, tb, pb,
                               p.h[l - 1], p.w[l - 1], na, nb);
            DCVC_LAUNCH_CHECK();
            pa = na;
            pb = nb;
            ta = tb = kF64;
        }
        hipLaunchKernelGGL(msssim_level_kernel, dim3(p.bx[l], p.by[l]), dim3(MB), 0, st, ta, pa, tb, pb, p.h[l], p.w[l], gw, c1,
                           c2, partial + p.part[l]);
        DCVC_LAUNCH_CHECK();
        const int nblk = p.bx[l] * p.by[l];
        for (int q = 0; q < 2; ++q) {
            sa.off[2 * l + q] = p.part[l] + q * nblk;
            sa.cnt[2 * l + q] = nblk;
            sa.div[2 * l + q] = (double)(p.h[l] - MS_HALO) * (double)(p.w[l] - MS_HALO);
        }
    }
    hipLaunchKernelGGL(sum_partials_kernel, dim3(2 * p.levels), dim3(MB), 0, st, (const double*)partial, sa, out_dev);
    DCVC_LAUNCH_CHECK();
    if (levels_out) *levels_out = p.levels;
    return 0;
}

}  // extern "C"
