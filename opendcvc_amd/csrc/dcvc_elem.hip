// dcvc_elem.hip - HBM-bound elementwise / layout kernels of the DCVC-RT path.
//  (1) layout kernels on HWC tensors, the z quantiser (round_z, z_from_int8) and copy_f32;
//  (2) the flat NCHW forms of the reference's operator module (inference_extensions_cuda,
//      kernel.cu:56-1004) with the reference's own signatures, for the operator seam.
// All arithmetic is fp32 with the shared deterministic math of include/dcvc_math.h; storage is
// _Float16 or float.
// (Frame I/O is dcvc_pixfmt.hip's; the checkerboard prior loop and the entropy hand-offs are dcvc_prior.hip's.)
#include "common.hpp"
#include "gemm_core.hpp"
#include "plane_math.hpp"   // ld / to_t / st / clampf

namespace {

using dcvc::typed;

constexpr int EB = 256;   // threads per block for 1-D kernels

inline int nblocks(int64_t n) { return (int)((n + EB - 1) / EB); }

// ------------------------------------------------------------------ layout kernels
template <typename T>
__global__ void unshuffle8_kernel(const T* x, int C, int H, int W, T* out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= (int64_t)C * H * W) return;
    const int xw = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / ((int64_t)W * H));
    const int W8 = W / 8;
    out[((int64_t)(y >> 3) * W8 + (xw >> 3)) * ldo + c * 64 + (y & 7) * 8 + (xw & 7)] = x[i];
}

// PixelUnshuffle(8) / PixelShuffle(8) through LDS: a block moves 32 output pixels of one row of the HWC map
// = C x 8 image rows x 256 columns.  Image rows are read / written as contiguous 512-byte (f16) runs,
// the HWC side as one contiguous run of 32 pixels x 64C channels; both sides use 16-byte accesses.
constexpr int S8_PIX = 32;

template <typename T>
__global__ __launch_bounds__(EB) void unshuffle8_tiled_kernel(const T* x, int C, int H, int W, T* out, int64_t ldo)
{
    constexpr int V = Traits<T>::kVec, COLS = S8_PIX * 8, VPR = COLS / V;   // vectors per image-row segment
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* tile = reinterpret_cast<T*>(smem);                                   // [C*8][COLS]
    const int W8 = W / 8, segs = (W8 + S8_PIX - 1) / S8_PIX;
    const int oh = blockIdx.x / segs, ow0 = (blockIdx.x % segs) * S8_PIX;
    const int npix = min(S8_PIX, W8 - ow0);
    const int rows = C * 8;
    for (int it = threadIdx.x; it < rows * VPR; it += EB) {
        const int r = it / VPR, v = it - r * VPR;                          // r = c*8 + (y & 7)
        if (v * V < npix * 8) {
            const int c = r >> 3, y = oh * 8 + (r & 7);
            *reinterpret_cast<Vec16*>(tile + r * COLS + v * V) =
                *reinterpret_cast<const Vec16*>(x + ((int64_t)c * H + y) * W + ow0 * 8 + v * V);
        }
    }
    __syncthreads();
    constexpr int G = 8 / V;                                               // 16-byte vectors per 8-element group
    for (int it = threadIdx.x; it < npix * rows * G; it += EB) {
        const int pix = it / (rows * G), rem = it - pix * (rows * G), r = rem / G, g = rem - r * G;
        *reinterpret_cast<Vec16*>(out + ((int64_t)oh * W8 + ow0 + pix) * ldo + r * 8 + g * V) =
            *reinterpret_cast<const Vec16*>(tile + r * COLS + pix * 8 + g * V);
    }
}

template <typename T>
__global__ __launch_bounds__(EB) void shuffle8_tiled_kernel(const T* x, int64_t ldx, const float* bias, int C, int H, int W,
                                                           int do_clamp, T* out)
{
    constexpr int V = Traits<T>::kVec, COLS = S8_PIX * 8, VPR = COLS / V, G = 8 / V;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* tile = reinterpret_cast<T*>(smem);                                   // [C*8][COLS]
    const int segs = (W + S8_PIX - 1) / S8_PIX;
    const int oh = blockIdx.x / segs, ow0 = (blockIdx.x % segs) * S8_PIX;
    const int npix = min(S8_PIX, W - ow0);
    const int rows = C * 8, HO = H * 8, WO = W * 8;
    for (int it = threadIdx.x; it < npix * rows * G; it += EB) {
        const int pix = it / (rows * G), rem = it - pix * (rows * G), r = rem / G, g = rem - r * G;
        float v[V];
        unpack16<T>(*reinterpret_cast<const Vec16*>(x + ((int64_t)oh * W + ow0 + pix) * ldx + r * 8 + g * V), v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (bias) v[j] = v[j] + bias[r * 8 + g * V + j];
            if (do_clamp) v[j] = clampf(v[j], 0.f, 1.f);
        }
        *reinterpret_cast<Vec16*>(tile + r * COLS + pix * 8 + g * V) = pack16<T>(v);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < rows * VPR; it += EB) {
        const int r = it / VPR, v = it - r * VPR;
        if (v * V < npix * 8) {
            const int c = r >> 3, y = oh * 8 + (r & 7);
            *reinterpret_cast<Vec16*>(out + ((int64_t)c * HO + y) * WO + ow0 * 8 + v * V) =
                *reinterpret_cast<const Vec16*>(tile + r * COLS + v * V);
        }
    }
}

template <typename T>
__global__ void shuffle8_kernel(const T* x, int64_t ldx, const float* bias, int C, int H, int W, int do_clamp, T* out)
{
    const int HO = H * 8, WO = W * 8;
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= (int64_t)C * HO * WO) return;
    const int xw = (int)(i % WO), y = (int)((i / WO) % HO), c = (int)(i / ((int64_t)WO * HO));
    const int ch = c * 64 + (y & 7) * 8 + (xw & 7);
    float v = ld(x, ((int64_t)(y >> 3) * W + (xw >> 3)) * ldx + ch);
    if (bias) v = v + bias[ch];
    if (do_clamp) v = clampf(v, 0.f, 1.f);
    st(out, i, v);
}

template <typename T>
__global__ void replicate_pad_hwc_kernel(const T* x, int64_t ldx, int H, int W, int C, int HO, int WO, T* out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= (int64_t)HO * WO * C) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int xw = (int)(p % WO), y = (int)(p / WO);
    const int sy = y < H ? y : H - 1, sx = xw < W ? xw : W - 1;
    out[p * ldo + c] = x[((int64_t)sy * W + sx) * ldx + c];
}

template <typename T>
__global__ void scale_channels_kernel(const T* x, int64_t ldx, const float* q, int64_t P, int C, T* out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= P * C) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    st(out, p * ldo + c, ld(x, p * ldx + c) * q[c]);
}

// same, 16 bytes per thread (C, ldx, ldo multiples of the vector width, 16-byte aligned bases)
template <typename T>
__global__ void scale_channels_vec_kernel(const T* x, int64_t ldx, const float* q, int64_t P, int C, T* out, int64_t ldo)
{
    constexpr int V = Traits<T>::kVec;
    const int gc = C / V;
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= P * gc) return;
    const int c = (int)(i % gc) * V;
    const int64_t p = i / gc;
    float v[V];
    unpack16<T>(*reinterpret_cast<const Vec16*>(x + p * ldx + c), v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = v[j] * q[c + j];
    *reinterpret_cast<Vec16*>(out + p * ldo + c) = pack16<T>(v);
}

template <typename T>
__global__ void copy_channels_kernel(const T* x, int64_t ldx, int64_t P, int C, T* out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= P * C) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    out[p * ldo + c] = x[p * ldx + c];
}

template <typename T>
__global__ void crop_hwc_kernel(const T* x, int64_t ldx, int W, int H2, int W2, int C, T* out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= (int64_t)H2 * W2 * C) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int xw = (int)(p % W2), y = (int)(p / W2);
    out[p * ldo + c] = x[((int64_t)y * W + xw) * ldx + c];
}

template <typename T>
__global__ void nchw_to_hwc_kernel(const T* x, int C, int64_t HW, T* out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= HW * C) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    out[p * ldo + c] = x[(int64_t)c * HW + p];
}

template <typename T>
__global__ void hwc_to_nchw_kernel(const T* x, int64_t ldx, int C, int64_t HW, T* out)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= HW * C) return;
    const int64_t p = i % HW;
    const int c = (int)(i / HW);
    out[i] = x[p * ldx + c];
}


// ------------------------------------------------------------------ z quantiser
template <typename T>
__global__ void round_z_kernel(T* z, int64_t ldz, int64_t HW, int C, int8_t* z_chw)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= HW * C) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const float v = clampf(dcvc_roundf(ld(z, p * ldz + c)), -128.f, 127.f);
    st(z, p * ldz + c, v);
    z_chw[(int64_t)c * HW + p] = (int8_t)v;
}

template <typename T>
__global__ void z_from_int8_kernel(const int8_t* z_chw, int64_t HW, int C, T* out, int64_t ldo)
{
    // consecutive threads read consecutive bytes of the CHW symbol array: it may live in pinned HOST memory (the decoder
    // hands the coder's output over without a copy command), where a strided byte read is a bus transaction each; the
    // scattered 2 / 4-byte writes go to device memory (65 K elements at 1080p)
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= HW * C) return;
    const int c = (int)(i / HW);
    const int64_t p = i - (int64_t)c * HW;
    st(out, p * ldo + c, (float)z_chw[i]);
}

// ------------------------------------------------------------------ operator-module (flat) kernels
template <typename T>
__global__ void op_process_with_mask_kernel(const T* y, const T* sc, const T* mu, const T* mask, float thres, T* y_res,
                                            T* y_q, T* y_hat, T* s_hat, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= n) return;
    const float mk = ld(mask, i);
    const float sh = ld(sc, i) * mk, mh = ld(mu, i) * mk;
    const float yr = (ld(y, i) - mh) * mk;
    float q = dcvc_roundf(yr);
    if (thres >= 0.f) q = q * (sh > thres ? 1.f : 0.f);
    q = clampf(q, -128.f, 127.f);
    st(y_res, i, yr);
    st(y_q, i, q);
    st(y_hat, i, q + mh);
    st(s_hat, i, sh);
}

template <typename T>
__global__ void op_combine_2x_kernel(T* out, const T* x, const T* mask, int64_t hn)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= hn) return;
    st(out, i, ld(x, i) * ld(mask, i) + ld(x, i + hn) * ld(mask, i + hn));
}

template <typename T>
__global__ void op_restore_kernel(T* out, const T* y, const T* mu, const T* mask, int64_t gn, int groups)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= gn) return;
    const float v = ld(y, i);
    for (int g = 0; g < groups; ++g) st(out, i + g * gn, (v + ld(mu, i + g * gn)) * ld(mask, i + g * gn));
}

template <typename T>
__global__ void op_build_index_kernel(int16_t* out_enc, uint8_t* out_dec, uint8_t* cond, const T* sym, const T* sc,
                                      float smin, float smax, float lmin, float lrec, float thres, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= n) return;
    const float s = clampf(ld(sc, i), smin, smax);
    const int idx = dcvc_scale_to_index(s, smin, smax, lmin, lrec);
    if (out_dec) out_dec[i] = (uint8_t)idx;
    if (out_enc) out_enc[i] = (int16_t)((int)ld(sym, i) * 256 + idx);
    if (cond) cond[i] = s > thres ? 1 : 0;
}

template <typename T>
__global__ void op_round_int8_kernel(T* z, int8_t* z8, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= n) return;
    const float v = clampf(dcvc_roundf(ld(z, i)), -128.f, 127.f);
    st(z, i, v);
    z8[i] = (int8_t)v;
}

template <typename T>
__global__ void op_clamp_recip_kernel(const T* q, T* y, float min_val, T* q_out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= n) return;
    float qv = ld(q, i);
    qv = qv < min_val ? min_val : qv;
    st(q_out, i, qv);
    st(y, i, ld(y, i) * (1.0f / qv));
}

template <typename T>
__global__ void op_add_mul_kernel(T* x0, const T* x1, const T* q, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= n) return;
    st(x0, i, (ld(x0, i) + ld(x1, i)) * ld(q, i));
}

template <typename T>
__global__ void op_bias_quant_kernel(T* x, const T* bias, const T* q, int C, int64_t HW)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= HW * C) return;
    const int c = (int)(i / HW);
    st(x, i, (ld(x, i) + ld(bias, c)) * ld(q, c));
}

template <typename T>
__global__ void op_ps8_kernel(T* out, const T* x, const T* bias, int C, int H, int W, int do_clamp)
{   // x: NCHW [C][H][W], out: [C/64][8H][8W]
    const int HO = H * 8, WO = W * 8, CO = C / 64;
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= (int64_t)CO * HO * WO) return;
    const int xw = (int)(i % WO), y = (int)((i / WO) % HO), c = (int)(i / ((int64_t)WO * HO));
    const int ch = c * 64 + (y & 7) * 8 + (xw & 7);
    float v = ld(x, ((int64_t)ch * H + (y >> 3)) * W + (xw >> 3)) + ld(bias, ch);
    if (do_clamp) v = clampf(v, 0.f, 1.f);
    st(out, i, v);
}

template <typename T>
__global__ void op_replicate_pad_kernel(const T* x, int C, int H, int W, int HO, int WO, T* out)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= (int64_t)C * HO * WO) return;
    const int xw = (int)(i % WO), y = (int)((i / WO) % HO), c = (int)(i / ((int64_t)WO * HO));
    const int sy = y < H ? y : H - 1, sx = xw < W ? xw : W - 1;
    out[i] = x[((int64_t)c * H + sy) * W + sx];
}

template <typename T>
__global__ void op_bias_wsilu_dw_kernel(const T* x, const T* w, const T* bias, int C, int H, int W, T* out)
{   // NCHW, w: [C][3][3]
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= (int64_t)C * H * W) return;
    const int xw = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / ((int64_t)W * H));
    const float b = ld(bias, c);
    float s = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y + ky - 1;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = xw + kx - 1;
            if (ix < 0 || ix >= W) continue;
            // activation rounded to the storage type like the reference's smem tile inputs
            const float av = (float)to_t<T>(dcvc_wsiluf(ld(x, ((int64_t)c * H + iy) * W + ix) + b));
            s = DCVC_FMAF(av, ld(w, c * 9 + ky * 3 + kx), s);
        }
    }
    st(out, i, s);
}

__global__ void copy_f32_kernel(float* dst, const float* src, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

}  // namespace

extern "C" {

int dcvc_unshuffle8(int dtype, const void* x, int C, int H, int W, void* out, int64_t ldo, void* stream)
{
    DCVC_REQUIRE(x && out && H % 8 == 0 && W % 8 == 0 && ldo >= C * 64, "dcvc_unshuffle8: bad arguments");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        constexpr int V = Traits<T>::kVec;
        const size_t lds = (size_t)C * 8 * S8_PIX * 8 * sizeof(T);
        const bool tiled = W % 8 == 0 && H % 8 == 0 && (W % V) == 0 && ldo % V == 0 && lds <= 64 * 1024 &&
                           ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
        if (tiled) {
            const int segs = (W / 8 + S8_PIX - 1) / S8_PIX;
            unshuffle8_tiled_kernel<T><<<(H / 8) * segs, EB, lds, (hipStream_t)stream>>>((const T*)x, C, H, W, (T*)out, ldo);
        } else {
            unshuffle8_kernel<T><<<nblocks((int64_t)C * H * W), EB, 0, (hipStream_t)stream>>>((const T*)x, C, H, W, (T*)out, ldo);
        }
    });
}

int dcvc_shuffle8_clamp(int dtype, const void* x, int64_t ld_, const float* bias, int C, int H, int W, int do_clamp,
                        void* out, void* stream)
{
    DCVC_REQUIRE(x && out && ld_ >= C * 64, "dcvc_shuffle8_clamp: bad arguments");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        constexpr int V = Traits<T>::kVec;
        const size_t lds = (size_t)C * 8 * S8_PIX * 8 * sizeof(T);
        const bool tiled = ld_ % V == 0 && lds <= 64 * 1024 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
        if (tiled) {
            const int segs = (W + S8_PIX - 1) / S8_PIX;
            shuffle8_tiled_kernel<T><<<H * segs, EB, lds, (hipStream_t)stream>>>((const T*)x, ld_, bias, C, H, W, do_clamp, (T*)out);
        } else {
            shuffle8_kernel<T><<<nblocks((int64_t)C * H * W * 64), EB, 0, (hipStream_t)stream>>>((const T*)x, ld_, bias, C, H, W, do_clamp, (T*)out);
        }
    });
}

int dcvc_replicate_pad_hwc(int dtype, const void* x, int64_t ldx, int H, int W, int C, int pad_b, int pad_r, void* out,
                           int64_t ldo, void* stream)
{
    DCVC_REQUIRE(x && out && pad_b >= 0 && pad_r >= 0 && H > 0 && W > 0, "dcvc_replicate_pad_hwc: bad arguments");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        replicate_pad_hwc_kernel<T><<<nblocks((int64_t)(H + pad_b) * (W + pad_r) * C), EB, 0, (hipStream_t)stream>>>((const T*)x, ldx, H, W, C,
                     H + pad_b, W + pad_r, (T*)out, ldo);
    });
}

int dcvc_scale_channels(int dtype, const void* x, int64_t ldx, const float* q, int64_t P, int C, void* out, int64_t ldo,
                        void* stream)
{
    DCVC_REQUIRE(x && out && q, "dcvc_scale_channels: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        constexpr int V = Traits<T>::kVec;
        const bool vec = C % V == 0 && ldx % V == 0 && ldo % V == 0 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
        if (vec)
            scale_channels_vec_kernel<T><<<nblocks(P * (C / V)), EB, 0, (hipStream_t)stream>>>((const T*)x, ldx, q, P, C, (T*)out, ldo);
        else
            scale_channels_kernel<T><<<nblocks(P * C), EB, 0, (hipStream_t)stream>>>((const T*)x, ldx, q, P, C, (T*)out, ldo);
    });
}

int dcvc_copy_channels(int dtype, const void* x, int64_t ldx, int64_t P, int C, void* out, int64_t ldo, void* stream)
{
    DCVC_REQUIRE(x && out, "dcvc_copy_channels: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        copy_channels_kernel<T><<<nblocks(P * C), EB, 0, (hipStream_t)stream>>>((const T*)x, ldx, P, C, (T*)out, ldo);
    });
}

int dcvc_crop_hwc(int dtype, const void* x, int64_t ldx, int W, int H2, int W2, int C, void* out, int64_t ldo, void* stream)
{
    DCVC_REQUIRE(x && out && W2 <= W, "dcvc_crop_hwc: bad arguments");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        crop_hwc_kernel<T><<<nblocks((int64_t)H2 * W2 * C), EB, 0, (hipStream_t)stream>>>((const T*)x, ldx, W, H2, W2, C, (T*)out, ldo);
    });
}

int dcvc_nchw_to_hwc(int dtype, const void* x, int C, int64_t HW, void* out, int64_t ldo, void* stream)
{
    DCVC_REQUIRE(x && out && ldo >= C, "dcvc_nchw_to_hwc: bad arguments");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        nchw_to_hwc_kernel<T><<<nblocks(HW * C), EB, 0, (hipStream_t)stream>>>((const T*)x, C, HW, (T*)out, ldo);
    });
}

int dcvc_hwc_to_nchw(int dtype, const void* x, int64_t ldx, int C, int64_t HW, void* out, void* stream)
{
    DCVC_REQUIRE(x && out && ldx >= C, "dcvc_hwc_to_nchw: bad arguments");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        hwc_to_nchw_kernel<T><<<nblocks(HW * C), EB, 0, (hipStream_t)stream>>>((const T*)x, ldx, C, HW, (T*)out);
    });
}

int dcvc_round_z(int dtype, void* z, int64_t ldz, int H, int W, int C, int8_t* z_chw, void* stream)
{
    DCVC_REQUIRE(z && z_chw, "dcvc_round_z: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        round_z_kernel<T><<<nblocks((int64_t)H * W * C), EB, 0, (hipStream_t)stream>>>((T*)z, ldz, (int64_t)H * W, C, z_chw);
    });
}

int dcvc_z_from_int8(int dtype, const int8_t* z_chw, int H, int W, int C, void* out, int64_t ldo, void* stream)
{
    DCVC_REQUIRE(z_chw && out, "dcvc_z_from_int8: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        z_from_int8_kernel<T><<<nblocks((int64_t)H * W * C), EB, 0, (hipStream_t)stream>>>(z_chw, (int64_t)H * W, C, (T*)out, ldo);
    });
}

// ---------------------------------------------------------------- operator-module seam
int dcvc_op_process_with_mask(int dtype, const void* y, const void* scales, const void* means, const void* mask,
                              float thres, void* y_res, void* y_q, void* y_hat, void* s_hat, int64_t n, void* stream)
{
    DCVC_REQUIRE(y && scales && means && mask && y_res && y_q && y_hat && s_hat, "dcvc_op_process_with_mask: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_process_with_mask_kernel<T><<<nblocks(n), EB, 0, (hipStream_t)stream>>>((const T*)y, (const T*)scales, (const T*)means,
                     (const T*)mask, thres, (T*)y_res, (T*)y_q, (T*)y_hat, (T*)s_hat, n);
    });
}

int dcvc_op_combine_for_reading_2x(int dtype, void* out, const void* x, const void* mask, int64_t half_n, void* stream)
{
    DCVC_REQUIRE(out && x && mask, "dcvc_op_combine_for_reading_2x: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_combine_2x_kernel<T><<<nblocks(half_n), EB, 0, (hipStream_t)stream>>>((T*)out, (const T*)x, (const T*)mask, half_n);
    });
}

int dcvc_op_restore_y_2x(int dtype, void* out, const void* y, const void* means, const void* mask, int64_t half_n,
                         void* stream)
{
    DCVC_REQUIRE(out && y && means && mask, "dcvc_op_restore_y_2x: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_restore_kernel<T><<<nblocks(half_n), EB, 0, (hipStream_t)stream>>>((T*)out, (const T*)y, (const T*)means, (const T*)mask, half_n, 2);
    });
}

int dcvc_op_restore_y_4x(int dtype, void* out, const void* y, const void* means, const void* mask, int64_t quarter_n,
                         void* stream)
{
    DCVC_REQUIRE(out && y && means && mask, "dcvc_op_restore_y_4x: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_restore_kernel<T><<<nblocks(quarter_n), EB, 0, (hipStream_t)stream>>>((T*)out, (const T*)y, (const T*)means, (const T*)mask, quarter_n, 4);
    });
}

int dcvc_op_build_index_dec(int dtype, uint8_t* out, uint8_t* cond_out, const void* scales, float scale_min,
                            float scale_max, float log_scale_min, float log_step_recip, float skip_thres, int64_t n,
                            void* stream)
{
    DCVC_REQUIRE(out && scales, "dcvc_op_build_index_dec: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_build_index_kernel<T><<<nblocks(n), EB, 0, (hipStream_t)stream>>>((int16_t*)nullptr, out, cond_out, (const T*)nullptr,
                     (const T*)scales, scale_min, scale_max, log_scale_min, log_step_recip, skip_thres, n);
    });
}

int dcvc_op_build_index_enc(int dtype, int16_t* out, uint8_t* cond_out, const void* symbols, const void* scales,
                            float scale_min, float scale_max, float log_scale_min, float log_step_recip,
                            float skip_thres, int64_t n, void* stream)
{
    DCVC_REQUIRE(out && symbols && scales, "dcvc_op_build_index_enc: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_build_index_kernel<T><<<nblocks(n), EB, 0, (hipStream_t)stream>>>(out, (uint8_t*)nullptr, cond_out, (const T*)symbols,
                     (const T*)scales, scale_min, scale_max, log_scale_min, log_step_recip, skip_thres, n);
    });
}

int dcvc_op_round_and_to_int8(int dtype, void* z, int8_t* z_int8, int64_t n, void* stream)
{
    DCVC_REQUIRE(z && z_int8, "dcvc_op_round_and_to_int8: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_round_int8_kernel<T><<<nblocks(n), EB, 0, (hipStream_t)stream>>>((T*)z, z_int8, n);
    });
}

int dcvc_op_clamp_reciprocal_with_quant(int dtype, const void* q_dec, void* y, float min_val, void* q_out, int64_t n,
                                        void* stream)
{
    DCVC_REQUIRE(q_dec && y && q_out, "dcvc_op_clamp_reciprocal_with_quant: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_clamp_recip_kernel<T><<<nblocks(n), EB, 0, (hipStream_t)stream>>>((const T*)q_dec, (T*)y, min_val, (T*)q_out, n);
    });
}

int dcvc_op_add_and_multiply(int dtype, void* x0, const void* x1, const void* q, int64_t n, void* stream)
{
    DCVC_REQUIRE(x0 && x1 && q, "dcvc_op_add_and_multiply: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_add_mul_kernel<T><<<nblocks(n), EB, 0, (hipStream_t)stream>>>((T*)x0, (const T*)x1, (const T*)q, n);
    });
}

int dcvc_op_bias_quant(int dtype, void* x, const void* bias, const void* quant, int C, int64_t HW, void* stream)
{
    DCVC_REQUIRE(x && bias && quant, "dcvc_op_bias_quant: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_bias_quant_kernel<T><<<nblocks(HW * C), EB, 0, (hipStream_t)stream>>>((T*)x, (const T*)bias, (const T*)quant, C, HW);
    });
}

int dcvc_op_bias_pixel_shuffle_8(int dtype, void* out, const void* x, const void* bias, int C, int H, int W, int do_clamp,
                                 void* stream)
{
    DCVC_REQUIRE(out && x && bias && C % 64 == 0, "dcvc_op_bias_pixel_shuffle_8: bad arguments");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_ps8_kernel<T><<<nblocks((int64_t)C * H * W), EB, 0, (hipStream_t)stream>>>((T*)out, (const T*)x, (const T*)bias, C, H, W, do_clamp);
    });
}

int dcvc_op_replicate_pad(int dtype, const void* x, int C, int H, int W, int pad_b, int pad_r, void* out, void* stream)
{
    DCVC_REQUIRE(x && out && pad_b >= 0 && pad_r >= 0, "dcvc_op_replicate_pad: bad arguments");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_replicate_pad_kernel<T><<<nblocks((int64_t)C * (H + pad_b) * (W + pad_r)), EB, 0, (hipStream_t)stream>>>((const T*)x, C, H, W,
                     H + pad_b, W + pad_r, (T*)out);
    });
}

int dcvc_op_bias_wsilu_depthwise_conv2d(int dtype, const void* x, const void* weight, const void* bias, int C, int H,
                                        int W, void* out, void* stream)
{
    DCVC_REQUIRE(x && weight && bias && out, "dcvc_op_bias_wsilu_depthwise_conv2d: null pointer");
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        op_bias_wsilu_dw_kernel<T><<<nblocks((int64_t)C * H * W), EB, 0, (hipStream_t)stream>>>((const T*)x, (const T*)weight, (const T*)bias, C,
                     H, W, (T*)out);
    });
}

int dcvc_copy_f32(float* dst, const float* src, int n, void* stream)
{
    DCVC_REQUIRE(dst && src && n >= 0, "dcvc_copy_f32: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(copy_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, dst, src, n);
    DCVC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
