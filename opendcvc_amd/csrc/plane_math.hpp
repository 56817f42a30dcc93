// plane_math.hpp - the device helpers the kernels share: storage-type load / store, clamps, the 8-pixel piece of a model
// row, wave and workgroup sums, and the plane arithmetic of a reconstruction [3][HP][WP] seen as YUV 4:2:0, shared by
// dcvc_pixfmt.hip (frame_to_yuv420_kernel: the 8-bit planes) and dcvc_metrics.hip (metric_planes_kernel: the same values
// before they are rounded / truncated).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

template <typename T>
__device__ __forceinline__ float ld(const T* p, int64_t i)
{
    return (float)p[i];
}
// fp32 VALUE -> storage type.  The empty asm hides the value's producer, so the compiler cannot fold the preceding
// fp32 add / multiply into v_fma_mixlo_f16 (one rounding) in one kernel and leave add + cvt (two roundings) in another:
// the encoder's and the decoder's y_hat kernels must round alike (see Traits<half_t>::from_f, gemm_core.hpp).
template <typename T>
__device__ __forceinline__ T to_t(float v)
{
    asm("" : "+v"(v));
    return (T)v;
}
template <typename T>
__device__ __forceinline__ void st(T* p, int64_t i, float v)
{
    p[i] = to_t<T>(v);
}

__device__ __forceinline__ float clampf(float v, float lo, float hi)
{
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <typename T>
struct alignas(16) Pix8 {        // 8 pixels of a model row: one 16-byte access in fp16, two in fp32
    T v[8];
};

// sum of an integer over the 64 lanes of a wave; every lane gets the result
template <typename I>
__device__ __forceinline__ I wave_sum(I v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// sum over a workgroup of N threads in a fixed order (tree over the thread index, red[N] in LDS); every thread gets the
// result
template <int N, typename V>
__device__ __forceinline__ V block_sum(V v, V* red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    const V r = red[0];
    __syncthreads();     // (red is reused by the next sum)
    return r;
}

// clamp(x * 255, 0, 255) of luma sample (y, xw): the product rounded to the storage type, as torch does
// (test_video.py:97,307); the value is exactly representable in T
template <typename T>
__device__ __forceinline__ float yuv420_luma(const T* x, int WP, int y, int xw)
{
    const float s = (float)to_t<T>(ld(x, (int64_t)y * WP + xw) * 255.0f);
    return clampf(s, 0.f, 255.f);
}

// clamp(avg_pool2d(plane, 2) * 255, 0, 255) at chroma sample (y, xw) of the full-resolution plane `pl`
// (transforms.py:56-63, test_video.py:98,308): the 2x2 mean and the product each rounded to the storage type
template <typename T>
__device__ __forceinline__ float yuv420_chroma(const T* pl, int WP, int y, int xw)
{
    const float a = ld(pl, (int64_t)(2 * y) * WP + 2 * xw), b = ld(pl, (int64_t)(2 * y) * WP + 2 * xw + 1);
    const float d = ld(pl, (int64_t)(2 * y + 1) * WP + 2 * xw), e = ld(pl, (int64_t)(2 * y + 1) * WP + 2 * xw + 1);
    const float m = (float)to_t<T>(((a + b) + (d + e)) * 0.25f);                 // avg_pool2d(2) result in the storage type
    return clampf((float)to_t<T>(m * 255.0f), 0.f, 255.f);
}

}  // namespace
