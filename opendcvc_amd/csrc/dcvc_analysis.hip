// dcvc_analysis.hip - per-frame analysis of the encoder's input for the scene-cut decision (no reference counterpart: the
// reference harness places I frames by fi % intra_period only, test_video.py:164-176).  The luma plane of the model
// input is read where it lies, quantised to 10 bits per sample (ONE fp32 multiply, rintf, clamp) and summed over 8 x 8
// blocks into a low-resolution uint16 plane; everything after the quantisation is integer arithmetic, so the result does
// not depend on the reduction order and equals a numpy restatement bit for bit (tests/analysis_ref.py):
//   inter = sum |L - L_prev|                       (0 without a previous plane)
//   intra = sum min(|L - left|, |L - top|)         (first row: left only, first column: top only, block (0, 0): 0)
//   total = sum L
// Three launches: the luma pass (streaming: a thread reads 8 consecutive samples of two rows, 16 bytes per access in fp16,
// the four row pairs of a block are combined across lanes), the statistics of the low-resolution planes as per-workgroup
// integer partials, and one small launch that sums the partials into pinned host memory.  No LDS in the luma pass, no
// atomics anywhere.
#include "common.hpp"
#include "plane_math.hpp"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int AB = 256;            // threads per workgroup
constexpr int kBlocksPerWave = 16; // 8 x 8 blocks a wave of the luma pass owns: 16 blocks x 4 row pairs = 64 lanes
constexpr int kBlocksPerWg = kBlocksPerWave * (AB / 64);
constexpr int kMaxStatWgs = 64;    // workgroups of the statistics pass (grid-stride above 64 * 256 blocks: 1080p has 32640)
constexpr float kScale = 1023.0f;

template <typename E, int VW>
struct alignas(sizeof(E) * VW) Pack {
    E v[VW];
};

__device__ __forceinline__ unsigned quant10(float v)
{
    // (fmaxf returns the other operand for a NaN: a NaN sample counts as 0)
    return (unsigned)(int)fminf(fmaxf(rintf(v * kScale), 0.0f), kScale);
}

// sum of the quantised samples row[0 .. 8), VW elements per access
template <typename T, int VW>
__device__ __forceinline__ unsigned row_sum8(const T* row)
{
    unsigned s = 0;
#pragma unroll
    for (int c = 0; c < 8; c += VW) {
        const Pack<T, VW> p = *reinterpret_cast<const Pack<T, VW>*>(row + c);
#pragma unroll
        for (int k = 0; k < VW; ++k) s += quant10((float)p.v[k]);
    }
    return s;
}

// lane = (row pair << 4) | block of the wave: the 16 lanes of a row pair read 16 consecutive blocks of one row, i.e.
// 256 contiguous bytes of fp16 per access where the blocks do not wrap to the next block row
template <typename T, int VW>
__global__ __launch_bounds__(AB) void lowres_kernel(const T* luma, int64_t ld, int bw, int nblk, uint16_t* out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = (blockIdx.x * (AB / 64) + wave) * kBlocksPerWave + (lane & 15);
    const int pair = lane >> 4;
    unsigned s = 0;
    if (g < nblk) {
        const int by = g / bw, bx = g - by * bw;
        const T* p = luma + (int64_t)(by * 8 + pair * 2) * ld + bx * 8;
        s = row_sum8<T, VW>(p) + row_sum8<T, VW>(p + ld);
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (pair == 0 && g < nblk) out[g] = (uint16_t)s;      // at most 64 * 1023 = 65472
}

__device__ __forceinline__ unsigned absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

// partial[3 * workgroup + {0, 1, 2}] = the workgroup's share of inter, intra, total
__global__ __launch_bounds__(AB) void stats_partial_kernel(const uint16_t* cur, const uint16_t* prev, int bw, int nblk,
                                                           unsigned long long* partial)
{
    __shared__ unsigned long long red[AB];
    unsigned long long inter = 0, intra = 0, total = 0;
    for (int i = blockIdx.x * AB + threadIdx.x; i < nblk; i += gridDim.x * AB) {
        const int by = i / bw, bx = i - by * bw;
        const unsigned v = cur[i];
        total += v;
        if (prev) inter += absdiff(v, prev[i]);
        const unsigned dl = bx > 0 ? absdiff(v, cur[i - 1]) : 0u, dt = by > 0 ? absdiff(v, cur[i - bw]) : 0u;
        intra += (bx > 0 && by > 0) ? min(dl, dt) : dl + dt;     // (one of dl, dt is 0 on the first row / column)
    }
    inter = block_sum<AB>(inter, red);
    intra = block_sum<AB>(intra, red);
    total = block_sum<AB>(total, red);
    if (threadIdx.x == 0) {
        partial[3 * blockIdx.x + 0] = inter;
        partial[3 * blockIdx.x + 1] = intra;
        partial[3 * blockIdx.x + 2] = total;
    }
}

// out[0 .. 4) = inter, intra, total, number of blocks; `out` is the device address of pinned host memory
__global__ __launch_bounds__(AB) void stats_finish_kernel(const unsigned long long* partial, int nwg, int nblk,
                                                          unsigned long long* out)
{
    __shared__ unsigned long long red[AB];
    unsigned long long s[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < nwg; i += AB)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += partial[3 * i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = block_sum<AB>(s[k], red);
    if (threadIdx.x == 0) {
        out[0] = s[0];
        out[1] = s[1];
        out[2] = s[2];
        out[3] = (unsigned long long)nblk;
    }
}

inline bool size_ok(int H, int W)
{
    return H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && (int64_t)H * W <= (1ll << 30);
}
inline int stat_wgs(int nblk) { return std::min(kMaxStatWgs, (nblk + AB - 1) / AB); }

// the widest access (elements, at most 16 bytes) the base address and the row stride allow
inline int access_width(const void* p, int64_t ld, int es)
{
    int vw = 16 / es;
    while (vw > 1 && (((uintptr_t)p % (uintptr_t)(vw * es)) != 0 || ld % vw != 0)) vw >>= 1;
    return vw;
}

template <typename T>
void launch_lowres(const void* luma, int64_t ld, int bw, int nblk, uint16_t* out, hipStream_t st)
{
    const unsigned grid = (unsigned)((nblk + kBlocksPerWg - 1) / kBlocksPerWg);
    const T* p = (const T*)luma;
    switch (access_width(luma, ld, (int)sizeof(T))) {
    case 8:
        if constexpr (sizeof(T) == 2) lowres_kernel<T, 8><<<grid, AB, 0, st>>>(p, ld, bw, nblk, out);
        break;
    case 4: lowres_kernel<T, 4><<<grid, AB, 0, st>>>(p, ld, bw, nblk, out); break;
    case 2: lowres_kernel<T, 2><<<grid, AB, 0, st>>>(p, ld, bw, nblk, out); break;
    default: lowres_kernel<T, 1><<<grid, AB, 0, st>>>(p, ld, bw, nblk, out); break;
    }
}

}  // namespace

extern "C" {

int64_t dcvc_frame_analysis_ws_bytes(int H, int W)
{
    if (!size_ok(H, W)) {
        dcvc::set_error("dcvc_frame_analysis_ws_bytes: H and W must be multiples of 8, at least 8 (got %d x %d)", H, W);
        return dcvc::E_ARG;
    }
    return (int64_t)3 * sizeof(unsigned long long) * stat_wgs((H / 8) * (W / 8));
}

int dcvc_frame_analyze(int dtype, const void* luma, int64_t ld, int H, int W, const uint16_t* lowres_prev, uint16_t* lowres_out,
                       void* workspace, uint64_t* out_host, void* stream)
{
    const char* who = "dcvc_frame_analyze";
    DCVC_REQUIRE(dtype == DCVC_F16 || dtype == DCVC_F32, "%s: bad dtype %d", who, dtype);
    DCVC_REQUIRE(size_ok(H, W), "%s: H and W must be multiples of 8, at least 8 (got %d x %d)", who, H, W);
    DCVC_REQUIRE(luma && lowres_out && workspace && out_host, "%s: null pointer", who);
    DCVC_REQUIRE(ld >= W, "%s: row stride %lld below the row length %d", who, (long long)ld, W);
    DCVC_REQUIRE(((uintptr_t)luma % dcvc::elem_size(dtype)) == 0 && ((uintptr_t)workspace & 7) == 0 &&
                     (((uintptr_t)lowres_out | (uintptr_t)lowres_prev) & 1) == 0,
                 "%s: misaligned pointer", who);
    DCVC_REQUIRE(lowres_prev != lowres_out, "%s: the previous and the new low-resolution plane must differ", who);
    unsigned long long* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, out_host, 0));
    const int bw = W / 8, nblk = (H / 8) * bw, nwg = stat_wgs(nblk);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* partial = (unsigned long long*)workspace;
    if (dtype == DCVC_F16)
        launch_lowres<_Float16>(luma, ld, bw, nblk, lowres_out, st);
    else
        launch_lowres<float>(luma, ld, bw, nblk, lowres_out, st);
    DCVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_partial_kernel, dim3(nwg), dim3(AB), 0, st, (const uint16_t*)lowres_out, lowres_prev, bw, nblk,
                       partial);
    DCVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(AB), 0, st, (const unsigned long long*)partial, nwg, nblk, out_dev);
    DCVC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
