// dcvc_grain.hip - film-grain synthesis and estimation on model frames [3][Hp][Wp] (docs/film_grain.md, the normative text;
// tests/grain_ref.py restates it in numpy).  The model is stateless and integer up to its last step:
//   n(t, c, y, x)  a counter-based hash of (seed, t, plane, row, column), four bytes summed minus 510
//   g              n itself (corr 0), its 3 x 3 (corr 1) or 5 x 5 (corr 2) binomial, in integers
//   out            v + float(g * gain * s) * 2^-30: ONE fp32 add, ONE rounding to the storage type; p == 0 or a NaN: v's bits
// grain_apply_kernel: one launch for the three planes, a workgroup per TH x TW tile of one plane.  corr 0 hashes per pixel.
// corr 1 / 2: the tile plus a halo of R samples is hashed ONCE into LDS (one hash per LDS element, not 9 or 25 per pixel), the
// binomial runs separably out of LDS (rows into a second LDS image, columns in registers, 16 bytes per LDS read), and the
// strength lookup and the add work on 8 pixels per thread, 16 bytes per access where the tensors' addresses and row length
// allow it and element by element where they do not.  A sample's neighbours are never read, so out may be x.  The
// parameters are a by-value kernel argument: no table, no allocation, no synchronisation.
// grain_stats_kernel: a wave per whole 16 x 16 block of the picture, four pixels of a row per lane; everything behind the two
// roundings to integers is integer arithmetic, so the table does not depend on the order of summation.  Flat blocks are
// added to a workgroup's table in LDS and that to the int64 table in memory: 24 integer vector atomics per workgroup.
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int RB = 256;          // threads per workgroup
constexpr int TW = 64;           // columns of a tile
constexpr int TH = 32;           // rows of a tile: RB / (TW / 8) threads of 8 columns
constexpr int HS = TW + 4;       // row stride of the row-filtered image in LDS (ints): rows start one 16-byte slot apart
constexpr int FLAT_T = 1 << 26;
constexpr int TABLE_WORDS = 24;
constexpr int STATS_MAX_GROUPS = 1024;

struct GrainArgs {               // dcvc_grain_params as the kernel reads it
    uint32_t key;                // seed | (t & 0x3FFF) << 18; the plane's bits are added per workgroup
    int gain;
    uint64_t scale_y;            // band k in bits 8k .. 8k + 7
    int scale_c[2];
};

struct alignas(16) I4 {
    int v[4];
};

__device__ __forceinline__ int white(uint32_t a, int y, int x)
{
    uint32_t h = a + (uint32_t)(y + 2) * 0x85EBCA77u + (uint32_t)(x + 2) * 0xC2B2AE3Du;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return (int)((h & 255u) + ((h >> 8) & 255u) + ((h >> 16) & 255u) + (h >> 24)) - 510;
}

template <int R>
__device__ __forceinline__ int tap(int k)
{
    return R == 1 ? (k == 1 ? 2 : 1) : (k == 2 ? 6 : (k == 1 || k == 3) ? 4 : 1);
}

__device__ __forceinline__ int luma_strength(float f, uint64_t sy)
{
    const int q = (int)rintf(fminf(fmaxf(f, 0.0f), 1.0f) * 255.0f);
    const int k = min(max((q - 16) >> 5, 0), 6), fr = (q - 16) & 31;
    const int lo = (int)(sy >> (8 * k)) & 255, hi = (int)(sy >> (8 * k + 8)) & 255;
    const int mid = (lo * (32 - fr) + hi * fr + 16) >> 5;
    return q <= 16 ? (int)sy & 255 : q >= 240 ? (int)(sy >> 56) & 255 : mid;
}

template <typename T>
__device__ __forceinline__ T grain_one(T v, int g, int plane, const GrainArgs& p)
{
    const float f = (float)v;
    const int s = plane == 0 ? luma_strength(f, p.scale_y) : p.scale_c[plane - 1];
    const int prod = g * p.gain * s;
    if (prod == 0 || f != f) return v;
    return to_t<T>(f + (float)prod * 0x1p-30f);
}

// VEC: both tensors are 16-byte aligned and the row length is a multiple of 16 bytes
template <typename T, int R, bool VEC>
__global__ __launch_bounds__(RB) void grain_apply_kernel(const T* x, int Hp, int Wp, int H, int W, T* out, GrainArgs p)
{
    constexpr int NR = TH + 2 * R, NS = TW + 2 * R;                 // the hashed image: rows, and columns = row stride
    __shared__ int nbuf[R ? NR * NS : 1];
    __shared__ __attribute__((aligned(16))) int hbuf[R ? NR * HS : 4];

    const int tid = threadIdx.x, plane = blockIdx.z;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const uint32_t a = (p.key | (uint32_t)plane << 16) * 0x9E3779B1u;
    const bool live = y0 < H && x0 < W;                             // (uniform) a tile of the pad alone is copied
    const int vr = tid >> 3, vc = (tid & 7) * 8;
    const int y = y0 + vr, xc = x0 + vc;
    int g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = 0;

    if (R > 0 && live) {
        for (int i = tid; i < NR * NS; i += RB) {
            const int r = i / NS, c = i - r * NS;
            nbuf[i] = white(a, y0 + r - R, x0 + c - R);
        }
        __syncthreads();
        for (int i = tid; i < NR * TW; i += RB) {
            const int r = i / TW, c = i - r * TW;
            int acc = 0;
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) acc += tap<R>(k) * nbuf[r * NS + c + k];
            hbuf[r * HS + c] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            const int* hp = hbuf + (vr + k) * HS + vc;
            const I4 lo = *reinterpret_cast<const I4*>(hp), hi = *reinterpret_cast<const I4*>(hp + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                g[i] += tap<R>(k) * lo.v[i];
                g[4 + i] += tap<R>(k) * hi.v[i];
            }
        }
    } else if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = white(a, y, xc + i);
    }

    if (y >= Hp || xc >= Wp) return;
    const int64_t at = ((int64_t)plane * Hp + y) * Wp + xc;
    const bool row_in = live && y < H;
    if (VEC && xc + 8 <= Wp) {
        Pix8<T> px = *reinterpret_cast<const Pix8<T>*>(x + at);
        if (row_in) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (xc + i < W) px.v[i] = grain_one<T>(px.v[i], g[i], plane, p);
        }
        *reinterpret_cast<Pix8<T>*>(out + at) = px;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (xc + i < Wp) {
                const T v = x[at + i];
                out[at + i] = (row_in && xc + i < W) ? grain_one<T>(v, g[i], plane, p) : v;
            }
        }
    }
}

template <typename F>
void with_corr(int corr, F&& f)
{
    switch (corr) {
    case 0: f(dcvc::IC<0>{}); break;
    case 1: f(dcvc::IC<1>{}); break;
    default: f(dcvc::IC<2>{}); break;
    }
}

// ---------------------------------------------------------------------------------- estimation
// four pixels of row (lane >> 2) of the block at `at`, widened
template <typename T, bool VEC>
__device__ __forceinline__ void load4(const T* p, int64_t at, float* f)
{
    if (VEC) {
        struct alignas(4 * sizeof(T)) P4 {
            T v[4];
        };
        const P4 q = *reinterpret_cast<const P4*>(p + at);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (float)q.v[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (float)p[at + i];
    }
}

__device__ __forceinline__ int quant_d(float noisy, float clean)
{
    return (int)fminf(fmaxf(rintf((noisy - clean) * 4096.0f), -2047.0f), 2047.0f);
}

__device__ __forceinline__ void lds_add(unsigned long long* t, int line, long long count, long long sum)
{
    atomicAdd(t + 2 * line, (unsigned long long)count);
    atomicAdd(t + 2 * line + 1, (unsigned long long)sum);
}

// VEC: both tensors are aligned to four elements and the row length is a multiple of four
template <typename T, bool VEC>
__global__ __launch_bounds__(RB) void grain_stats_kernel(const T* __restrict__ noisy, const T* __restrict__ clean, int Hp, int Wp,
                                                         int bh, int bw, unsigned long long* __restrict__ table)
{
    __shared__ unsigned long long s_table[TABLE_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < TABLE_WORDS) s_table[tid] = 0ull;
    __syncthreads();
    const int nblk = bh * bw;
    const int64_t plane = (int64_t)Hp * Wp;
    const int r = lane >> 2, c4 = (lane & 3) * 4;
    for (int b = blockIdx.x * (RB / 64) + wave; b < nblk; b += gridDim.x * (RB / 64)) {
        const int by = b / bw, bx = b - by * bw;
        const int64_t at = (int64_t)(by * 16 + r) * Wp + bx * 16 + c4;
        float fn[4], fc[4];
        int d[4];
        long long sum_c = 0, sum_cc = 0, sum_d[3], sum_dd[3], lag_h = 0, lag_v = 0;
        // chroma first, so that d[] is luma's for the lag products
#pragma unroll
        for (int pl = 2; pl >= 0; --pl) {
            load4<T, VEC>(noisy, pl * plane + at, fn);
            load4<T, VEC>(clean, pl * plane + at, fc);
            int s1 = 0, s2 = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                d[i] = quant_d(fn[i], fc[i]);
                s1 += d[i];
                s2 += d[i] * d[i];
            }
            sum_d[pl] = s1;
            sum_dd[pl] = s2;
        }
        {
            int s1 = 0, s2 = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int cq = (int)fminf(fmaxf(rintf(fc[i] * 4096.0f), 0.0f), 4096.0f);
                s1 += cq;
                s2 += cq * cq;
            }
            sum_c = s1;
            sum_cc = s2;
            int h = d[0] * d[1] + d[1] * d[2] + d[2] * d[3];
            const int right = __shfl_down(d[0], 1, 64);
            if ((lane & 3) != 3) h += d[3] * right;
            int v = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int below = __shfl_down(d[i], 4, 64);
                if (lane < 60) v += d[i] * below;
            }
            lag_h = h;
            lag_v = v;
        }
        sum_c = wave_sum(sum_c);
        sum_cc = wave_sum(sum_cc);
        lag_h = wave_sum(lag_h);
        lag_v = wave_sum(lag_v);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            sum_d[pl] = wave_sum(sum_d[pl]);
            sum_dd[pl] = wave_sum(sum_dd[pl]);
        }
        if (lane == 0 && 256 * sum_cc - sum_c * sum_c <= (long long)FLAT_T) {
            const int band = (int)min(sum_c >> 17, 7ll);
            lds_add(s_table, band, 1, 256 * sum_dd[0] - sum_d[0] * sum_d[0]);
            lds_add(s_table, 8, 1, 256 * sum_dd[1] - sum_d[1] * sum_d[1]);
            lds_add(s_table, 9, 1, 256 * sum_dd[2] - sum_d[2] * sum_d[2]);
            lds_add(s_table, 10, 1, 65536 * lag_h - 240 * sum_d[0] * sum_d[0]);
            lds_add(s_table, 11, 1, 65536 * lag_v - 240 * sum_d[0] * sum_d[0]);
        }
    }
    __syncthreads();
    if (tid < TABLE_WORDS && s_table[tid] != 0ull) atomicAdd(table + tid, s_table[tid]);
}

}  // namespace

extern "C" {

int dcvc_grain_apply(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* out_nchw, dcvc_grain_params params,
                     uint32_t t, void* stream)
{
    const char* who = "dcvc_grain_apply";
    if (int rc = dcvc::check_frame(who, "x", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = dcvc::check_frame(who, "out", dtype, out_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(params.corr <= 2, "%s: corr %d above 2", who, (int)params.corr);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, Wp, Hp, TW, TH, grid)) return rc;
    static const int gains[3] = {3547, 591, 51};
    GrainArgs a;
    a.key = (uint32_t)params.seed | (t & 0x3FFFu) << 18;
    a.gain = gains[params.corr];
    a.scale_y = 0;
    for (int k = 0; k < 8; ++k) a.scale_y |= (uint64_t)params.scale_y[k] << (8 * k);
    a.scale_c[0] = params.scale_cb;
    a.scale_c[1] = params.scale_cr;
    const size_t es = dcvc::elem_size(dtype);
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, x_nchw, out_nchw);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        with_corr(params.corr, [&](auto r) {
            dcvc::with_flag(vec, [&](auto v) {
                grain_apply_kernel<T, decltype(r)::value, decltype(v)::value><<<grid, RB, 0, (hipStream_t)stream>>>(
                    (const T*)x_nchw, Hp, Wp, H, W, (T*)out_nchw, a);
            });
        });
    });
}

int dcvc_grain_stats(int dtype, const void* noisy_nchw, const void* clean_nchw, int Hp, int Wp, int H, int W, int64_t* table,
                     void* stream)
{
    const char* who = "dcvc_grain_stats";
    if (int rc = dcvc::check_frame(who, "noisy", dtype, noisy_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = dcvc::check_frame(who, "clean", dtype, clean_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(table && ((uintptr_t)table & 7) == 0, "%s: the table is null or not 8-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    DCVC_HIP(hipMemsetAsync(table, 0, TABLE_WORDS * sizeof(int64_t), st));
    const int bh = H / 16, bw = W / 16;
    if (bh == 0 || bw == 0) return 0;
    DCVC_REQUIRE((int64_t)bh * bw < ((int64_t)1 << 30), "%s: too many blocks", who);
    const int groups = (int)std::min<int64_t>(((int64_t)bh * bw + RB / 64 - 1) / (RB / 64), STATS_MAX_GROUPS);
    const bool vec = dcvc::vec_ok(4, dcvc::elem_size(dtype), Wp, noisy_nchw, clean_nchw);
    unsigned long long* tb = reinterpret_cast<unsigned long long*>(table);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            grain_stats_kernel<T, decltype(v)::value><<<groups, RB, 0, st>>>((const T*)noisy_nchw, (const T*)clean_nchw, Hp, Wp, bh, bw, tb);
        });
    });
}

}  // extern "C"
