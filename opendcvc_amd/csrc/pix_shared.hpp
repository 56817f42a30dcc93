// pix_shared.hpp - what the streaming frame I/O kernels of dcvc_pixfmt.hip (4:2:0, 4:4:4) and dcvc_pix422.hip (4:2:2) share:
// the piece of a sample row a thread moves in the widest access its class allows, the two ends of the arithmetic
//   load   (float)s / (float)max_val, ONE rounding to the storage type
//   store  clip(., 0, 1) * max_val, rintf (nearest even), clip(0, max_val)      (Quant)
//   metric the store's value before the rounding                                (Metric)
// and the host check of the model frame these kernels read 8 pixels at a time.
#pragma once
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>

namespace {

constexpr int PB = 256;                       // threads per block

template <typename E, int VW>
struct alignas(sizeof(E) * VW) Pack {
    E v[VW];
};

constexpr int cmin(int a, int b) { return a < b ? a : b; }
constexpr int cmax(int a, int b) { return a > b ? a : b; }
// elements per access of an 8-element (luma, 4:4:4 chroma, UV pairs seen as samples) and of a 4-element (4:2:0 / 4:2:2 chroma
// samples or pairs) piece of a row at access class A (8, 4, 2, 1): at most 16 bytes
template <typename E>
constexpr int vw8(int A) { return cmin(A, 16 / (int)sizeof(E)); }
template <typename E>
constexpr int vw4(int A) { return cmin(cmax(A / 2, 1), 16 / (int)sizeof(E)); }

// o[0..N) = row[x .. x + N), columns past n - 1 clamped to n - 1 (replicate pad); VW elements per access where the
// whole piece lies inside the row
template <typename E, int N, int VW>
__device__ __forceinline__ void load_row(const E* row, int x, int n, E (&o)[N])
{
#pragma unroll
    for (int c = 0; c < N; c += VW) {
        if (x + c + VW <= n) {
            const Pack<E, VW> p = *reinterpret_cast<const Pack<E, VW>*>(row + x + c);
#pragma unroll
            for (int k = 0; k < VW; ++k) o[c + k] = p.v[k];
        } else {
#pragma unroll
            for (int k = 0; k < VW; ++k) o[c + k] = row[min(x + c + k, n - 1)];
        }
    }
}

// row[x .. x + N) = v[0..N) for the columns below n
template <typename E, int N, int VW>
__device__ __forceinline__ void store_row(E* row, int x, int n, const E (&v)[N])
{
#pragma unroll
    for (int c = 0; c < N; c += VW) {
        if (x + c + VW <= n) {
            Pack<E, VW> p;
#pragma unroll
            for (int k = 0; k < VW; ++k) p.v[k] = v[c + k];
            *reinterpret_cast<Pack<E, VW>*>(row + x + c) = p;
        } else {
#pragma unroll
            for (int k = 0; k < VW; ++k)
                if (x + c + k < n) row[x + c + k] = v[c + k];
        }
    }
}

template <typename T, typename S>
__device__ __forceinline__ T norm_sample(S s, int shift, float maxf)
{
    return to_t<T>((float)((unsigned)s >> shift) / maxf);
}

// what becomes of an fp32 plane value: the integer sample of a file ...
template <typename S>
struct Quant {
    typedef S E;
    int shift;
    float maxf;
    __device__ __forceinline__ S operator()(float v) const
    {
        v = clampf(v, 0.f, 1.f) * maxf;
        v = clampf(rintf(v), 0.f, maxf);
        return (S)((unsigned)v << shift);
    }
};
// ... or the value the metrics compare: the same product, not rounded
struct Metric {
    typedef float E;
    float maxf;
    __device__ __forceinline__ float operator()(float v) const { return clampf(v, 0.f, 1.f) * maxf; }
};

template <typename T>
__device__ __forceinline__ void load_pix8(const T* p, float (&f)[8])
{
    const Pix8<T> a = *reinterpret_cast<const Pix8<T>*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = (float)a.v[k];
}

// the frame the streaming storers read, 8 pixels per access
int check_frame8(const char* who, int dtype, const void* x, int Hp, int Wp, int H, int W)
{
    if (int rc = dcvc::check_frame(who, "the frame", dtype, x, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(Wp % 8 == 0 && ((uintptr_t)x & 15) == 0,
                 "%s: the frame (%d x %d) must be 16-byte aligned and have a width that is a multiple of 8", who, Hp, Wp);
    return 0;
}

inline unsigned blocks_for(int64_t threads) { return (unsigned)((threads + PB - 1) / PB); }

}  // namespace
