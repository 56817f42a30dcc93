// tf_shared.hpp - what the two translation units of the temporal pre-filter share (dcvc_tf.hip: pyramid, whole-pel search,
// gathering blend, noise estimate; dcvc_tf_subpel.hip: refinement, interpolating blend).  docs/temporal_filter.md defines each
// rule below once, and so does this file:
//   TB, TW, TH, NB, MAX_REFS, kScale, quant10     launch shapes and the 10-bit quantiser
//   U32x4, TfPlanes, TfRefs                       a 16-byte LDS access; kernel arguments: pyramids (or their Q0), frames + base weights
//   LevelDims / level_dims                        the three levels of a pyramid and their grids of 8 x 8 blocks
//   blend_level, blend_begin, block_weight, blend_accumulate, blend_finish, blend_total
//                                                 the blend around its sample fetch: level word, current row, weights, the unfused
//                                                 accumulation, the single rounding and the store, the luma statistic.  How the
//                                                 eight reference samples are obtained, the guards and the loads of mv / err are
//                                                 each kernel's own.
//   dcvc::overlaps, dcvc::check_planes, dcvc::blend
//                                                 host: byte ranges, the pyramid list of the search entries, and the blend's
//                                                 check-and-launch for a kernel the caller names
#pragma once
#include <cstdint>

#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

namespace {

constexpr int TB = 256;          // threads per workgroup, every kernel
constexpr int TW = 64;           // blend, noise: columns of a tile
constexpr int TH = 32;           // blend, noise: rows of a tile (TB / (TW / 8) threads of 8 columns)
constexpr int NB = 8;            // search, refinement: blocks per workgroup (32 lanes each)
constexpr int MAX_REFS = 4;
constexpr float kScale = 1023.0f;

__device__ __forceinline__ int quant10(float v)
{
    // (fmaxf returns the other operand for a NaN: a NaN sample counts as 0) - dcvc_frame_analyze's rule
    return (int)fminf(fmaxf(rintf(v * kScale), 0.0f), kScale);
}

struct alignas(16) U32x4 {
    uint32_t v[4];
};

struct TfPlanes {
    const uint16_t* cur;         // pyramids; a pyramid begins with its Q0
    const uint16_t* ref[MAX_REFS];
};

struct TfRefs {
    const void* ref[MAX_REFS];
    int base[MAX_REFS];          // B: 102 at distance 1, 77 at distance 2
};

struct LevelDims {
    int h[3], w[3];
    int64_t off[3];              // first element of a level in a pyramid
    int gh[3], gw[3];            // its grid of 8 x 8 blocks
    int64_t elems;
};

inline LevelDims level_dims(int H, int W)
{
    LevelDims d;
    d.h[0] = H;
    d.w[0] = W;
    for (int l = 1; l < 3; ++l) {
        d.h[l] = (d.h[l - 1] + 1) >> 1;
        d.w[l] = (d.w[l - 1] + 1) >> 1;
    }
    int64_t at = 0;
    for (int l = 0; l < 3; ++l) {
        d.off[l] = at;
        at += (int64_t)d.h[l] * d.w[l];
        d.gh[l] = (d.h[l] + 7) >> 3;
        d.gw[l] = (d.w[l] + 7) >> 3;
    }
    d.elems = at;
    return d;
}

// ---------------------------------------------------------------------------------- blend, device
// AUTO: the level is the word at level_dev (a compile-time switch: the fixed-level kernel keeps its code; its level_dev is
// null and not looked at).  One scalar load per workgroup, uniform.  level_dev is the kernel's FIRST parameter, and dcvc_tf.hip
// is built with the first two dwords of the kernel arguments preloaded into registers (csrc/Makefile): the pointer is there
// when a wave starts, so the word's cold scalar-cache miss runs beside that of the other arguments and not behind it.  With the
// pointer fetched like any argument tf_blend_kernel was 0.2 - 0.45 us slower than at a fixed level.
template <bool AUTO>
__device__ __forceinline__ void blend_level(const int32_t* level_dev, int& L, int& nref)
{
    if (AUTO) {
        L = *level_dev;
        if (L < 1 || L > 5) L = nref = 0;                 // level 0, or no level at all: every weight is 0
    }
}

// The current row's eight samples from column xc (a multiple of 8), sample i at column col(i) = min(xc + i, W - 1) - each
// kernel writes it the way its sample fetch forms the same column, so that the two are one computation; wide: the eight lie
// inside the picture and may be one 16-byte access.  acc starts as 256 x, wsum as 256.
template <typename T, typename Col>
__device__ __forceinline__ void blend_begin(const T* crow, int xc, bool wide, Col col, Pix8<T>& c, float* acc, int* qc, int* wsum)
{
    if (wide) {
        c = *reinterpret_cast<const Pix8<T>*>(crow + xc);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) c.v[i] = crow[col(i)];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float f = (float)c.v[i];
        qc[i] = quant10(f);
        acc[i] = 256.0f * f;
        wsum[i] = 256;
    }
}

// wb of a block whose error against the reference is err, at level L; base: the reference's B
__device__ __forceinline__ int block_weight(int base, uint32_t err, int L)
{
    const long long A = 1ll << (8 + L), E = (long long)err;
    return E < A ? (int)(((long long)base * (A * A - E * E)) >> (16 + 2 * L)) : 0;      // <= 102
}

// one reference's eight samples (fp32, or the storage type's: each is its fp32 value) at block weight wb: multiply and add stay
// two operations
template <typename S>
__device__ __forceinline__ void blend_accumulate(const S* rv, int wb, int L, const int* qc, float* acc, int* wsum)
{
    const int P = 1 << (3 + L);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float f = (float)rv[i];
        int d = qc[i] - quant10(f);
        d = d < 0 ? -d : d;
        const int w = d < P ? (wb * (P * P - d * d)) >> (6 + 2 * L) : 0;          // <= wb: 102 * 2^16 fits
        acc[i] = acc[i] + (float)w * f;
        wsum[i] += w;
    }
}

// ONE rounding to the storage type (an element no reference weighs on keeps its bits) and the store at orow + xc, clipped to
// Wp (VEC: one 16-byte access where all eight lie inside).  Returns the thread's part of the luma statistic, the sum of
// Wsum - 256 over its elements inside the picture's W columns, where `counted`; else 0.
template <typename T, bool VEC>
__device__ __forceinline__ long long blend_finish(const Pix8<T>& c, const float* acc, const int* wsum, T* orow, int xc, int Wp, int W,
                                                  bool counted)
{
    Pix8<T> o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float q = acc[i] * (1.0f / (float)wsum[i]);                     // (IEEE division: the fp32 nearest to 1 / Wsum)
        o.v[i] = wsum[i] == 256 ? c.v[i] : to_t<T>(q);
    }
    if (VEC && xc + 8 <= Wp) {
        *reinterpret_cast<Pix8<T>*>(orow + xc) = o;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (xc + i < Wp) orow[xc + i] = o.v[i];
    }
    long long stat = 0;
    if (counted) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (xc + i < W) stat += wsum[i] - 256;
    }
    return stat;
}

// the workgroup's statistic: wave -> LDS (s_part[TB / 64]) -> ONE 64-bit integer vector atomic, none for a sum of 0.  Every
// thread of the workgroup calls it.
__device__ __forceinline__ void blend_total(long long stat, long long* s_part, unsigned long long* total)
{
    const int tid = threadIdx.x;
    stat = wave_sum(stat);
    if ((tid & 63) == 0) s_part[tid >> 6] = stat;
    __syncthreads();
    if (tid == 0) {
        long long s = 0;
#pragma unroll
        for (int i = 0; i < TB / 64; ++i) s += s_part[i];
        if (s != 0) atomicAdd(total, (unsigned long long)s);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------- host
namespace dcvc {

inline bool overlaps(const void* a, uint64_t abytes, const void* b, uint64_t bbytes)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bbytes && pb < pa + abytes;
}

// the current pyramid and the list of nref (checked by the caller: 1 .. MAX_REFS) reference pyramids of a search entry
inline int check_planes(const char* who, const uint16_t* cur, const uint16_t* const* refs, int nref, TfPlanes& p)
{
    DCVC_REQUIRE(cur && refs, "%s: null pointer", who);
    DCVC_REQUIRE(((uintptr_t)cur & 1) == 0, "%s: a pointer is not 2-byte aligned", who);
    p = {};
    p.cur = cur;
    for (int r = 0; r < nref; ++r) {
        DCVC_REQUIRE(refs[r], "%s: null pointer", who);
        DCVC_REQUIRE(((uintptr_t)refs[r] & 1) == 0, "%s: a pyramid is not 2-byte aligned", who);
        p.ref[r] = refs[r];
    }
    return 0;
}

// The blend entries' checks and launch.  level_dev null: the level is the argument; else the word it points to, and level is
// not looked at.  K names the kernel: K::template kernel<T, VEC, AUTO>() is a __global__ function of tf_blend_kernel's
// parameters.  mv / err: whole-pel or quarter-pel, as the kernel reads them.
template <typename K>
int blend(const char* who, K, int dtype, const void* cur_nchw, const void* const* refs_nchw, const int* dists, int nref, int Hp, int Wp,
          int H, int W, const int16_t* mv, const uint32_t* err, int level, const int32_t* level_dev, void* out_nchw,
          uint64_t* weight_sum, void* stream)
{
    if (int rc = check_frame(who, "the current frame", dtype, cur_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = check_frame(who, "out", dtype, out_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(level_dev || (level >= 1 && level <= 5), "%s: level %d outside 1 .. 5", who, level);
    DCVC_REQUIRE(((uintptr_t)level_dev & 3) == 0, "%s: the level's word is not 4-byte aligned", who);
    DCVC_REQUIRE(nref >= 0 && nref <= MAX_REFS, "%s: %d references, at most %d are supported", who, nref, MAX_REFS);
    DCVC_REQUIRE(weight_sum && (nref == 0 || (refs_nchw && dists && mv && err)), "%s: null pointer", who);
    DCVC_REQUIRE((int64_t)H * W < ((int64_t)1 << 30), "%s: picture too large", who);
    const size_t es = elem_size(dtype);
    const uint64_t bytes = (uint64_t)3 * Hp * Wp * es;
    DCVC_REQUIRE(!overlaps(out_nchw, bytes, cur_nchw, bytes), "%s: out overlaps the current frame (neighbours are read)", who);
    TfRefs refs = {};
    for (int r = 0; r < nref; ++r) {
        if (int rc = check_frame(who, "a reference", dtype, refs_nchw[r], Hp, Wp, H, W)) return rc;
        DCVC_REQUIRE(!overlaps(out_nchw, bytes, refs_nchw[r], bytes), "%s: out overlaps reference %d (neighbours are read)", who, r);
        DCVC_REQUIRE(dists[r] == 1 || dists[r] == -1 || dists[r] == 2 || dists[r] == -2, "%s: distance %d is not +-1 or +-2", who,
                     dists[r]);
        refs.ref[r] = refs_nchw[r];
        refs.base[r] = (dists[r] == 1 || dists[r] == -1) ? 102 : 77;
    }
    DCVC_REQUIRE(((uintptr_t)mv & 1) == 0 && ((uintptr_t)err & 3) == 0 && ((uintptr_t)weight_sum & 7) == 0,
                 "%s: mv, err or the weight sum is not aligned to its element size", who);
    dim3 grid;
    if (int rc = tile_grid(who, Wp, Hp, TW, TH, grid)) return rc;
    const LevelDims d = level_dims(H, W);
    const bool vec = vec_ok(16 / (int)es, es, Wp, cur_nchw, out_nchw);
    unsigned long long* total = reinterpret_cast<unsigned long long*>(weight_sum);
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        with_flag(vec, [&](auto v) {
            with_flag(level_dev != nullptr, [&](auto a) {
                K::template kernel<T, decltype(v)::value, decltype(a)::value>()<<<grid, TB, 0, (hipStream_t)stream>>>(
                    level_dev, (const T*)cur_nchw, refs, nref, Hp, Wp, H, W, mv, err, d.gh[0], d.gw[0], level, (T*)out_nchw, total);
            });
        });
    });
}

}  // namespace dcvc
