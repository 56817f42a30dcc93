// dcvc_pix422.hip - 4:2:2 frame I/O (docs/pixel_formats_422.md): planar 8 .. 16 bits (yuv422p..), the packed 8-bit surfaces
// UYVY / YUYV and the packed 10-bit surface v210 <-> model frames.  The arithmetic continues dcvc_pixfmt.hip's:
//   load   (float)s / (float)max_val, ONE rounding to the storage type, chroma columns doubled (nearest), replicate pad
//   store  fp32 chroma (a + b) * 0.5f over the pixel pair, clip(., 0, 1) * max_val, rintf (nearest even), clip(0, max_val)
//   metric the store's values before the rounding, fp32 planes (dcvc_frame_to_metric_planes, chroma = 422)
// Streaming kernels, no LDS, no atomics, 16-byte accesses on the model side.  A planar or UYVY / YUYV thread owns 8 pixels of a
// row; the sample side moves in the widest access the addresses and pitches allow (chosen per launch, uniform over the grid;
// a packed surface is seen as 4-byte macropixels, so the classes are 16, 8 and 4 bytes).  A v210 thread owns 24 pixels: four
// 16-byte groups of 6 pixels on the surface, three 8-pixel pieces per plane on the model side.
#include "common.hpp"
#include "frame_host.hpp"
#include "pix_shared.hpp"
#include "plane_math.hpp"

#include <algorithm>
#include <cstdint>

namespace {

// ------------------------------------------------------------------ planar
template <typename T, typename S, int A>
__global__ __launch_bounds__(PB) void planar422_to_frame_kernel(const S* yp, const S* up, const S* vp, int64_t ys, int64_t cs, int H,
                                                                int W, int HO, int WO, float maxf, T* out)
{
    const int tw = WO >> 3;
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const int ty = (int)(i / tw), tx = (int)(i - (int64_t)ty * tw);
    if (ty >= HO) return;
    const int x0 = tx * 8, sy = min(ty, H - 1);
    const int64_t plane = (int64_t)HO * WO, o = (int64_t)ty * WO + x0;
    S s[8], u[4], v[4];
    load_row<S, 8, vw8<S>(A)>(yp + sy * ys, x0, W, s);
    // the clamped chroma column is the clamped luma column halved, W being even
    load_row<S, 4, vw4<S>(A)>(up + sy * cs, tx * 4, W >> 1, u);
    load_row<S, 4, vw4<S>(A)>(vp + sy * cs, tx * 4, W >> 1, v);
    Pix8<T> oy, ou, ov;
#pragma unroll
    for (int k = 0; k < 8; ++k) oy.v[k] = norm_sample<T, S>(s[k], 0, maxf);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ou.v[2 * k] = ou.v[2 * k + 1] = norm_sample<T, S>(u[k], 0, maxf);
        ov.v[2 * k] = ov.v[2 * k + 1] = norm_sample<T, S>(v[k], 0, maxf);
    }
    *reinterpret_cast<Pix8<T>*>(out + o) = oy;
    *reinterpret_cast<Pix8<T>*>(out + plane + o) = ou;
    *reinterpret_cast<Pix8<T>*>(out + 2 * plane + o) = ov;
}

// the 8 luma and the 4 + 4 chroma values of columns x0 .. x0 + 7 of row y, fp32, chroma (a + b) * 0.5f over the pair
template <typename T>
__device__ __forceinline__ void load_piece422(const T* x, int64_t plane, int64_t o, float (&fy)[8], float (&fu)[4], float (&fv)[4])
{
    float f[8];
    load_pix8(x + o, fy);
    load_pix8(x + plane + o, f);
#pragma unroll
    for (int k = 0; k < 4; ++k) fu[k] = (f[2 * k] + f[2 * k + 1]) * 0.5f;
    load_pix8(x + 2 * plane + o, f);
#pragma unroll
    for (int k = 0; k < 4; ++k) fv[k] = (f[2 * k] + f[2 * k + 1]) * 0.5f;
}

template <typename T, typename C, int A>
__global__ __launch_bounds__(PB) void frame_to_planar422_kernel(const T* x, int HP, int WP, int H, int W, C cvt, typename C::E* yp,
                                                                typename C::E* up, typename C::E* vp, int64_t ys, int64_t cs)
{
    typedef typename C::E E;
    const int tw = (W + 7) >> 3;
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const int ty = (int)(i / tw), tx = (int)(i - (int64_t)ty * tw);
    if (ty >= H) return;
    const int x0 = tx * 8;                                   // x0 + 7 < WP: WP is a multiple of 8 and x0 < W <= WP
    float fy[8], fu[4], fv[4];
    load_piece422(x, (int64_t)HP * WP, (int64_t)ty * WP + x0, fy, fu, fv);
    E qy[8], qu[4], qv[4];
#pragma unroll
    for (int k = 0; k < 8; ++k) qy[k] = cvt(fy[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        qu[k] = cvt(fu[k]);
        qv[k] = cvt(fv[k]);
    }
    store_row<E, 8, vw8<E>(A)>(yp + ty * ys, x0, W, qy);
    store_row<E, 4, vw4<E>(A)>(up + ty * cs, tx * 4, W >> 1, qu);
    store_row<E, 4, vw4<E>(A)>(vp + ty * cs, tx * 4, W >> 1, qv);
}

// ------------------------------------------------------------------ UYVY / YUYV: a surface of 4-byte macropixels
// byte k of a macropixel: UYVY = U Y0 V Y1, YUYV = Y0 U Y1 V (YFIRST)
template <bool YFIRST>
__device__ __forceinline__ void split_macro(uint32_t m, uint8_t& y0, uint8_t& y1, uint8_t& u, uint8_t& v)
{
    const uint8_t b0 = (uint8_t)m, b1 = (uint8_t)(m >> 8), b2 = (uint8_t)(m >> 16), b3 = (uint8_t)(m >> 24);
    if (YFIRST) {
        y0 = b0, u = b1, y1 = b2, v = b3;
    } else {
        u = b0, y0 = b1, v = b2, y1 = b3;
    }
}
template <bool YFIRST>
__device__ __forceinline__ uint32_t join_macro(uint32_t y0, uint32_t y1, uint32_t u, uint32_t v)
{
    return YFIRST ? (y0 | u << 8 | y1 << 16 | v << 24) : (u | y0 << 8 | v << 16 | y1 << 24);
}

// ms: the pitch in macropixels; VW: macropixels per access (4, 2, 1)
template <typename T, bool YFIRST, int VW>
__global__ __launch_bounds__(PB) void packed8_to_frame_kernel(const uint32_t* sp, int64_t ms, int H, int W, int HO, int WO, T* out)
{
    const int tw = WO >> 3;
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const int ty = (int)(i / tw), tx = (int)(i - (int64_t)ty * tw);
    if (ty >= HO) return;
    const int x0 = tx * 8, sy = min(ty, H - 1), n = W >> 1;
    const int64_t plane = (int64_t)HO * WO, o = (int64_t)ty * WO + x0;
    uint32_t m[4];
    load_row<uint32_t, 4, VW>(sp + sy * ms, tx * 4, n, m);
    Pix8<T> oy, ou, ov;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint8_t y0, y1, u, v;
        split_macro<YFIRST>(m[k], y0, y1, u, v);
        if (tx * 4 + k >= n) y0 = y1;                        // past the picture: column W - 1 is the last macropixel's Y1
        oy.v[2 * k] = norm_sample<T, uint8_t>(y0, 0, 255.0f);
        oy.v[2 * k + 1] = norm_sample<T, uint8_t>(y1, 0, 255.0f);
        ou.v[2 * k] = ou.v[2 * k + 1] = norm_sample<T, uint8_t>(u, 0, 255.0f);
        ov.v[2 * k] = ov.v[2 * k + 1] = norm_sample<T, uint8_t>(v, 0, 255.0f);
    }
    *reinterpret_cast<Pix8<T>*>(out + o) = oy;
    *reinterpret_cast<Pix8<T>*>(out + plane + o) = ou;
    *reinterpret_cast<Pix8<T>*>(out + 2 * plane + o) = ov;
}

template <typename T, bool YFIRST, int VW>
__global__ __launch_bounds__(PB) void frame_to_packed8_kernel(const T* x, int HP, int WP, int H, int W, uint32_t* sp, int64_t ms)
{
    const int tw = (W + 7) >> 3;
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const int ty = (int)(i / tw), tx = (int)(i - (int64_t)ty * tw);
    if (ty >= H) return;
    const int x0 = tx * 8;                                   // x0 + 7 < WP, as above
    float fy[8], fu[4], fv[4];
    load_piece422(x, (int64_t)HP * WP, (int64_t)ty * WP + x0, fy, fu, fv);
    const Quant<uint8_t> q{0, 255.0f};
    uint32_t m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = join_macro<YFIRST>(q(fy[2 * k]), q(fy[2 * k + 1]), q(fu[k]), q(fv[k]));
    store_row<uint32_t, 4, VW>(sp + ty * ms, tx * 4, W >> 1, m);
}

// ------------------------------------------------------------------ v210
// A group is 16 bytes, four little-endian words of three 10-bit slots each, 6 pixels (docs/pixel_formats_422.md):
//   slot   0   1   2   3   4   5   6   7   8   9   10  11
//          Cb0 Y0  Cr0 Y1  Cb1 Y2  Cr1 Y3  Cb2 Y4  Cr2 Y5          Y_k: slot 2 k + 1, Cb_j: slot 4 j, Cr_j: slot 4 j + 2
constexpr int V210_UNIT = 24;          // pixels of a thread: 4 groups, 3 pieces of 8

struct alignas(16) Group {
    uint32_t w[4];
};

// slot s of a group, s a compile-time constant after unrolling
__device__ __forceinline__ unsigned slot_of(const Group& g, int s) { return (g.w[s / 3] >> (10 * (s % 3))) & 1023u; }
// slot s of a group for an s only known at run time, without indexing the registers
__device__ __forceinline__ unsigned slot_dyn(const Group& g, int s)
{
    const int wi = s / 3;
    const uint32_t w = wi == 0 ? g.w[0] : (wi == 1 ? g.w[1] : (wi == 2 ? g.w[2] : g.w[3]));
    return (w >> (10 * (s - 3 * wi))) & 1023u;
}

// bs: the pitch in groups
template <typename T>
__global__ __launch_bounds__(PB) void v210_to_frame_kernel(const Group* sp, int64_t bs, int H, int W, int HO, int WO, T* out)
{
    const int tw = (WO + V210_UNIT - 1) / V210_UNIT;
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const int ty = (int)(i / tw), tx = (int)(i - (int64_t)ty * tw);
    if (ty >= HO) return;
    const int x0 = tx * V210_UNIT, sy = min(ty, H - 1);
    const int last = (W - 1) / 6;                            // the group that holds column W - 1; nothing past it is read
    const Group* row = sp + sy * bs;
    unsigned y[24], u[12], v[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const Group g = row[min(tx * 4 + j, last)];
#pragma unroll
        for (int k = 0; k < 6; ++k) y[6 * j + k] = slot_of(g, 2 * k + 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u[3 * j + k] = slot_of(g, 4 * k);
            v[3 * j + k] = slot_of(g, 4 * k + 2);
        }
    }
    if (x0 + V210_UNIT > W) {
        // columns at or past W (the replicate pad, and what the last group holds past the picture when W % 6 != 0) take
        // column W - 1, an odd column: pixel p = 1, 3 or 5 of the last group, chroma pair p >> 1
        const Group g = row[last];
        const int p = W - 1 - 6 * last;
        const unsigned ey = slot_dyn(g, 2 * p + 1), eu = slot_dyn(g, 4 * (p >> 1)), ev = slot_dyn(g, 4 * (p >> 1) + 2);
#pragma unroll
        for (int k = 0; k < 24; ++k)
            if (x0 + k >= W) y[k] = ey;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (x0 + 2 * k >= W) u[k] = eu, v[k] = ev;
    }
    const int64_t plane = (int64_t)HO * WO, o = (int64_t)ty * WO + x0;
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        if (x0 + 8 * pc >= WO) break;                        // a model row is a multiple of 8 wide, not of 24
        Pix8<T> oy, ou, ov;
#pragma unroll
        for (int k = 0; k < 8; ++k) oy.v[k] = to_t<T>((float)y[8 * pc + k] / 1023.0f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ou.v[2 * k] = ou.v[2 * k + 1] = to_t<T>((float)u[4 * pc + k] / 1023.0f);
            ov.v[2 * k] = ov.v[2 * k + 1] = to_t<T>((float)v[4 * pc + k] / 1023.0f);
        }
        *reinterpret_cast<Pix8<T>*>(out + o + 8 * pc) = oy;
        *reinterpret_cast<Pix8<T>*>(out + plane + o + 8 * pc) = ou;
        *reinterpret_cast<Pix8<T>*>(out + 2 * plane + o + 8 * pc) = ov;
    }
}

// a row is written for row_groups groups = dcvc_v210_row_bytes(W) / 16 (a multiple of 8): four per thread, samples of
// pixels at or past W zero
template <typename T>
__global__ __launch_bounds__(PB) void frame_to_v210_kernel(const T* x, int HP, int WP, int H, int W, int row_groups, Group* sp,
                                                           int64_t bs)
{
    const int tw = row_groups >> 2;
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const int ty = (int)(i / tw), tx = (int)(i - (int64_t)ty * tw);
    if (ty >= H) return;
    const int x0 = tx * V210_UNIT;
    const int64_t plane = (int64_t)HP * WP, o = (int64_t)ty * WP + x0;
    const Quant<uint16_t> q{0, 1023.0f};
    unsigned y[24], u[12], v[12];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        float fy[8], fu[4], fv[4];
        if (x0 + 8 * pc < WP)                                // (WP is a multiple of 8: the whole piece lies in the frame)
            load_piece422(x, plane, o + 8 * pc, fy, fu, fv);
        else {
#pragma unroll
            for (int k = 0; k < 8; ++k) fy[k] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) fu[k] = fv[k] = 0.f;
        }
        // by column, not by value: the frame may hold anything, NaN included, past the picture
#pragma unroll
        for (int k = 0; k < 8; ++k) y[8 * pc + k] = x0 + 8 * pc + k < W ? (unsigned)q(fy[k]) : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = x0 + 8 * pc + 2 * k < W;
            u[4 * pc + k] = in ? (unsigned)q(fu[k]) : 0u;
            v[4 * pc + k] = in ? (unsigned)q(fv[k]) : 0u;
        }
    }
    Group* dst = sp + ty * bs + tx * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned *yy = y + 6 * j, *uu = u + 3 * j, *vv = v + 3 * j;
        Group g;
        g.w[0] = uu[0] | yy[0] << 10 | vv[0] << 20;
        g.w[1] = yy[1] | uu[1] << 10 | yy[2] << 20;
        g.w[2] = vv[1] | yy[3] << 10 | uu[2] << 20;
        g.w[3] = yy[4] | vv[2] << 10 | yy[5] << 20;
        dst[j] = g;
    }
}

// ------------------------------------------------------------------ host side
using dcvc::IC;

template <typename F>
void with_access(int a, F&& f)
{
    switch (a) {
    case 8: f(IC<8>{}); break;
    case 4: f(IC<4>{}); break;
    case 2: f(IC<2>{}); break;
    default: f(IC<1>{}); break;
    }
}

// planar: the widest class (8, 4, 2, 1) the three planes allow, luma in vw8 and chroma in vw4 elements of `es` bytes
int planar_class(int es, const void* y, const void* u, const void* v, int64_t ys, int64_t cs)
{
    const int cap = 16 / es;
    int a = 8;
    for (; a > 1; a >>= 1)
        if (dcvc::vec_ok(std::min(a, cap), es, ys, y) && dcvc::vec_ok(std::min(std::max(a / 2, 1), cap), es, cs, u, v)) break;
    return a;
}

// UYVY / YUYV: macropixels per access (4, 2, 1 - 16, 8, 4 bytes); ms: the pitch in macropixels
int packed_class(const void* s, int64_t ms)
{
    int a = 4;
    for (; a > 1; a >>= 1)
        if (dcvc::vec_ok(a, 4, ms, s)) break;
    return a;
}

struct Fmt422 {
    int layout, ss;            // ss: bytes per sample of a planar plane
    float maxf;
    int64_t row_bytes;         // of a packed surface
};

// the argument checks both entries share; no device is touched
int check_422(const char* who, int dtype, int layout, int bit_depth, const void* y, const void* u, const void* v, int64_t ys,
              int64_t cs, int H, int W, Fmt422& f)
{
    DCVC_REQUIRE(dtype == DCVC_F16 || dtype == DCVC_F32, "%s: bad dtype %d", who, dtype);
    DCVC_REQUIRE(layout >= DCVC_422_PLANAR && layout <= DCVC_422_V210, "%s: unknown layout %d", who, layout);
    DCVC_REQUIRE(H > 0 && W > 0, "%s: bad size %d x %d", who, H, W);
    DCVC_REQUIRE(W % 2 == 0, "%s: 4:2:2 needs an even width (got %d x %d)", who, H, W);
    f.layout = layout;
    f.ss = bit_depth > 8 ? 2 : 1;
    f.maxf = (float)((1 << (bit_depth & 31)) - 1);
    f.row_bytes = 0;
    if (layout == DCVC_422_PLANAR) {
        DCVC_REQUIRE(bit_depth >= 8 && bit_depth <= 16, "%s: bit depth %d outside 8 .. 16", who, bit_depth);
        DCVC_REQUIRE(y && u && v, "%s: null plane", who);
        DCVC_REQUIRE(ys >= W && cs >= W / 2, "%s: row stride below the row length (%lld < %d or %lld < %d)", who, (long long)ys, W,
                     (long long)cs, W / 2);
        DCVC_REQUIRE((((uintptr_t)y | (uintptr_t)u | (uintptr_t)v) & (uintptr_t)(f.ss - 1)) == 0,
                     "%s: 16-bit plane not 2-byte aligned", who);
        return 0;
    }
    const bool v210 = layout == DCVC_422_V210;
    DCVC_REQUIRE(bit_depth == (v210 ? 10 : 8), "%s: bit depth %d (%s)", who, bit_depth,
                 v210 ? "v210 is 10 bits" : "UYVY / YUYV are 8 bits");
    DCVC_REQUIRE(y, "%s: null surface", who);
    f.row_bytes = v210 ? dcvc_v210_row_bytes(W) : (int64_t)2 * W;
    DCVC_REQUIRE(ys >= f.row_bytes, "%s: pitch %lld below the row length of %lld bytes", who, (long long)ys, (long long)f.row_bytes);
    const int unit = v210 ? 16 : 4;
    DCVC_REQUIRE((uintptr_t)y % unit == 0 && ys % unit == 0, "%s: the surface and its pitch must be multiples of %d bytes (%s)", who,
                 unit, v210 ? "a v210 group" : "a macropixel");
    return 0;
}

// f(S{}) with S the sample type of `ss` bytes
template <typename F>
void with_sample(int ss, F&& f)
{
    if (ss == 1)
        f(uint8_t{});
    else
        f(uint16_t{});
}

template <typename T, typename C>
void launch_planar_store(const C& cvt, const void* x, int HP, int WP, int H, int W, void* y, void* u, void* v, int64_t ys,
                         int64_t cs, hipStream_t st)
{
    typedef typename C::E E;
    const int a = planar_class((int)sizeof(E), y, u, v, ys, cs);
    const int64_t threads = (int64_t)((W + 7) / 8) * H;
    with_access(a, [&](auto at) {
        frame_to_planar422_kernel<T, C, decltype(at)::value><<<blocks_for(threads), PB, 0, st>>>((const T*)x, HP, WP, H, W, cvt,
                                                                                                (E*)y, (E*)u, (E*)v, ys, cs);
    });
}

}  // namespace

namespace dcvc {

int metric_planes_422(int dtype, int max_val, const void* x_nchw, int Hp, int Wp, int H, int W, float* y, float* u, float* v,
                      hipStream_t stream)
{
    const Metric m{(float)max_val};
    return typed(dtype, [&](auto tag) { launch_planar_store<decltype(tag)>(m, x_nchw, Hp, Wp, H, W, y, u, v, W, W / 2, stream); });
}

}  // namespace dcvc

extern "C" {

int64_t dcvc_v210_row_bytes(int W) { return W <= 0 ? -1 : ((int64_t)W + 47) / 48 * 128; }

int dcvc_yuv422_to_frame(int dtype, int layout, int bit_depth, const void* y_or_packed, const void* u, const void* v,
                         int64_t y_stride, int64_t c_stride, int H, int W, int pad_b, int pad_r, void* out_nchw, void* stream)
{
    const char* who = "dcvc_yuv422_to_frame";
    Fmt422 f;
    if (int rc = check_422(who, dtype, layout, bit_depth, y_or_packed, u, v, y_stride, c_stride, H, W, f)) return rc;
    DCVC_REQUIRE(out_nchw && pad_b >= 0 && pad_r >= 0, "%s: bad output arguments", who);
    const int HO = H + pad_b, WO = W + pad_r;
    DCVC_REQUIRE(WO % 8 == 0 && ((uintptr_t)out_nchw & 15) == 0,
                 "%s: the padded frame (%d x %d) must be 16-byte aligned and its width a multiple of 8", who, HO, WO);
    DCVC_REQUIRE((int64_t)3 * HO * WO < ((int64_t)1 << 40), "%s: the padded frame (%d x %d) is too large", who, HO, WO);
    hipStream_t st = (hipStream_t)stream;
    const int64_t threads8 = (int64_t)(WO / 8) * HO;
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        if (layout == DCVC_422_PLANAR) {
            const int a = planar_class(f.ss, y_or_packed, u, v, y_stride, c_stride);
            with_sample(f.ss, [&](auto s) {
                using S = decltype(s);
                with_access(a, [&](auto at) {
                    planar422_to_frame_kernel<T, S, decltype(at)::value><<<blocks_for(threads8), PB, 0, st>>>(
                        (const S*)y_or_packed, (const S*)u, (const S*)v, y_stride, c_stride, H, W, HO, WO, f.maxf, (T*)out_nchw);
                });
            });
        } else if (layout == DCVC_422_V210) {
            const int64_t threads = (int64_t)((WO + V210_UNIT - 1) / V210_UNIT) * HO;
            v210_to_frame_kernel<T><<<blocks_for(threads), PB, 0, st>>>((const Group*)y_or_packed, y_stride / 16, H, W, HO, WO,
                                                                        (T*)out_nchw);
        } else {
            const int64_t ms = y_stride / 4;
            dcvc::with_flag(layout == DCVC_422_YUYV, [&](auto yf) {
                with_access(packed_class(y_or_packed, ms), [&](auto at) {
                    constexpr int VW = decltype(at)::value > 4 ? 4 : decltype(at)::value;
                    packed8_to_frame_kernel<T, decltype(yf)::value, VW><<<blocks_for(threads8), PB, 0, st>>>(
                        (const uint32_t*)y_or_packed, ms, H, W, HO, WO, (T*)out_nchw);
                });
            });
        }
    });
}

int dcvc_frame_to_yuv422(int dtype, int layout, int bit_depth, const void* x_nchw, int Hp, int Wp, int H, int W, void* y_or_packed,
                         void* u, void* v, int64_t y_stride, int64_t c_stride, void* stream)
{
    const char* who = "dcvc_frame_to_yuv422";
    Fmt422 f;
    if (int rc = check_422(who, dtype, layout, bit_depth, y_or_packed, u, v, y_stride, c_stride, H, W, f)) return rc;
    if (int rc = check_frame8(who, dtype, x_nchw, Hp, Wp, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        if (layout == DCVC_422_PLANAR) {
            with_sample(f.ss, [&](auto s) {
                const Quant<decltype(s)> q{0, f.maxf};
                launch_planar_store<T>(q, x_nchw, Hp, Wp, H, W, y_or_packed, u, v, y_stride, c_stride, st);
            });
        } else if (layout == DCVC_422_V210) {
            const int row_groups = (int)(f.row_bytes / 16);
            frame_to_v210_kernel<T><<<blocks_for((int64_t)(row_groups / 4) * H), PB, 0, st>>>((const T*)x_nchw, Hp, Wp, H, W, row_groups,
                                                                                             (Group*)y_or_packed, y_stride / 16);
        } else {
            const int64_t ms = y_stride / 4;
            dcvc::with_flag(layout == DCVC_422_YUYV, [&](auto yf) {
                with_access(packed_class(y_or_packed, ms), [&](auto at) {
                    constexpr int VW = decltype(at)::value > 4 ? 4 : decltype(at)::value;
                    frame_to_packed8_kernel<T, decltype(yf)::value, VW><<<blocks_for((int64_t)((W + 7) / 8) * H), PB, 0, st>>>(
                        (const T*)x_nchw, Hp, Wp, H, W, (uint32_t*)y_or_packed, ms);
                });
            });
        }
    });
}

}  // extern "C"
