// dcvc_pixfmt.hip - frame I/O: raw planes and RGB pictures <-> model frames.  First the streaming kernels of the raw formats:
// bit depths 8 .. 16 (little-endian 16-bit words above 8 bits, value in the low or in the top bits), 4:2:0 and 4:4:4, planar
// and semi-planar (NV12 / P010: one interleaved UV plane), rows with a pitch.  The arithmetic is the reference family's
// YUVReader / YUVWriter
// (DCVC-FM src/utils/video_reader.py:130-181, video_writer.py:85-128, src/transforms/functional.py:98-131):
//   load   (float)s / (float)max_val, ONE rounding to the storage type, nearest chroma up-sampling, replicate pad
//   store  fp32: 4:2:0 chroma ((a + b) + (d + e)) * 0.25f, clip(., 0, 1) * max_val, rintf (nearest even), clip(0, max_val)
//   metric the store's values before the rounding, fp32 planes
// These are streaming kernels: a thread owns 8 consecutive pixels of a row (4:2:0: an 8 x 2 luma block and the 4 chroma
// samples of both planes under it, read / formed once), the model side moves in 16-byte accesses, the sample side in the
// widest access the planes' addresses and strides allow (chosen per launch, uniform over the grid).  No LDS, no atomics.
// Then the older element-per-thread kernels of tight planar 8-bit 4:2:0 and of RGB (PNG sources), with the rounding rules
// of DCVC-RT's test_video.py.
#include "common.hpp"
#include "dcvc_math.h"
#include "frame_host.hpp"
#include "pix_shared.hpp"
#include "plane_math.hpp"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace dcvc {
// 4:2:2 metric planes: dcvc_pix422.hip's kernel behind dcvc_frame_to_metric_planes (arguments already checked)
int metric_planes_422(int dtype, int max_val, const void* x_nchw, int Hp, int Wp, int H, int W, float* y, float* u, float* v,
                      hipStream_t stream);
}  // namespace dcvc

namespace {

enum { L_420P = 0, L_420SP = 1, L_444P = 2 }; // plane layout of a launch

// an interleaved (U, V) pair of samples as one element: U in the low half (little-endian memory order U, V)
template <typename S>
struct PairOf;
template <>
struct PairOf<uint8_t> {
    typedef uint16_t type;
};
template <>
struct PairOf<uint16_t> {
    typedef uint32_t type;
};

// ------------------------------------------------------------------ planes -> padded model frame
template <typename T, typename S, int N, int VW>
__device__ __forceinline__ void load_plane_row(const S* row, int x0, int W, int shift, float maxf, T* dst)
{
    S s[N];
    load_row<S, N, VW>(row, x0, W, s);
    Pix8<T> o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o.v[k] = norm_sample<T, S>(s[k], shift, maxf);
    *reinterpret_cast<Pix8<T>*>(dst) = o;
}

template <typename T, typename S, int LAYOUT, int A>
__global__ __launch_bounds__(PB) void planes_to_frame_kernel(const S* yp, const void* up_, const S* vp, int64_t ys, int64_t cs,
                                                             int H, int W, int HO, int WO, int shift, float maxf, T* out)
{
    constexpr int RY = LAYOUT == L_444P ? 1 : 2;            // rows of the frame a thread owns
    const int tw = WO >> 3;
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const int ty = (int)(i / tw), tx = (int)(i - (int64_t)ty * tw);
    if (ty >= HO / RY) return;
    const int x0 = tx * 8;
    const int64_t plane = (int64_t)HO * WO;
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const int y = ty * RY + r, sy = min(y, H - 1);
        load_plane_row<T, S, 8, vw8<S>(A)>(yp + sy * ys, x0, W, shift, maxf, out + (int64_t)y * WO + x0);
    }
    if constexpr (LAYOUT == L_444P) {
        const int sy = min(ty, H - 1);
        load_plane_row<T, S, 8, vw8<S>(A)>(static_cast<const S*>(up_) + sy * cs, x0, W, shift, maxf,
                                           out + plane + (int64_t)ty * WO + x0);
        load_plane_row<T, S, 8, vw8<S>(A)>(vp + sy * cs, x0, W, shift, maxf, out + 2 * plane + (int64_t)ty * WO + x0);
    } else {
        // 4 chroma samples of each plane, each used for two columns and both rows (nearest up-sampling); the clamped
        // chroma coordinate is the clamped luma coordinate halved, H and W being even
        const int cy = min(ty, (H >> 1) - 1), cx0 = tx * 4, cn = W >> 1;
        S u[4], v[4];
        if constexpr (LAYOUT == L_420P) {
            load_row<S, 4, vw4<S>(A)>(static_cast<const S*>(up_) + cy * cs, cx0, cn, u);
            load_row<S, 4, vw4<S>(A)>(vp + cy * cs, cx0, cn, v);
        } else {
            typedef typename PairOf<S>::type P;
            P p[4];
            load_row<P, 4, vw4<P>(A)>(reinterpret_cast<const P*>(static_cast<const S*>(up_) + cy * cs), cx0, cn, p);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u[k] = (S)p[k];
                v[k] = (S)(p[k] >> (8 * sizeof(S)));
            }
        }
        Pix8<T> ou, ov;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ou.v[2 * k] = ou.v[2 * k + 1] = norm_sample<T, S>(u[k], shift, maxf);
            ov.v[2 * k] = ov.v[2 * k + 1] = norm_sample<T, S>(v[k], shift, maxf);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int64_t o = (int64_t)(2 * ty + r) * WO + x0;
            *reinterpret_cast<Pix8<T>*>(out + plane + o) = ou;
            *reinterpret_cast<Pix8<T>*>(out + 2 * plane + o) = ov;
        }
    }
}

// ------------------------------------------------------------------ model frame -> planes / metric planes
// (what becomes of an fp32 plane value, Quant or Metric: pix_shared.hpp)
template <typename T, typename C, int LAYOUT, int A>
__global__ __launch_bounds__(PB) void frame_to_planes_kernel(const T* x, int HP, int WP, int H, int W, C cvt, typename C::E* yp,
                                                             void* up_, typename C::E* vp, int64_t ys, int64_t cs)
{
    typedef typename C::E E;
    constexpr int RY = LAYOUT == L_444P ? 1 : 2;
    const int tw = (W + 7) >> 3;
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const int ty = (int)(i / tw), tx = (int)(i - (int64_t)ty * tw);
    if (ty >= H / RY) return;
    const int x0 = tx * 8;                                   // x0 + 7 < WP: WP is a multiple of 8 and x0 < W <= WP
    const int64_t plane = (int64_t)HP * WP;
    float f[8];
    E q[8];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const int y = ty * RY + r;
        load_pix8(x + (int64_t)y * WP + x0, f);
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = cvt(f[k]);
        store_row<E, 8, vw8<E>(A)>(yp + y * ys, x0, W, q);
    }
    if constexpr (LAYOUT == L_444P) {
#pragma unroll
        for (int c = 1; c < 3; ++c) {
            load_pix8(x + c * plane + (int64_t)ty * WP + x0, f);
#pragma unroll
            for (int k = 0; k < 8; ++k) q[k] = cvt(f[k]);
            store_row<E, 8, vw8<E>(A)>((c == 1 ? static_cast<E*>(up_) : vp) + ty * cs, x0, W, q);
        }
    } else {
        E uv[2][4];
#pragma unroll
        for (int c = 1; c < 3; ++c) {
            float d[8];
            load_pix8(x + c * plane + (int64_t)(2 * ty) * WP + x0, f);
            load_pix8(x + c * plane + (int64_t)(2 * ty + 1) * WP + x0, d);
#pragma unroll
            for (int k = 0; k < 4; ++k) uv[c - 1][k] = cvt(((f[2 * k] + f[2 * k + 1]) + (d[2 * k] + d[2 * k + 1])) * 0.25f);
        }
        const int cx0 = tx * 4, cn = W >> 1;
        if constexpr (LAYOUT == L_420P) {
            store_row<E, 4, vw4<E>(A)>(static_cast<E*>(up_) + ty * cs, cx0, cn, uv[0]);
            store_row<E, 4, vw4<E>(A)>(vp + ty * cs, cx0, cn, uv[1]);
        } else if constexpr (!std::is_same<E, float>::value) {
            typedef typename PairOf<E>::type P;
            P p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = (P)((P)uv[0][k] | ((P)uv[1][k] << (8 * sizeof(E))));
            store_row<P, 4, vw4<P>(A)>(reinterpret_cast<P*>(static_cast<E*>(up_) + ty * cs), cx0, cn, p);
        }
    }
}

// ------------------------------------------------------------------ YUV 4:2:0 <-> model frame
template <typename T>
__global__ void yuv420_to_frame_kernel(const uint8_t* yp, const uint8_t* up, const uint8_t* vp, int H, int W, int HO,
                                       int WO, T* out)
{
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= (int64_t)3 * HO * WO) return;
    const int xw = (int)(i % WO), y = (int)((i / WO) % HO), c = (int)(i / ((int64_t)WO * HO));
    const int sy = y < H ? y : H - 1, sx = xw < W ? xw : W - 1;        // replicate pad of the 4:4:4 frame
    int v;
    if (c == 0)
        v = yp[(int64_t)sy * W + sx];
    else
        v = (c == 1 ? up : vp)[(int64_t)(sy >> 1) * (W >> 1) + (sx >> 1)];   // nearest chroma upsampling
    st(out, i, (float)v / 255.0f);
}

template <typename T>
__global__ void frame_to_yuv420_kernel(const T* x, int HP, int WP, int H, int W, int round_uv, uint8_t* yp, uint8_t* up,
                                       uint8_t* vp)
{
    const int64_t ny = (int64_t)H * W, nc = (int64_t)(H >> 1) * (W >> 1);
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= ny + 2 * nc) return;
    if (i < ny) {
        const int xw = (int)(i % W), y = (int)(i / W);
        yp[i] = (uint8_t)dcvc_roundf(yuv420_luma<T>(x, WP, y, xw));
        return;
    }
    const int64_t j = i - ny;
    const int c = j < nc ? 1 : 2;
    const int64_t k = c == 1 ? j : j - nc;
    const int w2 = W >> 1;
    const int xw = (int)(k % w2), y = (int)(k / w2);
    float s = yuv420_chroma<T>(x + (int64_t)c * HP * WP, WP, y, xw);
    if (round_uv) s = dcvc_roundf(s);
    (c == 1 ? up : vp)[k] = (uint8_t)s;                                      // truncation like `.to(uint8)`
}

// ------------------------------------------------------------------ RGB (PNG sources) <-> model frame
// ITU-R BT.709 weights as the reference's transforms.py:7-10 spells them; the scalars below are the fp32 values torch
// uses when a Python float meets a float32 / float16 tensor.
__device__ __forceinline__ void rgb_consts(float& kr, float& kg, float& kb)
{
    kr = 0.2126f;
    kg = 0.7152f;
    kb = 0.0722f;
}

// uint8 planar RGB [3][H][W] -> padded YCbCr model input: /255 (test_video.py:60-63), rgb2ycbcr in fp32 with the reference's
// operation order and clamp (transforms.py:27-38), ONE rounding to the storage type (test_video.py:90), replicate pad (:179)
template <typename T>
__global__ void rgb_to_frame_kernel(const uint8_t* rgb, int H, int W, int HO, int WO, T* out)
{
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= (int64_t)HO * WO) return;
    const int xw = (int)(i % WO), y = (int)(i / WO);
    const int sy = y < H ? y : H - 1, sx = xw < W ? xw : W - 1;
    const int64_t sp = (int64_t)sy * W + sx, plane = (int64_t)H * W;
    const float r = (float)rgb[sp] / 255.0f, g = (float)rgb[plane + sp] / 255.0f, b = (float)rgb[2 * plane + sp] / 255.0f;
    float kr, kg, kb;
    rgb_consts(kr, kg, kb);
    const float yy = (kr * r + kg * g) + kb * b;
    const float cb = (0.5f * (b - yy)) / (float)(1.0 - 0.0722) + 0.5f;
    const float cr = (0.5f * (r - yy)) / (float)(1.0 - 0.2126) + 0.5f;
    const int64_t op = (int64_t)HO * WO;
    st(out, i, clampf(yy, 0.f, 1.f));
    st(out, op + i, clampf(cb, 0.f, 1.f));
    st(out, 2 * op + i, clampf(cr, 0.f, 1.f));
}

// reconstruction [3][HP][WP] (YCbCr) -> clamp(ycbcr2rgb(x) * 255, 0, 255) of the HxW picture as [3][H][W] in the storage type:
// every operation of transforms.py:41-53 + test_video.py:118-119 rounded to the storage type like the reference's tensors
// (fp16 reconstructions are converted in fp16 there); what the reference's RGB PSNR / MS-SSIM / PNG writer read
template <typename T>
__global__ void frame_to_rgb_kernel(const T* x, int HP, int WP, int H, int W, T* out)
{
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int xw = (int)(i % W), y = (int)(i / W);
    const int64_t sp = (int64_t)y * WP + xw, plane = (int64_t)HP * WP;
    auto q = [](float v) { return (float)to_t<T>(v); };
    const float yy = ld(x, sp), cb = ld(x, plane + sp), cr = ld(x, 2 * plane + sp);
    float kr, kg, kb;
    rgb_consts(kr, kg, kb);
    // (a Python scalar next to a half tensor enters torch's kernels in fp32 - the op-math type - not rounded to fp16)
    const float sr = (float)(2.0 - 2.0 * 0.2126), sb = (float)(2.0 - 2.0 * 0.0722);
    const float r = q(yy + q(sr * q(cr - 0.5f)));
    const float b = q(yy + q(sb * q(cb - 0.5f)));
    const float g = q(q(q(yy - q(kr * r)) - q(kb * b)) / kg);
    const int64_t op = (int64_t)H * W;
    st(out, i, clampf(q(clampf(r, 0.f, 1.f) * 255.0f), 0.f, 255.f));
    st(out, op + i, clampf(q(clampf(g, 0.f, 1.f) * 255.0f), 0.f, 255.f));
    st(out, 2 * op + i, clampf(q(clampf(b, 0.f, 1.f) * 255.0f), 0.f, 255.f));
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
template <typename F>
void with_layout(int layout, F&& f)
{
    switch (layout) {
    case L_420P: f(IC<L_420P>{}); break;
    case L_420SP: f(IC<L_420SP>{}); break;
    default: f(IC<L_444P>{}); break;
    }
}

// the widest access class (8, 4, 2, 1) every plane of the launch allows: `es` bytes per element; the luma plane (and
// 4:4:4 chroma, and UV pairs seen as samples) moves vw8 elements per access, planar 4:2:0 chroma vw4
int access_class(int layout, int es, const void* y, const void* u, const void* v, int64_t ys, int64_t cs)
{
    const int cap = 16 / es;
    int a = 8;
    for (; a > 1; a >>= 1) {
        const int w8 = std::min(a, cap), w4 = std::min(std::max(a / 2, 1), cap);
        bool ok = dcvc::vec_ok(w8, es, ys, y);
        if (layout == L_444P) ok = ok && dcvc::vec_ok(w8, es, cs, u, v);
        if (layout == L_420P) ok = ok && dcvc::vec_ok(w4, es, cs, u, v);
        if (layout == L_420SP) ok = ok && dcvc::vec_ok(2 * std::min(std::max(a / 2, 1), 16 / (2 * es)), es, cs, u);
        if (ok) break;
    }
    return a;
}

struct Fmt {
    int layout, shift, ss;     // ss: bytes per sample
    float maxf;
};

// the argument checks every entry shares; no device is touched
int check_format(const char* who, int dtype, int chroma, int bit_depth, int semi_planar, int msb_aligned, int H, int W, Fmt& f)
{
    DCVC_REQUIRE(dtype == DCVC_F16 || dtype == DCVC_F32, "%s: bad dtype %d", who, dtype);
    DCVC_REQUIRE(chroma == 420 || chroma == 444, "%s: chroma %d (420 or 444)", who, chroma);
    DCVC_REQUIRE(bit_depth >= 8 && bit_depth <= 16, "%s: bit depth %d outside 8 .. 16", who, bit_depth);
    DCVC_REQUIRE(!(msb_aligned && bit_depth == 8), "%s: 8-bit samples fill their byte, msb_aligned has no meaning", who);
    DCVC_REQUIRE(!(semi_planar && chroma != 420), "%s: the semi-planar layout is 4:2:0 (NV12 / P010)", who);
    DCVC_REQUIRE(H > 0 && W > 0, "%s: bad size %d x %d", who, H, W);
    DCVC_REQUIRE(chroma == 444 || (H % 2 == 0 && W % 2 == 0), "%s: 4:2:0 needs an even height and width (got %d x %d)", who, H, W);
    f.layout = chroma == 444 ? L_444P : (semi_planar ? L_420SP : L_420P);
    f.shift = msb_aligned ? 16 - bit_depth : 0;
    f.ss = bit_depth > 8 ? 2 : 1;
    f.maxf = (float)((1 << bit_depth) - 1);
    return 0;
}

int check_planes(const char* who, const Fmt& f, const void* y, const void* u, const void* v, int64_t ys, int64_t cs, int W)
{
    const bool sp = f.layout == L_420SP;
    DCVC_REQUIRE(y && u && (sp || v), "%s: null plane", who);
    const int64_t crow = f.layout == L_420P ? W / 2 : W;      // samples per chroma row (an interleaved row holds W)
    DCVC_REQUIRE(ys >= W && cs >= crow, "%s: row stride below the row length (%lld < %d or %lld < %lld)", who, (long long)ys, W,
                 (long long)cs, (long long)crow);
    const uintptr_t m = (uintptr_t)f.ss - 1;
    DCVC_REQUIRE((((uintptr_t)y | (uintptr_t)u | (uintptr_t)v) & m) == 0, "%s: 16-bit plane not 2-byte aligned", who);
    DCVC_REQUIRE(!sp || ((uintptr_t)u % (uintptr_t)(2 * f.ss) == 0 && cs % 2 == 0),
                 "%s: the interleaved plane and its stride must be aligned to a (U, V) pair", who);
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

template <typename T, typename S>
void launch_load(const Fmt& f, const void* y, const void* u, const void* v, int64_t ys, int64_t cs, int H, int W, int HO, int WO,
                 void* out, hipStream_t st)
{
    const int a = access_class(f.layout, f.ss, y, u, v, ys, cs);
    const int64_t threads = (int64_t)(WO / 8) * (HO / (f.layout == L_444P ? 1 : 2));
    with_layout(f.layout, [&](auto lt) {
        with_access(a, [&](auto at) {
            planes_to_frame_kernel<T, S, decltype(lt)::value, decltype(at)::value><<<blocks_for(threads), PB, 0, st>>>(
                (const S*)y, u, (const S*)v, ys, cs, H, W, HO, WO, f.shift, f.maxf, (T*)out);
        });
    });
}

template <typename T, typename C>
void launch_store(int layout, const C& cvt, const void* x, int HP, int WP, int H, int W, void* y, void* u, void* v, int64_t ys,
                  int64_t cs, hipStream_t st)
{
    typedef typename C::E E;
    const int a = access_class(layout, (int)sizeof(E), y, u, v, ys, cs);
    const int64_t threads = (int64_t)((W + 7) / 8) * (H / (layout == L_444P ? 1 : 2));
    with_layout(layout, [&](auto lt) {
        with_access(a, [&](auto at) {
            frame_to_planes_kernel<T, C, decltype(lt)::value, decltype(at)::value><<<blocks_for(threads), PB, 0, st>>>(
                (const T*)x, HP, WP, H, W, cvt, (E*)y, u, (E*)v, ys, cs);
        });
    });
}

}  // namespace

extern "C" {

int dcvc_planes_to_frame(int dtype, int chroma, int bit_depth, int semi_planar, int msb_aligned, const void* y,
                         const void* u_or_uv, const void* v, int64_t y_stride, int64_t c_stride, int H, int W, int pad_b,
                         int pad_r, void* out_nchw, void* stream)
{
    const char* who = "dcvc_planes_to_frame";
    Fmt f;
    if (int rc = check_format(who, dtype, chroma, bit_depth, semi_planar, msb_aligned, H, W, f)) return rc;
    if (int rc = check_planes(who, f, y, u_or_uv, v, y_stride, c_stride, W)) return rc;
    DCVC_REQUIRE(out_nchw && pad_b >= 0 && pad_r >= 0, "%s: bad output arguments", who);
    const int HO = H + pad_b, WO = W + pad_r;
    DCVC_REQUIRE(WO % 8 == 0 && ((uintptr_t)out_nchw & 15) == 0 && (f.layout == L_444P || HO % 2 == 0),
                 "%s: the padded frame (%d x %d) must be 16-byte aligned, its width a multiple of 8 and, for 4:2:0, its "
                 "height even", who, HO, WO);
    return dcvc::typed(dtype, [&](auto tag) {
        with_sample(f.ss, [&](auto s) {
            launch_load<decltype(tag), decltype(s)>(f, y, u_or_uv, v, y_stride, c_stride, H, W, HO, WO, out_nchw, (hipStream_t)stream);
        });
    });
}

int dcvc_frame_to_planes(int dtype, int chroma, int bit_depth, int semi_planar, int msb_aligned, const void* x_nchw, int Hp,
                         int Wp, int H, int W, void* y, void* u_or_uv, void* v, int64_t y_stride, int64_t c_stride, void* stream)
{
    const char* who = "dcvc_frame_to_planes";
    Fmt f;
    if (int rc = check_format(who, dtype, chroma, bit_depth, semi_planar, msb_aligned, H, W, f)) return rc;
    if (int rc = check_planes(who, f, y, u_or_uv, v, y_stride, c_stride, W)) return rc;
    if (int rc = check_frame8(who, dtype, x_nchw, Hp, Wp, H, W)) return rc;
    return dcvc::typed(dtype, [&](auto tag) {
        with_sample(f.ss, [&](auto s) {
            const Quant<decltype(s)> q{f.shift, f.maxf};
            launch_store<decltype(tag)>(f.layout, q, x_nchw, Hp, Wp, H, W, y, u_or_uv, v, y_stride, c_stride, (hipStream_t)stream);
        });
    });
}

int dcvc_frame_to_metric_planes(int dtype, int chroma, int max_val, const void* x_nchw, int Hp, int Wp, int H, int W, float* y,
                                float* u, float* v, void* stream)
{
    const char* who = "dcvc_frame_to_metric_planes";
    DCVC_REQUIRE(chroma == 420 || chroma == 422 || chroma == 444, "%s: chroma %d (420, 422 or 444)", who, chroma);
    DCVC_REQUIRE(max_val >= 255 && max_val <= 65535, "%s: max_val %d outside 255 .. 65535", who, max_val);
    DCVC_REQUIRE(chroma != 420 || (H % 2 == 0 && W % 2 == 0), "%s: 4:2:0 needs an even height and width (got %d x %d)", who, H, W);
    DCVC_REQUIRE(chroma != 422 || W % 2 == 0, "%s: 4:2:2 needs an even width (got %d x %d)", who, H, W);
    DCVC_REQUIRE(y && u && v && (((uintptr_t)y | (uintptr_t)u | (uintptr_t)v) & 3) == 0, "%s: null or misaligned plane", who);
    if (int rc = check_frame8(who, dtype, x_nchw, Hp, Wp, H, W)) return rc;
    if (chroma == 422) return dcvc::metric_planes_422(dtype, max_val, x_nchw, Hp, Wp, H, W, y, u, v, (hipStream_t)stream);
    const int layout = chroma == 444 ? L_444P : L_420P;
    const int64_t cs = chroma == 444 ? W : W / 2;
    const Metric m{(float)max_val};
    return dcvc::typed(dtype, [&](auto tag) {
        launch_store<decltype(tag)>(layout, m, x_nchw, Hp, Wp, H, W, y, u, v, W, cs, (hipStream_t)stream);
    });
}

// ------------------------------------------------------------------ tight planar 8-bit 4:2:0 and RGB
int dcvc_yuv420_to_frame(int dtype, const uint8_t* y, const uint8_t* u, const uint8_t* v, int H, int W, int pad_b,
                         int pad_r, void* out_nchw, void* stream)
{
    DCVC_REQUIRE(y && u && v && out_nchw && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && pad_b >= 0 && pad_r >= 0,
                 "dcvc_yuv420_to_frame: bad arguments (%dx%d)", H, W);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        yuv420_to_frame_kernel<T><<<blocks_for((int64_t)3 * (H + pad_b) * (W + pad_r)), PB, 0, (hipStream_t)stream>>>(
            y, u, v, H, W, H + pad_b, W + pad_r, (T*)out_nchw);
    });
}

int dcvc_frame_to_yuv420(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, int round_uv, uint8_t* y,
                         uint8_t* u, uint8_t* v, void* stream)
{
    const char* who = "dcvc_frame_to_yuv420";
    if (int rc = dcvc::check_frame(who, "the frame", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(y && u && v && H % 2 == 0 && W % 2 == 0, "%s: a null plane or an odd size (%d x %d)", who, H, W);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        frame_to_yuv420_kernel<T><<<blocks_for((int64_t)H * W * 3 / 2), PB, 0, (hipStream_t)stream>>>(
            (const T*)x_nchw, Hp, Wp, H, W, round_uv, y, u, v);
    });
}

int dcvc_rgb_to_frame(int dtype, const uint8_t* rgb, int H, int W, int pad_b, int pad_r, void* out_nchw, void* stream)
{
    DCVC_REQUIRE(rgb && out_nchw && H > 0 && W > 0 && pad_b >= 0 && pad_r >= 0, "dcvc_rgb_to_frame: bad arguments (%dx%d)", H, W);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        rgb_to_frame_kernel<T><<<blocks_for((int64_t)(H + pad_b) * (W + pad_r)), PB, 0, (hipStream_t)stream>>>(
            rgb, H, W, H + pad_b, W + pad_r, (T*)out_nchw);
    });
}

int dcvc_frame_to_rgb(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* out_chw, void* stream)
{
    const char* who = "dcvc_frame_to_rgb";
    if (int rc = dcvc::check_frame(who, "the frame", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(out_chw && (uintptr_t)out_chw % dcvc::elem_size(dtype) == 0, "%s: out is null or not aligned to its element size", who);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        frame_to_rgb_kernel<T><<<blocks_for((int64_t)H * W), PB, 0, (hipStream_t)stream>>>((const T*)x_nchw, Hp, Wp, H, W, (T*)out_chw);
    });
}

}  // extern "C"
