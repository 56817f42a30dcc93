// dcvc_bars.hip - active-area coding on model frames [3][Hp][Wp] (docs/active_area.md): the letterbox / pillarbox bars of a
// sequence are found on the device, the encoder codes the window between them, the decode side pastes the window back.
//   dcvc_bars_reset / dcvc_bars_scan   the envelope of any number of frames: per plane, per row and per column the smallest
//                                      and the largest sample, as ORDERED KEYS (below) in device memory, no read-back
//   dcvc_bars_extent                   the normative rule on the envelope: one workgroup, 8 words into pinned host memory
//   dcvc_frame_window                  out = x[top : top + HO, left : left + WO] with its replicate pad
//   dcvc_frame_paste                   out = the bar colour with x at (top, left), with its replicate pad
// Ordered key of a sample: u = the bits of (float)x; key = u ^ 0x80000000 if the sign bit is clear, else ~u.  The key is
// monotonic over all non-NaN floats (-0 below +0), a positive NaN lies above +inf and a negative one below -inf, so a NaN
// in a line is that line's max or min and fails every fp32 comparison of the rule.  Integer min / max is order independent:
// the envelope is exact whatever the order of the tiles and of the atomics.
// Scan: a workgroup per STW x STH tile of one plane.  A thread carries 8 columns (one 16-byte access in fp16, two in fp32;
// element by element where the tensor's address or row length, or the picture's right edge, do not allow it) through the
// tile's STH / 32 row passes: its columns' min / max stay in registers, a row's are reduced over the 8 threads of the row by
// shuffles.  At the end the columns are reduced over the rows of a wave by shuffles and over the 4 waves through LDS, and
// the tile issues one atomicMin and one atomicMax per row and per column, consecutive threads to consecutive words.  STH =
// 128: a tile then issues 2 * 64 column atomics against 2 * 128 row atomics for 8192 samples, and the column words of a
// 1080-row plane are hit by 9 tiles each.  Nothing outside H x W is read.
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>

namespace {

constexpr int SB = 256;              // threads per workgroup, every kernel here
constexpr int STW = 64;              // columns of a scan tile: 8 threads of 8 columns
constexpr int STH = 128;             // rows of a scan tile
constexpr int SRP = SB / (STW / 8);  // rows of one pass over the tile
constexpr int CTW = 256;             // columns of a window / paste tile: 32 threads of 8 columns
constexpr int CTH = SB / (CTW / 8);  // its rows
constexpr int MAX_DIM = 1 << 20;     // rows / columns of an envelope

__device__ __forceinline__ uint32_t key_of(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// the envelope in the workspace: mins then maxes (a reset is two byte fills), each rows[3][H] then columns[3][W]
struct Envelope {
    uint32_t *rowmin, *colmin, *rowmax, *colmax;
};
__host__ __device__ __forceinline__ Envelope envelope(uint32_t* ws, int H, int W)
{
    return {ws, ws + 3 * (int64_t)H, ws + 3 * ((int64_t)H + W), ws + 3 * ((int64_t)H + W) + 3 * (int64_t)H};
}

// VEC: the tensor is 16-byte aligned and its row length a multiple of 16 bytes
template <typename T, bool VEC>
__global__ __launch_bounds__(SB) void bars_scan_kernel(const T* __restrict__ x, int Hp, int Wp, int H, int W, uint32_t* ws)
{
    __shared__ uint32_t s_row[2][STH];
    __shared__ uint32_t s_col[2][SB / 64][STW];
    const int tid = threadIdx.x, cx = tid & 7, ry = tid >> 3, p = blockIdx.z;
    const int x0 = blockIdx.x * STW + cx * 8, y0 = blockIdx.y * STH;
    const T* xp = x + (int64_t)p * Hp * Wp;

    uint32_t cmin[8], cmax[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        cmin[j] = 0xFFFFFFFFu;
        cmax[j] = 0u;
    }
#pragma unroll
    for (int i = 0; i < STH / SRP; ++i) {
        const int r = ry + i * SRP, y = y0 + r;
        uint32_t rmin = 0xFFFFFFFFu, rmax = 0u;
        if (y < H && x0 < W) {
            const T* row = xp + (int64_t)y * Wp + x0;
            if (VEC && x0 + 8 <= W) {
                const Pix8<T> v = *reinterpret_cast<const Pix8<T>*>(row);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t k = key_of((float)v.v[j]);
                    cmin[j] = min(cmin[j], k);
                    cmax[j] = max(cmax[j], k);
                    rmin = min(rmin, k);
                    rmax = max(rmax, k);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (x0 + j < W) {
                        const uint32_t k = key_of((float)row[j]);
                        cmin[j] = min(cmin[j], k);
                        cmax[j] = max(cmax[j], k);
                        rmin = min(rmin, k);
                        rmax = max(rmax, k);
                    }
            }
        }
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) {              // over the 8 threads of the row
            rmin = min(rmin, (uint32_t)__shfl_xor((int)rmin, m, 64));
            rmax = max(rmax, (uint32_t)__shfl_xor((int)rmax, m, 64));
        }
        if (cx == 0) {
            s_row[0][r] = rmin;
            s_row[1][r] = rmax;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int m = 8; m < 64; m <<= 1) {             // over the 8 rows of the wave
            cmin[j] = min(cmin[j], (uint32_t)__shfl_xor((int)cmin[j], m, 64));
            cmax[j] = max(cmax[j], (uint32_t)__shfl_xor((int)cmax[j], m, 64));
        }
    }
    if ((tid & 63) < 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s_col[0][tid >> 6][cx * 8 + j] = cmin[j];
            s_col[1][tid >> 6][cx * 8 + j] = cmax[j];
        }
    }
    __syncthreads();

    const Envelope e = envelope(ws, H, W);
    if (tid < STH) {                                   // waves 0, 1: the tile's rows
        const int y = y0 + tid;
        if (y < H) {
            atomicMin(e.rowmin + (int64_t)p * H + y, s_row[0][tid]);
            atomicMax(e.rowmax + (int64_t)p * H + y, s_row[1][tid]);
        }
    } else if (tid < STH + STW) {                      // wave 2: its columns
        const int c = tid - STH, xc = blockIdx.x * STW + c;
        if (xc < W) {
            uint32_t lo = s_col[0][0][c], hi = s_col[1][0][c];
#pragma unroll
            for (int w = 1; w < SB / 64; ++w) {
                lo = min(lo, s_col[0][w][c]);
                hi = max(hi, s_col[1][w][c]);
            }
            atomicMin(e.colmin + (int64_t)p * W + xc, lo);
            atomicMax(e.colmax + (int64_t)p * W + xc, hi);
        }
    }
}

// max - min <= tol on every plane of line i (n lines per plane)
__device__ __forceinline__ bool line_flat(const uint32_t* lo, const uint32_t* hi, int n, int i, float tol, float* c)
{
    bool flat = true;
    for (int p = 0; p < 3; ++p) {
        const float mn = key_value(lo[(int64_t)p * n + i]), mx = key_value(hi[(int64_t)p * n + i]);
        c[p] = mn;
        if (!(mx - mn <= tol)) flat = false;
    }
    return flat;
}
// max <= c + tol and min >= c - tol on every plane of line i
__device__ __forceinline__ bool line_bar(const uint32_t* lo, const uint32_t* hi, int n, int i, float tol, const float* c)
{
    bool bar = true;
    for (int p = 0; p < 3; ++p) {
        const float mn = key_value(lo[(int64_t)p * n + i]), mx = key_value(hi[(int64_t)p * n + i]);
        if (!(mx <= c[p] + tol && mn >= c[p] - tol)) bar = false;
    }
    return bar;
}

__global__ __launch_bounds__(SB) void bars_extent_kernel(uint32_t* ws, int H, int W, float tol, int32_t* out)
{
    __shared__ int s_found;
    __shared__ float s_c[3];
    __shared__ int s_e[4];           // first and last row that is no bar, first and last such column
    const Envelope e = envelope(ws, H, W);
    const int tid = threadIdx.x;
    if (tid == 0) {
        float c[3];
        bool found = line_flat(e.rowmin, e.rowmax, H, 0, tol, c);
        if (!found) found = line_flat(e.rowmin, e.rowmax, H, H - 1, tol, c);
        if (!found) found = line_flat(e.colmin, e.colmax, W, 0, tol, c);
        if (!found) found = line_flat(e.colmin, e.colmax, W, W - 1, tol, c);
        s_found = found;
        for (int p = 0; p < 3; ++p) s_c[p] = c[p];
        s_e[0] = H;
        s_e[1] = -1;
        s_e[2] = W;
        s_e[3] = -1;
    }
    __syncthreads();
    if (!s_found) {
        if (tid < 8) out[tid] = 0;
        return;
    }
    const float c[3] = {s_c[0], s_c[1], s_c[2]};
    int first_row = H, last_row = -1, first_col = W, last_col = -1;      // the thread's own lines that are no bars
    for (int y = tid; y < H; y += SB)
        if (!line_bar(e.rowmin, e.rowmax, H, y, tol, c)) {
            first_row = min(first_row, y);
            last_row = y;
        }
    for (int xc = tid; xc < W; xc += SB)
        if (!line_bar(e.colmin, e.colmax, W, xc, tol, c)) {
            first_col = min(first_col, xc);
            last_col = xc;
        }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {                 // over the wave, then one LDS atomic per wave and word
        first_row = min(first_row, __shfl_xor(first_row, m, 64));
        last_row = max(last_row, __shfl_xor(last_row, m, 64));
        first_col = min(first_col, __shfl_xor(first_col, m, 64));
        last_col = max(last_col, __shfl_xor(last_col, m, 64));
    }
    if ((tid & 63) == 0) {
        atomicMin(&s_e[0], first_row);
        atomicMax(&s_e[1], last_row);
        atomicMin(&s_e[2], first_col);
        atomicMax(&s_e[3], last_col);
    }
    __syncthreads();
    if (tid == 0) {
        out[0] = 1;
        out[1] = s_e[0];
        out[2] = H - 1 - s_e[1];
        out[3] = s_e[2];
        out[4] = W - 1 - s_e[3];
        for (int p = 0; p < 3; ++p) out[5 + p] = (int32_t)__float_as_uint(c[p]);
    }
}

template <typename T, int A>
struct alignas(A) Piece {            // A bytes of a row
    T v[A / (int)sizeof(T)];
};

// 8 consecutive elements from `from`, which is aligned to A bytes, in accesses of A bytes
template <typename T, int A>
__device__ __forceinline__ Pix8<T> load8(const T* from)
{
    constexpr int N = A / (int)sizeof(T);
    Pix8<T> o;
#pragma unroll
    for (int g = 0; g < 8 / N; ++g) {
        const Piece<T, A> pc = *reinterpret_cast<const Piece<T, A>*>(from + g * N);
#pragma unroll
        for (int i = 0; i < N; ++i) o.v[g * N + i] = pc.v[i];
    }
    return o;
}

// A: the source tensor, its row length and `left` elements are all multiples of A bytes
template <typename T, int A>
__global__ __launch_bounds__(SB) void frame_window_kernel(const T* __restrict__ x, int Hp, int Wp, int top, int left,
                                                          T* __restrict__ out, int HOp, int WOp, int HO, int WO)
{
    const int ox = blockIdx.x * CTW + (threadIdx.x & (CTW / 8 - 1)) * 8, oy = blockIdx.y * CTH + threadIdx.x / (CTW / 8);
    if (ox >= WOp || oy >= HOp) return;              // (WOp is a multiple of 8: the 8 columns are inside or outside)
    const T* row = x + ((int64_t)blockIdx.z * Hp + top + min(oy, HO - 1)) * Wp + left;
    Pix8<T> o;
    if (ox + 8 <= WO) {
        o = load8<T, A>(row + ox);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = row[min(ox + i, WO - 1)];
    }
    *reinterpret_cast<Pix8<T>*>(out + ((int64_t)blockIdx.z * HOp + oy) * WOp + ox) = o;
}

struct Colour {
    float c[3];
};

// A as above; x: the H x W window that belongs at (top, left) of the HO x WO picture
template <typename T, int A>
__global__ __launch_bounds__(SB) void frame_paste_kernel(const T* __restrict__ x, int Hp, int Wp, int H, int W,
                                                         T* __restrict__ out, int HOp, int WOp, int HO, int WO, int top,
                                                         int left, Colour colour)
{
    const int ox = blockIdx.x * CTW + (threadIdx.x & (CTW / 8 - 1)) * 8, oy = blockIdx.y * CTH + threadIdx.x / (CTW / 8);
    if (ox >= WOp || oy >= HOp) return;
    const int p = blockIdx.z, sy = min(oy, HO - 1) - top;                 // the window's row
    const T bar = to_t<T>(colour.c[p]);
    const int lo = min(ox, WO - 1) - left, hi = min(ox + 7, WO - 1) - left;   // the window's columns of the first and last pixel
    Pix8<T> o;
    if (sy < 0 || sy >= H || hi < 0 || lo >= W) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = bar;
    } else {
        const T* row = x + ((int64_t)p * Hp + sy) * Wp;
        if (ox + 8 <= WO && lo >= 0 && hi < W) {
            o = load8<T, A>(row + lo);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int sx = min(ox + i, WO - 1) - left;
                o.v[i] = (sx >= 0 && sx < W) ? row[sx] : bar;
            }
        }
    }
    *reinterpret_cast<Pix8<T>*>(out + ((int64_t)p * HOp + oy) * WOp + ox) = o;
}

// the widest access, 16 bytes at most and one element at least, that the source tensor and `left` allow for every row
int load_bytes(size_t es, const void* x, int Wp, int left)
{
    int a = 16;
    while (a > (int)es && !(dcvc::vec_ok(a / (int)es, es, Wp, x) && (left * (int64_t)es) % a == 0)) a >>= 1;
    return a;
}

// f(IC<A>) for the A of load_bytes
template <typename T, typename F>
void with_load_bytes(int a, F&& f)
{
    if (a == 16)
        f(dcvc::IC<16>{});
    else if (a == 8)
        f(dcvc::IC<8>{});
    else if (a == 4)
        f(dcvc::IC<4>{});
    else
        f(dcvc::IC<(int)sizeof(T)>{});
}

int check_envelope(const char* who, const void* ws, int H, int W)
{
    DCVC_REQUIRE(H > 0 && W > 0 && H <= MAX_DIM && W <= MAX_DIM, "%s: bad picture size %d x %d", who, H, W);
    DCVC_REQUIRE(ws, "%s: the workspace is a null pointer", who);
    DCVC_REQUIRE(((uintptr_t)ws & 3) == 0, "%s: the workspace is not 4-byte aligned", who);
    return 0;
}

// the output tensor of window / paste: stored 16 bytes per access
int check_out(const char* who, int dtype, const void* out, int HOp, int WOp, int HO, int WO)
{
    if (int rc = dcvc::check_frame(who, "the output", dtype, out, HOp, WOp, HO, WO)) return rc;
    DCVC_REQUIRE(((uintptr_t)out & 15) == 0 && WOp % 8 == 0,
                 "%s: the output tensor (%d x %d) must be 16-byte aligned and its width a multiple of 8", who, HOp, WOp);
    return 0;
}

}  // namespace

extern "C" {

int64_t dcvc_bars_ws_bytes(int H, int W)
{
    if (H <= 0 || W <= 0 || H > MAX_DIM || W > MAX_DIM) {
        dcvc::set_error("dcvc_bars_ws_bytes: bad picture size %d x %d", H, W);
        return dcvc::E_ARG;
    }
    return (int64_t)4 * 2 * 3 * ((int64_t)H + W);
}

int dcvc_bars_reset(void* ws, int H, int W, void* stream)
{
    if (int rc = check_envelope("dcvc_bars_reset", ws, H, W)) return rc;
    const size_t half = (size_t)4 * 3 * ((size_t)H + W);
    DCVC_HIP(hipMemsetAsync(ws, 0xFF, half, (hipStream_t)stream));
    DCVC_HIP(hipMemsetAsync((char*)ws + half, 0x00, half, (hipStream_t)stream));
    return 0;
}

int dcvc_bars_scan(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* ws, void* stream)
{
    const char* who = "dcvc_bars_scan";
    if (int rc = dcvc::check_frame(who, "the source", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = check_envelope(who, ws, H, W)) return rc;
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, W, H, STW, STH, grid)) return rc;
    const size_t es = dcvc::elem_size(dtype);
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, x_nchw);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            bars_scan_kernel<T, decltype(v)::value><<<grid, SB, 0, (hipStream_t)stream>>>((const T*)x_nchw, Hp, Wp, H, W,
                                                                                         (uint32_t*)ws);
        });
    });
}

int dcvc_bars_extent(const void* ws, int H, int W, float tol, int32_t* out8, void* stream)
{
    const char* who = "dcvc_bars_extent";
    if (int rc = check_envelope(who, ws, H, W)) return rc;
    DCVC_REQUIRE(tol >= 0.0f, "%s: tol %g is not a tolerance (>= 0)", who, (double)tol);
    DCVC_REQUIRE(out8 && ((uintptr_t)out8 & 3) == 0, "%s: the result buffer is null or not 4-byte aligned", who);
    int32_t* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, out8, 0));
    bars_extent_kernel<<<1, SB, 0, (hipStream_t)stream>>>((uint32_t*)ws, H, W, tol, out_dev);
    DCVC_LAUNCH_CHECK();
    return 0;
}

int dcvc_frame_window(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, int top, int left, void* out_nchw, int HOp,
                      int WOp, int HO, int WO, void* stream)
{
    const char* who = "dcvc_frame_window";
    if (int rc = dcvc::check_frame(who, "the source", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = check_out(who, dtype, out_nchw, HOp, WOp, HO, WO)) return rc;
    DCVC_REQUIRE(top >= 0 && left >= 0 && (int64_t)top + HO <= H && (int64_t)left + WO <= W,
                 "%s: the window %d x %d at (%d, %d) is not inside the picture (%d x %d)", who, HO, WO, top, left, H, W);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, WOp, HOp, CTW, CTH, grid)) return rc;
    const int a = load_bytes(dcvc::elem_size(dtype), x_nchw, Wp, left);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        with_load_bytes<T>(a, [&](auto A) {
            frame_window_kernel<T, decltype(A)::value><<<grid, SB, 0, (hipStream_t)stream>>>((const T*)x_nchw, Hp, Wp, top, left,
                                                                                            (T*)out_nchw, HOp, WOp, HO, WO);
        });
    });
}

int dcvc_frame_paste(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* out_nchw, int HOp, int WOp, int HO,
                     int WO, int top, int left, const float* colour, void* stream)
{
    const char* who = "dcvc_frame_paste";
    if (int rc = dcvc::check_frame(who, "the source", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = check_out(who, dtype, out_nchw, HOp, WOp, HO, WO)) return rc;
    DCVC_REQUIRE(colour, "%s: the colour is a null pointer", who);
    DCVC_REQUIRE(top >= 0 && left >= 0 && (int64_t)top + H <= HO && (int64_t)left + W <= WO,
                 "%s: the window %d x %d at (%d, %d) is not inside the picture (%d x %d)", who, H, W, top, left, HO, WO);
    const size_t es = dcvc::elem_size(dtype);
    const uintptr_t xa = (uintptr_t)x_nchw, xb = xa + (size_t)3 * Hp * Wp * es;
    const uintptr_t oa = (uintptr_t)out_nchw, ob = oa + (size_t)3 * HOp * WOp * es;
    DCVC_REQUIRE(xb <= oa || ob <= xa, "%s: the source and the output overlap", who);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, WOp, HOp, CTW, CTH, grid)) return rc;
    const int a = load_bytes(es, x_nchw, Wp, left);
    const Colour col = {{colour[0], colour[1], colour[2]}};
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        with_load_bytes<T>(a, [&](auto A) {
            frame_paste_kernel<T, decltype(A)::value><<<grid, SB, 0, (hipStream_t)stream>>>(
                (const T*)x_nchw, Hp, Wp, H, W, (T*)out_nchw, HOp, WOp, HO, WO, top, left, col);
        });
    });
}

}  // extern "C"
