// dcvc_resize.hip - separable polyphase resampler on model frames [3][Hp][Wp] (docs/reduced_resolution.md): the scaler in
// front of the encoder and behind the decoder of a reduced-resolution run.  Table driven: per output column (row) the
// first source column (row) of its window and `taps` fp32 weights, made by the caller (opendcvc_amd/resize.py); the kernel
// knows no filter.  The arithmetic is fixed (fp32 multiply and add in tap order, no fma, ONE rounding to the storage type):
//   t[y][j]   = c_h[j][0] * x[y][i_0],  then  t = t + c_h[j][k] * x[y][i_k],   i_k = min(max(first_h[j] + k, 0), W - 1)
//   out[i][j] = c_v[i][0] * t[y_0][j],  then  o = o + c_v[i][k] * t[y_k][j],   y_k = min(max(first_v[i] + k, 0), H - 1)
// The clamps are the contract: whatever the tables hold, only the valid H x W region of the source is read.  Output rows and
// columns past HO x WO are computed from the clamped output coordinate, which is the replicate pad bit for bit.
// One launch, a workgroup per TH x TW output tile of one plane.  The intermediate t lives in LDS: the horizontal pass runs
// over the source rows the tile's windows reach (a wave per row, a lane per output column), the vertical pass reads it back
// 8 columns per thread and stores 16 bytes per access.  The LDS image holds RMAX rows; a tile whose windows span more
// (large ratios, or a table that jumps) goes through it in several groups of output rows, each group's span at most RMAX -
// a single row always fits (taps <= 64 <= RMAX).
// Where the horizontal windows of the tile span at most SC source columns and have at most CT taps (ratios up to about 3.5),
// the source goes through LDS too: strips of SR rows are loaded 16 bytes per access (element by element where the tensor's
// address or row length, or the picture's right edge, do not allow it) and the tile's weights are kept transposed, so the
// gathers of the taps and the weight reads are LDS reads.  Wider windows gather from memory.  No atomics, no workspace.
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>

namespace {

constexpr int RB = 256;          // threads per workgroup
constexpr int TW = 64;           // output columns of a tile: one wave per row in the horizontal pass
constexpr int TH = 32;           // output rows of a tile: RB / (TW / 8) threads of 8 columns in the vertical pass
constexpr int RMAX = 88;         // rows of t in LDS
constexpr int SR = 16;           // source rows of a strip in LDS: HR for each of the RB / TW waves
constexpr int SC = 256;          // source columns of a strip in LDS
constexpr int CT = 24;           // taps of the tile's horizontal weights in LDS
constexpr int TS = TW + 4;       // row stride of t in LDS (floats): rows of the vertical pass start one 16-byte slot apart
constexpr int HR = 4;            // source rows a wave carries through one sweep over the taps (one weight load serves all)
constexpr int MAX_TAPS = 64;

struct alignas(16) F4 {
    float v[4];
};

// a table's first index brought into [-MAX_TAPS, n - 1]: min(max(first + k, 0), n - 1) is the same for every k < taps, and
// first + k cannot overflow whatever the table holds
__device__ __forceinline__ int first_of(const int32_t* first, int i, int n) { return clampi(first[i], -MAX_TAPS, n - 1); }

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

// VEC: the source tensor is 16-byte aligned and its row length a multiple of 16 bytes
template <typename T, bool VEC>
__global__ __launch_bounds__(RB) void resize_kernel(const T* __restrict__ x, int Hp, int Wp, int H, int W, T* __restrict__ out,
                                                    int HOp, int WOp, int HO, int WO, const int32_t* __restrict__ first_h,
                                                    const float* __restrict__ coef_h, int taps_h,
                                                    const int32_t* __restrict__ first_v, const float* __restrict__ coef_v,
                                                    int taps_v)
{
    __shared__ __attribute__((aligned(16))) float t[RMAX * TS];
    __shared__ int s_lo[TH], s_hi[TH];                       // per output row of the tile: first and last source row, clamped
    __shared__ __attribute__((aligned(16))) T src[SR * SC];   // a strip of the source, columns from c0
    __shared__ float wh[CT * TW];                             // the tile's horizontal weights, [tap][column]
    constexpr int G = 16 / (int)sizeof(T);                    // elements of a 16-byte piece

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int th = min(TH, HOp - y0);                         // rows of the tile inside the output tensor
    const T* xp = x + (int64_t)blockIdx.z * Hp * Wp;
    T* op = out + (int64_t)blockIdx.z * HOp * WOp;

    if (tid < th) {
        const int f = first_of(first_v, min(y0 + tid, HO - 1), H);
        s_lo[tid] = clampi(f, 0, H - 1);
        s_hi[tid] = clampi(f + taps_v - 1, 0, H - 1);
    }
    // horizontal pass: lane -> output column (the clamped one past WO), wave -> source rows
    const int hx = tid & (TW - 1), hw = tid >> 6;
    const int jh = min(x0 + hx, WO - 1);
    const int fh = first_of(first_h, jh, W);
    const float* ch = coef_h + (int64_t)jh * taps_h;
    // the source columns the tile's windows reach, from the 16-byte piece the first lies in (every wave forms the same)
    const int c0 = wave_min(clampi(fh, 0, W - 1)) & ~(G - 1), c1 = wave_max(clampi(fh + taps_h - 1, 0, W - 1));
    const bool staged = taps_h <= CT && c1 - c0 < SC;
    if (staged)
        for (int k = hw; k < taps_h; k += RB / TW) wh[k * TW + hx] = ch[k];
    __syncthreads();
    // vertical pass: 8 threads per output row
    const int vr = tid >> 3, vc = (tid & 7) * 8;

    for (int r0 = 0; r0 < th;) {
        // the group of output rows [r0, r1) whose windows together span at most RMAX source rows (uniform over the block)
        int lo = s_lo[r0], hi = s_hi[r0], r1 = r0 + 1;
        for (; r1 < th; ++r1) {
            const int nlo = min(lo, s_lo[r1]), nhi = max(hi, s_hi[r1]);
            if (nhi - nlo + 1 > RMAX) break;
            lo = nlo;
            hi = nhi;
        }
        const int rows = hi - lo + 1;                         // 1 .. RMAX, and lo + rows - 1 <= H - 1

        if (staged) {
            const int pieces = (c1 - c0) / G + 1;             // 16-byte pieces of a strip's row, at most SC / G
            for (int s0 = 0; s0 < rows; s0 += SR) {
                const int srows = min(SR, rows - s0);
                for (int g = tid; g < srows * pieces; g += RB) {
                    const int r = g / pieces, c = (g - r * pieces) * G;
                    const T* from = xp + (int64_t)(lo + s0 + r) * Wp + c0 + c;
                    T* to = src + r * SC + c;
                    if (VEC && c0 + c + G <= W) {
                        *reinterpret_cast<F4*>(to) = *reinterpret_cast<const F4*>(from);
                    } else {
#pragma unroll
                        for (int i = 0; i < G; ++i)
                            if (c0 + c + i < W) to[i] = from[i];
                    }
                }
                __syncthreads();
                const int rb = hw * HR;                       // the wave's rows of the strip
                if (rb < srows) {
                    const T* row[HR];
#pragma unroll
                    for (int i = 0; i < HR; ++i) row[i] = src + min(rb + i, srows - 1) * SC;
                    float acc[HR];
                    {
                        const float c = wh[hx];
                        const int ix = clampi(fh, 0, W - 1) - c0;
#pragma unroll
                        for (int i = 0; i < HR; ++i) acc[i] = c * (float)row[i][ix];
                    }
                    for (int k = 1; k < taps_h; ++k) {
                        const float c = wh[k * TW + hx];
                        const int ix = clampi(fh + k, 0, W - 1) - c0;
#pragma unroll
                        for (int i = 0; i < HR; ++i) acc[i] = acc[i] + c * (float)row[i][ix];
                    }
#pragma unroll
                    for (int i = 0; i < HR; ++i)
                        if (rb + i < srows) t[(s0 + rb + i) * TS + hx] = acc[i];
                }
                __syncthreads();
            }
        } else {
            for (int rb = hw * HR; rb < rows; rb += (RB / TW) * HR) {
                const T* row[HR];
#pragma unroll
                for (int i = 0; i < HR; ++i) row[i] = xp + (int64_t)(lo + min(rb + i, rows - 1)) * Wp;
                float acc[HR];
                {
                    const float c = ch[0];
                    const int ix = clampi(fh, 0, W - 1);
#pragma unroll
                    for (int i = 0; i < HR; ++i) acc[i] = c * (float)row[i][ix];
                }
                for (int k = 1; k < taps_h; ++k) {
                    const float c = ch[k];
                    const int ix = clampi(fh + k, 0, W - 1);
#pragma unroll
                    for (int i = 0; i < HR; ++i) acc[i] = acc[i] + c * (float)row[i][ix];
                }
#pragma unroll
                for (int i = 0; i < HR; ++i)
                    if (rb + i < rows) t[(rb + i) * TS + hx] = acc[i];
            }
            __syncthreads();
        }

        const int e = r0 + vr;
        if (e < r1 && x0 + vc < WOp) {                        // (WOp is a multiple of 8: the 8 columns are inside or outside)
            const int oy = min(y0 + e, HO - 1);
            const int fv = first_of(first_v, oy, H);
            const float* cv = coef_v + (int64_t)oy * taps_v;
            float acc[8];
            {
                const float c = cv[0];
                const float* tp = t + (clampi(fv, 0, H - 1) - lo) * TS + vc;
                const F4 a = *reinterpret_cast<const F4*>(tp), b = *reinterpret_cast<const F4*>(tp + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i] = c * a.v[i];
                    acc[4 + i] = c * b.v[i];
                }
            }
            for (int k = 1; k < taps_v; ++k) {
                const float c = cv[k];
                const float* tp = t + (clampi(fv + k, 0, H - 1) - lo) * TS + vc;
                const F4 a = *reinterpret_cast<const F4*>(tp), b = *reinterpret_cast<const F4*>(tp + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i] = acc[i] + c * a.v[i];
                    acc[4 + i] = acc[4 + i] + c * b.v[i];
                }
            }
            Pix8<T> o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o.v[i] = to_t<T>(acc[i]);
            *reinterpret_cast<Pix8<T>*>(op + (int64_t)(y0 + e) * WOp + x0 + vc) = o;
        }
        __syncthreads();
        r0 = r1;
    }
}

}  // namespace

extern "C" {

int dcvc_resize_frame(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* out_nchw, int HOp, int WOp, int HO,
                      int WO, const int32_t* first_h, const float* coef_h, int taps_h, const int32_t* first_v,
                      const float* coef_v, int taps_v, void* stream)
{
    const char* who = "dcvc_resize_frame";
    if (int rc = dcvc::check_frame(who, "the source", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(HO > 0 && WO > 0, "%s: bad output size %d x %d", who, HO, WO);
    DCVC_REQUIRE(HOp >= HO && WOp >= WO, "%s: the output tensor (%d x %d) does not hold its valid region (%d x %d)", who, HOp,
                 WOp, HO, WO);
    DCVC_REQUIRE(taps_h >= 1 && taps_h <= MAX_TAPS && taps_v >= 1 && taps_v <= MAX_TAPS, "%s: taps %d / %d outside 1 .. %d", who,
                 taps_h, taps_v, MAX_TAPS);
    DCVC_REQUIRE(out_nchw && first_h && coef_h && first_v && coef_v, "%s: null pointer", who);
    DCVC_REQUIRE(((uintptr_t)out_nchw & 15) == 0 && WOp % 8 == 0,
                 "%s: the output tensor (%d x %d) must be 16-byte aligned and its width a multiple of 8", who, HOp, WOp);
    DCVC_REQUIRE((((uintptr_t)first_h | (uintptr_t)coef_h | (uintptr_t)first_v | (uintptr_t)coef_v) & 3) == 0,
                 "%s: a table is not 4-byte aligned", who);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, WOp, HOp, TW, TH, grid)) return rc;
    const size_t es = dcvc::elem_size(dtype);
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, x_nchw);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            resize_kernel<T, decltype(v)::value><<<grid, RB, 0, (hipStream_t)stream>>>(
                (const T*)x_nchw, Hp, Wp, H, W, (T*)out_nchw, HOp, WOp, HO, WO, first_h, coef_h, taps_h, first_v, coef_v, taps_v);
        });
    });
}

}  // extern "C"
