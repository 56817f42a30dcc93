// dcvc_repeat.hip - repeated-frame coding on model frames [3][Hp][Wp] (docs/frame_repeat.md): is this frame the picture of
// the frame coded last?  A hash would find bit-identical frames only and could drop a frame on a collision; the answer here
// is an exact number, the largest sample difference per plane, which the host holds against a tolerance.
//   dcvc_frame_maxdiff   out4[p] = max over the H x W picture of plane p of the KEY of |a - b|, out4[3] = 0
// Key of a sample pair: d = fabsf((float)a - (float)b), one fp32 subtraction (the build contracts nothing into an FMA), key =
// the bits of d.  d has no sign bit, so the keys of the finite differences order as the differences do and an integer max is
// the float max, whatever the order of the tiles and of the atomics: the result is exact.  +0 against -0 is key 0.  A NaN on
// either side, or inf - inf, is a NaN: a key above 0x7f800000, above every finite tolerance and +inf itself.
// A workgroup carries TW x TH tiles of one plane, every gridDim.x-th one.  A thread reads 8 columns of both frames per row
// pass (one 16-byte access each in fp16, two in fp32; element by element where an address or the row length, or the
// picture's right edge, do not allow it; a tile that has all its rows issues the loads of its four passes together) and
// keeps the running max in a register; at the end the max goes over the wave by shuffles, over the 4 waves through LDS and
// into the plane's word of the workspace with ONE atomicMax per workgroup.  Nothing outside H x W is read.
// Atomics of many workgroups on ONE word run one after the other - the first form, a workgroup per tile and one count for
// all of them, spent 26 of its 33 us at 1080p there (profiles/r21_frame_repeat.txt) - so a plane has at most MAX_GROUPS
// workgroups and a count of its own.  The workspace is six words: the three maxima, then per plane the count of the
// workgroups that have added theirs.  The workgroup that counts last in its plane takes the plane's maximum out with an
// atomic exchange against 0, writes it to out4 (and the 0 of out4[3]) and puts the count back to 0: the workspace - zero
// before its first use - is zero again when the kernel ends, no memset between two compares.  Every access to the six words
// is a device-scope atomic (they are never read through a CU's L1), the fence between a workgroup's atomicMax and its count
// orders the two.  One compare at a time per workspace.
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>

namespace {

constexpr int RB = 256;              // threads per workgroup
constexpr int TW = 256;              // columns of a tile: 32 threads of 8 columns
constexpr int RP = RB / (TW / 8);    // rows of one pass over the tile
constexpr int TH = 4 * RP;           // rows of a tile
constexpr int MAX_GROUPS = 96;       // workgroups of a plane
constexpr int WS_WORDS = 8;          // 3 maxima, 3 counts, 2 unused

__device__ __forceinline__ uint32_t diff_key(float a, float b) { return __float_as_uint(fabsf(a - b)); }

// VEC: both tensors are 16-byte aligned and their row length a multiple of 16 bytes; the plane is tiles_x x tiles_y tiles
template <typename T, bool VEC>
__global__ __launch_bounds__(RB) void frame_maxdiff_kernel(const T* __restrict__ a, const T* __restrict__ b, int Hp, int Wp, int H,
                                                           int W, int tiles_x, int tiles_y, uint32_t* ws, uint32_t* out)
{
    __shared__ uint32_t s_max[RB / 64];
    const int tid = threadIdx.x, p = blockIdx.y;
    const int64_t plane = (int64_t)p * Hp * Wp;

    uint32_t m = 0u;
    for (int t = blockIdx.x; t < tiles_x * tiles_y; t += gridDim.x) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x0 = tx * TW + (tid & (TW / 8 - 1)) * 8, y0 = ty * TH + tid / (TW / 8);
        if (VEC && x0 + 8 <= W && ty * TH + TH <= H) {   // a tile with all its rows: every load is issued before the first use
            Pix8<T> va[TH / RP], vb[TH / RP];
#pragma unroll
            for (int i = 0; i < TH / RP; ++i) {
                const int64_t at = plane + (int64_t)(y0 + i * RP) * Wp + x0;
                va[i] = *reinterpret_cast<const Pix8<T>*>(a + at);
                vb[i] = *reinterpret_cast<const Pix8<T>*>(b + at);
            }
#pragma unroll
            for (int i = 0; i < TH / RP; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) m = max(m, diff_key((float)va[i].v[j], (float)vb[i].v[j]));
        } else if (x0 < W) {
#pragma unroll
            for (int i = 0; i < TH / RP; ++i) {
                const int y = y0 + i * RP;
                if (y >= H) break;
                const int64_t at = plane + (int64_t)y * Wp + x0;
                if (VEC && x0 + 8 <= W) {
                    const Pix8<T> va = *reinterpret_cast<const Pix8<T>*>(a + at), vb = *reinterpret_cast<const Pix8<T>*>(b + at);
#pragma unroll
                    for (int j = 0; j < 8; ++j) m = max(m, diff_key((float)va.v[j], (float)vb.v[j]));
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (x0 + j < W) m = max(m, diff_key((float)a[at + j], (float)b[at + j]));
                }
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = m;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < RB / 64; ++w) m = max(m, s_max[w]);
    atomicMax(ws + p, m);
    __threadfence();                                   // the max is in memory before the count says so
    if (atomicAdd(ws + 3 + p, 1u) != gridDim.x - 1) return;
    __threadfence();
    out[p] = atomicExch(ws + p, 0u);                   // the plane's last workgroup: the result out, the workspace ready again
    out[3] = 0u;
    atomicExch(ws + 3 + p, 0u);
}

}  // namespace

extern "C" {

int64_t dcvc_frame_maxdiff_ws_bytes(void) { return (int64_t)4 * WS_WORDS; }

int dcvc_frame_maxdiff(int dtype, const void* a_nchw, const void* b_nchw, int Hp, int Wp, int H, int W, void* workspace,
                       uint32_t* out4, void* stream)
{
    const char* who = "dcvc_frame_maxdiff";
    if (int rc = dcvc::check_frame(who, "the first frame", dtype, a_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = dcvc::check_frame(who, "the second frame", dtype, b_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0, "%s: the workspace is null or not 4-byte aligned", who);
    DCVC_REQUIRE(out4 && ((uintptr_t)out4 & 3) == 0, "%s: the result buffer is null or not 4-byte aligned", who);
    dim3 tiles;
    if (int rc = dcvc::tile_grid(who, W, H, TW, TH, tiles)) return rc;
    // as many workgroups per plane as give each the same number of tiles (but for the last), MAX_GROUPS at most
    const int64_t n = (int64_t)tiles.x * tiles.y, each = (n + MAX_GROUPS - 1) / MAX_GROUPS;
    const dim3 grid((unsigned)((n + each - 1) / each), 3);
    const size_t es = dcvc::elem_size(dtype);
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, a_nchw, b_nchw);
    uint32_t* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, out4, 0));
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            frame_maxdiff_kernel<T, decltype(v)::value><<<grid, RB, 0, (hipStream_t)stream>>>(
                (const T*)a_nchw, (const T*)b_nchw, Hp, Wp, H, W, (int)tiles.x, (int)tiles.y, (uint32_t*)workspace, out_dev);
        });
    });
}

}  // extern "C"
