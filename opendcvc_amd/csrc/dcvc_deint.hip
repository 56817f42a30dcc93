// dcvc_deint.hip - motion-adaptive, edge-directed deinterlacing of model frames [3][Hp][Wp] in front of the encoder
// (docs/deinterlace.md is the normative text, tests/deint_ref.py its numpy restatement; both are followed here operation for
// operation: fp32 on widened samples, every multiply, add and compare its own - the build contracts nothing - and ONE rounding
// to the storage type).
//   dcvc_deinterlace    the rows of the kept field are the bits of `cur`; every sample of a missing row is an edge-directed
//                       mean of the lines above and below it (five directions, the straight one preferred by 1 / 255), held
//                       by the previous frame - where there is one - to within what the temporal neighbourhood allows.
//                       Rows are counted per plane in units of L rows: 1 for luma, chroma_lines for the two chroma planes.
//                       Output samples past H x W are computed at the clamped coordinate: the replicate pad of the result.
//                       With a decision word that reads 0 the launch writes cur's picture and its replicate pad instead.
//   dcvc_comb_detect    is the luma picture interlaced?  Three integer sums over 10-bit samples of the kept rows, the
//                       rule, the decision word and two running counters, in one launch.
// dcvc_deinterlace: ONE launch, a workgroup per TW x TH tile of one plane's Hp x Wp.  It stages, in the storage type and in
// LDS, the rows of `cur` its output rows reach (2 L above to 2 L below, HALO columns either side, 16 bytes per access where the
// addresses allow and the piece lies inside the picture, element by element with clamped columns otherwise) and the same rows
// of `prev` without the halo.  A staged sample sits at the LDS place of its UNCLAMPED coordinate and holds the sample at the
// clamped one, so the arithmetic indexes LDS by the unclamped coordinate and never leaves H x W in memory.  A thread then
// makes 8 columns of TWO rows, a kept one and a missing one of the same pair of lines, one after the other - so the lanes of a
// wave copy together and compute together (with a row per thread half of every wave sat idle through the arithmetic) - and
// stores each with one 16-byte access in fp16 (two in fp32).  The kernel itself is deint_shared.hpp's deinterlace_kernel, which
// dcvc_deint_field.hip (the second picture of field-rate output) launches as well, with FIELD set.  The decision word is the
// kernel's FIRST parameter and this file is built with the first two dwords of the kernel arguments preloaded (csrc/Makefile),
// as dcvc_tf.hip is for tf_blend_kernel's level: the word's load does not wait for the argument fetch.  The host never reads it.
// dcvc_comb_detect: at most MAX_GROUPS workgroups, each striding over 256-column x 8-kept-row tiles; per-thread integer sums
// go wave (shuffles) -> LDS -> ONE 64-bit atomicAdd per sum per workgroup.  Workspace, eight 64-bit words, zero before the
// first call: [0] dc, [1] dp (with a previous frame) or ds (without), [2] workgroups done, [3] frames judged, [4] frames
// found interlaced.  The workgroup that counts last takes the sums out with atomic exchanges against 0, applies the rule,
// writes the decision word, adds to [3] and [4] and zeroes [2]: words [0 .. 2] are zero again when the kernel ends
// (dcvc_frame_maxdiff's way).  Integer atomics only: the result is exact whatever the order.  One call at a time per workspace.
#include "common.hpp"
#include "deint_shared.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>

namespace {

constexpr int CTW = 256;             // comb: columns of a tile (32 threads of 8 columns)
constexpr int CTH = DB / (CTW / 8);  // comb: kept rows of a tile
constexpr int MAX_GROUPS = 128;      // comb: workgroups
constexpr int WS_WORDS = 8;          // comb: 64-bit words of the workspace

__device__ __forceinline__ int quant10(float v)
{
    // (fmaxf returns the other operand for a NaN: a NaN sample counts as 0) - the temporal filter's quantiser
    return (int)fminf(fmaxf(rintf(v * 1023.0f), 0.0f), 1023.0f);
}

// 8 quantised luma samples of row y from column x0 (a multiple of 8, x0 < W); samples past W are 0 and not counted
template <typename T, bool VEC>
__device__ __forceinline__ void qrow8(const T* __restrict__ luma, int Wp, int W, int y, int x0, int* q)
{
    const T* row = luma + (int64_t)y * Wp;
    if (VEC && x0 + 8 <= W) {
        const Pix8<T> p = *reinterpret_cast<const Pix8<T>*>(row + x0);
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = quant10((float)p.v[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = x0 + i < W ? quant10((float)row[x0 + i]) : 0;
    }
}

// VEC: both frames are 16-byte aligned and so is every row; PREV: there is a previous frame.  tiles_x x tiles_y tiles of
// CTW columns x CTH kept rows; kept row k of the picture is row 2 k + parity
template <typename T, bool VEC, bool PREV>
__global__ __launch_bounds__(DB) void comb_detect_kernel(const T* __restrict__ cur, const T* __restrict__ prev, int Wp, int H, int W,
                                                         int parity, int tiles_x, int tiles_y, unsigned long long* ws,
                                                         uint32_t* decision)
{
    __shared__ unsigned long long s_part[2][DB / 64];
    const int tid = threadIdx.x;
    unsigned long long sum_c = 0, sum_o = 0;
    for (int t = blockIdx.x; t < tiles_x * tiles_y; t += gridDim.x) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x0 = tx * CTW + (tid & (CTW / 8 - 1)) * 8;
        const int y = 2 * (ty * CTH + tid / (CTW / 8)) + parity;
        if (x0 >= W || y < 1 || y > H - 2) continue;
        int q[8], a[8], b[8], pa[8], pb[8];
        qrow8<T, VEC>(cur, Wp, W, y, x0, q);
        qrow8<T, VEC>(cur, Wp, W, y - 1, x0, a);
        qrow8<T, VEC>(cur, Wp, W, y + 1, x0, b);
        if (PREV) {
            qrow8<T, VEC>(prev, Wp, W, y - 1, x0, pa);
            qrow8<T, VEC>(prev, Wp, W, y + 1, x0, pb);
        } else {
            qrow8<T, VEC>(cur, Wp, W, row_at(y, -2, H), x0, pa);
            qrow8<T, VEC>(cur, Wp, W, row_at(y, 2, H), x0, pb);
        }
        uint32_t c = 0, o = 0;                               // (a sample past W is 0 in all five rows: it adds nothing)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            c += (uint32_t)abs(2 * q[i] - a[i] - b[i]);
            o += (uint32_t)abs(2 * q[i] - pa[i] - pb[i]);
        }
        sum_c += c;
        sum_o += o;
    }
    sum_c = wave_sum(sum_c);
    sum_o = wave_sum(sum_o);
    if ((tid & 63) == 0) {
        s_part[0][tid >> 6] = sum_c;
        s_part[1][tid >> 6] = sum_o;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < DB / 64; ++w) {
        sum_c += s_part[0][w];
        sum_o += s_part[1][w];
    }
    atomicAdd(ws + 0, sum_c);
    atomicAdd(ws + 1, sum_o);
    __threadfence();                                         // the sums are in memory before the count says so
    if (atomicAdd(ws + 2, 1ull) != (unsigned long long)(gridDim.x - 1)) return;
    __threadfence();
    const unsigned long long dc = atomicExch(ws + 0, 0ull), other = atomicExch(ws + 1, 0ull);
    const bool interlaced = PREV ? !(8ull * dc < 7ull * other) : dc > other;
    *decision = interlaced ? 1u : 0u;
    atomicAdd(ws + 3, 1ull);
    if (interlaced) atomicAdd(ws + 4, 1ull);
    atomicExch(ws + 2, 0ull);                                // the last workgroup: the workspace is ready again
}

}  // namespace

extern "C" {

int dcvc_deinterlace(int dtype, const void* cur_nchw, const void* prev_nchw, int Hp, int Wp, int H, int W, int keep_parity,
                     int chroma_lines, const uint32_t* decision, void* out_nchw, void* stream)
{
    const char* who = "dcvc_deinterlace";
    if (int rc = dcvc::check_frame(who, "the current frame", dtype, cur_nchw, Hp, Wp, H, W)) return rc;
    if (prev_nchw)
        if (int rc = dcvc::check_frame(who, "the previous frame", dtype, prev_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = dcvc::check_frame(who, "out", dtype, out_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(keep_parity == 0 || keep_parity == 1, "%s: keep_parity %d is not 0 (top field) or 1 (bottom field)", who, keep_parity);
    DCVC_REQUIRE(chroma_lines == 1 || chroma_lines == 2, "%s: chroma_lines %d is not 1 or 2", who, chroma_lines);
    DCVC_REQUIRE(H % (2 * chroma_lines) == 0, "%s: height %d is not a multiple of %d (two fields of %d-row lines)", who, H,
                 2 * chroma_lines, chroma_lines);
    DCVC_REQUIRE(((uintptr_t)decision & 3) == 0, "%s: the decision word is not 4-byte aligned", who);
    const size_t es = dcvc::elem_size(dtype);
    const uint64_t bytes = (uint64_t)3 * Hp * Wp * es;
    const auto overlaps = [&](const void* p) {
        return (uintptr_t)out_nchw < (uintptr_t)p + bytes && (uintptr_t)p < (uintptr_t)out_nchw + bytes;
    };
    DCVC_REQUIRE(!overlaps(cur_nchw), "%s: out overlaps the current frame (neighbours are read)", who);
    DCVC_REQUIRE(!prev_nchw || !overlaps(prev_nchw), "%s: out overlaps the previous frame (neighbours are read)", who);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, Wp, Hp, TW, TH, grid)) return rc;
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, cur_nchw, out_nchw) && dcvc::vec_ok(16 / (int)es, es, Wp, prev_nchw);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            dcvc::with_flag(prev_nchw != nullptr, [&](auto p) {
                deinterlace_kernel<T, decltype(v)::value, decltype(p)::value, false><<<grid, DB, 0, (hipStream_t)stream>>>(
                    decision, (const T*)cur_nchw, (const T*)prev_nchw, nullptr, Hp, Wp, H, W, keep_parity, chroma_lines,
                    (T*)out_nchw);
            });
        });
    });
}

int64_t dcvc_comb_ws_bytes(void) { return (int64_t)8 * WS_WORDS; }

int dcvc_comb_detect(int dtype, const void* cur_nchw, const void* prev_nchw, int Hp, int Wp, int H, int W, int keep_parity,
                     void* workspace, uint32_t* decision, void* stream)
{
    const char* who = "dcvc_comb_detect";
    if (int rc = dcvc::check_frame(who, "the current frame", dtype, cur_nchw, Hp, Wp, H, W)) return rc;
    if (prev_nchw)
        if (int rc = dcvc::check_frame(who, "the previous frame", dtype, prev_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(keep_parity == 0 || keep_parity == 1, "%s: keep_parity %d is not 0 (top field) or 1 (bottom field)", who, keep_parity);
    DCVC_REQUIRE(H % 2 == 0, "%s: height %d is not even (two fields)", who, H);
    DCVC_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: the workspace is null or not 8-byte aligned", who);
    DCVC_REQUIRE(decision && ((uintptr_t)decision & 3) == 0, "%s: the decision word is null or not 4-byte aligned", who);
    dim3 tiles;
    if (int rc = dcvc::tile_grid(who, W, H / 2, CTW, CTH, tiles)) return rc;
    // as many workgroups as give each the same number of tiles (but for the last), MAX_GROUPS at most
    const int64_t n = (int64_t)tiles.x * tiles.y, each = (n + MAX_GROUPS - 1) / MAX_GROUPS;
    const unsigned groups = (unsigned)((n + each - 1) / each);
    const size_t es = dcvc::elem_size(dtype);
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, cur_nchw, prev_nchw);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            dcvc::with_flag(prev_nchw != nullptr, [&](auto p) {
                comb_detect_kernel<T, decltype(v)::value, decltype(p)::value><<<groups, DB, 0, (hipStream_t)stream>>>(
                    (const T*)cur_nchw, (const T*)prev_nchw, Wp, H, W, keep_parity, (int)tiles.x, (int)tiles.y,
                    (unsigned long long*)workspace, decision);
            });
        });
    });
}

}  // extern "C"
