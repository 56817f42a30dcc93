// dcvc_fieldmatch.hip - the deinterlacer's film mode (docs/deinterlace.md, "Film mode", is the normative text,
// tests/fieldmatch_ref.py its numpy restatement): which field completes the kept field of this frame - the other field of the
// same frame (candidate c) or the other field of the previous frame (candidate p)?
//   dcvc_field_match    per candidate the largest number of combed samples in one 16 x 16 block of the luma picture, the rule,
//                       the two decision words (filter, weave) and four running counters, in one launch.  Integer and exact.
//   dcvc_field_weave    behind a weave word that reads 1: the rows that are not kept take the previous frame's bits, in the
//                       three planes, and the replicate pad follows.  Behind a 0 the launch writes nothing.
// dcvc_field_match: a workgroup of four waves per 256 x 64 tile of the H x W luma picture, a wave per 128 x 32 of it: lane l
// owns the 8 columns from 8 * (l % 16) in the 8 rows from 8 * (l / 16) - a quarter of a block, so a block's count is the sum
// over lanes l, l ^ 1, l ^ 16 and l ^ 17.  A lane walks down its four judged rows with a window of five quantised rows
// (a, s, e of each candidate's other field, b, d of the kept field): per judged row it loads one row of prev and two of cur,
// 16 bytes per access where the addresses allow (two in fp32).  Block counts -> wave maximum (shuffles) -> LDS -> ONE
// atomicMax per candidate and workgroup (none where the maximum is 0).  Workspace, sixteen 32-bit words, zero before the first
// call: [0] max_c, [1] max_p, [2] workgroups done - zero again when the kernel ends (dcvc_comb_detect's way) - [4] frames
// judged, [5] passed, [6] woven, [7] filtered, running; [8], [9] max_c and max_p of the last call, for the log and the tests.
// The workgroup that counts last takes the maxima out, applies the rule and writes the decision words.
// dcvc_field_weave: a workgroup per 128 x 32 tile of one plane's Hp x Wp; a thread copies 8 columns of the rows of its pair
// of lines that are not kept.  The weave word is the kernel's FIRST parameter and the file is built with the first two dwords
// of the kernel arguments preloaded (csrc/Makefile), as dcvc_deint.hip is: a launch that has nothing to do ends on one load.
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>
#include <type_traits>

namespace {

constexpr int DB = 256;              // threads per workgroup, both kernels
constexpr int COMB_T = 36;           // the measure's threshold T in 10-bit codes (9 eight-bit codes)
constexpr int COMB_MI = 20;          // combed samples a block may hold
constexpr int MTW = 256, MTH = 64;   // match: a workgroup's tile (2 x 2 waves of 128 x 32)
constexpr int SR = 8;                // match: rows of a lane's strip (half a block)
constexpr int WTW = 128, WTH = 32;   // weave: a workgroup's tile (16 threads of 8 columns x 16 pairs of rows)
constexpr int WS_WORDS = 16;         // match: 32-bit words of the workspace

__device__ __forceinline__ int quant10(float v)
{
    // (fmaxf returns the other operand for a NaN: a NaN sample counts as 0) - dcvc_comb_detect's quantiser
    return (int)fminf(fmaxf(rintf(v * 1023.0f), 0.0f), 1023.0f);
}

// 8 quantised luma samples of row y (0 <= y < H) from column x0 (a multiple of 8, x0 < W); samples past W are 0 in every
// row, so they are never combed
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

// the combed samples among 8 columns of one judged row: a, s, e the other field's rows y - 2, y, y + 2; b, d the kept field's
__device__ __forceinline__ int combed8(const int* a, const int* b, const int* s, const int* d, const int* e)
{
    int n = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int d1 = s[i] - b[i], d2 = s[i] - d[i];
        const bool comb = (d1 > COMB_T && d2 > COMB_T) || (d1 < -COMB_T && d2 < -COMB_T);
        n += (comb && abs(a[i] + 4 * s[i] + e[i] - 3 * (b[i] + d[i])) > 6 * COMB_T) ? 1 : 0;
    }
    return n;
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

// VEC: both frames are 16-byte aligned and so is every row; PREV: there is a previous frame
template <typename T, bool VEC, bool PREV>
__global__ __launch_bounds__(DB) void field_match_kernel(const T* __restrict__ cur, const T* __restrict__ prev, int Wp, int H, int W,
                                                         int parity, uint32_t* ws, uint32_t* decision2)
{
    __shared__ int s_max[2][DB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * MTW + (wave & 1) * (MTW / 2) + (lane & 15) * 8;
    const int r0 = blockIdx.y * MTH + (wave >> 1) * (MTH / 2) + (lane >> 4) * SR;
    int n_c = 0, n_p = 0;
    if (x0 < W && r0 < H) {
        // judged rows of the strip: y = y0, y0 + 2, ..; a row is read at its coordinate clamped into the picture, and a judged
        // row with 2 <= y <= H - 3 reaches no clamped one - the others are not counted
        const int y0 = r0 + 1 - parity;
        const auto at = [&](int y) { return clampi(y, 0, H - 1); };
        int ca[8], cs[8], ce[8], pa[8], ps[8], pe[8], b[8], d[8];
        qrow8<T, VEC>(cur, Wp, W, at(y0 - 2), x0, ca);
        qrow8<T, VEC>(cur, Wp, W, at(y0 - 1), x0, b);
        qrow8<T, VEC>(cur, Wp, W, at(y0), x0, cs);
        if (PREV) {
            qrow8<T, VEC>(prev, Wp, W, at(y0 - 2), x0, pa);
            qrow8<T, VEC>(prev, Wp, W, at(y0), x0, ps);
        }
#pragma unroll
        for (int k = 0; k < SR / 2; ++k) {
            const int y = y0 + 2 * k;
            qrow8<T, VEC>(cur, Wp, W, at(y + 1), x0, d);
            qrow8<T, VEC>(cur, Wp, W, at(y + 2), x0, ce);
            if (PREV) qrow8<T, VEC>(prev, Wp, W, at(y + 2), x0, pe);
            const bool judged = y >= 2 && y <= H - 3;
            n_c += judged ? combed8(ca, b, cs, d, ce) : 0;
            if (PREV) n_p += judged ? combed8(pa, b, ps, d, pe) : 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                ca[i] = cs[i];
                cs[i] = ce[i];
                b[i] = d[i];
                if (PREV) {
                    pa[i] = ps[i];
                    ps[i] = pe[i];
                }
            }
        }
    }
    // a block: this lane, its neighbour in the row of 16 lanes and the two in the strip below or above
    n_c += __shfl_xor(n_c, 1, 64);
    n_c += __shfl_xor(n_c, 16, 64);
    n_c = wave_max(n_c);
    if (PREV) {
        n_p += __shfl_xor(n_p, 1, 64);
        n_p += __shfl_xor(n_p, 16, 64);
        n_p = wave_max(n_p);
    }
    if (lane == 0) {
        s_max[0][wave] = n_c;
        s_max[1][wave] = n_p;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < DB / 64; ++w) {
        n_c = max(n_c, s_max[0][w]);
        n_p = max(n_p, s_max[1][w]);
    }
    if (n_c > 0) atomicMax(ws + 0, (uint32_t)n_c);
    if (n_p > 0) atomicMax(ws + 1, (uint32_t)n_p);
    __threadfence();                                         // the maxima are in memory before the count says so
    if (atomicAdd(ws + 2, 1u) != gridDim.x * gridDim.y - 1) return;
    __threadfence();
    const uint32_t max_c = atomicExch(ws + 0, 0u), max_p = atomicExch(ws + 1, 0u);
    const bool pass = max_c <= (uint32_t)COMB_MI;
    const bool weave = !pass && PREV && max_p <= (uint32_t)COMB_MI;
    decision2[0] = (pass || weave) ? 0u : 1u;
    decision2[1] = weave ? 1u : 0u;
    atomicAdd(ws + 4, 1u);
    atomicAdd(ws + (pass ? 5 : weave ? 6 : 7), 1u);
    atomicExch(ws + 8, max_c);
    atomicExch(ws + 9, max_p);
    atomicExch(ws + 2, 0u);                                  // the last workgroup: the workspace is ready again
}

// U: the storage type's bits.  VEC: prev and out are 16-byte aligned and so is every row
template <typename U, bool VEC>
__global__ __launch_bounds__(DB) void field_weave_kernel(const uint32_t* __restrict__ weave, const U* __restrict__ prev, int Hp, int Wp,
                                                         int H, int W, int parity, int chroma_lines, U* __restrict__ out)
{
    if (*weave == 0u) return;
    const int tid = threadIdx.x;
    const int64_t plane = (int64_t)blockIdx.z * Hp * Wp;
    const int L = blockIdx.z == 0 ? 1 : chroma_lines;
    const int vr = tid >> 4, x = blockIdx.x * WTW + (tid & 15) * 8;
    if (x >= Wp) return;
    // the thread's two rows: row vr % L of the first and of the second line of pair vr / L of the tile's pairs of lines
    const int yl = blockIdx.y * WTH + 2 * L * (vr / L) + vr % L;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int y = yl + s * L;
        if (y >= Hp) continue;
        const int sy = min(y, H - 1);                        // below the picture: the replicate pad of its last row
        if (((sy / L) & 1) == parity) continue;              // a kept row: cur's bits stay
        const U* row = prev + plane + (int64_t)sy * Wp;
        Pix8<U> o;
        if (VEC && x + 8 <= W) {
            o = *reinterpret_cast<const Pix8<U>*>(row + x);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) o.v[i] = row[min(x + i, W - 1)];
        }
        U* dst = out + plane + (int64_t)y * Wp + x;
        if (VEC && x + 8 <= Wp) {
            *reinterpret_cast<Pix8<U>*>(dst) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (x + i < Wp) dst[i] = o.v[i];
        }
    }
}

}  // namespace

extern "C" {

int64_t dcvc_field_match_ws_bytes(void) { return (int64_t)4 * WS_WORDS; }

int dcvc_field_match(int dtype, const void* cur_nchw, const void* prev_nchw, int Hp, int Wp, int H, int W, int keep_parity,
                     void* workspace, uint32_t* decision2, void* stream)
{
    const char* who = "dcvc_field_match";
    if (int rc = dcvc::check_frame(who, "the current frame", dtype, cur_nchw, Hp, Wp, H, W)) return rc;
    if (prev_nchw)
        if (int rc = dcvc::check_frame(who, "the previous frame", dtype, prev_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(keep_parity == 0 || keep_parity == 1, "%s: keep_parity %d is not 0 (top field) or 1 (bottom field)", who, keep_parity);
    DCVC_REQUIRE(H % 2 == 0, "%s: height %d is not even (two fields)", who, H);
    DCVC_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: the workspace is null or not 8-byte aligned", who);
    DCVC_REQUIRE(decision2 && ((uintptr_t)decision2 & 3) == 0, "%s: the decision words are null or not 4-byte aligned", who);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, W, H, MTW, MTH, grid)) return rc;
    grid.z = 1;                                              // luma only
    const size_t es = dcvc::elem_size(dtype);
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, cur_nchw, prev_nchw);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            dcvc::with_flag(prev_nchw != nullptr, [&](auto p) {
                field_match_kernel<T, decltype(v)::value, decltype(p)::value><<<grid, DB, 0, (hipStream_t)stream>>>(
                    (const T*)cur_nchw, (const T*)prev_nchw, Wp, H, W, keep_parity, (uint32_t*)workspace, decision2);
            });
        });
    });
}

int dcvc_field_weave(int dtype, const void* prev_nchw, int Hp, int Wp, int H, int W, int keep_parity, int chroma_lines,
                     const uint32_t* weave, void* out_nchw, void* stream)
{
    const char* who = "dcvc_field_weave";
    if (int rc = dcvc::check_frame(who, "the previous frame", dtype, prev_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = dcvc::check_frame(who, "out", dtype, out_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(keep_parity == 0 || keep_parity == 1, "%s: keep_parity %d is not 0 (top field) or 1 (bottom field)", who, keep_parity);
    DCVC_REQUIRE(chroma_lines == 1 || chroma_lines == 2, "%s: chroma_lines %d is not 1 or 2", who, chroma_lines);
    DCVC_REQUIRE(H % (2 * chroma_lines) == 0, "%s: height %d is not a multiple of %d (two fields of %d-row lines)", who, H,
                 2 * chroma_lines, chroma_lines);
    DCVC_REQUIRE(weave && ((uintptr_t)weave & 3) == 0, "%s: the weave word is null or not 4-byte aligned", who);
    const size_t es = dcvc::elem_size(dtype);
    const uint64_t bytes = (uint64_t)3 * Hp * Wp * es;
    DCVC_REQUIRE(!((uintptr_t)out_nchw < (uintptr_t)prev_nchw + bytes && (uintptr_t)prev_nchw < (uintptr_t)out_nchw + bytes),
                 "%s: out overlaps the previous frame", who);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, Wp, Hp, WTW, WTH, grid)) return rc;
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, prev_nchw, out_nchw);
    return dcvc::typed(dtype, [&](auto tag) {
        using U = std::conditional_t<sizeof(decltype(tag)) == 2, uint16_t, uint32_t>;      // a copy of bits: no float is formed
        dcvc::with_flag(vec, [&](auto v) {
            field_weave_kernel<U, decltype(v)::value><<<grid, DB, 0, (hipStream_t)stream>>>(
                weave, (const U*)prev_nchw, Hp, Wp, H, W, keep_parity, chroma_lines, (U*)out_nchw);
        });
    });
}

}  // extern "C"
