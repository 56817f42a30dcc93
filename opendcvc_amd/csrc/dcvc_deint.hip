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
// stores each with one 16-byte access in fp16 (two in fp32).  The decision word is the
// kernel's FIRST parameter and this file is built with the first two dwords of the kernel arguments preloaded (csrc/Makefile),
// as dcvc_tf.hip is for tf_blend_kernel's level: the word's load does not wait for the argument fetch.  The host never reads it.
// dcvc_comb_detect: at most MAX_GROUPS workgroups, each striding over 256-column x 8-kept-row tiles; per-thread integer sums
// go wave (shuffles) -> LDS -> ONE 64-bit atomicAdd per sum per workgroup.  Workspace, eight 64-bit words, zero before the
// first call: [0] dc, [1] dp (with a previous frame) or ds (without), [2] workgroups done, [3] frames judged, [4] frames
// found interlaced.  The workgroup that counts last takes the sums out with atomic exchanges against 0, applies the rule,
// writes the decision word, adds to [3] and [4] and zeroes [2]: words [0 .. 2] are zero again when the kernel ends
// (dcvc_frame_maxdiff's way).  Integer atomics only: the result is exact whatever the order.  One call at a time per workspace.
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>

namespace {

constexpr int DB = 256;              // threads per workgroup, both kernels
constexpr int TW = 128;              // deinterlace: columns of a tile (16 threads of 8 columns)
constexpr int TH = 32;               // deinterlace: rows of a tile (16 threads of a kept and a missing row; a multiple of 4)
constexpr int HALO = 8;              // staged columns either side of a tile (3 are read; 8 keeps the 16-byte pieces)
constexpr int RMAX = TH + 8;         // staged rows: 2 L above and below, L <= 2
constexpr int CS = TW + 2 * HALO + 8;   // row stride of cur in LDS, elements (rows stay 16-byte aligned)
constexpr int PS = TW + 8;           // row stride of prev in LDS
constexpr int CTW = 256;             // comb: columns of a tile (32 threads of 8 columns)
constexpr int CTH = DB / (CTW / 8);  // comb: kept rows of a tile
constexpr int MAX_GROUPS = 128;      // comb: workgroups
constexpr int WS_WORDS = 8;          // comb: 64-bit words of the workspace

// the document's max / min: a select, so a NaN or an equal pair gives the second operand - on any machine
__device__ __forceinline__ float mx2(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float mn2(float a, float b) { return a < b ? a : b; }

// row y + off; an offset that leaves [0, H) takes the opposite sign; if that leaves as well it becomes 0
__device__ __forceinline__ int row_at(int y, int off, int H)
{
    int r = y + off;
    if (r >= 0 && r < H) return r;
    r = y - off;
    return (r >= 0 && r < H) ? r : y;
}

// rows [r0, r0 + nrows) x columns [c0, c0 + 8 * pieces) of a plane into LDS, each sample taken at its clamped coordinate
template <typename T, bool VEC>
__device__ __forceinline__ void stage(const T* __restrict__ plane, int Wp, int H, int W, int r0, int nrows, int c0, int pieces,
                                      T* lds, int stride)
{
    for (int g = threadIdx.x; g < nrows * pieces; g += DB) {
        const int r = g / pieces, k = g - r * pieces, x = c0 + 8 * k;
        const T* row = plane + (int64_t)clampi(r0 + r, 0, H - 1) * Wp;
        Pix8<T> v;
        if (VEC && x >= 0 && x + 8 <= W) {
            v = *reinterpret_cast<const Pix8<T>*>(row + x);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v.v[i] = row[clampi(x + i, 0, W - 1)];
        }
        *reinterpret_cast<Pix8<T>*>(lds + r * stride + 8 * k) = v;
    }
}

// 8 samples of an LDS row as fp32: from column c (a multiple of 8) where `wide`, else sample i from column cc[i] + shift
template <typename T>
__device__ __forceinline__ void row8(const T* row, bool wide, int c, const int* cc, int shift, float* v)
{
    if (wide) {
        const Pix8<T> p = *reinterpret_cast<const Pix8<T>*>(row + c);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)p.v[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)row[cc[i] + shift];
    }
}

// the spatial predictor of one sample: u / d are the lines above and below, u[3] / d[3] the sample's own column
__device__ __forceinline__ float spatial_px(const float* u, const float* d)
{
    auto score = [&](int j) {
        return (fabsf(u[3 + j - 1] - d[3 - j - 1]) + fabsf(u[3 + j] - d[3 - j])) + fabsf(u[3 + j + 1] - d[3 - j + 1]);
    };
    auto pred = [&](int j) { return (u[3 + j] + d[3 - j]) * 0.5f; };
    float s = score(0) - 1.0f / 255.0f, pr = pred(0);
#pragma unroll
    for (int sg = -1; sg <= 1; sg += 2) {
        const float s1 = score(sg);
        const bool take = s1 < s;
        s = take ? s1 : s;
        pr = take ? pred(sg) : pr;
        const float s2 = score(2 * sg);
        const bool take2 = take && s2 < s;
        s = take2 ? s2 : s;
        pr = take2 ? pred(2 * sg) : pr;
    }
    return pr;
}

// VEC: cur, prev (where given) and out are 16-byte aligned and so is every row; PREV: there is a previous frame
template <typename T, bool VEC, bool PREV>
__global__ __launch_bounds__(DB) void deinterlace_kernel(const uint32_t* __restrict__ decision, const T* __restrict__ cur,
                                                         const T* __restrict__ prev, int Hp, int Wp, int H, int W, int parity,
                                                         int chroma_lines, T* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) T s_cur[RMAX * CS];
    __shared__ __attribute__((aligned(16))) T s_prev[PREV ? RMAX * PS : 8];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t plane = (int64_t)blockIdx.z * Hp * Wp;
    const T* cp = cur + plane;
    T* op = out + plane;
    const int vr = tid >> 4, vc = (tid & 15) * 8;
    const int x = x0 + vc;
    const int L = blockIdx.z == 0 ? 1 : chroma_lines;
    // the thread's two rows: row vr % L of the kept line and of the missing line of pair vr / L of the tile's pairs of lines
    const int yl = y0 + 2 * L * (vr / L) + vr % L;
    const int y_kept = yl + L * parity, y_missing = yl + L * (1 - parity);

    auto store = [&](int y, const Pix8<T>& o) {
        if (VEC && x + 8 <= Wp) {
            *reinterpret_cast<Pix8<T>*>(op + (int64_t)y * Wp + x) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (x + i < Wp) op[(int64_t)y * Wp + x + i] = o.v[i];
        }
    };

    if (decision != nullptr && *decision == 0u) {           // a progressive frame: cur's picture and its pad, nothing else
        if (x >= Wp) return;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int y = s == 0 ? y_kept : y_missing;
            if (y >= Hp) continue;
            const T* row = cp + (int64_t)min(y, H - 1) * Wp;
            Pix8<T> o;
            if (VEC && x + 8 <= W) {
                o = *reinterpret_cast<const Pix8<T>*>(row + x);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) o.v[i] = row[min(x + i, W - 1)];
            }
            store(y, o);
        }
        return;
    }

    const int xb = min(x0, (W - 1) & ~7);                    // first column the tile's outputs come from (a multiple of 8)
    const int rb = min(y0, H - 1) - 2 * L;                   // first staged row (unclamped)
    stage<T, VEC>(cp, Wp, H, W, rb, TH + 4 * L, xb - HALO, (TW + 2 * HALO) / 8, s_cur, CS);
    if (PREV) stage<T, VEC>(prev + plane, Wp, H, W, rb, TH + 4 * L, xb, TW / 8, s_prev, PS);
    __syncthreads();
    if (x >= Wp) return;

    const bool wide = xb == x0 && x + 8 <= W;                // the 8 columns lie inside the picture, side by side in LDS
    const int cb = vc + HALO;                                // their first column in s_cur where wide
    int cc[8];                                               // column of sample i in s_cur
#pragma unroll
    for (int i = 0; i < 8; ++i) cc[i] = min(x + i, W - 1) - xb + HALO;

#pragma unroll 1
    for (int s = 0; s < 2; ++s) {                            // the kept row, then the missing one (past H - 1 either may be either)
    const int y = s == 0 ? y_kept : y_missing;
    if (y >= Hp) continue;
    const int oy = min(y, H - 1);                            // the output row's source coordinate: the replicate pad
    Pix8<T> o;
    if (((oy / L) & 1) == parity) {                          // a kept row: cur's bits
        const T* row = s_cur + (oy - rb) * CS;
        if (wide) {
            o = *reinterpret_cast<const Pix8<T>*>(row + cb);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) o.v[i] = row[cc[i]];
        }
    } else {
        const T* ru = s_cur + (row_at(oy, -L, H) - rb) * CS;
        const T* rd = s_cur + (row_at(oy, L, H) - rb) * CS;
        float pr[8], c0[8], e0[8];
        if (wide) {
            float wu[24], wd[24];                            // columns cb - 8 .. cb + 15: sample i's own column is 8 + i
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                row8(ru, true, cb - 8 + 8 * k, cc, 0, wu + 8 * k);
                row8(rd, true, cb - 8 + 8 * k, cc, 0, wd + 8 * k);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pr[i] = spatial_px(wu + 5 + i, wd + 5 + i);
                c0[i] = wu[8 + i];
                e0[i] = wd[8 + i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float u[7], d[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    u[k] = (float)ru[cc[i] - 3 + k];
                    d[k] = (float)rd[cc[i] - 3 + k];
                }
                pr[i] = spatial_px(u, d);
                c0[i] = u[3];
                e0[i] = d[3];
            }
        }
        if (PREV) {
            const int ym = row_at(oy, -L, H) - rb, yp = row_at(oy, L, H) - rb;
            const int ym2 = row_at(oy, -2 * L, H) - rb, yp2 = row_at(oy, 2 * L, H) - rb, yc = oy - rb;
            float cy[8], cm2[8], cp2[8], py[8], pm[8], pp[8], pm2[8], pp2[8];
            row8(s_cur + yc * CS, wide, cb, cc, 0, cy);
            row8(s_cur + ym2 * CS, wide, cb, cc, 0, cm2);
            row8(s_cur + yp2 * CS, wide, cb, cc, 0, cp2);
            row8(s_prev + yc * PS, wide, vc, cc, -HALO, py);
            row8(s_prev + ym * PS, wide, vc, cc, -HALO, pm);
            row8(s_prev + yp * PS, wide, vc, cc, -HALO, pp);
            row8(s_prev + ym2 * PS, wide, vc, cc, -HALO, pm2);
            row8(s_prev + yp2 * PS, wide, vc, cc, -HALO, pp2);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float d = (py[i] + cy[i]) * 0.5f;
                const float t0 = fabsf(py[i] - cy[i]) * 0.5f;
                const float t1 = (fabsf(pm[i] - c0[i]) + fabsf(pp[i] - e0[i])) * 0.5f;
                float diff = mx2(t0, t1);
                const float b = (pm2[i] + cm2[i]) * 0.5f - c0[i];
                const float f = (pp2[i] + cp2[i]) * 0.5f - e0[i];
                const float dc = d - c0[i], de = d - e0[i];
                const float mx = mx2(mx2(de, dc), mn2(b, f));
                const float mn = mn2(mn2(de, dc), mx2(b, f));
                diff = mx2(mx2(diff, mn), -mx);
                pr[i] = mn2(mx2(pr[i], d - diff), d + diff);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = to_t<T>(pr[i]);
    }
    store(y, o);
    }
}

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
                deinterlace_kernel<T, decltype(v)::value, decltype(p)::value><<<grid, DB, 0, (hipStream_t)stream>>>(
                    decision, (const T*)cur_nchw, (const T*)prev_nchw, Hp, Wp, H, W, keep_parity, chroma_lines, (T*)out_nchw);
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
