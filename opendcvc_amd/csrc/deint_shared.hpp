// deint_shared.hpp - what the two translation units of the deinterlacer's filter share (dcvc_deint.hip: dcvc_deinterlace, a
// picture per frame; dcvc_deint_field.hip: dcvc_deinterlace_field, the second picture of field-rate output).
// docs/deinterlace.md defines each rule below once, and so does this file:
//   DB, TW, TH, HALO, RMAX, CS, PS     the launch shape and the two LDS tiles
//   mx2, mn2, row_at                   the document's max / min (selects) and its reflected row offset
//   stage                              rows of a plane into LDS at their unclamped place; the plane a row comes from is the
//                                      caller's: one frame, or one of two by the row's parity (field rate)
//   row8, spatial_px                   eight LDS samples as fp32; the edge-directed predictor
//   deinterlace_kernel                 THE kernel of both entries: staging, the kept row's bits, the missing row's arithmetic
//                                      with the temporal bound, the single rounding, the stores
#pragma once
#include <cstdint>

#include "common.hpp"
#include "plane_math.hpp"

namespace {

constexpr int DB = 256;              // threads per workgroup, every kernel
constexpr int TW = 128;              // deinterlace: columns of a tile (16 threads of 8 columns)
constexpr int TH = 32;               // deinterlace: rows of a tile (16 threads of a kept and a missing row; a multiple of 4)
constexpr int HALO = 8;              // staged columns either side of a tile (3 are read; 8 keeps the 16-byte pieces)
constexpr int RMAX = TH + 8;         // staged rows: 2 L above and below, L <= 2
constexpr int CS = TW + 2 * HALO + 8;   // row stride of cur in LDS, elements (rows stay 16-byte aligned)
constexpr int PS = TW + 8;           // row stride of prev in LDS

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

// rows [r0, r0 + nrows) x columns [c0, c0 + 8 * pieces) into LDS, each sample taken at its clamped coordinate;
// plane_of(row) is the plane that holds the (clamped) row: uniform over a row, a select on a pointer
template <typename T, bool VEC, typename PlaneOf>
__device__ __forceinline__ void stage(PlaneOf plane_of, int Wp, int H, int W, int r0, int nrows, int c0, int pieces, T* lds,
                                      int stride)
{
    for (int g = threadIdx.x; g < nrows * pieces; g += DB) {
        const int r = g / pieces, k = g - r * pieces, x = c0 + 8 * k;
        const int rc = clampi(r0 + r, 0, H - 1);
        const T* row = plane_of(rc) + (int64_t)rc * Wp;
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

// The filter D(cur, prev, parity) of both entries, a workgroup per TW x TH tile of one plane.  VEC: every frame given and out are
// 16-byte aligned and so is every row; PREV: there is a previous frame.  FIELD false, dcvc_deinterlace: the frames are cur and
// prev as they lie in memory, `after` is not looked at, and a decision word that reads 0 makes the launch a copy.  FIELD true,
// dcvc_deinterlace_field: the frames are the field-shifted S_n and S_(n-1), never made - per plane a row with (y / L) % 2 ==
// shift is read from `after` for the cur tile and from `cur` for the prev tile, every other row from `cur` resp. `prev`
// (= before); parity is then the kept parity of the SHIFTED frames, 1 - shift, and there is no decision word.
// The body is written out here, in the kernel, and not behind a helper: the same lines behind an inlined function are
// scheduled differently (126 VGPRs against 120 in fp16) and dcvc_deinterlace then takes 1.1 us longer per 1080p launch
template <typename T, bool VEC, bool PREV, bool FIELD>
__global__ __launch_bounds__(DB) void deinterlace_kernel(const uint32_t* __restrict__ decision, const T* __restrict__ cur,
                                                         const T* __restrict__ prev, const T* __restrict__ after, int Hp, int Wp,
                                                         int H, int W, int parity, int chroma_lines, T* __restrict__ out)
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

    if (!FIELD && decision != nullptr && *decision == 0u) {           // a progressive frame: cur's picture and its pad, nothing else
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
    if (FIELD && PREV) {
        const int shift = 1 - parity;
        const T* ap = after + plane;
        const T* bp = prev + plane;
        stage<T, VEC>([&](int r) { return ((r / L) & 1) == shift ? ap : cp; }, Wp, H, W, rb, TH + 4 * L, xb - HALO,
                      (TW + 2 * HALO) / 8, s_cur, CS);
        stage<T, VEC>([&](int r) { return ((r / L) & 1) == shift ? cp : bp; }, Wp, H, W, rb, TH + 4 * L, xb, TW / 8, s_prev, PS);
    } else {
        stage<T, VEC>([&](int) { return cp; }, Wp, H, W, rb, TH + 4 * L, xb - HALO, (TW + 2 * HALO) / 8, s_cur, CS);
        if (PREV) stage<T, VEC>([&](int) { return prev + plane; }, Wp, H, W, rb, TH + 4 * L, xb, TW / 8, s_prev, PS);
    }
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

}  // namespace
