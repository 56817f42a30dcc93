// dcvc_tf_subpel.hip - quarter-pel motion for the temporal pre-filter (docs/temporal_filter.md, "Quarter-pel motion", the
// normative text; tests/tf_subpel_ref.py restates it in numpy).  Opt-in: with the option off nothing of this file is launched
// and dcvc_tf.hip's kernels do all the work.  Encoder side only.  Its own translation unit: dcvc_tf.hip is built with a kernarg
// preload this file's kernels do not want; what the two share is tf_shared.hpp's.
//   tf_refine_kernel        one launch, the reference in gridDim.z.  32 lanes per 8 x 8 block, eight blocks per workgroup, as in
//                           the whole-pel search.  The block of the current Q0 and the 16 x 16 window of the reference's Q0
//                           around the whole-pel vector (rows / columns -4 .. 11 of the block: every tap of every candidate of
//                           both stages, the clamps applied) are staged in LDS once.  A stage has 3 x 3 candidates that share
//                           three horizontal and three vertical phases: the lanes first form the three horizontal passes over
//                           the window's 16 rows (3 x 16 x 8 int32 in LDS; a lane takes whole rows: two 16-byte reads, the
//                           eight positions from registers, two 16-byte writes), then a lane owns two neighbouring positions
//                           of the block, reads their nine rows per horizontal pass once and runs the vertical pass of the
//                           nine candidates from registers - one v_sad_u16 per candidate and lane, summed over the 32 lanes
//                           by shuffles.  The winner is the minimum of the packed key
//                           R << 8 | order << 4 | candidate, R the penalised rank (17 bits) and order the place of (dy, dx) in
//                           (|dy| + |dx|, dy, dx); the unpenalised SAD is picked back by the candidate's number.  A workgroup
//                           all of whose blocks have a level-0 SAD of 0 writes its centres and leaves: nothing ranks below
//                           R = 0 at distance 0 (static and clean integer-pel material costs a load per block).
//   tf_blend_subpel_kernel  dcvc_tf_blend's launch shape (a workgroup per 32 x 64 tile of a plane, a thread per row of a block),
//                           arithmetic and statistic (tf_shared.hpp's), with the reference sample interpolated in fp32.  The eight threads of a
//                           block share its 15 source rows: each filters at most two of them horizontally (15 contiguous
//                           samples -> 8 values, straight from memory: a source sample is loaded once per block) into LDS, and
//                           after a barrier runs the vertical pass down its own column of 8 x 8 values.  A block with a whole
//                           vertical part (fy == 0) needs its own row only and stays in registers; with fx == 0 too that is
//                           the direct gather.  Multiplies and adds are separate fp32 operations in the document's order.
// No allocation and no synchronisation in any entry point.
#include "tf_shared.hpp"

#include <cstdint>

namespace {

constexpr int RW = 16;           // refinement: side of the reference window

// C[f][k]: the HEVC luma filters; tap k applies to the sample at offset k - 3
#define DCVC_TF_TAPS {{0, 0, 0, 64, 0, 0, 0, 0}, {-1, 4, -10, 58, 17, -5, 1, 0}, {-1, 4, -11, 40, 40, -11, 4, -1}, {0, 1, -5, 17, 58, -10, 4, -1}}
__constant__ int c_tap[4][8] = DCVC_TF_TAPS;
constexpr int tap(int f, int k)                           // (the same table where the phase is known at compile time)
{
    constexpr int C[4][8] = DCVC_TF_TAPS;
    return C[f][k];
}

// ---------------------------------------------------------------------------------- refinement
// stages: 1 (half pel) or 2 (then quarter pel).  mv / err: dcvc_tf_motion's; mvq [ref][gh * gw][2], errq [ref][gh * gw]
__global__ __launch_bounds__(TB) void tf_refine_kernel(TfPlanes p, int H, int W, int gh, int gw, int stages,
                                                       const int16_t* __restrict__ mv, const uint32_t* __restrict__ err,
                                                       int16_t* __restrict__ mvq, uint32_t* __restrict__ errq)
{
    __shared__ uint32_t s_cur[NB * 32];                   // [block][row][4 pairs of uint16]
    __shared__ __attribute__((aligned(16))) uint16_t s_win[NB * RW * RW];      // [block][window row][window column]
    __shared__ __attribute__((aligned(16))) int s_h[NB * 3 * RW * 8];          // [block][horizontal candidate][window row][position column]
    __shared__ int s_tap[32];

    const int g = threadIdx.x >> 5, l = threadIdx.x & 31, ref = blockIdx.z;
    const int nblk = gh * gw;
    const int b = blockIdx.x * NB + g;
    const bool live = b < nblk;                           // (uniform over the 32 lanes of a block)
    const int64_t at = (int64_t)ref * nblk + (live ? b : 0);
    const int cy = live ? (int)mv[2 * at] : 0, cx = live ? (int)mv[2 * at + 1] : 0;
    const uint32_t e0 = live ? err[at] : 0u;
    if (!__syncthreads_or(e0 != 0u)) {                    // every block matches exactly: the centres win with SAD 0
        if (live && l == 0) {
            mvq[2 * at] = (int16_t)(4 * cy);
            mvq[2 * at + 1] = (int16_t)(4 * cx);
            errq[at] = 0u;
        }
        return;
    }
    const uint16_t* qc = p.cur;
    const uint16_t* qr = p.ref[ref];
    const int by = live ? b / gw : 0, bx = live ? b - by * gw : 0;
    const int y0 = by * 8, x0 = bx * 8;
    if (threadIdx.x < 32) s_tap[threadIdx.x] = c_tap[threadIdx.x >> 3][threadIdx.x & 7];
    if (live) {
        // position (y, x) of the block holds Qc[min(y, H - 1)][min(x, W - 1)]
        uint16_t* sc = reinterpret_cast<uint16_t*>(s_cur + g * 32);
        for (int i = l; i < 64; i += 32) sc[i] = qc[(int64_t)min(y0 + (i >> 3), H - 1) * W + min(x0 + (i & 7), W - 1)];
        // window row r: reference row clamp(y0 + cy + r - 4), column c: reference column clamp(x0 + cx + c - 4)
        for (int i = l; i < RW * RW; i += 32) {
            const int r = i / RW, c = i - r * RW;
            s_win[g * RW * RW + i] = qr[(int64_t)clampi(y0 + cy + r - 4, 0, H - 1) * W + clampi(x0 + cx + c - 4, 0, W - 1)];
        }
    }
    __syncthreads();
    // a position past the picture's edge is the edge's
    const int hy = live ? min(7, H - 1 - y0) : 0, hx = live ? min(7, W - 1 - x0) : 0;
    const int py = min(l >> 2, hy), pp = l & 3;           // the lane's two positions: row l >> 2, columns 2 pp and 2 pp + 1
    const uint32_t cpair = s_cur[g * 32 + (l >> 2) * 4 + pp];
    int oy = 0, ox = 0;                                   // the stage's centre, in quarter pels from 4 * (cy, cx): -2 .. 2
    unsigned won = 0u;
    for (int st = 0; st < stages; ++st) {
        const int s = st == 0 ? 2 : 1;
        // the three horizontal passes (candidate column offsets ox - s, ox, ox + s), each over the 16 window rows: a lane takes
        // whole rows - the 16 samples in two 16-byte reads, the 8 positions' values from registers, two 16-byte writes
        for (int task = l; task < 3 * RW; task += 32) {
            const int dxi = task >> 4, wr = task & (RW - 1);
            const int d = ox + (dxi - 1) * s, f = d & 3;
            const bool next = (d >> 2) == 0;              // tap 0 of position 0 at window column 1 (whole part 0) or 0 (whole part -1)
            const U32x4* row = reinterpret_cast<const U32x4*>(s_win + g * RW * RW + wr * RW);
            const U32x4 lo = row[0], hi = row[1];
            int w[16], c[8], e[15], h[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[2 * i] = (int)(lo.v[i] & 0xFFFFu);
                w[2 * i + 1] = (int)(lo.v[i] >> 16);
                w[8 + 2 * i] = (int)(hi.v[i] & 0xFFFFu);
                w[8 + 2 * i + 1] = (int)(hi.v[i] >> 16);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) c[k] = s_tap[f * 8 + k];
#pragma unroll
            for (int i = 0; i < 15; ++i) e[i] = next ? w[i + 1] : w[i];
#pragma unroll
            for (int px = 0; px < 8; ++px) {
                h[px] = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) h[px] += c[k] * e[px + k];
                if (px > hx) h[px] = h[px - 1];           // a position past the edge is the edge's
            }
            U32x4* dst = reinterpret_cast<U32x4*>(s_h + (g * 3 + dxi) * RW * 8 + wr * 8);
            U32x4 o0, o1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                o0.v[i] = (uint32_t)h[i];
                o1.v[i] = (uint32_t)h[4 + i];
            }
            dst[0] = o0;
            dst[1] = o1;
        }
        __syncthreads();
        // the vertical passes: per horizontal candidate the lane's two columns over the 9 rows its three row offsets touch
        int cv[3][8];
        bool nextv[3];
#pragma unroll
        for (int dyi = 0; dyi < 3; ++dyi) {
            const int d = oy + (dyi - 1) * s, f = d & 3;
            nextv[dyi] = (d >> 2) == 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) cv[dyi][j] = s_tap[f * 8 + j];
        }
        unsigned sad[9];
#pragma unroll
        for (int dxi = 0; dxi < 3; ++dxi) {
            const int* hc = s_h + (g * 3 + dxi) * RW * 8 + py * 8 + 2 * pp;
            int r0[9], r1[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                r0[i] = hc[i * 8];
                r1[i] = hc[i * 8 + 1];
            }
#pragma unroll
            for (int dyi = 0; dyi < 3; ++dyi) {
                int v0 = 0, v1 = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v0 += cv[dyi][j] * (nextv[dyi] ? r0[j + 1] : r0[j]);
                    v1 += cv[dyi][j] * (nextv[dyi] ? r1[j + 1] : r1[j]);
                }
                const uint32_t s0 = (uint32_t)clampi((v0 + 2048) >> 12, 0, 1023), s1 = (uint32_t)clampi((v1 + 2048) >> 12, 0, 1023);
                sad[dyi * 3 + dxi] = __builtin_amdgcn_sad_u16(cpair, s0 | s1 << 16, 0u);
            }
        }
        unsigned best = 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
#pragma unroll
            for (int m = 16; m > 0; m >>= 1) sad[c] += (unsigned)__shfl_xor((int)sad[c], m, 32);
            // order: the place of (dy, dx) in (|dy| + |dx|, dy, dx) - the signs of the offsets, whatever the step
            constexpr unsigned order[9] = {5u, 1u, 6u, 2u, 0u, 3u, 7u, 4u, 8u};
            const unsigned rank = c == 4 ? sad[c] : sad[c] + (sad[c] >> 3);             // < 2^17
            best = min(best, rank << 8 | order[c] << 4 | (unsigned)c);
        }
        const int w = (int)(best & 15u);
#pragma unroll
        for (int c = 0; c < 9; ++c)
            if (c == w) won = sad[c];
        oy += (w / 3 - 1) * s;
        ox += (w % 3 - 1) * s;
        __syncthreads();                                  // (the next stage writes s_h)
    }
    if (live && l == 0) {
        mvq[2 * at] = (int16_t)(4 * cy + oy);
        mvq[2 * at + 1] = (int16_t)(4 * cx + ox);
        errq[at] = won;
    }
}

// ---------------------------------------------------------------------------------- blend
// the phase-F filter of v[0 .. 7]: the sum over the non-zero taps in rising order, begun with the first product, times 1 / 64
template <int F>
__device__ __forceinline__ float taps8(const float* v)
{
    float a = 0.0f;
    bool first = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (tap(F, k) != 0) {
            const float prod = (float)tap(F, k) * v[k];
            a = first ? prod : a + prod;
            first = false;
        }
    }
    return a * 0.015625f;
}

// f in 1 .. 3
__device__ __forceinline__ float taps8(int f, const float* v) { return f == 1 ? taps8<1>(v) : f == 2 ? taps8<2>(v) : taps8<3>(v); }

// g[i], i = 0 .. 7: the horizontally filtered value of reference row rrow at the position columns min(xc + i, W - 1) - i
// above hx repeats hx.  xbase: the column of tap 0 at i = 0.  With fx == 0 the eight samples themselves.
template <typename T>
__device__ __forceinline__ void filter_row(const T* __restrict__ rrow, int xbase, int W, int fx, int hx, float* g)
{
    float e[15];                                          // e[c]: the sample at column clamp(xbase + c)
    const int c0 = fx ? 0 : 3, c1 = fx ? 15 : 11;
    if (xbase + c0 >= 0 && xbase + c1 <= W) {             // contiguous, aligned to its element only
#pragma unroll
        for (int c = 0; c < 15; ++c)
            if (c >= c0 && c < c1) e[c] = (float)rrow[xbase + c];
    } else {
#pragma unroll
        for (int c = 0; c < 15; ++c)
            if (c >= c0 && c < c1) e[c] = (float)rrow[clampi(xbase + c, 0, W - 1)];
    }
    if (fx == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = e[i + 3];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = taps8(fx, e + i);
    }
#pragma unroll
    for (int i = 1; i < 8; ++i)
        if (i > hx) g[i] = g[i - 1];
}

// VEC, AUTO: as in tf_blend_kernel
template <typename T, bool VEC, bool AUTO>
__global__ __launch_bounds__(TB) void tf_blend_subpel_kernel(const int32_t* __restrict__ level_dev, const T* __restrict__ cur, TfRefs refs, int nref, int Hp, int Wp,
                                                             int H, int W, const int16_t* __restrict__ mvq, const uint32_t* __restrict__ errq,
                                                             int gh, int gw, int L, T* __restrict__ out, unsigned long long* __restrict__ total)
{
    __shared__ long long s_part[TB / 64];
    __shared__ float s_g[TB / 8][15][8];                  // [block of the tile][source row][position column]
    const int tid = threadIdx.x, plane = blockIdx.z;
    blend_level<AUTO>(level_dev, L, nref);
    // Every thread works at clamped coordinates, also one whose row or columns lie outside the frame: the eight threads of a
    // block filter its source rows for each other.  Only the store and the statistic look at where the thread is.
    const int y = blockIdx.y * TH + (tid >> 3), xc = blockIdx.x * TW + (tid & 7) * 8;
    const int ye = min(y, H - 1), xe = min(xc, W - 1);
    const int by = ye >> 3, bx = xe >> 3;                 // (the eight threads of a slot share both: rows 8 k .. 8 k + 7, one xc)
    const int hx = min(7, W - 1 - xe);                    // sample i stands at column xe + min(i, hx)
    const bool full = xc + 8 <= W;
    const int slot = (tid >> 6) * 8 + (tid & 7), t = (tid >> 3) & 7;
    const int64_t plane_at = (int64_t)plane * Hp * Wp;
    Pix8<T> c;
    float acc[8];
    int qc[8], wsum[8];
    blend_begin(cur + plane_at + (int64_t)ye * Wp, xc, VEC && full, [&](int i) { return xe + min(i, hx); }, c, acc, qc, wsum);
    const int64_t nblk = (int64_t)gh * gw;
    for (int r = 0; r < nref; ++r) {                      // (nref is uniform over the workgroup: so are the barriers)
        const int64_t at = r * nblk + (int64_t)by * gw + bx;
        const int my = mvq[2 * at], mx = mvq[2 * at + 1];
        const int wb = block_weight(refs.base[r], errq[at], L);
        const int iy = my >> 2, fy = my & 3, ix = mx >> 2, fx = mx & 3;
        const T* rpl = (const T*)refs.ref[r] + plane_at;
        const int xbase = xe + ix - 3;
        float rv[8];
        if (fy == 0) {                                    // the thread's own row is all it needs
            filter_row(rpl + (int64_t)clampi(ye + iy, 0, H - 1) * Wp, xbase, W, fx, hx, rv);
        } else {                                          // source row wr of the block: picture row 8 by + iy - 3 + wr
            for (int wr = t; wr < 15; wr += 8) {
                float g[8];
                filter_row(rpl + (int64_t)clampi(by * 8 + iy - 3 + wr, 0, H - 1) * Wp, xbase, W, fx, hx, g);
#pragma unroll
                for (int i = 0; i < 8; ++i) s_g[slot][wr][i] = g[i];
            }
        }
        __syncthreads();
        if (fy != 0) {
            const int w0 = ye - by * 8;                   // tap j of this thread's row: source row w0 + j
            float col[8][8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i) col[i][j] = s_g[slot][w0 + j][i];
#pragma unroll
            for (int i = 0; i < 8; ++i) rv[i] = taps8(fy, col[i]);
        }
        blend_accumulate(rv, wb, L, qc, acc, wsum);
        __syncthreads();                                  // (the next reference writes s_g)
    }
    long long stat = 0;
    if (y < Hp && xc < Wp) stat = blend_finish<T, VEC>(c, acc, wsum, out + plane_at + (int64_t)y * Wp, xc, Wp, W, plane == 0 && y < H);
    if (plane == 0) blend_total(stat, s_part, total);     // (uniform over the workgroup)
}

struct InterpolatingBlend {      // names the kernel for dcvc::blend
    template <typename T, bool VEC, bool AUTO>
    static auto kernel() { return &tf_blend_subpel_kernel<T, VEC, AUTO>; }
};

}  // namespace

extern "C" {

int dcvc_tf_refine(const uint16_t* cur_pyramid, const uint16_t* const* ref_pyramids, int nref, int H, int W, int subpel,
                   const int16_t* mv, const uint32_t* err, int16_t* mvq, uint32_t* errq, void* stream)
{
    const char* who = "dcvc_tf_refine";
    DCVC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 30), "%s: bad size %d x %d", who, H, W);
    DCVC_REQUIRE(nref >= 1 && nref <= MAX_REFS, "%s: %d references, 1 .. %d are supported", who, nref, MAX_REFS);
    DCVC_REQUIRE(subpel == 1 || subpel == 2, "%s: subpel %d is not 1 (half pel) or 2 (quarter pel)", who, subpel);
    DCVC_REQUIRE(mv && err && mvq && errq, "%s: null pointer", who);
    TfPlanes p;
    if (int rc = dcvc::check_planes(who, cur_pyramid, ref_pyramids, nref, p)) return rc;
    DCVC_REQUIRE(((uintptr_t)mv & 1) == 0 && ((uintptr_t)mvq & 1) == 0, "%s: a pointer is not 2-byte aligned", who);
    DCVC_REQUIRE(((uintptr_t)err & 3) == 0 && ((uintptr_t)errq & 3) == 0, "%s: err or errq is not 4-byte aligned", who);
    using dcvc::overlaps;
    const LevelDims d = level_dims(H, W);
    const int gh = d.gh[0], gw = d.gw[0];
    const uint64_t vbytes = (uint64_t)nref * gh * gw * 2 * sizeof(int16_t), ebytes = (uint64_t)nref * gh * gw * sizeof(uint32_t);
    DCVC_REQUIRE(!overlaps(mvq, vbytes, mv, vbytes) && !overlaps(mvq, vbytes, err, ebytes) && !overlaps(errq, ebytes, mv, vbytes) &&
                     !overlaps(errq, ebytes, err, ebytes) && !overlaps(mvq, vbytes, errq, ebytes),
                 "%s: mvq or errq overlaps an input or the other output", who);
    const dim3 grid((unsigned)((gh * gw + NB - 1) / NB), 1, (unsigned)nref);
    tf_refine_kernel<<<grid, TB, 0, (hipStream_t)stream>>>(p, H, W, gh, gw, subpel, mv, err, mvq, errq);
    DCVC_LAUNCH_CHECK();
    return 0;
}

int dcvc_tf_blend_subpel(int dtype, const void* cur_nchw, const void* const* refs_nchw, const int* dists, int nref, int Hp, int Wp,
                         int H, int W, const int16_t* mvq, const uint32_t* errq, int level, const int32_t* level_dev, void* out_nchw,
                         uint64_t* weight_sum, void* stream)
{
    return dcvc::blend("dcvc_tf_blend_subpel", InterpolatingBlend{}, dtype, cur_nchw, refs_nchw, dists, nref, Hp, Wp, H, W, mvq, errq,
                       level, level_dev, out_nchw, weight_sum, stream);
}

}  // extern "C"
