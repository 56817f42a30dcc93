// dcvc_tf.hip - motion-compensated temporal pre-filter on model frames [3][Hp][Wp] (docs/temporal_filter.md, the normative
// text; tests/tf_ref.py restates it in numpy).  Encoder side only: nothing here is seen by a decoder.  Integer up to the blend:
//   tf_pyramid_kernel   luma -> Q0 | Q1 | Q2 (uint16): the 10-bit quantiser of dcvc_frame_analyze and two 2 x 2 means.  A thread
//                       per Q2 sample forms the 4 x 4 Q0 and 2 x 2 Q1 samples under it, so one launch writes the three levels.
//   tf_motion_kernel    one launch per level, the reference in gridDim.z.  32 lanes per 8 x 8 block, eight blocks per workgroup:
//                       the block of the current level and the reference window around its centre (the parent's vector times
//                       two) are staged in LDS as uint16 with the clamps applied, so that the candidates' SADs are LDS reads
//                       and integer ops: per row a 16-byte broadcast read of the block's row and five dwords of the window,
//                       aligned by v_alignbit and summed two samples per v_sad_u16 (a block cut by the level's edge reads
//                       its window sample by sample: its positions past the edge repeat the edge's).  A lane owns the
//                       candidates lane, lane + 32, ...; the winner is the minimum of the packed key
//                       SAD << 12 | (|dy| + |dx|) << 8 | (dy + 4) << 4 | (dx + 4), the document's total order.
//   tf_blend_kernel     one launch for the three planes, a workgroup per 32 x 64 tile of one plane, a thread per row of an
//                       8 x 8 block (8 samples: one vector, one weight wb per reference).  The reference rows are gathered at
//                       the block's vector: contiguous where the shifted row lies inside the picture (nothing is assumed about
//                       its alignment), element by element with clamped columns where it does not.  fp32 multiply and add in
//                       reference order, never fused; ONE rounding to the storage type.  Elements outside the picture are
//                       computed at the clamped coordinate: the replicate pad of the filtered picture.  The luma plane's
//                       sum of (Wsum - 256) goes wave -> LDS -> ONE 64-bit integer vector atomic per workgroup.  Its level
//                       is an argument, or (dcvc_tf_blend_auto) a word of device memory read once, uniformly.
//   tf_noise_kernel     the level's choice, part one: one value per 8 x 8 block and table - the Laplacian sum S >> 2 of the
//                       current Q0 and the level-0 SADs of the references at distance +-1, clipped to 4095 - counted into
//                       4096-bin histograms.  A workgroup walks 32 x 64 tiles of Q0, each staged in LDS with a one-sample
//                       halo and the clamps applied (every sample is read from memory once per tile); a thread forms the
//                       8 responses of one row of a block (the mask is [1 -2 1]' [1 -2 1]: columns first), a wave sums a row
//                       of 8 blocks.  Integer atomics into the workgroup's LDS histograms, whose non-zero bins go to the
//                       global ones at the end: no result depends on the order of arrival.
//   tf_level_kernel     part two, one workgroup: per table the number of positive values and the value of rank n_pos >> 2
//                       among them (a prefix sum over the bins), the minimum over the tables, the level rule, the totals.
// tf_shared.hpp holds what dcvc_tf_subpel.hip (quarter-pel motion) has in common with this file: constants and argument
// structs, the blend's arithmetic around its sample fetch, and the host check and launch of the blend entries.  This file owns
// the gather, tf_blend_kernel's guard (memory is touched only inside the frame) and its loads of all references' vectors and
// errors ahead of the gathers.  No allocation and no synchronisation in any entry point.
#include "tf_shared.hpp"

#include <cstdint>

namespace {

// ---------------------------------------------------------------------------------- pyramid
template <typename T>
__global__ __launch_bounds__(TB) void tf_pyramid_kernel(const T* __restrict__ x, int Wp, int H, int W, uint16_t* __restrict__ pyr)
{
    const int H1 = (H + 1) >> 1, W1 = (W + 1) >> 1, H2 = (H1 + 1) >> 1, W2 = (W1 + 1) >> 1;
    uint16_t* q0 = pyr;
    uint16_t* q1 = q0 + (int64_t)H * W;
    uint16_t* q2 = q1 + (int64_t)H1 * W1;
    const int x2 = blockIdx.x * 64 + (threadIdx.x & 63), y2 = blockIdx.y * (TB / 64) + (threadIdx.x >> 6);
    if (x2 >= W2 || y2 >= H2) return;
    int s2 = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool own1 = 2 * y2 + i < H1 && 2 * x2 + j < W1;          // (a clamped Q1 sample is its neighbour's to write)
            const int r1 = min(2 * y2 + i, H1 - 1), c1 = min(2 * x2 + j, W1 - 1);
            int s1 = 0;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int r0 = min(2 * r1 + a, H - 1), c0 = min(2 * c1 + b, W - 1);
                    const int q = quant10((float)x[(int64_t)r0 * Wp + c0]);
                    s1 += q;
                    if (own1 && 2 * r1 + a < H && 2 * c1 + b < W) q0[(int64_t)r0 * W + c0] = (uint16_t)q;
                }
            }
            const int v1 = (s1 + 2) >> 2;
            if (own1) q1[(int64_t)r1 * W1 + c1] = (uint16_t)v1;
            s2 += v1;
        }
    }
    q2[(int64_t)y2 * W2 + x2] = (uint16_t)((s2 + 2) >> 2);
}

// ---------------------------------------------------------------------------------- motion
struct alignas(16) U16x8 {
    uint16_t v[8];
};

// R: the offsets' range (4 at level 2, 2 below).  parent: the coarser level's vectors [ref][ph * pw][2], or nullptr (centre 0).
// mv [ref][gh * gw][2] as (y, x); err [ref][gh * gw] or nullptr.
template <int R>
__global__ __launch_bounds__(TB) void tf_motion_kernel(TfPlanes p, int64_t level_off, int Hl, int Wl, int gh, int gw,
                                                       const int16_t* __restrict__ parent, int ph, int pw,
                                                       int16_t* __restrict__ mv, uint32_t* __restrict__ err)
{
    constexpr int WIN = 8 + 2 * R, SIDE = 2 * R + 1, NC = SIDE * SIDE;
    __shared__ U16x8 s_cur[NB * 8];                       // [block][row]
    __shared__ uint32_t s_ref32[NB * WIN * WIN / 2 + 1];  // [block][window row][window column] of uint16, one dword of slack
    uint16_t* s_ref = reinterpret_cast<uint16_t*>(s_ref32);

    const int g = threadIdx.x >> 5, l = threadIdx.x & 31, ref = blockIdx.z;
    const int nblk = gh * gw;
    const int b = blockIdx.x * NB + g;
    const bool live = b < nblk;                           // (uniform over the 32 lanes of a block)
    const uint16_t* qc = p.cur + level_off;
    const uint16_t* qr = p.ref[ref] + level_off;
    const int by = live ? b / gw : 0, bx = live ? b - by * gw : 0;
    const int y0 = by * 8, x0 = bx * 8;
    int cy = 0, cx = 0;
    if (live && parent != nullptr) {
        const int16_t* m = parent + ((int64_t)ref * ph * pw + (int64_t)min(by >> 1, ph - 1) * pw + min(bx >> 1, pw - 1)) * 2;
        cy = 2 * (int)m[0];
        cx = 2 * (int)m[1];
    }
    if (live) {
        // position (y, x) of the block holds Qc[min(y, Hl - 1)][min(x, Wl - 1)]
        uint16_t* sc = reinterpret_cast<uint16_t*>(s_cur + g * 8);
        for (int i = l; i < 64; i += 32)
            sc[i] = qc[(int64_t)min(y0 + (i >> 3), Hl - 1) * Wl + min(x0 + (i & 7), Wl - 1)];
        // window row r holds reference row clamp(y0 + r - R + cy), column c reference column clamp(x0 + c - R + cx)
        for (int i = l; i < WIN * WIN; i += 32) {
            const int r = i / WIN, c = i - r * WIN;
            s_ref[g * WIN * WIN + i] = qr[(int64_t)clampi(y0 + r - R + cy, 0, Hl - 1) * Wl + clampi(x0 + c - R + cx, 0, Wl - 1)];
        }
    }
    __syncthreads();
    // a position past the level's edge is the edge's: yc = min(y, Hl - 1) moves with the candidate as the edge sample does
    const int hy = live ? min(7, Hl - 1 - y0) : 0, hx = live ? min(7, Wl - 1 - x0) : 0;
    unsigned best = 0xFFFFFFFFu;
    for (int c = l; c < NC; c += 32) {
        const int dy = c / SIDE - R, dx = c - (c / SIDE) * SIDE - R;
        unsigned sad = 0;
        if (hy == 7 && hx == 7) {
            // a whole block (uniform over its 32 lanes): a row of the window is 8 contiguous samples from an even or an odd
            // one - five dwords, brought into line by v_alignbit, against the block's row two samples per v_sad_u16
            const uint32_t* rw = s_ref32 + ((g * WIN * WIN + (dy + R) * WIN + dx + R) >> 1);      // (WIN and WIN * WIN are even)
            const unsigned odd16 = (unsigned)((dx + R) & 1) * 16u;
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                const U32x4 cr = reinterpret_cast<const U32x4*>(s_cur)[g * 8 + y];
                uint32_t w[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) w[i] = rw[y * (WIN / 2) + i];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    sad = __builtin_amdgcn_sad_u16(cr.v[i], __builtin_amdgcn_alignbit(w[i + 1], w[i], odd16), sad);
            }
        } else {
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                const U16x8 cr = s_cur[g * 8 + y];
                const uint16_t* rr = s_ref + g * WIN * WIN + (min(y, hy) + dy + R) * WIN + dx + R;
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const int d = (int)cr.v[x] - (int)rr[min(x, hx)];
                    sad += (unsigned)(d < 0 ? -d : d);
                }
            }
        }
        const unsigned key = sad << 12 | (unsigned)((dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx)) << 8 | (unsigned)(dy + 4) << 4 |
                             (unsigned)(dx + 4);                    // sad <= 64 * 1023 < 2^16
        best = min(best, key);
    }
#pragma unroll
    for (int m = 16; m > 0; m >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, m, 32));
    if (live && l == 0) {
        const int64_t at = (int64_t)ref * nblk + b;
        mv[2 * at] = (int16_t)(cy + (int)((best >> 4) & 15u) - 4);
        mv[2 * at + 1] = (int16_t)(cx + (int)(best & 15u) - 4);
        if (err != nullptr) err[at] = best >> 12;
    }
}

// ---------------------------------------------------------------------------------- blend
// VEC: cur and out are 16-byte aligned and the row length is a multiple of 16 bytes.  AUTO: blend_level (tf_shared.hpp)
template <typename T, bool VEC, bool AUTO>
__global__ __launch_bounds__(TB) void tf_blend_kernel(const int32_t* __restrict__ level_dev, const T* __restrict__ cur, TfRefs refs, int nref, int Hp, int Wp, int H, int W,
                                                      const int16_t* __restrict__ mv, const uint32_t* __restrict__ err, int gh,
                                                      int gw, int L, T* __restrict__ out, unsigned long long* __restrict__ total)
{
    __shared__ long long s_part[TB / 64];
    const int tid = threadIdx.x, plane = blockIdx.z;
    blend_level<AUTO>(level_dev, L, nref);
    const int y = blockIdx.y * TH + (tid >> 3), xc = blockIdx.x * TW + (tid & 7) * 8;
    long long stat = 0;

    if (y < Hp && xc < Wp) {                                       // (memory is touched only in here)
        const int ye = min(y, H - 1);
        const int by = ye >> 3, bx = min(xc, W - 1) >> 3;          // xc is a multiple of 8: the 8 clamped columns share a block
        const bool full = xc + 8 <= W;
        const int64_t plane_at = (int64_t)plane * Hp * Wp;
        Pix8<T> c;
        float acc[8];
        int qc[8], wsum[8];
        const auto col = [&](int i) { return min(xc + i, W - 1); };          // element i stands at this column; the gather adds its vector
        blend_begin(cur + plane_at + (int64_t)ye * Wp, xc, VEC && full, col, c, acc, qc, wsum);
        const int64_t nblk = (int64_t)gh * gw;
        int mvys[MAX_REFS], mvxs[MAX_REFS], wbs[MAX_REFS];                 // (loaded together: the gathers wait for them)
#pragma unroll
        for (int r = 0; r < MAX_REFS; ++r) {
            mvys[r] = mvxs[r] = wbs[r] = 0;
            if (r < nref) {
                const int64_t at = r * nblk + (int64_t)by * gw + bx;
                mvys[r] = mv[2 * at];
                mvxs[r] = mv[2 * at + 1];
                wbs[r] = block_weight(refs.base[r], err[at], L);
            }
        }
#pragma unroll
        for (int r = 0; r < MAX_REFS; ++r) {
            if (r >= nref) break;
            const int mvx = mvxs[r];
            const T* rrow = (const T*)refs.ref[r] + plane_at + (int64_t)clampi(ye + mvys[r], 0, H - 1) * Wp;
            const int xs = xc + mvx;
            Pix8<T> rv;
            if (full && xs >= 0 && xs + 8 <= W) {
                struct __attribute__((packed, aligned(sizeof(T)))) Row {      // contiguous, aligned to its element only
                    T v[8];
                };
                const Row row = *reinterpret_cast<const Row*>(rrow + xs);
#pragma unroll
                for (int i = 0; i < 8; ++i) rv.v[i] = row.v[i];
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) rv.v[i] = rrow[clampi(col(i) + mvx, 0, W - 1)];
            }
            blend_accumulate(rv.v, wbs[r], L, qc, acc, wsum);
        }
        stat = blend_finish<T, VEC>(c, acc, wsum, out + plane_at + (int64_t)y * Wp, xc, Wp, W, plane == 0 && y < H);
    }
    if (plane == 0) blend_total(stat, s_part, total);                        // (uniform over the workgroup)
}

struct GatherBlend {             // names the kernel for dcvc::blend
    template <typename T, bool VEC, bool AUTO>
    static auto kernel() { return &tf_blend_kernel<T, VEC, AUTO>; }
};

// ---------------------------------------------------------------------------------- noise estimate
constexpr int BINS = 4096;       // a block value is clipped to BINS - 1
constexpr int MAX_TABLES = 3;    // the spatial table, then the references at distance -1 / +1
constexpr int NOISE_WGS = 512;   // at most so many workgroups share the tiles: each flushes its histograms once
int g_noise_wgs = NOISE_WGS;     // (dcvc_tf_noise_workgroups: a developer's knob, tools/tf_time.py sweeps it)

struct TfTables {
    int ntemporal;               // 0 .. 2
    int ref[MAX_TABLES - 1];     // which of err's tables
};

// hist [MAX_TABLES][BINS], zero on entry: table 0 the spatial one, 1 .. the temporal ones
__global__ __launch_bounds__(TB) void tf_noise_kernel(const uint16_t* __restrict__ q0, int H, int W, int gh, int gw, int tiles_x,
                                                      int tiles, const uint32_t* __restrict__ err, TfTables tabs,
                                                      uint32_t* __restrict__ hist)
{
    constexpr int SW = TW + 2, SH = TH + 2;
    __shared__ uint32_t s_hist[MAX_TABLES * BINS];
    __shared__ uint16_t s_q[SH * SW];                     // row r, column c: Q0[clamp(y0 - 1 + r)][clamp(x0 - 1 + c)]
    const int tid = threadIdx.x, ntab = 1 + tabs.ntemporal;
    for (int i = tid; i < ntab * BINS; i += TB) s_hist[i] = 0u;
    const int lane = tid & 63, wave = tid >> 6;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int y0 = ty * TH, x0 = tx * TW;
        // a wave: the 8 rows of 8 blocks; lanes 0 .. 7 count their spatial values, lanes 8 .. 15 and 16 .. 23 the same blocks'
        // values of the temporal tables (loaded here, ahead of the staging)
        const int by = (y0 >> 3) + wave, bx = (x0 >> 3) + (lane & 7), t = (lane >> 3) - 1;
        const bool counted = by < gh && bx < gw;
        uint32_t e = 0u;
        if (counted && t >= 0 && t < tabs.ntemporal) e = err[(int64_t)tabs.ref[t] * gh * gw + (int64_t)by * gw + bx];
        __syncthreads();                                  // (the histograms are cleared; the last tile is done with)
        for (int i = tid; i < SH * SW; i += TB) {
            const int r = i / SW, c = i - r * SW;
            s_q[i] = q0[(int64_t)clampi(y0 - 1 + r, 0, H - 1) * W + clampi(x0 - 1 + c, 0, W - 1)];
        }
        __syncthreads();
        // a thread: row tid >> 3 of the tile, the 8 columns of block tid & 7
        const int y = y0 + (tid >> 3), xb = x0 + (tid & 7) * 8;
        int sum = 0;
        if (xb < W) {                                     // (else the block lies past the grid)
            const int r = min(y, H - 1) - y0 + 1;         // the edge position stands for a position past the edge
            const uint16_t* up = s_q + (r - 1) * SW + (tid & 7) * 8;
            int v[10];                                    // the column sums under the 10 columns the 8 positions touch
#pragma unroll
            for (int j = 0; j < 10; ++j) v[j] = (int)up[j] - 2 * (int)up[SW + j] + (int)up[2 * SW + j];
            const int hx = min(7, W - 1 - xb);
            int resp = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int a = v[i] - 2 * v[i + 1] + v[i + 2];
                if (i <= hx) resp = a < 0 ? -a : a;
                sum += resp;
            }
        }
#pragma unroll
        for (int m = 8; m < 64; m <<= 1) sum += __shfl_xor(sum, m, 64);
        if (counted && t < tabs.ntemporal)
            atomicAdd(&s_hist[(t + 1) * BINS + (t < 0 ? min(sum >> 2, BINS - 1) : (int)min(e, (uint32_t)(BINS - 1)))], 1u);
    }
    __syncthreads();
    for (int i = tid; i < ntab * BINS; i += TB) {
        const uint32_t n = s_hist[i];
        if (n != 0u) atomicAdd(&hist[i], n);
    }
}

// one workgroup.  result: {level, N, smallest temporal figure or -1, spatial figure}; totals: nullptr or
// [level 0 .. 5 counts, sum of N, frames]
__global__ __launch_bounds__(TB) void tf_level_kernel(const uint32_t* __restrict__ hist, int ntab, int nblk, int32_t* __restrict__ result,
                                                      long long* __restrict__ totals)
{
    constexpr int PER = BINS / TB;                        // consecutive bins of a thread
    __shared__ uint32_t s_scan[TB];
    __shared__ int s_fig[MAX_TABLES];
    const int tid = threadIdx.x;
    for (int t = 0; t < ntab; ++t) {
        uint32_t c[PER], mine = 0u;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            c[i] = (tid == 0 && i == 0) ? 0u : hist[t * BINS + tid * PER + i];      // exact zeros are left out
            mine += c[i];
        }
        if (tid == 0) s_fig[t] = 0;
        s_scan[tid] = mine;
        __syncthreads();
        for (int d = 1; d < TB; d <<= 1) {                // inclusive prefix sums of the threads' counts
            const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        const uint32_t n_pos = s_scan[TB - 1], rank = n_pos >> 2;
        uint32_t below = s_scan[tid] - mine;              // positive values in the bins before this thread's
        if ((int64_t)n_pos * 8 >= (int64_t)nblk && below <= rank && rank < below + mine) {      // (one thread)
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if (rank >= below && rank < below + c[i]) s_fig[t] = tid * PER + i;
                below += c[i];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int spatial = s_fig[0];
        int temporal = -1, n = spatial;
        for (int t = 1; t < ntab; ++t) temporal = temporal < 0 ? s_fig[t] : min(temporal, s_fig[t]);
        if (temporal >= 0) n = min(n, temporal);
        int level = 0;
        if (n >= 40) {
            level = 5;
            for (int l = 4; l >= 1; --l)
                if (n <= (80 << l)) level = l;
        }
        result[0] = level;
        result[1] = n;
        result[2] = temporal;
        result[3] = spatial;
        if (totals != nullptr) {                          // (launches on a stream run in order: no other adder)
            totals[level] += 1;
            totals[6] += n;
            totals[7] += 1;
        }
    }
}

}  // namespace

extern "C" {

int64_t dcvc_tf_pyramid_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    return level_dims(H, W).elems * (int64_t)sizeof(uint16_t);
}

int64_t dcvc_tf_motion_ws_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    const LevelDims d = level_dims(H, W);
    return (int64_t)MAX_REFS * 2 * sizeof(int16_t) * ((int64_t)d.gh[1] * d.gw[1] + (int64_t)d.gh[2] * d.gw[2]);
}

int dcvc_tf_pyramid(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, uint16_t* pyramid, void* stream)
{
    const char* who = "dcvc_tf_pyramid";
    if (int rc = dcvc::check_frame(who, "x", dtype, x_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(pyramid && ((uintptr_t)pyramid & 1) == 0, "%s: the pyramid is null or not 2-byte aligned", who);
    DCVC_REQUIRE((int64_t)H * W < ((int64_t)1 << 30), "%s: picture too large", who);
    const LevelDims d = level_dims(H, W);
    const dim3 grid((unsigned)((d.w[2] + 63) / 64), (unsigned)((d.h[2] + TB / 64 - 1) / (TB / 64)), 1);
    DCVC_REQUIRE(grid.y <= 65535u, "%s: height %d too large", who, H);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        tf_pyramid_kernel<T><<<grid, TB, 0, (hipStream_t)stream>>>((const T*)x_nchw, Wp, H, W, pyramid);
    });
}

int dcvc_tf_motion(const uint16_t* cur_pyramid, const uint16_t* const* ref_pyramids, int nref, int H, int W, int16_t* mv,
                   uint32_t* err, void* ws, void* stream)
{
    const char* who = "dcvc_tf_motion";
    DCVC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 30), "%s: bad size %d x %d", who, H, W);
    DCVC_REQUIRE(nref >= 1 && nref <= MAX_REFS, "%s: %d references, 1 .. %d are supported", who, nref, MAX_REFS);
    DCVC_REQUIRE(mv && err && ws, "%s: null pointer", who);
    TfPlanes p;
    if (int rc = dcvc::check_planes(who, cur_pyramid, ref_pyramids, nref, p)) return rc;
    DCVC_REQUIRE(((uintptr_t)mv & 1) == 0 && ((uintptr_t)ws & 1) == 0, "%s: a pointer is not 2-byte aligned", who);
    DCVC_REQUIRE(((uintptr_t)err & 3) == 0, "%s: err is not 4-byte aligned", who);
    const LevelDims d = level_dims(H, W);
    int16_t* mv1 = (int16_t*)ws;                                             // [MAX_REFS][gh1 * gw1][2]
    int16_t* mv2 = mv1 + (int64_t)MAX_REFS * 2 * d.gh[1] * d.gw[1];          // [MAX_REFS][gh2 * gw2][2]
    hipStream_t st = (hipStream_t)stream;
    auto grid = [&](int l) { return dim3((unsigned)((d.gh[l] * d.gw[l] + NB - 1) / NB), 1, (unsigned)nref); };
    tf_motion_kernel<4><<<grid(2), TB, 0, st>>>(p, d.off[2], d.h[2], d.w[2], d.gh[2], d.gw[2], nullptr, 0, 0, mv2, nullptr);
    tf_motion_kernel<2><<<grid(1), TB, 0, st>>>(p, d.off[1], d.h[1], d.w[1], d.gh[1], d.gw[1], mv2, d.gh[2], d.gw[2], mv1, nullptr);
    tf_motion_kernel<2><<<grid(0), TB, 0, st>>>(p, d.off[0], d.h[0], d.w[0], d.gh[0], d.gw[0], mv1, d.gh[1], d.gw[1], mv, err);
    DCVC_LAUNCH_CHECK();
    return 0;
}

int64_t dcvc_tf_noise_ws_bytes(void) { return (int64_t)MAX_TABLES * BINS * sizeof(uint32_t); }

int dcvc_tf_noise_workgroups(int n)
{
    const int was = g_noise_wgs;
    if (n >= 1 && n <= 65535) g_noise_wgs = n;
    return was;
}

int dcvc_tf_noise(const uint16_t* cur_pyramid, const uint32_t* err, const int* dists, int nref, int H, int W, void* ws,
                  int32_t* result, int64_t* totals, void* stream)
{
    const char* who = "dcvc_tf_noise";
    DCVC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 30), "%s: bad size %d x %d", who, H, W);
    DCVC_REQUIRE(nref >= 0 && nref <= MAX_REFS, "%s: %d references, 0 .. %d are supported", who, nref, MAX_REFS);
    DCVC_REQUIRE(cur_pyramid && ws && result && (nref == 0 || (err && dists)), "%s: null pointer", who);
    DCVC_REQUIRE(((uintptr_t)cur_pyramid & 1) == 0, "%s: the pyramid is not 2-byte aligned", who);
    DCVC_REQUIRE(((uintptr_t)err & 3) == 0 && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)result & 3) == 0 && ((uintptr_t)totals & 7) == 0,
                 "%s: err, ws, result or totals is not aligned to its element size", who);
    TfTables tabs = {};
    for (int r = 0; r < nref; ++r) {
        DCVC_REQUIRE(dists[r] == 1 || dists[r] == -1 || dists[r] == 2 || dists[r] == -2, "%s: distance %d is not +-1 or +-2", who,
                     dists[r]);
        if ((dists[r] == 1 || dists[r] == -1) && tabs.ntemporal < MAX_TABLES - 1) tabs.ref[tabs.ntemporal++] = r;
    }
    const LevelDims d = level_dims(H, W);
    const int tiles_x = (W + TW - 1) / TW, tiles = tiles_x * ((H + TH - 1) / TH), ntab = 1 + tabs.ntemporal;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* hist = (uint32_t*)ws;
    DCVC_HIP(hipMemsetAsync(hist, 0, (size_t)ntab * BINS * sizeof(uint32_t), st));
    tf_noise_kernel<<<(unsigned)(tiles < g_noise_wgs ? tiles : g_noise_wgs), TB, 0, st>>>(cur_pyramid, H, W, d.gh[0], d.gw[0], tiles_x, tiles,
                                                                                     err, tabs, hist);
    tf_level_kernel<<<1, TB, 0, st>>>(hist, ntab, d.gh[0] * d.gw[0], result, reinterpret_cast<long long*>(totals));
    DCVC_LAUNCH_CHECK();
    return 0;
}

int dcvc_tf_blend(int dtype, const void* cur_nchw, const void* const* refs_nchw, const int* dists, int nref, int Hp, int Wp, int H,
                  int W, const int16_t* mv, const uint32_t* err, int level, void* out_nchw, uint64_t* weight_sum, void* stream)
{
    return dcvc::blend("dcvc_tf_blend", GatherBlend{}, dtype, cur_nchw, refs_nchw, dists, nref, Hp, Wp, H, W, mv, err, level, nullptr, out_nchw,
                 weight_sum, stream);
}

int dcvc_tf_blend_auto(int dtype, const void* cur_nchw, const void* const* refs_nchw, const int* dists, int nref, int Hp, int Wp,
                       int H, int W, const int16_t* mv, const uint32_t* err, const int32_t* level_dev, void* out_nchw,
                       uint64_t* weight_sum, void* stream)
{
    DCVC_REQUIRE(level_dev && ((uintptr_t)level_dev & 3) == 0, "dcvc_tf_blend_auto: the level's word is null or not 4-byte aligned");
    return dcvc::blend("dcvc_tf_blend_auto", GatherBlend{}, dtype, cur_nchw, refs_nchw, dists, nref, Hp, Wp, H, W, mv, err, 0, level_dev, out_nchw,
                 weight_sum, stream);
}

}  // extern "C"
