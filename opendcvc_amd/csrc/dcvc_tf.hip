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
//                       sum of (Wsum - 256) goes wave -> LDS -> ONE 64-bit integer vector atomic per workgroup.
// No allocation and no synchronisation in any entry point.
#include "common.hpp"
#include "frame_host.hpp"
#include "plane_math.hpp"

#include <cstdint>

namespace {

constexpr int TB = 256;          // threads per workgroup, all three kernels
constexpr int TW = 64;           // blend: columns of a tile
constexpr int TH = 32;           // blend: rows of a tile (TB / (TW / 8) threads of 8 columns)
constexpr int NB = 8;            // motion: blocks per workgroup (32 lanes each)
constexpr int MAX_REFS = 4;
constexpr float kScale = 1023.0f;

__device__ __forceinline__ int quant10(float v)
{
    // (fmaxf returns the other operand for a NaN: a NaN sample counts as 0) - dcvc_frame_analyze's rule
    return (int)fminf(fmaxf(rintf(v * kScale), 0.0f), kScale);
}

struct LevelDims {
    int h[3], w[3];
    int64_t off[3];              // first element of a level in a pyramid
    int gh[3], gw[3];            // its grid of 8 x 8 blocks
    int64_t elems;
};

inline LevelDims level_dims(int H, int W)
{
    LevelDims d;
    d.h[0] = H;
    d.w[0] = W;
    for (int l = 1; l < 3; ++l) {
        d.h[l] = (d.h[l - 1] + 1) >> 1;
        d.w[l] = (d.w[l - 1] + 1) >> 1;
    }
    int64_t at = 0;
    for (int l = 0; l < 3; ++l) {
        d.off[l] = at;
        at += (int64_t)d.h[l] * d.w[l];
        d.gh[l] = (d.h[l] + 7) >> 3;
        d.gw[l] = (d.w[l] + 7) >> 3;
    }
    d.elems = at;
    return d;
}

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
struct TfPyramids {
    const uint16_t* cur;
    const uint16_t* ref[MAX_REFS];
};

struct alignas(16) U16x8 {
    uint16_t v[8];
};
struct alignas(16) U32x4 {
    uint32_t v[4];
};

// R: the offsets' range (4 at level 2, 2 below).  parent: the coarser level's vectors [ref][ph * pw][2], or nullptr (centre 0).
// mv [ref][gh * gw][2] as (y, x); err [ref][gh * gw] or nullptr.
template <int R>
__global__ __launch_bounds__(TB) void tf_motion_kernel(TfPyramids p, int64_t level_off, int Hl, int Wl, int gh, int gw,
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
struct TfRefs {
    const void* ref[MAX_REFS];
    int base[MAX_REFS];          // B: 102 at distance 1, 77 at distance 2
};

// VEC: cur and out are 16-byte aligned and the row length is a multiple of 16 bytes
template <typename T, bool VEC>
__global__ __launch_bounds__(TB) void tf_blend_kernel(const T* __restrict__ cur, TfRefs refs, int nref, int Hp, int Wp, int H, int W,
                                                      const int16_t* __restrict__ mv, const uint32_t* __restrict__ err, int gh,
                                                      int gw, int L, T* __restrict__ out, unsigned long long* __restrict__ total)
{
    __shared__ long long s_part[TB / 64];
    const int tid = threadIdx.x, plane = blockIdx.z;
    const int y = blockIdx.y * TH + (tid >> 3), xc = blockIdx.x * TW + (tid & 7) * 8;
    long long stat = 0;

    if (y < Hp && xc < Wp) {
        const int ye = min(y, H - 1);
        const int by = ye >> 3, bx = min(xc, W - 1) >> 3;          // xc is a multiple of 8: the 8 clamped columns share a block
        const bool full = xc + 8 <= W;
        const int64_t plane_at = (int64_t)plane * Hp * Wp;
        const T* crow = cur + plane_at + (int64_t)ye * Wp;
        Pix8<T> c;
        if (VEC && full) {
            c = *reinterpret_cast<const Pix8<T>*>(crow + xc);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) c.v[i] = crow[min(xc + i, W - 1)];
        }
        float acc[8];
        int qc[8], wsum[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float f = (float)c.v[i];
            qc[i] = quant10(f);
            acc[i] = 256.0f * f;
            wsum[i] = 256;
        }
        const int P = 1 << (3 + L);
        const long long A = 1ll << (8 + L);
        const int64_t nblk = (int64_t)gh * gw;
        int mvys[MAX_REFS], mvxs[MAX_REFS], wbs[MAX_REFS];                 // (loaded together: the gathers wait for them)
#pragma unroll
        for (int r = 0; r < MAX_REFS; ++r) {
            mvys[r] = mvxs[r] = wbs[r] = 0;
            if (r < nref) {
                const int64_t at = r * nblk + (int64_t)by * gw + bx;
                mvys[r] = mv[2 * at];
                mvxs[r] = mv[2 * at + 1];
                const long long E = (long long)err[at];
                wbs[r] = E < A ? (int)(((long long)refs.base[r] * (A * A - E * E)) >> (16 + 2 * L)) : 0;      // <= 102
            }
        }
#pragma unroll
        for (int r = 0; r < MAX_REFS; ++r) {
            if (r >= nref) break;
            const int mvy = mvys[r], mvx = mvxs[r], wb = wbs[r];
            const T* rrow = (const T*)refs.ref[r] + plane_at + (int64_t)clampi(ye + mvy, 0, H - 1) * Wp;
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
                for (int i = 0; i < 8; ++i) rv.v[i] = rrow[clampi(min(xc + i, W - 1) + mvx, 0, W - 1)];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float f = (float)rv.v[i];
                int d = qc[i] - quant10(f);
                d = d < 0 ? -d : d;
                const int w = d < P ? (wb * (P * P - d * d)) >> (6 + 2 * L) : 0;          // <= wb: 102 * 2^16 fits
                acc[i] = acc[i] + (float)w * f;
                wsum[i] += w;
            }
        }
        Pix8<T> o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float q = acc[i] * (1.0f / (float)wsum[i]);                 // (IEEE division: the fp32 nearest to 1 / Wsum)
            o.v[i] = wsum[i] == 256 ? c.v[i] : to_t<T>(q);
        }
        T* orow = out + plane_at + (int64_t)y * Wp;
        if (VEC && xc + 8 <= Wp) {
            *reinterpret_cast<Pix8<T>*>(orow + xc) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (xc + i < Wp) orow[xc + i] = o.v[i];
        }
        if (plane == 0 && y < H) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (xc + i < W) stat += wsum[i] - 256;
        }
    }
    if (plane == 0) {                                                        // (uniform over the workgroup)
        stat = wave_sum(stat);
        if ((tid & 63) == 0) s_part[tid >> 6] = stat;
        __syncthreads();
        if (tid == 0) {
            long long s = 0;
#pragma unroll
            for (int i = 0; i < TB / 64; ++i) s += s_part[i];
            if (s != 0) atomicAdd(total, (unsigned long long)s);
        }
    }
}

bool overlaps(const void* a, const void* b, uint64_t bytes)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bytes && pb < pa + bytes;
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
    DCVC_REQUIRE(cur_pyramid && ref_pyramids && mv && err && ws, "%s: null pointer", who);
    TfPyramids p = {};
    p.cur = cur_pyramid;
    for (int r = 0; r < nref; ++r) {
        DCVC_REQUIRE(ref_pyramids[r], "%s: null pointer", who);
        DCVC_REQUIRE(((uintptr_t)ref_pyramids[r] & 1) == 0, "%s: a pyramid is not 2-byte aligned", who);
        p.ref[r] = ref_pyramids[r];
    }
    DCVC_REQUIRE(((uintptr_t)cur_pyramid & 1) == 0 && ((uintptr_t)mv & 1) == 0 && ((uintptr_t)ws & 1) == 0,
                 "%s: a pointer is not 2-byte aligned", who);
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

int dcvc_tf_blend(int dtype, const void* cur_nchw, const void* const* refs_nchw, const int* dists, int nref, int Hp, int Wp, int H,
                  int W, const int16_t* mv, const uint32_t* err, int level, void* out_nchw, uint64_t* weight_sum, void* stream)
{
    const char* who = "dcvc_tf_blend";
    if (int rc = dcvc::check_frame(who, "the current frame", dtype, cur_nchw, Hp, Wp, H, W)) return rc;
    if (int rc = dcvc::check_frame(who, "out", dtype, out_nchw, Hp, Wp, H, W)) return rc;
    DCVC_REQUIRE(level >= 1 && level <= 5, "%s: level %d outside 1 .. 5", who, level);
    DCVC_REQUIRE(nref >= 0 && nref <= MAX_REFS, "%s: %d references, at most %d are supported", who, nref, MAX_REFS);
    DCVC_REQUIRE(weight_sum && (nref == 0 || (refs_nchw && dists && mv && err)), "%s: null pointer", who);
    DCVC_REQUIRE((int64_t)H * W < ((int64_t)1 << 30), "%s: picture too large", who);
    const size_t es = dcvc::elem_size(dtype);
    const uint64_t bytes = (uint64_t)3 * Hp * Wp * es;
    DCVC_REQUIRE(!overlaps(out_nchw, cur_nchw, bytes), "%s: out overlaps the current frame (neighbours are read)", who);
    TfRefs refs = {};
    for (int r = 0; r < nref; ++r) {
        if (int rc = dcvc::check_frame(who, "a reference", dtype, refs_nchw[r], Hp, Wp, H, W)) return rc;
        DCVC_REQUIRE(!overlaps(out_nchw, refs_nchw[r], bytes), "%s: out overlaps reference %d (neighbours are read)", who, r);
        DCVC_REQUIRE(dists[r] == 1 || dists[r] == -1 || dists[r] == 2 || dists[r] == -2, "%s: distance %d is not +-1 or +-2", who,
                     dists[r]);
        refs.ref[r] = refs_nchw[r];
        refs.base[r] = (dists[r] == 1 || dists[r] == -1) ? 102 : 77;
    }
    DCVC_REQUIRE(((uintptr_t)mv & 1) == 0 && ((uintptr_t)err & 3) == 0 && ((uintptr_t)weight_sum & 7) == 0,
                 "%s: mv, err or the weight sum is not aligned to its element size", who);
    dim3 grid;
    if (int rc = dcvc::tile_grid(who, Wp, Hp, TW, TH, grid)) return rc;
    const LevelDims d = level_dims(H, W);
    const bool vec = dcvc::vec_ok(16 / (int)es, es, Wp, cur_nchw, out_nchw);
    unsigned long long* total = reinterpret_cast<unsigned long long*>(weight_sum);
    return dcvc::typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        dcvc::with_flag(vec, [&](auto v) {
            tf_blend_kernel<T, decltype(v)::value><<<grid, TB, 0, (hipStream_t)stream>>>(
                (const T*)cur_nchw, refs, nref, Hp, Wp, H, W, mv, err, d.gh[0], d.gw[0], level, (T*)out_nchw, total);
        });
    });
}

}  // extern "C"
