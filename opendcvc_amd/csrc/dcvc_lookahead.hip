// dcvc_lookahead.hip - the pair cost of the frame lookahead (docs/lookahead.md is the normative text; no reference counterpart).
// The operands are two of dcvc_frame_analyze's low-resolution planes, uint16 [bh][bw].  Integers throughout, so the words do
// not depend on the order of summation and equal the numpy restatement bit for bit (tests/lookahead_ref.py):
//   mean = (sum L + n / 2) / n,  ac = sum |L - mean|                                       per plane, n = bh * bw
//   w = ac_ref == 0 ? 64 : clamp((64 ac_cur + ac_ref / 2) / ac_ref, 0, 255),  o = mean_cur - ((mean_ref w + 32) >> 6)
//   wp(r) = clamp(((r w + 32) >> 6) + o, 0, 65535)
//   mc = sum over the 8 x 8 tiles of the smallest SAD over the 49 candidates (dy, dx) in [-3, 3]^2, reference coordinates
//        clamped to the plane;  wp = the same against wp(ref)
// Three launches.  moments: one workgroup per plane, two passes over it (the second finds it in L2), four samples per access
// where both planes are 8-byte aligned, single samples otherwise.  search: a wave per tile;
// the tile's 14 x 14 reference window and its weighted copy lie in LDS as one 8-byte pair per sample, w and o are derived by
// every workgroup from the four moment words (no host read in between); lane = candidate, so the 64 samples of the tile are a
// loop of one broadcast read and one 8-byte read, and the minimum is one wave reduction; per-workgroup partials.  finish: sums
// the partials into pinned host memory.  No atomics.
#include "common.hpp"
#include "plane_math.hpp"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kMomThreads = 1024;  // threads of a moments workgroup
constexpr int LB = 256;            // threads of a search / finish workgroup
constexpr int kWaves = LB / 64;
constexpr int kTile = 8;
constexpr int kRange = 3;
constexpr int kWin = kTile + 2 * kRange;      // 14
constexpr int kCand = 2 * kRange + 1;         // 7 x 7 candidates
constexpr int kMaxSearchWgs = 1024;           // the waves stride over the tiles above 4096 of them (4K has 2040)
constexpr int kMomWords = 4;                  // workspace: mean_cur, ac_cur, mean_ref, ac_ref, then two words per search workgroup

typedef unsigned long long u64;

__device__ __forceinline__ unsigned absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

template <int VW>
struct alignas(2 * VW) Samples {
    uint16_t v[VW];
};

// the thread's share of sum f(p[i]): VW samples per access, the n % VW samples at the end one by one.  A thread sees at most
// 2^24 / 1024 samples of at most 65535: 32 bits hold its sum
template <int VW, typename F>
__device__ __forceinline__ unsigned thread_sum(const uint16_t* p, int n, F f)
{
    unsigned s = 0;
    const int nv = n / VW;
#pragma unroll 4
    for (int i = threadIdx.x; i < nv; i += kMomThreads) {
        const Samples<VW> q = reinterpret_cast<const Samples<VW>*>(p)[i];
#pragma unroll
        for (int k = 0; k < VW; ++k) s += f((unsigned)q.v[k]);
    }
    if (VW > 1)
        for (int i = nv * VW + threadIdx.x; i < n; i += kMomThreads) s += f((unsigned)p[i]);
    return s;
}

// mom[2 * blockIdx.x + {0, 1}] = mean, ac of plane blockIdx.x (0: cur, 1: ref); VW = 4 needs both planes 8-byte aligned
template <int VW>
__global__ __launch_bounds__(kMomThreads) void moments_kernel(const uint16_t* cur, const uint16_t* ref, int n, u64* mom)
{
    __shared__ u64 red[kMomThreads];
    const uint16_t* p = blockIdx.x == 0 ? cur : ref;
    const u64 total = block_sum<kMomThreads>((u64)thread_sum<VW>(p, n, [](unsigned v) { return v; }), red);
    const unsigned mean = (unsigned)((total + (u64)(n / 2)) / (u64)n);
    const u64 ac = block_sum<kMomThreads>((u64)thread_sum<VW>(p, n, [mean](unsigned v) { return absdiff(v, mean); }), red);
    if (threadIdx.x == 0) {
        mom[2 * blockIdx.x + 0] = mean;
        mom[2 * blockIdx.x + 1] = ac;
    }
}

struct Weight {
    int w, o;
};

__device__ __forceinline__ Weight weight_of(const u64* mom)
{
    const u64 mean_cur = mom[0], ac_cur = mom[1], mean_ref = mom[2], ac_ref = mom[3];
    Weight k;
    k.w = ac_ref == 0 ? 64 : (int)min((64 * ac_cur + ac_ref / 2) / ac_ref, (u64)255);      // (ac < 2^40: nothing overflows)
    k.o = (int)mean_cur - (int)(((unsigned)mean_ref * (unsigned)k.w + 32u) >> 6);
    return k;
}

// partial[2 * workgroup + {0, 1}] = the workgroup's share of mc, wp
__global__ __launch_bounds__(LB) void search_kernel(const uint16_t* cur, const uint16_t* ref, int bh, int bw, int tiles_x,
                                                    int ntiles, const u64* mom, u64* partial)
{
    __shared__ uint2 win[kWaves][kWin * kWin];      // (ref, wp(ref)) of the window of the wave's tile
    __shared__ unsigned tile[kWaves][kTile * kTile];
    __shared__ u64 sums[kWaves][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Weight k = weight_of(mom);
    const int cy = lane / kCand, cx = lane - cy * kCand;      // the lane's candidate: (dy, dx) = (cy - 3, cx - 3); lanes 49 .. 63 idle
    u64 mc = 0, wp = 0;
    // (the trip count is the same for every wave of the workgroup: the barriers are reached by all)
    for (int t0 = blockIdx.x * kWaves; t0 < ntiles; t0 += gridDim.x * kWaves) {
        const int t = t0 + wave;
        const bool live = t < ntiles;
        const int ty = live ? t / tiles_x : 0, tx = live ? t - ty * tiles_x : 0;
        const int y0 = ty * kTile, x0 = tx * kTile;
        const int th = min(kTile, bh - y0), tw = min(kTile, bw - x0);       // the samples that exist
        if (live) {
            for (int i = lane; i < kWin * kWin; i += 64) {
                const int wy = i / kWin, wx = i - wy * kWin;
                const int y = min(max(y0 + wy - kRange, 0), bh - 1), x = min(max(x0 + wx - kRange, 0), bw - 1);
                const int r = ref[(int64_t)y * bw + x];
                const int v = ((int)(((unsigned)r * (unsigned)k.w + 32u) >> 6)) + k.o;
                win[wave][i] = make_uint2((unsigned)r, (unsigned)min(max(v, 0), 65535));
            }
            const int sy = lane >> 3, sx = lane & 7;
            tile[wave][lane] = (sy < th && sx < tw) ? cur[(int64_t)(y0 + sy) * bw + x0 + sx] : 0u;
        }
        __syncthreads();
        unsigned sad = 0xffffffffu, sadw = 0xffffffffu;
        if (live && lane < kCand * kCand) {
            sad = sadw = 0;
            for (int sy = 0; sy < th; ++sy)
                for (int sx = 0; sx < tw; ++sx) {
                    const unsigned c = tile[wave][sy * kTile + sx];
                    const uint2 r = win[wave][(sy + cy) * kWin + sx + cx];
                    sad += absdiff(c, r.x);
                    sadw += absdiff(c, r.y);
                }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            sad = min(sad, (unsigned)__shfl_xor((int)sad, s));
            sadw = min(sadw, (unsigned)__shfl_xor((int)sadw, s));
        }
        if (live) {
            mc += sad;
            wp += sadw;
        }
        __syncthreads();      // the next tile's window overwrites this one's
    }
    if (lane == 0) {
        sums[wave][0] = mc;
        sums[wave][1] = wp;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 s = 0;
        for (int v = 0; v < kWaves; ++v) s += sums[v][threadIdx.x];
        partial[2 * blockIdx.x + threadIdx.x] = s;
    }
}

// out[0 .. 8) = mc, wp, w, o (two's complement), mean_cur, ac_cur, mean_ref, ac_ref; `out` is the device address of pinned
// host memory
__global__ __launch_bounds__(LB) void finish_kernel(const u64* mom, const u64* partial, int nwg, u64* out)
{
    __shared__ u64 red[LB];
    u64 s[2] = {0, 0};
    for (int i = threadIdx.x; i < nwg; i += LB) {
        s[0] += partial[2 * i + 0];
        s[1] += partial[2 * i + 1];
    }
    s[0] = block_sum<LB>(s[0], red);
    s[1] = block_sum<LB>(s[1], red);
    if (threadIdx.x == 0) {
        const Weight k = weight_of(mom);
        out[0] = s[0];
        out[1] = s[1];
        out[2] = (u64)k.w;
        out[3] = (u64)(long long)k.o;
        for (int i = 0; i < kMomWords; ++i) out[4 + i] = mom[i];
    }
}

inline bool size_ok(int bh, int bw) { return bh >= 1 && bw >= 1 && (int64_t)bh * bw <= (1ll << 24); }
inline int tiles_of(int v) { return (v + kTile - 1) / kTile; }
inline int search_wgs(int ntiles) { return std::min(kMaxSearchWgs, (ntiles + kWaves - 1) / kWaves); }

}  // namespace

extern "C" {

int64_t dcvc_lookahead_ws_bytes(int bh, int bw)
{
    if (!size_ok(bh, bw)) {
        dcvc::set_error("dcvc_lookahead_ws_bytes: a plane of bh x bw samples, each at least 1, at most 2^24 in all (got %d x %d)", bh,
                        bw);
        return dcvc::E_ARG;
    }
    return (int64_t)sizeof(u64) * (kMomWords + 2 * search_wgs(tiles_of(bh) * tiles_of(bw)));
}

int dcvc_lookahead_cost(const uint16_t* cur, const uint16_t* ref, int bh, int bw, void* workspace, uint64_t* out_host,
                        void* stream)
{
    const char* who = "dcvc_lookahead_cost";
    DCVC_REQUIRE(size_ok(bh, bw), "%s: a plane of bh x bw samples, each at least 1, at most 2^24 in all (got %d x %d)", who, bh, bw);
    DCVC_REQUIRE(cur, "%s: cur is a null pointer", who);
    DCVC_REQUIRE(ref, "%s: ref is a null pointer", who);
    DCVC_REQUIRE(workspace, "%s: workspace is a null pointer", who);
    DCVC_REQUIRE(out_host, "%s: out_host is a null pointer", who);
    DCVC_REQUIRE(((uintptr_t)cur & 1) == 0, "%s: cur is not aligned to its 2-byte samples", who);
    DCVC_REQUIRE(((uintptr_t)ref & 1) == 0, "%s: ref is not aligned to its 2-byte samples", who);
    DCVC_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace is not 8-byte aligned", who);
    DCVC_REQUIRE(((uintptr_t)out_host & 7) == 0, "%s: out_host is not 8-byte aligned", who);
    u64* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, out_host, 0));
    const int tiles_x = tiles_of(bw), ntiles = tiles_of(bh) * tiles_x, nwg = search_wgs(ntiles);
    hipStream_t st = (hipStream_t)stream;
    u64* mom = (u64*)workspace;
    u64* partial = mom + kMomWords;
    if ((((uintptr_t)cur | (uintptr_t)ref) & 7) == 0)
        hipLaunchKernelGGL(moments_kernel<4>, dim3(2), dim3(kMomThreads), 0, st, cur, ref, bh * bw, mom);
    else
        hipLaunchKernelGGL(moments_kernel<1>, dim3(2), dim3(kMomThreads), 0, st, cur, ref, bh * bw, mom);
    DCVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(search_kernel, dim3(nwg), dim3(LB), 0, st, cur, ref, bh, bw, tiles_x, ntiles, (const u64*)mom, partial);
    DCVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(LB), 0, st, (const u64*)mom, (const u64*)partial, nwg, out_dev);
    DCVC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
