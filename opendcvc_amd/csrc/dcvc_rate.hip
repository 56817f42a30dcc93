// dcvc_rate.hip - the size of a frame's entropy-coded payload, estimated on the device from the symbols the front run
// has just produced (no reference counterpart: the reference has no rate control).  The estimate is the sum of the code
// lengths the quantised CDF tables give, as Q16 bits from uint32 cost tables built on the host in fp64
// (entropy.cost_table):
//   row t = { meta, cost[0 .. stride - 2] },  meta = (max_value << 16) | (offset & 0xffff),  max_value = sizes[t] - 2
//   cost[v] = rint(65536 * (16 - log2(cdf[v + 1] - cdf[v]))),  v = 0 .. max_value (max_value = the escape symbol)
// A symbol inside its table costs cost[value]; any other one costs cost[max_value] + 2 bits for every 2-bit bypass group
// its escape takes in the stream (rans_core.hpp).  Everything is integer arithmetic, so the result does not depend on the
// reduction order and equals tests/rate_ref.py bit for bit.
// Two launches: per-thread -> per-wave -> per-workgroup uint64 partials (the y parts read 16 bytes per access against the
// Gaussian cost tables in LDS, z against its qp's rows in global memory), then one small launch that sums the partials
// into pinned host memory.  No atomics, no host read in between.
#include "common.hpp"
#include "plane_math.hpp"
#include "rans_core.hpp"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int RB = 256;               // threads per workgroup
constexpr int kMaxPartWgs = 128;      // workgroups per y part (1080p: 130560 accesses of 16 bytes per part, 4 per thread)
constexpr int kMaxZWgs = 16;          // workgroups of z (1080p: 65280 symbols, 4080 accesses)
constexpr int kMaxLdsWords = 12288;   // 48 KB of cost table in LDS (the Gaussian group: 128 rows of 19 words, 9.5 KB)
constexpr unsigned kOne = 65536;      // one bit in Q16

struct alignas(16) Vec16 {
    uint32_t w[4];
};

// cost of one symbol against its table row; esc is set for a symbol outside the table
__device__ __forceinline__ unsigned symbol_cost(const uint32_t* row, int sym, bool& esc)
{
    const uint32_t meta = row[0];
    const int max_value = (int)(meta >> 16), offset = (int)(int16_t)(meta & 0xffff);
    const int value = sym - offset;
    esc = (unsigned)value >= (unsigned)max_value;
    if (!esc) return row[1 + value];
    const unsigned groups = rans::escape_group_count(rans::bypass_groups(rans::escape_raw(value, max_value)));
    return row[1 + max_value] + (unsigned)rans::kBypassBits * kOne * groups;
}

// partial[3 * workgroup + {0, 1, 2}] = the workgroup's Q16 bits, coded symbols, escapes
__device__ __forceinline__ void store_partial(unsigned long long bits, unsigned long long cnt, unsigned long long esc,
                                              unsigned long long* red, unsigned long long* partial)
{
    bits = wave_sum(bits);
    cnt = wave_sum(cnt);
    esc = wave_sum(esc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[3 * wave + 0] = bits;
        red[3 * wave + 1] = cnt;
        red[3 * wave + 2] = esc;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < RB / 64; ++w) s += red[3 * w + threadIdx.x];
        partial[3 * (size_t)blockIdx.x + threadIdx.x] = s;
    }
}

// workgroups [0, parts * wg_part): part = blockIdx.x / wg_part of `packed` [parts][nsym]; the rest: z
__global__ __launch_bounds__(RB) void rate_partial_kernel(const int16_t* packed, int nsym, int parts, int wg_part,
                                                          const uint32_t* gcost, int g_n, int g_stride, const int8_t* z8,
                                                          int nz, int zhw, const uint32_t* zrows, int z_stride, int wg_z,
                                                          unsigned long long* partial)
{
    extern __shared__ uint32_t lds_cost[];
    __shared__ unsigned long long red[3 * (RB / 64)];
    unsigned long long bits = 0;
    unsigned cnt = 0, nesc = 0;
    if ((int)blockIdx.x < parts * wg_part) {
        for (int i = threadIdx.x; i < g_n * g_stride; i += RB) lds_cost[i] = gcost[i];
        __syncthreads();
        const int part = blockIdx.x / wg_part, wg = blockIdx.x - part * wg_part;
        const Vec16* src = reinterpret_cast<const Vec16*>(packed + (size_t)part * nsym);
        const int nvec = nsym >> 3;
        for (int v = wg * RB + threadIdx.x; v < nvec; v += wg_part * RB) {
            const Vec16 p = src[v];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int cs = (int)(int16_t)(p.w[k >> 1] >> (16 * (k & 1)));
                const int idx = cs & 0xff;
                if (idx < g_n) {         // (0xFF, the sentinel of a skipped entry, and any index without a table: not coded)
                    bool esc;
                    bits += symbol_cost(lds_cost + idx * g_stride, cs >> 8, esc);
                    ++cnt;
                    nesc += esc;
                }
            }
        }
    } else {
        const int wg = blockIdx.x - parts * wg_part;
        const bool aligned = ((uintptr_t)z8 & 15) == 0;
        for (int v = wg * RB + threadIdx.x; v * 16 < nz; v += wg_z * RB) {
            const int i0 = v * 16, n = min(16, nz - i0);
            Vec16 p = {{0, 0, 0, 0}};
            if (aligned && n == 16) {
                p = *reinterpret_cast<const Vec16*>(z8 + i0);
            } else {
                for (int k = 0; k < n; ++k) p.w[k >> 2] |= (uint32_t)(uint8_t)z8[i0 + k] << (8 * (k & 3));
            }
            for (int k = 0; k < n; ++k) {
                const int sym = (int)(int8_t)(p.w[k >> 2] >> (8 * (k & 3)));
                bool esc;
                bits += symbol_cost(zrows + (size_t)((i0 + k) / zhw) * z_stride, sym, esc);
                ++cnt;
                nesc += esc;
            }
        }
    }
    store_partial(bits, cnt, nesc, red, partial);
}

// workgroup s < parts: out[3 s + {0, 1, 2}] = Q16 bits, kept symbols, escapes of part s; workgroup `parts`:
// out[3 parts + {0, 1}] = Q16 bits and escapes of z.  `out` is the device address of pinned host memory
__global__ __launch_bounds__(64) void rate_finish_kernel(const unsigned long long* partial, int parts, int wg_part, int wg_z,
                                                         unsigned long long* out)
{
    const int s = blockIdx.x;
    const int first = s < parts ? s * wg_part : parts * wg_part, n = s < parts ? wg_part : wg_z;
    unsigned long long a[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < n; i += 64)
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] += partial[3 * (size_t)(first + i) + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = wave_sum(a[k]);
    if (threadIdx.x == 0) {
        out[3 * s + 0] = a[0];
        if (s < parts) {
            out[3 * s + 1] = a[1];
            out[3 * s + 2] = a[2];
        } else {
            out[3 * s + 1] = a[2];
        }
    }
}

inline int part_wgs(int nsym) { return std::max(1, std::min(kMaxPartWgs, (nsym / 8 + 2 * RB - 1) / (2 * RB))); }
inline int z_wgs(int nz) { return std::max(1, std::min(kMaxZWgs, ((nz + 15) / 16 + RB - 1) / RB)); }
inline bool sizes_ok(int nsym, int parts, int nz)
{
    return nsym >= 8 && nsym % 8 == 0 && parts >= 1 && parts <= 8 && nz >= 1 && nz <= (1 << 30) && nsym <= (1 << 30);
}

}  // namespace

extern "C" {

int64_t dcvc_rate_estimate_ws_bytes(int nsym, int parts, int nz)
{
    if (!sizes_ok(nsym, parts, nz)) {
        dcvc::set_error("dcvc_rate_estimate_ws_bytes: nsym %d (a multiple of 8), parts %d (1 .. 8), nz %d", nsym, parts, nz);
        return dcvc::E_ARG;
    }
    return (int64_t)3 * sizeof(unsigned long long) * (parts * part_wgs(nsym) + z_wgs(nz));
}

int dcvc_rate_estimate(const int16_t* packed, int nsym, int parts, const uint32_t* gcost, int g_n, int g_stride,
                       const int8_t* z8, int nz, int zhw, const uint32_t* zcost, int z_n, int z_stride, int z_start,
                       void* workspace, uint64_t* out_host, void* stream)
{
    const char* who = "dcvc_rate_estimate";
    DCVC_REQUIRE(sizes_ok(nsym, parts, nz), "%s: nsym %d (a multiple of 8), parts %d (1 .. 8), nz %d", who, nsym, parts, nz);
    DCVC_REQUIRE(packed && gcost && z8 && zcost && workspace && out_host, "%s: null pointer", who);
    DCVC_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 7) == 0 &&
                     (((uintptr_t)gcost | (uintptr_t)zcost) & 3) == 0,
                 "%s: misaligned pointer (the symbols are read 16 bytes at a time)", who);
    DCVC_REQUIRE(g_n >= 1 && g_n <= 255 && g_stride >= 2 && g_n * g_stride <= kMaxLdsWords,
                 "%s: %d Gaussian cost rows of %d words do not fit the LDS", who, g_n, g_stride);
    DCVC_REQUIRE(zhw >= 1 && z_stride >= 2 && z_start >= 0 && z_n >= 1 && (int64_t)z_start + (nz + zhw - 1) / zhw <= z_n,
                 "%s: z channels %d + %d exceed the %d cost rows", who, z_start, zhw >= 1 ? (nz + zhw - 1) / zhw : 0, z_n);
    unsigned long long* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, out_host, 0));
    const int wg_part = part_wgs(nsym), wg_z = z_wgs(nz);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* partial = (unsigned long long*)workspace;
    hipLaunchKernelGGL(rate_partial_kernel, dim3(parts * wg_part + wg_z), dim3(RB), (size_t)g_n * g_stride * sizeof(uint32_t), st,
                       packed, nsym, parts, wg_part, gcost, g_n, g_stride, z8, nz, zhw, zcost + (size_t)z_start * z_stride,
                       z_stride, wg_z, partial);
    DCVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(rate_finish_kernel, dim3(parts + 1), dim3(64), 0, st, (const unsigned long long*)partial, parts, wg_part,
                       wg_z, out_dev);
    DCVC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
