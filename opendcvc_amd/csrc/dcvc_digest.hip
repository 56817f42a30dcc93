// dcvc_digest.hip - a 64-bit digest of a device buffer: what the stream's digest units carry of the entry a frame puts into
// the DPB (docs/state_digest.md; no reference counterpart).  The buffer is m = nbytes / 8 little-endian uint64 words:
//   digest = sum_j mix(w_j + (j + 1) * G) + mix(nbytes * G)   (mod 2^64),  mix = the splitmix64 finaliser, G = 0x9E3779B97F4A7C15
// The sum is commutative: the result does not depend on the reduction order and equals tests/digest_ref.py bit for bit.
// Two launches: per-thread -> per-wave -> per-workgroup uint64 partials (16 bytes per access: a base that is 8- but not
// 16-byte aligned gives one head word, an odd rest one tail word, both taken by workgroup 0), then one small launch that
// adds the partials by index, compares and writes {digest, status} into pinned host memory.  No atomics, no host read in
// between.  A drift and damage check, not a cryptographic hash.
#include "common.hpp"
#include "plane_math.hpp"

#include <algorithm>
#include <cstdint>

namespace {

typedef unsigned long long u64;

constexpr int DB = 256;                                         // threads per workgroup
constexpr int kMaxWgs = DCVC_DIGEST_PASS_WORDS / (2 * DB);      // 2048: 8 workgroups per CU, 32 KB of loads in flight per CU
constexpr u64 G = 0x9E3779B97F4A7C15ull;

static_assert(kMaxWgs * 2 * DB == DCVC_DIGEST_PASS_WORDS, "one grid-stride pass: every thread of the full grid reads two words");

__host__ __device__ __forceinline__ u64 mix(u64 z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// partial[workgroup] = the sum of mix(w_j + (j + 1) G) over the words the workgroup reads.  head: 1 if w is not 16-byte
// aligned (word 0 is then read on its own and the pairs start at word 1)
__global__ __launch_bounds__(DB) void digest_partial_kernel(const u64* w, long long m, int head, u64* partial)
{
    __shared__ u64 red[DB / 64];
    const ulonglong2* body = reinterpret_cast<const ulonglong2*>(w + head);
    const long long npair = (m - head) >> 1, stride = (long long)gridDim.x * DB;
    long long p = (long long)blockIdx.x * DB + threadIdx.x;
    u64 pos = ((u64)head + 2 * (u64)p + 1) * G;                 // (j + 1) G of the pair's first word, advanced by addition
    const u64 step = 2 * (u64)stride * G;
    u64 acc = 0;
    for (; p < npair; p += stride, pos += step) {
        const ulonglong2 v = body[p];
        acc += mix(v.x + pos) + mix(v.y + pos + G);
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && head) acc += mix(w[0] + G);
        if (threadIdx.x == 1 && ((m - head) & 1)) acc += mix(w[m - 1] + (u64)m * G);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
#pragma unroll
        for (int k = 0; k < DB / 64; ++k) s += red[k];
        partial[blockIdx.x] = s;
    }
}

// out[0] = the digest, out[1] = 0 (not compared) / 1 (equal to `expected`) / 2 (differs).  `out` is the device address of
// pinned host memory
__global__ __launch_bounds__(DB) void digest_finish_kernel(const u64* partial, int n, u64 nbytes, u64 expected, int have_expected,
                                                           u64* out)
{
    __shared__ u64 red[DB / 64];
    u64 acc = 0;
    for (int i = threadIdx.x; i < n; i += DB) acc += partial[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = mix(nbytes * G);
#pragma unroll
        for (int k = 0; k < DB / 64; ++k) s += red[k];
        out[0] = s;
        out[1] = have_expected ? (s == expected ? 1u : 2u) : 0u;
    }
}

inline bool size_ok(int64_t nbytes) { return nbytes > 0 && nbytes % 8 == 0; }
inline int digest_wgs(int64_t nbytes)
{
    const int64_t pairs = nbytes / 16 + 1;                      // (covers the pairs of either alignment)
    return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxWgs, (pairs + DB - 1) / DB));
}

}  // namespace

extern "C" {

int64_t dcvc_state_digest_ws_bytes(int64_t nbytes)
{
    if (!size_ok(nbytes)) {
        dcvc::set_error("dcvc_state_digest_ws_bytes: nbytes %lld (positive, a multiple of 8)", (long long)nbytes);
        return dcvc::E_ARG;
    }
    return (int64_t)sizeof(u64) * digest_wgs(nbytes);
}

int dcvc_state_digest(const void* data, int64_t nbytes, void* workspace, uint64_t expected, int have_expected,
                      uint64_t* out_host, void* stream)
{
    const char* who = "dcvc_state_digest";
    DCVC_REQUIRE(size_ok(nbytes), "%s: nbytes %lld (positive, a multiple of 8: the buffer is hashed as 64-bit words)", who,
                 (long long)nbytes);
    DCVC_REQUIRE(data && workspace && out_host, "%s: null pointer", who);
    DCVC_REQUIRE((((uintptr_t)data | (uintptr_t)workspace | (uintptr_t)out_host) & 7) == 0,
                 "%s: misaligned pointer (data, workspace and out_host are read and written as 64-bit words)", who);
    u64* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, out_host, 0));
    const int wgs = digest_wgs(nbytes);
    hipStream_t st = (hipStream_t)stream;
    u64* partial = (u64*)workspace;
    hipLaunchKernelGGL(digest_partial_kernel, dim3(wgs), dim3(DB), 0, st, (const u64*)data, (long long)(nbytes / 8),
                       (int)(((uintptr_t)data & 15) != 0), partial);
    DCVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(digest_finish_kernel, dim3(1), dim3(DB), 0, st, (const u64*)partial, wgs, (u64)nbytes, (u64)expected,
                       have_expected, out_dev);
    DCVC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
