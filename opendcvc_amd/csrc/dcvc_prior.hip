// dcvc_prior.hip - the latent side of the entropy hand-off (Python owner: handoff.py), between "the network produced params"
// and "the coder has symbols / the network has y_hat": the checkerboard prior loop on HWC maps with the masks computed from
// (h, w, c), the encoder's compaction of kept symbols and the decoder's compacted hand-off.  Encoder and decoder must agree
// bit for bit here, so each invariant is written once: check_step / check_map / check_yhat on the host, pixel_group /
// step_update / wide16 / load_run16 / group_sum on the device.  Arithmetic is fp32 (include/dcvc_math.h), storage _Float16 or float.
#include "common.hpp"
#include "gemm_core.hpp"    // dcvc_math.h
#include "plane_math.hpp"   // ld / to_t / st / clampf / wave_sum

namespace {

using dcvc::typed;

constexpr int EB = 256;   // threads per block for 1-D kernels

inline int nblocks(int64_t n) { return (int)((n + EB - 1) / EB); }

constexpr float kScaleMin = 0.11f, kScaleMax = 16.0f;
// log(0.11) and 127 / (log(16) - log(0.11)) rounded to float exactly as the reference's python
// floats are when passed into torch fp32 expressions (entropy_models.py:235-238)
constexpr float kLogScaleMin = -2.2072749131897207f;
constexpr float kLogStepRecip = 25.50270635855404f;

// active channel group for checkerboard step `step` at pixel (h, w): see common_model.py:99-131
__device__ __forceinline__ int active_group(int n_groups, int step, int h, int w)
{
    if (n_groups == 2) return ((h + w) & 1) ^ (step & 1);
    const int pos = ((h & 1) << 1) | (w & 1);
    const int x = (step == 0) ? 0 : (step == 1) ? 3 : (step == 2) ? 2 : 1;
    return pos ^ x;
}

// the active group at pixel p = h * W + w of the map (H * W < 2^31, check_step: 32-bit division)
__device__ __forceinline__ int pixel_group(int n_groups, int step, int64_t p, int W)
{
    const int h = (int)p / W, w = (int)p - h * W;
    return active_group(n_groups, step, h, w);
}

// One (pixel, collapsed channel) of a checkerboard step - the only code that writes y_hat in such a step: the active group's
// channel takes step 0 ? v : prev + v with v = active(ch), already rounded through to_t<T> like the reference's y_hat_k
// tensors (stored in the model dtype); the other groups carry y_hat over.
template <typename T, typename F>
__device__ __forceinline__ void step_update(int n_groups, int step, int ga, int cc, int Cg, int64_t p, const T* hin, int64_t ldhi,
                                            T* hout, int64_t ldho, F&& active)
{
    for (int g = 0; g < n_groups; ++g) {
        const int ch = cc + g * Cg;
        const float prev = step == 0 ? 0.f : ld(hin, p * ldhi + ch);
        if (g != ga) {
            st(hout, p * ldho + ch, prev);
            continue;
        }
        const float yh = active(ch);
        st(hout, p * ldho + ch, step == 0 ? yh : prev + yh);
    }
}

constexpr int PT = 16;    // pixels per block of the prior kernels = positions per run of the CHW byte arrays

// A channel's PT pixels of a block are 16 contiguous bytes of a CHW byte array (which may live in pinned HOST memory, read
// or written in place by the host coder): one 16-byte access where the rows are aligned (H W a multiple of 16: 1080p, 4K),
// bytes otherwise.
__device__ __forceinline__ bool wide16(int64_t HW, const void* p)
{
    return (HW & (PT - 1)) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// the 16 positions of the run at src = array + cc * HW + p0; positions past HW read as the sentinel
__device__ __forceinline__ void load_run16(const uint8_t* src, int64_t p0, int64_t HW, bool wide, uint8_t* v)
{
    if (wide) {
        *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(src);
    } else {
        for (int j = 0; j < PT; ++j) v[j] = p0 + j < HW ? src[j] : (uint8_t)0xFF;
    }
}

constexpr int CB = 256;   // threads per compaction block

// sum of an integer over a workgroup of CB threads, one LDS word per wave (red[CB / 64]); every thread gets the result
__device__ __forceinline__ int group_sum(int v, int* red)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------ checkerboard prior loop
// One block = PT consecutive pixels x all collapsed channels.  Phase 1 walks (pixel, channel) with
// the channel fastest (coalesced HWC reads / y_hat writes); the packed symbols go through LDS so
// phase 2 can write them pixel-fastest in the reference's CHW order.
struct PriorEncArgs {
    int n_groups, step, q_mode;
    const void* y;
    int64_t ldy;
    const void* qsrc;
    int64_t ldq;
    const void* scales;
    int64_t lds;
    const void* means;
    int64_t ldm;
    int H, W, C;
    float thres;
    const void* yhat_in;
    int64_t ldhi;
    void* yhat_out;
    int64_t ldho;
    int16_t* packed;
};

template <typename T>
__global__ __launch_bounds__(EB) void prior_enc_kernel(PriorEncArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int16_t* sp = reinterpret_cast<int16_t*>(smem);   // [Cg][PT]
    const int Cg = a.C / a.n_groups;
    const int64_t HW = (int64_t)a.H * a.W;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    const T* y = (const T*)a.y;
    const T* qs = (const T*)a.qsrc;
    const T* sc = (const T*)a.scales;
    const T* mu = (const T*)a.means;
    const T* hin = (const T*)a.yhat_in;
    T* hout = (T*)a.yhat_out;
    for (int it = threadIdx.x; it < PT * Cg; it += EB) {
        const int pl = it / Cg, cc = it - pl * Cg;
        const int64_t p = p0 + pl;
        if (p >= HW) continue;
        const int ga = pixel_group(a.n_groups, a.step, p, a.W);
        int16_t packed = 0;
        step_update(a.n_groups, a.step, ga, cc, Cg, p, hin, a.ldhi, hout, a.ldho, [&](int ch) {
            float qe;
            if (a.q_mode == 0) {
                float qd = ld(qs, p * a.ldq + ch);
                qd = qd < 0.5f ? 0.5f : qd;
                qe = 1.0f / qd;
            } else {
                qe = dcvc_sigmoidf(ld(qs, p * a.ldq)) * 1.5f + 0.5f;
            }
            const float yq = ld(y, p * a.ldy + ch) * qe;
            const float s = ld(sc, p * a.lds + ch), m = ld(mu, p * a.ldm + ch);
            float v = dcvc_roundf(yq - m);
            const bool use_thres = a.thres >= 0.f;
            if (use_thres && !(s > a.thres)) v = v * 0.f;
            v = clampf(v, -128.f, 127.f);
            const float scl = clampf(s, kScaleMin, kScaleMax);
            const bool keep = !use_thres || (scl > a.thres);
            const int idx = keep ? (int)dcvc_scale_to_index(scl, kScaleMin, kScaleMax, kLogScaleMin, kLogStepRecip) : 0xFF;
            packed = (int16_t)((int)v * 256 + idx);
            return (float)to_t<T>(v + m);
        });
        sp[cc * PT + pl] = packed;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < PT * Cg; it += EB) {
        const int cc = it / PT, pl = it - cc * PT;
        const int64_t p = p0 + pl;
        if (p < HW) a.packed[(int64_t)cc * HW + p] = sp[cc * PT + pl];
    }
}

template <typename T>
__global__ __launch_bounds__(EB) void prior_dec_index_kernel(int n_groups, int step, const T* sc, int64_t lds, int H, int W,
                                                            int C, float thres, uint8_t* idx_chw, uint8_t* cnt16)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint8_t* sp = reinterpret_cast<uint8_t*>(smem);   // [Cg][PT]
    const int Cg = C / n_groups;
    const int64_t HW = (int64_t)H * W;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    for (int it = threadIdx.x; it < PT * Cg; it += EB) {
        const int pl = it / Cg, cc = it - pl * Cg;
        const int64_t p = p0 + pl;
        if (p >= HW) continue;
        const int ch = cc + pixel_group(n_groups, step, p, W) * Cg;
        const float scl = clampf(ld(sc, p * lds + ch), kScaleMin, kScaleMax);
        const bool keep = thres < 0.f || scl > thres;
        sp[cc * PT + pl] = keep ? dcvc_scale_to_index(scl, kScaleMin, kScaleMax, kLogScaleMin, kLogStepRecip) : (uint8_t)0xFF;
    }
    __syncthreads();
    // kept entries of each (channel, 16-pixel run): what dec_compact_kernel scans (the compacted hand-off)
    if (cnt16 != nullptr) {
        for (int cc = threadIdx.x; cc < Cg; cc += EB) {
            int c = 0;
            for (int pl = 0; pl < PT; ++pl) c += (p0 + pl < HW && sp[cc * PT + pl] != 0xFF) ? 1 : 0;
            cnt16[(int64_t)cc * gridDim.x + blockIdx.x] = (uint8_t)c;
        }
    }
    if (wide16(HW, idx_chw)) {
        for (int cc = threadIdx.x; cc < Cg; cc += EB)
            *reinterpret_cast<uint4*>(idx_chw + (int64_t)cc * HW + p0) = *reinterpret_cast<const uint4*>(sp + cc * PT);
        return;
    }
    for (int it = threadIdx.x; it < PT * Cg; it += EB) {
        const int cc = it / PT, pl = it - cc * PT;
        const int64_t p = p0 + pl;
        if (p < HW) idx_chw[(int64_t)cc * HW + p] = sp[cc * PT + pl];
    }
}

template <typename T>
__global__ __launch_bounds__(EB) void prior_dec_restore_kernel(int n_groups, int step, const int8_t* sym_chw, const T* mu,
                                                              int64_t ldm, int H, int W, int C, const T* hin,
                                                              int64_t ldhi, T* hout, int64_t ldho)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int8_t* sp = reinterpret_cast<int8_t*>(smem);   // [Cg][PT]
    const int Cg = C / n_groups;
    const int64_t HW = (int64_t)H * W;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    if (wide16(HW, sym_chw)) {
        for (int cc = threadIdx.x; cc < Cg; cc += EB)
            *reinterpret_cast<uint4*>(sp + cc * PT) = *reinterpret_cast<const uint4*>(sym_chw + (int64_t)cc * HW + p0);
    } else {
        for (int it = threadIdx.x; it < PT * Cg; it += EB) {
            const int cc = it / PT, pl = it - cc * PT;
            const int64_t p = p0 + pl;
            sp[cc * PT + pl] = p < HW ? sym_chw[(int64_t)cc * HW + p] : (int8_t)0;
        }
    }
    __syncthreads();
    for (int it = threadIdx.x; it < PT * Cg; it += EB) {
        const int pl = it / Cg, cc = it - pl * Cg;
        const int64_t p = p0 + pl;
        if (p >= HW) continue;
        step_update(n_groups, step, pixel_group(n_groups, step, p, W), cc, Cg, p, hin, ldhi, hout, ldho,
                    [&](int ch) { return (float)to_t<T>((float)sp[cc * PT + pl] + ld(mu, p * ldm + ch)); });
    }
}

template <typename T>
__global__ void prior_finish_kernel(int q_mode, T* yh, int64_t ldh, const T* qs, int64_t ldq, int64_t HW, int C)
{
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= HW * C) return;
    const int64_t p = (int)i / C;           // (H * W * C < 2^31, checked by the caller: 32-bit division)
    const int c = (int)i - (int)p * C;
    float q;
    if (q_mode == 0) {
        q = ld(qs, p * ldq + c);
        q = q < 0.5f ? 0.5f : q;
    } else {
        q = dcvc_sigmoidf(ld(qs, p * ldq + 1)) * 1.5f + 0.5f;
    }
    st(yh, p * ldh + c, ld(yh, p * ldh + c) * q);
}

// ------------------------------------------------------------------------------------------
// Symbol hand-off of the encoder without a copy command: the kept symbols of each part of `packed` ((sym << 8) | index,
// low byte 0xFF = skipped) are compacted IN ORDER (the order is the bit stream) and written straight into pinned host
// memory, part p at [p * n_per_part, + counts[p]).  Two launches: per-block counts, then prefix + scatter.
// (reference: the boolean-mask compaction out[skip_cond] + .cpu() of cuda_inference.py:159 / entropy_models.py:48, which
// costs a device synchronisation for the size.)
__global__ __launch_bounds__(CB) void compact_count_kernel(const int16_t* packed, int n_per_part, int seg, int* block_counts)
{
    const int part = blockIdx.y, b = blockIdx.x, lo = b * seg, hi = min(lo + seg, n_per_part);
    const int16_t* src = packed + (size_t)part * n_per_part;
    int c = 0;
    for (int i = lo + threadIdx.x; i < hi; i += CB) c += ((src[i] & 0xFF) != 0xFF);
    __shared__ int red[CB / 64];
    c = group_sum(c, red);
    if (threadIdx.x == 0) block_counts[part * gridDim.x + b] = c;
}

__global__ __launch_bounds__(CB) void compact_scatter_kernel(const int16_t* packed, int n_per_part, int seg, const int* block_counts,
                                                             int16_t* out, int* counts)
{
    const int part = blockIdx.y, b = blockIdx.x, nb = gridDim.x, lo = b * seg, hi = min(lo + seg, n_per_part);
    const int16_t* src = packed + (size_t)part * n_per_part;
    int16_t* dst = out + (size_t)part * n_per_part;
    __shared__ int red[CB / 64];
    // symbols kept by the blocks in front of this one
    int pre = 0;
    for (int i = threadIdx.x; i < b; i += CB) pre += block_counts[part * nb + i];
    int base = group_sum(pre, red);
    if (threadIdx.x == 0 && b == nb - 1) counts[part] = base + block_counts[part * nb + b];
    // the segment in rounds of CB consecutive symbols: ballot-based ranks keep the order
    __shared__ int wsum[CB / 64];
    for (int i0 = lo; i0 < hi; i0 += CB) {
        const int i = i0 + threadIdx.x;
        const int16_t v = i < hi ? src[i] : (int16_t)0xFF;
        const bool keep = (v & 0xFF) != 0xFF;
        const unsigned long long m = __ballot(keep);
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();     // (wsum of the previous round has been read)
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        int off = 0;
        for (int k = 0; k < w; ++k) off += wsum[k];
        if (keep) dst[base + off + rank] = v;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

// ------------------------------------------------------------------------------------------
// Decoder hand-off with the kept entries compacted on the device (round 4).  The index array of a checkerboard step is
// ~96 % sentinels at the benchmarked rates: instead of copying all of it to the host (1 MB per step at 1080p, a copy
// command) and all decoded symbols back, the kept table indexes are written IN STREAM ORDER (CHW order, the order of the
// reference's boolean-mask compaction, entropy_models.py:330-341) into pinned host memory by a kernel, the host decodes
// exactly that many symbols, and the restore step fetches them back with coalesced 16-byte reads and finds each position's
// symbol by its rank.  Unit of the scan: one (channel, 16-pixel run) = 16 consecutive CHW positions; prior_dec_index_kernel
// counts the kept entries of every run (cnt16), dec_compact_kernel turns them into offsets (off16) and writes the entries.
__global__ __launch_bounds__(CB) void dec_compact_kernel(const uint8_t* idx_chw, const uint8_t* cnt16, int n16, int nblk, int64_t HW,
                                                         uint8_t* out_host, int32_t* count_host, uint32_t* off16, int32_t* total_dev)
{
    const int b = blockIdx.x, nb = gridDim.x;
    const int per = (n16 + nb - 1) / nb;
    const int lo = min(b * per, n16), hi = min(lo + per, n16);
    __shared__ int red[CB / 64];
    __shared__ int wsum[CB / 64];
    __shared__ __attribute__((aligned(16))) uint8_t stage[CB * PT];
    // entries kept by the runs in front of this block's (cnt16 is 4-byte aligned: whole words, then the tail)
    int pre = 0;
    const uint32_t* cw = reinterpret_cast<const uint32_t*>(cnt16);
    const int nw = lo >> 2;
    for (int i = threadIdx.x; i < nw; i += CB) {
        const uint32_t v = cw[i];
        pre += (int)((v & 0xFF) + ((v >> 8) & 0xFF) + ((v >> 16) & 0xFF) + (v >> 24));
    }
    if (threadIdx.x < (lo & 3)) pre += cnt16[(nw << 2) + threadIdx.x];
    int base = group_sum(pre, red);
    const bool wide = wide16(HW, idx_chw);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int r0 = lo; r0 < hi; r0 += CB) {
        const int r = r0 + threadIdx.x;
        const bool live = r < hi;
        const int c = live ? cnt16[r] : 0;
        // exclusive scan of c over the block: inside the wave by shuffles, across the four waves through LDS
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        __syncthreads();          // (stage / wsum of the previous round have been read)
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int off = inc - c;
        for (int k = 0; k < w; ++k) off += wsum[k];
        const int round_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (live) {
            off16[r] = (uint32_t)(base + off);
            if (c) {
                const int cc = r / nblk, blk = r - cc * nblk;
                const int64_t p0 = (int64_t)blk * PT;
                __attribute__((aligned(16))) uint8_t v[PT];
                load_run16(idx_chw + (int64_t)cc * HW + p0, p0, HW, wide, v);
                int o = off;
#pragma unroll
                for (int j = 0; j < PT; ++j)
                    if (v[j] != 0xFF) stage[o++] = v[j];
            }
        }
        __syncthreads();
        // consecutive lanes write consecutive bytes of the pinned buffer: whole lines over the host link
        for (int j = threadIdx.x; j < round_total; j += CB) out_host[base + j] = stage[j];
        base += round_total;
    }
    if (b == nb - 1 && threadIdx.x == 0) {
        *count_host = base;
        *total_dev = base;
    }
}

// the decoded symbols of the step (compacted, `*total` of them, written by the host coder into pinned memory) -> device
__global__ void dec_gather_kernel(const uint4* src_host, uint4* dst, const int32_t* total_dev, int cap16)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n16 = (*total_dev + 15) >> 4;
    if (i < n16 && i < cap16) dst[i] = src_host[i];
}

// prior_dec_restore_kernel on compacted symbols: the symbol of a kept position is csym[off16[run] + rank inside the run]
template <typename T>
__global__ __launch_bounds__(EB) void prior_dec_restore_compact_kernel(int n_groups, int step, const int8_t* csym,
                                                                      const uint8_t* idx_chw, const uint32_t* off16,
                                                                      const T* mu, int64_t ldm, int H, int W, int C,
                                                                      const T* hin, int64_t ldhi, T* hout, int64_t ldho)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* bs = reinterpret_cast<uint32_t*>(smem);            // [Cg] offset of the run's first kept entry
    uint32_t* mk = bs + C / n_groups;                            // [Cg] kept mask of the run's 16 positions
    const int Cg = C / n_groups;
    const int64_t HW = (int64_t)H * W;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    const bool wide = wide16(HW, idx_chw);
    for (int cc = threadIdx.x; cc < Cg; cc += EB) {
        __attribute__((aligned(16))) uint8_t v[PT];
        load_run16(idx_chw + (int64_t)cc * HW + p0, p0, HW, wide, v);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < PT; ++j) m |= (uint32_t)(v[j] != 0xFF) << j;
        mk[cc] = m;
        bs[cc] = off16[(int64_t)cc * gridDim.x + blockIdx.x];
    }
    __syncthreads();
    for (int it = threadIdx.x; it < PT * Cg; it += EB) {
        const int pl = it / Cg, cc = it - pl * Cg;
        const int64_t p = p0 + pl;
        if (p >= HW) continue;
        const uint32_t m = mk[cc];
        const float sym = (m >> pl) & 1u ? (float)csym[bs[cc] + __popc(m & ((1u << pl) - 1u))] : 0.f;
        step_update(n_groups, step, pixel_group(n_groups, step, p, W), cc, Cg, p, hin, ldhi, hout, ldho,
                    [&](int ch) { return (float)to_t<T>(sym + ld(mu, p * ldm + ch)); });
    }
}

// ------------------------------------------------------------------ host: one check per kind of argument
// None of these touches a device: an entry runs all of its checks before its first HIP call, so a refused call is E_ARG
// on any machine.

// the step of entry `who`: storage type, group count, step and map size
int check_step(const char* who, int dtype, int n_groups, int step, int H, int W, int C)
{
    DCVC_REQUIRE(dtype == DCVC_F16 || dtype == DCVC_F32, "%s: bad dtype %d", who, dtype);
    DCVC_REQUIRE((n_groups == 2 || n_groups == 4) && step >= 0 && step < n_groups && C > 0 && C % n_groups == 0 && H > 0 &&
                     W > 0 && (int64_t)H * W < (1ll << 31),
                 "%s: bad step %d of %d groups on a %d x %d map of %d channels", who, step, n_groups, H, W, C);
    return 0;
}

// the HWC operand `what` of entry `who`: `channels` channels per pixel, `ld` elements from pixel to pixel
int check_map(const char* who, const char* what, const void* p, int64_t ld, int channels)
{
    DCVC_REQUIRE(p, "%s: %s is a null pointer", who, what);
    DCVC_REQUIRE(ld >= channels, "%s: leading dimension %lld of %s is below its %d channels", who, (long long)ld, what, channels);
    return 0;
}

// y_hat of a step: step 0 starts from nothing and looks at neither yhat_in nor its ld
int check_yhat(const char* who, int step, const void* yhat_in, int64_t ldhi, const void* yhat_out, int64_t ldho, int C)
{
    DCVC_REQUIRE(step == 0 || yhat_in, "%s: yhat_in required after step 0", who);
    if (step > 0)
        if (int rc = check_map(who, "yhat_in", yhat_in, ldhi, C)) return rc;
    return check_map(who, "yhat_out", yhat_out, ldho, C);
}

// the dynamic LDS of a prior kernel (its staging of the C / n_groups collapsed channels of a block)
int check_lds(const char* who, size_t bytes)
{
    DCVC_REQUIRE(bytes <= 64 * 1024, "%s: the channels of a group need %zu bytes of LDS, above 64 KiB", who, bytes);
    return 0;
}

// *out = the device's address of p: p itself, or the mapping of pinned host memory (dcvc_host_alloc)
template <typename P>
int dev_ptr(P* p, bool pinned, P** out)
{
    *out = p;
    if (pinned) DCVC_HIP(hipHostGetDevicePointer((void**)out, (void*)p, 0));
    return 0;
}

int grid_of(int H, int W) { return (int)(((int64_t)H * W + PT - 1) / PT); }

// workspace of the compacted decoder hand-off (device): [total: 16 bytes][off16: n16 x 4 -> 16][cnt16: n16 -> 16][csym: n -> 16]
// (every part starts on a 16-byte boundary: dec_gather_kernel writes csym with 16-byte stores for any C / n_groups)
struct DecWs {
    int64_t n16, n, off_off16, off_cnt16, off_csym, bytes;
    int nblk;
};
DecWs dec_ws(int H, int W, int C, int n_groups)
{
    DecWs w{};
    w.nblk = grid_of(H, W);
    w.n16 = (int64_t)(C / n_groups) * w.nblk;
    w.n = (int64_t)(C / n_groups) * H * W;
    w.off_off16 = 16;
    w.off_cnt16 = w.off_off16 + (w.n16 * 4 + 15) / 16 * 16;
    w.off_csym = w.off_cnt16 + (w.n16 + 15) / 16 * 16;
    w.bytes = w.off_csym + (w.n + 15) / 16 * 16;
    return w;
}

// pinned: idx_out / count_out are dcvc_host_alloc buffers (the public form); else device memory (the _dev form)
int prior_dec_index_compact(const char* who, int dtype, int n_groups, int step, const void* scales, int64_t lds_, int H, int W,
                            int C, float thres, uint8_t* idx_chw, void* workspace, uint8_t* idx_out, int32_t* count_out,
                            void* stream, bool pinned)
{
    if (int rc = check_step(who, dtype, n_groups, step, H, W, C)) return rc;
    if (int rc = check_map(who, "scales", scales, lds_, C)) return rc;
    DCVC_REQUIRE(idx_chw && workspace && idx_out && count_out, "%s: null pointer", who);
    DCVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const size_t lds = (size_t)(C / n_groups) * PT;
    if (int rc = check_lds(who, lds)) return rc;
    const DecWs w = dec_ws(H, W, C, n_groups);
    DCVC_REQUIRE(w.n < (1ll << 31), "%s: too many symbols", who);
    char* ws = (char*)workspace;
    uint8_t* cnt16 = (uint8_t*)(ws + w.off_cnt16);
    if (int rc = dev_ptr(idx_out, pinned, &idx_out)) return rc;
    if (int rc = dev_ptr(count_out, pinned, &count_out)) return rc;
    int rc = typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        prior_dec_index_kernel<T><<<w.nblk, EB, lds, (hipStream_t)stream>>>(n_groups,
                                    step, (const T*)scales, lds_, H, W, C, thres, idx_chw, cnt16);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(dec_compact_kernel, dim3(DCVC_COMPACT_BLOCKS), dim3(CB), 0, (hipStream_t)stream, idx_chw, cnt16, (int)w.n16,
                       w.nblk, (int64_t)H * W, idx_out, count_out, (uint32_t*)(ws + w.off_off16), (int32_t*)ws);
    DCVC_LAUNCH_CHECK();
    return 0;
}

// pinned: `sym` is a dcvc_host_alloc buffer the host coder filled (the public form: the symbols are fetched into the workspace
// first); else they are in device memory already (the _dev form, written by dcvc_rans_dev_decode_y: no gather)
int prior_dec_restore_compact(const char* who, int dtype, int n_groups, int step, const int8_t* sym, const uint8_t* idx_chw,
                              void* workspace, const void* means, int64_t ldm, int H, int W, int C, const void* yhat_in,
                              int64_t ldhi, void* yhat_out, int64_t ldho, void* stream, bool pinned)
{
    if (int rc = check_step(who, dtype, n_groups, step, H, W, C)) return rc;
    if (int rc = check_map(who, "means", means, ldm, C)) return rc;
    if (int rc = check_yhat(who, step, yhat_in, ldhi, yhat_out, ldho, C)) return rc;
    DCVC_REQUIRE(sym && idx_chw && workspace, "%s: null pointer", who);
    DCVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const size_t lds = (size_t)(C / n_groups) * 8;
    if (int rc = check_lds(who, lds)) return rc;
    const DecWs w = dec_ws(H, W, C, n_groups);
    char* ws = (char*)workspace;
    const int8_t* csym = sym;
    if (pinned) {
        if (int rc = dev_ptr(sym, pinned, &sym)) return rc;
        // (the one check that needs the device's address)
        DCVC_REQUIRE((reinterpret_cast<uintptr_t>(sym) & 15) == 0, "%s: symbol buffer must be 16-byte aligned", who);
        const int cap16 = (int)((w.n + 15) / 16);
        hipLaunchKernelGGL(dec_gather_kernel, dim3((cap16 + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const uint4*)sym,
                           (uint4*)(ws + w.off_csym), (const int32_t*)ws, cap16);
        DCVC_LAUNCH_CHECK();
        csym = (const int8_t*)(ws + w.off_csym);
    }
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        prior_dec_restore_compact_kernel<T><<<w.nblk, EB, lds, (hipStream_t)stream>>>(n_groups, step,
                                    csym, idx_chw, (const uint32_t*)(ws + w.off_off16),
                                    (const T*)means, ldm, H, W, C, (const T*)yhat_in, ldhi, (T*)yhat_out, ldho);
    });
}

int compact_symbols(const char* who, const int16_t* packed, int n_per_part, int n_parts, int16_t* out, int32_t* counts,
                    int32_t* workspace, void* stream, bool pinned)
{
    DCVC_REQUIRE(packed && out && counts && workspace, "%s: null pointer", who);
    DCVC_REQUIRE(n_per_part > 0 && n_parts > 0 && n_parts <= 8, "%s: bad sizes %d x %d", who, n_parts, n_per_part);
    const int nb = DCVC_COMPACT_BLOCKS, seg = (n_per_part + nb - 1) / nb;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dev_ptr(out, pinned, &out)) return rc;
    if (int rc = dev_ptr(counts, pinned, &counts)) return rc;
    hipLaunchKernelGGL(compact_count_kernel, dim3(nb, n_parts), dim3(CB), 0, st, packed, n_per_part, seg, workspace);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(nb, n_parts), dim3(CB), 0, st, packed, n_per_part, seg, workspace, out, counts);
    DCVC_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int dcvc_prior_enc_step(int dtype, int n_groups, int step, int q_mode, const void* y, int64_t ldy, const void* qsrc,
                        int64_t ldq, const void* scales, int64_t lds_, const void* means, int64_t ldm, int H, int W, int C,
                        float thres, const void* yhat_in, int64_t ldhi, void* yhat_out, int64_t ldho, int16_t* packed_chw,
                        void* stream)
{
    const char* who = "dcvc_prior_enc_step";
    if (int rc = check_step(who, dtype, n_groups, step, H, W, C)) return rc;
    if (int rc = check_map(who, "y", y, ldy, C)) return rc;
    if (int rc = check_map(who, "qsrc", qsrc, ldq, q_mode == 0 ? C : 2)) return rc;   // (intra: the two raw q of params)
    if (int rc = check_map(who, "scales", scales, lds_, C)) return rc;
    if (int rc = check_map(who, "means", means, ldm, C)) return rc;
    if (int rc = check_yhat(who, step, yhat_in, ldhi, yhat_out, ldho, C)) return rc;
    DCVC_REQUIRE(packed_chw, "%s: packed_chw is a null pointer", who);
    const size_t lds = (size_t)(C / n_groups) * PT * sizeof(int16_t);
    if (int rc = check_lds(who, lds)) return rc;
    PriorEncArgs a{n_groups, step, q_mode, y, ldy, qsrc, ldq, scales, lds_, means, ldm, H, W, C, thres,
                   yhat_in, ldhi, yhat_out, ldho, packed_chw};
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        prior_enc_kernel<T><<<grid_of(H, W), EB, lds, (hipStream_t)stream>>>(a);
    });
}

int dcvc_prior_dec_index(int dtype, int n_groups, int step, const void* scales, int64_t lds_, int H, int W, int C,
                         float thres, uint8_t* idx_chw, void* stream)
{
    const char* who = "dcvc_prior_dec_index";
    if (int rc = check_step(who, dtype, n_groups, step, H, W, C)) return rc;
    if (int rc = check_map(who, "scales", scales, lds_, C)) return rc;
    DCVC_REQUIRE(idx_chw, "%s: idx_chw is a null pointer", who);
    const size_t lds = (size_t)(C / n_groups) * PT;
    if (int rc = check_lds(who, lds)) return rc;
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        prior_dec_index_kernel<T><<<grid_of(H, W), EB, lds, (hipStream_t)stream>>>(n_groups,
                                    step, (const T*)scales, lds_, H, W, C, thres, idx_chw, (uint8_t*)nullptr);
    });
}

int dcvc_prior_dec_restore(int dtype, int n_groups, int step, const int8_t* sym_chw, const void* means, int64_t ldm, int H,
                           int W, int C, const void* yhat_in, int64_t ldhi, void* yhat_out, int64_t ldho, void* stream)
{
    const char* who = "dcvc_prior_dec_restore";
    if (int rc = check_step(who, dtype, n_groups, step, H, W, C)) return rc;
    if (int rc = check_map(who, "means", means, ldm, C)) return rc;
    if (int rc = check_yhat(who, step, yhat_in, ldhi, yhat_out, ldho, C)) return rc;
    DCVC_REQUIRE(sym_chw, "%s: sym_chw is a null pointer", who);
    const size_t lds = (size_t)(C / n_groups) * PT;
    if (int rc = check_lds(who, lds)) return rc;
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        prior_dec_restore_kernel<T><<<grid_of(H, W), EB, lds, (hipStream_t)stream>>>(n_groups,
                                    step, sym_chw, (const T*)means, ldm, H, W, C, (const T*)yhat_in, ldhi, (T*)yhat_out,
                                    ldho);
    });
}

int64_t dcvc_prior_dec_compact_ws_bytes(int H, int W, int C, int n_groups)
{
    if (H <= 0 || W <= 0 || C <= 0 || (n_groups != 2 && n_groups != 4) || C % n_groups) return 0;
    return dec_ws(H, W, C, n_groups).bytes;
}

int dcvc_prior_dec_index_compact(int dtype, int n_groups, int step, const void* scales, int64_t lds_, int H, int W, int C,
                                 float thres, uint8_t* idx_chw, void* workspace, uint8_t* idx_host, int32_t* count_host,
                                 void* stream)
{
    return prior_dec_index_compact("dcvc_prior_dec_index_compact", dtype, n_groups, step, scales, lds_, H, W, C, thres, idx_chw,
                                   workspace, idx_host, count_host, stream, true);
}

int dcvc_prior_dec_index_compact_dev(int dtype, int n_groups, int step, const void* scales, int64_t lds_, int H, int W, int C,
                                     float thres, uint8_t* idx_chw, void* workspace, uint8_t* idx_dev, int32_t* count_dev,
                                     void* stream)
{
    return prior_dec_index_compact("dcvc_prior_dec_index_compact_dev", dtype, n_groups, step, scales, lds_, H, W, C, thres,
                                   idx_chw, workspace, idx_dev, count_dev, stream, false);
}

int dcvc_prior_dec_restore_compact(int dtype, int n_groups, int step, const int8_t* sym_host, const uint8_t* idx_chw,
                                   void* workspace, const void* means, int64_t ldm, int H, int W, int C,
                                   const void* yhat_in, int64_t ldhi, void* yhat_out, int64_t ldho, void* stream)
{
    return prior_dec_restore_compact("dcvc_prior_dec_restore_compact", dtype, n_groups, step, sym_host, idx_chw, workspace, means,
                                     ldm, H, W, C, yhat_in, ldhi, yhat_out, ldho, stream, true);
}

int dcvc_prior_dec_restore_compact_dev(int dtype, int n_groups, int step, const int8_t* sym_dev, const uint8_t* idx_chw,
                                       void* workspace, const void* means, int64_t ldm, int H, int W, int C,
                                       const void* yhat_in, int64_t ldhi, void* yhat_out, int64_t ldho, void* stream)
{
    return prior_dec_restore_compact("dcvc_prior_dec_restore_compact_dev", dtype, n_groups, step, sym_dev, idx_chw, workspace,
                                     means, ldm, H, W, C, yhat_in, ldhi, yhat_out, ldho, stream, false);
}

int dcvc_prior_finish(int dtype, int q_mode, void* yhat, int64_t ldh, const void* qsrc, int64_t ldq, int H, int W, int C,
                      void* stream)
{
    const char* who = "dcvc_prior_finish";
    DCVC_REQUIRE(dtype == DCVC_F16 || dtype == DCVC_F32, "%s: bad dtype %d", who, dtype);
    DCVC_REQUIRE(H > 0 && W > 0 && C > 0 && (int64_t)H * W * C < (1ll << 31), "%s: bad latent size %d x %d x %d", who, H, W, C);
    if (int rc = check_map(who, "qsrc", qsrc, ldq, q_mode == 0 ? C : 2)) return rc;   // (intra: the two raw q of params)
    if (int rc = check_map(who, "yhat", yhat, ldh, C)) return rc;
    return typed(dtype, [&](auto tag) {
        using T = decltype(tag);
        prior_finish_kernel<T><<<nblocks((int64_t)H * W * C), EB, 0, (hipStream_t)stream>>>(q_mode, (T*)yhat, ldh, (const T*)qsrc, ldq,
                     (int64_t)H * W, C);
    });
}

int dcvc_compact_symbols(const int16_t* packed, int n_per_part, int n_parts, int16_t* out_host, int32_t* counts_host,
                         int32_t* workspace, void* stream)
{
    return compact_symbols("dcvc_compact_symbols", packed, n_per_part, n_parts, out_host, counts_host, workspace, stream, true);
}

int dcvc_compact_symbols_dev(const int16_t* packed, int n_per_part, int n_parts, int16_t* out_dev, int32_t* counts_dev,
                             int32_t* workspace, void* stream)
{
    return compact_symbols("dcvc_compact_symbols_dev", packed, n_per_part, n_parts, out_dev, counts_dev, workspace, stream, false);
}

}  // extern "C"
