// dcvc_rans_dev.hip - device entropy coder of the chunked y units (docs/chunked_stream.md; the format: rans_core.hpp).
//
// A unit is ceil(count / S) independent rANS chunks behind a table of uint16 chunk lengths, so ONE LANE codes ONE CHUNK
// (the lane's body: rans_lane.hpp) and a whole unit is a handful of launches on the caller's stream: no host step, no host
// read of the symbol count (it stays in device memory).  The bytes are those of dcvc_rans_chunked_encode_y, which tests compare.
//
//   encode: enc_chunks_kernel (lane = chunk, bytes downwards into the lane's scratch slot) -> enc_scan_kernel (exclusive
//           scan of the chunk lengths, length table + info into pinned memory) -> enc_gather_kernel (bodies into pinned memory)
//   decode: dec_scan_kernel (validates the length table against the unit size and the count, exclusive scan) ->
//           dec_chunks_kernel (lane = chunk; every byte read is clamped to the chunk, the end state is checked)
//
// The tables (20 KB for the 128 Gaussian ones) are staged into LDS once per workgroup.
#include <algorithm>
#include <new>
#include <vector>

#include "rans_lane.hpp"

namespace {

using namespace rans;

constexpr int WG = 64;                  // lanes (= chunks) per workgroup of the coding kernels
constexpr int SB = 256;                 // threads of the single-block scans
constexpr int kSlotAllowance = 64;      // default slot = 2 * S + this (4 of it: the flush)

// the same tables copied into LDS by the whole workgroup: a Tables whose pointers lead there
__device__ inline Tables stage_tables(const Tables& t, uint32_t* lds)
{
    const int nw = table_words(t.n, t.stride);
    for (int i = threadIdx.x; i < nw; i += blockDim.x) lds[i] = t.sym[i];
    __syncthreads();
    return tables_at(lds, t.n, t.stride);
}


// ws: [lens: nch_max x 4][offs: nch_max x 4][flag / valid: 16 bytes][slots: nch_max x slot]
__global__ __launch_bounds__(WG) void enc_chunks_kernel(Tables t, const int16_t* sym, const int32_t* count_p, int64_t max_symbols,
                                                        int log2_s, int slot, uint32_t* lens, int32_t* flag, uint8_t* slots)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int64_t count = *count_p;
    const bool bad_count = count < 0 || count > max_symbols;
    if (bad_count) count = 0;
    if (bad_count && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(flag, 1);
    const int64_t S = (int64_t)1 << log2_s, nch = chunks(count, log2_s);
    if ((int64_t)blockIdx.x * WG >= nch) return;                     // (whole workgroup: before the barrier below)
    const Tables T = stage_tables(t, reinterpret_cast<uint32_t*>(smem));
    const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (c >= nch) return;
    const int64_t a = c << log2_s, b = min(count, a + S);
    // encode_chunk's blocks of 8 symbols: one 16-byte load; a block not whole, aligned and inside the array: entry by entry
    const bool wide = (reinterpret_cast<uintptr_t>(sym) & 15) == 0;
    auto fetch = [&](int64_t j0) {      // entries [j0, j0 + 8), j0 a multiple of 8
        uint4 v = make_uint4(0, 0, 0, 0);
        if (j0 < a - 7 || j0 >= b) return v;
        if (wide && j0 + 8 <= max_symbols) return *reinterpret_cast<const uint4*>(sym + j0);
        uint32_t w[4] = {0, 0, 0, 0};
        for (int k = 0; k < 8; ++k)
            if (j0 + k >= a && j0 + k < b) w[k >> 1] |= (uint32_t)(uint16_t)sym[j0 + k] << ((k & 1) * 16);
        return make_uint4(w[0], w[1], w[2], w[3]);
    };
    const uint32_t len = encode_chunk(T, fetch, a, b, slots + c * slot, slot);
    lens[c] = len;
    if (!len) atomicOr(flag, 1);
}

// exclusive scan of n 32-bit lengths by one block: thread t owns the entries [t * per, (t + 1) * per); returns the total
template <typename LenOf, typename Put>
__device__ inline unsigned long long block_scan(int64_t n, LenOf len_of, Put put, unsigned long long* sh)
{
    const int64_t per = (n + SB - 1) / SB, lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    unsigned long long s = 0;
    for (int64_t i = lo; i < hi; ++i) s += len_of(i);
    sh[threadIdx.x] = s;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int k = 0; k < SB; ++k) {
        const unsigned long long v = sh[k];
        before += k < (int)threadIdx.x ? v : 0;
        total += v;
    }
    for (int64_t i = lo; i < hi; ++i) {
        put(i, before);
        before += len_of(i);
    }
    return total;
}

__global__ __launch_bounds__(SB) void enc_scan_kernel(const int32_t* count_p, int64_t max_symbols, int log2_s, const uint32_t* lens,
                                                      uint32_t* offs, int32_t* flag, int32_t* info, uint8_t* unit, int64_t capacity)
{
    __shared__ unsigned long long sh[SB];
    int64_t count = *count_p;
    if (count < 0 || count > max_symbols) count = 0;                // (flagged by enc_chunks_kernel)
    const int64_t nch = chunks(count, log2_s);
    const unsigned long long total = block_scan(nch, [&](int64_t i) { return (unsigned long long)lens[i]; },
                                                [&](int64_t i, unsigned long long o) { offs[i] = (uint32_t)o; }, sh);
    const unsigned long long bytes = 2ull * (unsigned long long)nch + total;
    const bool ovf = flag[0] != 0 || bytes > (unsigned long long)capacity;
    if (!ovf)
        for (int64_t i = threadIdx.x; i < nch; i += SB) put_chunk_len(unit, i, lens[i]);
    if (threadIdx.x == 0) {
        info[0] = ovf ? 0 : (int32_t)bytes;
        info[1] = ovf ? 1 : 0;
        info[2] = (int32_t)count;
        info[3] = (int32_t)nch;
        flag[1] = ovf ? 0 : (int32_t)nch;                           // chunks the gather may copy
    }
}

__global__ __launch_bounds__(SB) void enc_gather_kernel(int slot, const uint32_t* lens, const uint32_t* offs, const int32_t* flag,
                                                        const uint8_t* slots, uint8_t* unit)
{
    const int64_t nch = flag[1];
    uint8_t* bodies = unit + 2 * nch;
    for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const uint32_t len = lens[c];
        const uint8_t* src = slots + c * slot + (slot - (int)len);
        uint8_t* dst = bodies + offs[c];
        for (uint32_t j = threadIdx.x; j < len; j += SB) dst[j] = src[j];
    }
}

// ------------------------------------------------------------------------------------------ decoder
// ws: [valid chunks, unit offset, chunks: 16 bytes][offs: nch_max x 4]
__global__ __launch_bounds__(SB) void dec_scan_kernel(const uint8_t* payload, int64_t payload_capacity, const int32_t* desc,
                                                      const int32_t* count_p, int64_t max_symbols, int log2_s, int32_t* head,
                                                      uint32_t* offs, int32_t* err)
{
    __shared__ unsigned long long sh[SB];
    const int64_t uoff = desc[0], ubytes = desc[1], count = *count_p;
    int e = 0;
    if (uoff < 0 || ubytes < 0 || uoff + ubytes > payload_capacity || count < 0 || count > max_symbols) e = DCVC_RANS_DEV_E_RANGE;
    const int64_t nch = e ? 0 : chunks(count, log2_s);
    if (!e && 2 * nch > ubytes) e = DCVC_RANS_DEV_E_COUNT;
    const uint8_t* tab = payload + uoff;                             // (read only when e == 0: 2 * nch bytes lie inside the unit)
    const int64_t n = e ? 0 : nch;
    auto len_of = [&](int64_t i) { return (unsigned long long)chunk_len(tab, i); };
    const unsigned long long total = block_scan(n, len_of, [&](int64_t i, unsigned long long o) { offs[i] = (uint32_t)o; }, sh);
    if (!e && 2ull * (unsigned long long)nch + total != (unsigned long long)ubytes) e = DCVC_RANS_DEV_E_TABLE;
    // (with the sum equal to the unit's size every offs[i] + len_i lies inside the unit: what dec_chunks_kernel relies on)
    if (threadIdx.x == 0) {
        head[0] = e ? 0 : (int32_t)nch;
        if (e) atomicOr(err, e);
    }
}

constexpr int kIoBytes = 16384;         // LDS: the workgroup's table indexes, replaced in place by the decoded symbols
constexpr int kPayBytes = 24576;        // LDS: the workgroup's chunk bodies
__host__ __device__ inline int dec_lanes(int log2_s) { return (kIoBytes >> log2_s) < WG ? (kIoBytes >> log2_s) : WG; }

// One lane decodes one chunk; a workgroup takes dec_lanes(log2 S) consecutive chunks (64 at S = 256, 4 at S = 4096) so that
// their indexes fit kIoBytes.  Everything a lane touches while it walks its chunk is in LDS: the workgroup first copies the
// indexes and the chunk bodies there with coalesced loads and writes the symbols back the same way afterwards - a lane's own
// global accesses would each wait out a memory latency inside the walk.  The 60 KB of LDS (tables 20, indexes / symbols 16,
// bodies 24) leave room for two such workgroups per CU: two waves per CU is all the occupancy this kernel can have.
__global__ __launch_bounds__(WG) void dec_chunks_kernel(Tables t, const uint8_t* payload, uint32_t payload_capacity,
                                                        const int32_t* desc, const uint8_t* idx, const int32_t* count_p,
                                                        int log2_s, const int32_t* head, const uint32_t* offs, int8_t* out,
                                                        int32_t* err)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t nch = head[0];
    const int lanes = dec_lanes(log2_s);
    const int64_t c0 = (int64_t)blockIdx.x * lanes;
    if (c0 >= nch) return;                                           // (whole workgroup: before any barrier)
    const int64_t c1 = min(nch, c0 + lanes);
    uint32_t* tab_lds = reinterpret_cast<uint32_t*>(smem);
    const int tab_bytes = table_words(t.n, t.stride) * 4;            // (a multiple of 16: dcvc_rans_dev_create)
    uint8_t* io = reinterpret_cast<uint8_t*>(smem + tab_bytes);
    uint32_t* pay = reinterpret_cast<uint32_t*>(smem + tab_bytes + kIoBytes);
    const int64_t count = *count_p;
    const int64_t lo = c0 << log2_s, hi = min(count, c1 << log2_s);
    const int n_io = (int)(hi - lo);                                 // <= kIoBytes
    // ---- stage: indexes (16 bytes per lane where source and count allow), then the bodies of chunks c0 .. c1 - 1
    const bool wide = (reinterpret_cast<uintptr_t>(idx) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int n_vec = wide ? n_io >> 4 : 0;
    for (int j = threadIdx.x; j < n_vec; j += WG)
        reinterpret_cast<uint4*>(io)[j] = reinterpret_cast<const uint4*>(idx + lo)[j];
    for (int j = (n_vec << 4) + threadIdx.x; j < n_io; j += WG) io[j] = idx[lo + j];
    const uint32_t uoff = (uint32_t)desc[0];
    const uint8_t* unit = payload + uoff;
    const uint32_t last = (uint32_t)(c1 - 1);
    const uint32_t body0 = uoff + 2 * (uint32_t)nch;
    const uint32_t p_lo = body0 + offs[c0];
    const uint32_t p_hi = body0 + offs[last] + chunk_len(unit, last);
    const uint32_t lo4 = p_lo & ~3u;
    uint32_t hi4 = (p_hi + 3) & ~3u;
    if (hi4 > (payload_capacity & ~3u)) hi4 = payload_capacity & ~3u;      // (whole words inside the buffer only)
    if (hi4 - lo4 > (uint32_t)kPayBytes) hi4 = lo4 + kPayBytes;
    if (hi4 < lo4) hi4 = lo4;
    for (uint32_t j = threadIdx.x; j < (hi4 - lo4) >> 2; j += WG) pay[j] = *reinterpret_cast<const uint32_t*>(payload + lo4 + 4 * j);
    const Tables T = stage_tables(t, tab_lds);                    // (ends with the barrier that also covers io / pay)
    // ---- walk
    const int64_t c = c0 + threadIdx.x;
    if ((int)threadIdx.x < lanes && c < c1) {
        const int a = (int)threadIdx.x << log2_s, b = min(n_io, a + (1 << log2_s));      // positions inside io
        Reader r;
        r.base = payload, r.staged = pay, r.lo4 = lo4, r.hi4 = hi4, r.cap = payload_capacity;
        r.open(body0 + offs[c], chunk_len(unit, c));
        uint32_t x = get_state(r);
        int e = 0;
        int ti_next = a < b ? io[a] : 0;
        for (int i = a; i < b; ++i) {
            int ti = ti_next;
            ti_next = i + 1 < b ? io[i + 1] : 0;
            if (ti >= T.n) {
                e |= DCVC_RANS_DEV_E_RANGE;
                ti = 0;
            }
            const uint32_t m = T.meta[ti];
            const uint32_t max_value = m & kMask;
            const int32_t offset = (int16_t)(m >> 16);
            const uint32_t* row = T.sym + ti * T.stride;
            const uint32_t cum = x & kMask;
            const uint32_t g = cum >> (kScaleBits - kLaneLutBits);
            uint32_t s = (T.lut[ti * (kLaneLut / 4) + (g >> 2)] >> ((g & 3) * 8)) & 0xff;
            uint32_t ent = T.lute[ti * kLaneLut + g];
            uint32_t d = cum - entry_start(ent);
            while (d >= entry_freq(ent) && s < max_value) {       // (s stays inside the row whatever the tables hold)
                ent = row[++s];
                d = cum - entry_start(ent);
            }
            x = entry_freq(ent) * (x >> kScaleBits) + d;
            renorm_after_symbol(x, r);
            int32_t value = (int32_t)s;
            if (s == max_value) {       // rans_core.hpp's decode_escape in place: through the call this kernel takes 77 SGPRs for 75
                uint32_t val = get_bits(x, r);
                uint32_t n = val;
                while (val == kBypassMax && !r.overrun) {
                    val = get_bits(x, r);
                    n = n < 1024u ? n + val : n;
                }
                uint32_t raw = 0;
                for (uint32_t j = 0; j < n && j < 16; ++j) raw |= get_bits(x, r) << (j * kBypassBits);
                value = escape_value(raw, (int32_t)max_value);
            }
            io[i] = (uint8_t)(value + offset);                // in place: index i has been read
        }
        if (r.overrun || r.pos != r.end || x != kRansL) e |= DCVC_RANS_DEV_E_CHUNK;
        if (e) atomicOr(err, e);
    }
    __syncthreads();
    // ---- the symbols of positions [lo, hi), nothing past the count
    for (int j = threadIdx.x; j < n_vec; j += WG) reinterpret_cast<uint4*>(out + lo)[j] = reinterpret_cast<const uint4*>(io)[j];
    for (int j = (n_vec << 4) + threadIdx.x; j < n_io; j += WG) out[lo + j] = (int8_t)io[j];
}

int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }
int slot_of(int log2_s, int slot_bytes) { return slot_bytes > 0 ? slot_bytes : 2 * (1 << log2_s) + kSlotAllowance; }
bool slot_ok(int slot_bytes) { return slot_bytes >= 0 && slot_bytes <= 0xfffc && slot_bytes % 4 == 0; }

}  // namespace

struct dcvc_rans_dev {
    uint32_t* dev = nullptr;            // sym | meta | lut | lute in one allocation
    Tables t{};
    size_t lds = 0;
};

extern "C" {

int dcvc_rans_dev_create(const int32_t* cdf, int n, int stride, const int32_t* sizes, const int32_t* offsets, dcvc_rans_dev** out)
{
    const char* who = "dcvc_rans_dev_create";
    DCVC_REQUIRE(out && n <= 255, "%s: bad table group (n=%d stride=%d)", who, n, stride);
    std::vector<uint32_t> h;
    if (!build_tables(who, cdf, n, stride, sizes, offsets, h)) return dcvc::E_ARG;
    // (the decoder keeps the tables, 16 KB of indexes / symbols and 24 KB of chunk bodies in 64 KB of LDS)
    DCVC_REQUIRE(h.size() * 4 + kIoBytes + kPayBytes <= 65536 && h.size() % 4 == 0,
                 "%s: tables of %zu bytes do not fit the decoder's LDS budget (n a multiple of 4, n * (stride + 21) <= 6144)", who,
                 h.size() * 4);
    dcvc_rans_dev* d = new (std::nothrow) dcvc_rans_dev();
    DCVC_REQUIRE(d, "dcvc_rans_dev_create: out of memory");
    const size_t bytes = h.size() * 4;
    hipError_t rc = hipMalloc((void**)&d->dev, bytes);
    if (rc == hipSuccess) rc = hipMemcpy(d->dev, h.data(), bytes, hipMemcpyHostToDevice);
    if (rc != hipSuccess) {
        dcvc::set_error("dcvc_rans_dev_create: %s", hipGetErrorString(rc));
        if (d->dev) (void)hipFree(d->dev);
        delete d;
        return dcvc::E_HIP;
    }
    d->t = tables_at(d->dev, n, stride);
    d->lds = bytes;
    *out = d;
    return 0;
}

void dcvc_rans_dev_destroy(dcvc_rans_dev* d)
{
    if (!d) return;
    (void)hipFree(d->dev);
    delete d;
}

int64_t dcvc_rans_dev_enc_ws_bytes(int64_t max_symbols, int log2_s, int slot_bytes)
{
    if (max_symbols < 0 || !chunked_args_ok(log2_s) || !slot_ok(slot_bytes)) return 0;
    const int64_t nch = chunks(max_symbols, log2_s);
    return 2 * up16(nch * 4) + 16 + up16(nch * slot_of(log2_s, slot_bytes));
}

int dcvc_rans_dev_encode_y(const dcvc_rans_dev* d, const int16_t* sym_dev, const int32_t* count_dev, int64_t max_symbols,
                           int log2_s, int slot_bytes, void* workspace, uint8_t* unit_host, int64_t unit_capacity, void* stream)
{
    DCVC_REQUIRE(d && sym_dev && count_dev && workspace && unit_host, "dcvc_rans_dev_encode_y: null pointer");
    DCVC_REQUIRE(chunked_args_ok(log2_s), "dcvc_rans_dev_encode_y: log2 of the chunk size is %d (8 .. 12)", log2_s);
    // a slot of at most 65535 bytes is also what keeps every chunk length inside its uint16 field
    DCVC_REQUIRE(slot_ok(slot_bytes), "dcvc_rans_dev_encode_y: slot of %d bytes (a multiple of 4, 0 .. 65532)", slot_bytes);
    DCVC_REQUIRE(max_symbols >= 0 && max_symbols < (1ll << 31) && unit_capacity >= 0 && unit_capacity < (1ll << 31),
                 "dcvc_rans_dev_encode_y: bad sizes");
    DCVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "dcvc_rans_dev_encode_y: workspace must be 16-byte aligned");
    const int64_t nch = chunks(max_symbols, log2_s);
    const int slot = slot_of(log2_s, slot_bytes);
    char* ws = (char*)workspace;
    uint32_t* lens = (uint32_t*)ws;
    uint32_t* offs = (uint32_t*)(ws + up16(nch * 4));
    int32_t* flag = (int32_t*)(ws + 2 * up16(nch * 4));
    uint8_t* slots = (uint8_t*)(ws + 2 * up16(nch * 4) + 16);
    uint8_t* out_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&out_dev, unit_host, 0));
    hipStream_t st = (hipStream_t)stream;
    DCVC_HIP(hipMemsetAsync(flag, 0, 16, st));
    const int64_t blocks = (nch + WG - 1) / WG;
    if (blocks > 0)
        hipLaunchKernelGGL(enc_chunks_kernel, dim3((unsigned)blocks), dim3(WG), d->lds, st, d->t, sym_dev, count_dev, max_symbols,
                           log2_s, slot, lens, flag, slots);
    hipLaunchKernelGGL(enc_scan_kernel, dim3(1), dim3(SB), 0, st, count_dev, max_symbols, log2_s, lens, offs, flag,
                       (int32_t*)out_dev, out_dev + 16, unit_capacity);
    if (blocks > 0)
        hipLaunchKernelGGL(enc_gather_kernel, dim3((unsigned)std::min<int64_t>(nch, 256)), dim3(SB), 0, st, slot, lens, offs, flag,
                           slots, out_dev + 16);
    DCVC_LAUNCH_CHECK();
    return 0;
}

int64_t dcvc_rans_dev_dec_ws_bytes(int64_t max_symbols, int log2_s)
{
    if (max_symbols < 0 || !chunked_args_ok(log2_s)) return 0;
    return 16 + up16(chunks(max_symbols, log2_s) * 4);
}

int dcvc_rans_dev_decode_y(const dcvc_rans_dev* d, const uint8_t* payload_dev, int64_t payload_capacity,
                           const int32_t* unit_desc_dev, const uint8_t* idx_dev, const int32_t* count_dev, int64_t max_symbols,
                           int log2_s, void* workspace, int8_t* sym_dev, int32_t* error_host, void* stream)
{
    DCVC_REQUIRE(d && payload_dev && unit_desc_dev && idx_dev && count_dev && workspace && sym_dev && error_host,
                 "dcvc_rans_dev_decode_y: null pointer");
    DCVC_REQUIRE(chunked_args_ok(log2_s), "dcvc_rans_dev_decode_y: log2 of the chunk size is %d (8 .. 12)", log2_s);
    DCVC_REQUIRE(max_symbols >= 0 && max_symbols < (1ll << 31) && payload_capacity >= 0 && payload_capacity < (1ll << 31),
                 "dcvc_rans_dev_decode_y: bad sizes");
    DCVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "dcvc_rans_dev_decode_y: workspace must be 16-byte aligned");
    DCVC_REQUIRE((reinterpret_cast<uintptr_t>(payload_dev) & 3) == 0, "dcvc_rans_dev_decode_y: payload must be 4-byte aligned");
    int32_t* err_dev = nullptr;
    DCVC_HIP(hipHostGetDevicePointer((void**)&err_dev, error_host, 0));
    int32_t* head = (int32_t*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + 16);
    hipStream_t st = (hipStream_t)stream;
    const int lanes = dec_lanes(log2_s);
    const int64_t blocks = (chunks(max_symbols, log2_s) + lanes - 1) / lanes;
    hipLaunchKernelGGL(dec_scan_kernel, dim3(1), dim3(SB), 0, st, payload_dev, payload_capacity, unit_desc_dev, count_dev,
                       max_symbols, log2_s, head, offs, err_dev);
    if (blocks > 0)
        hipLaunchKernelGGL(dec_chunks_kernel, dim3((unsigned)blocks), dim3(WG), d->lds + kIoBytes + kPayBytes, st, d->t, payload_dev,
                           (uint32_t)payload_capacity, unit_desc_dev, idx_dev, count_dev, log2_s, head, offs, sym_dev, err_dev);
    DCVC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
