// dcvc_rans_dev.hip - device entropy coder of the chunked y units (docs/chunked_stream.md).
//
// A unit is ceil(count / S) independent rANS chunks (rans_host.cpp: 32-bit state from 1 << 23, byte renormalisation, 16-bit
// probabilities, escape + bypass bits, symbols pushed in reverse, 4-byte flush) behind a table of uint16 chunk lengths, so
// ONE LANE codes ONE CHUNK and a whole unit is a handful of launches on the caller's stream: no host step, no host read of
// the symbol count (it stays in device memory).  The bytes are those of dcvc_rans_chunked_encode_y, which tests compare.
//
//   encode: enc_chunks_kernel (lane = chunk, bytes downwards into the lane's scratch slot) -> enc_scan_kernel (exclusive
//           scan of the chunk lengths, length table + info into pinned memory) -> enc_gather_kernel (bodies into pinned memory)
//   decode: dec_scan_kernel (validates the length table against the unit size and the count, exclusive scan) ->
//           dec_chunks_kernel (lane = chunk; every byte read is clamped to the chunk, the end state is checked)
//
// Tables: (start | freq << 16) per (table, value), (max_value | offset << 16) per table and a 16-entry first-guess LUT per
// table (value and entry); 20 KB for the 128 Gaussian tables, staged into LDS once per workgroup.  The encoder
// divides by freq instead of the host's reciprocal multiply: both are exact, ((x / f) << 16) + x % f + start.
#include <algorithm>
#include <new>
#include <vector>

#include "common.hpp"

namespace {

constexpr int kScaleBits = 16;
constexpr uint32_t kRansL = 1u << 23;
constexpr int kBypassBits = 2;
constexpr uint32_t kBypassMax = (1u << kBypassBits) - 1;
constexpr uint32_t kMask = (1u << kScaleBits) - 1;
constexpr int kLutBits = 4;
constexpr int kLut = 1 << kLutBits;
constexpr int WG = 64;                  // lanes (= chunks) per workgroup of the coding kernels
constexpr int SB = 256;                 // threads of the single-block scans
constexpr int kSlotAllowance = 64;      // default slot = 2 * S + this (4 of it: the flush)

struct Tables {                         // pointers (device memory, or its LDS copy) + geometry, passed by value
    const uint32_t* sym;                // [n][stride]
    const uint32_t* meta;               // [n] max_value | (uint16)offset << 16
    const uint32_t* lut;                // [n][kLut / 4] first-guess value per bucket, bytes packed in words
    const uint32_t* lute;               // [n][kLut] the guessed value's entry itself: ONE LDS read on the state chain
    int n, stride;
};

__host__ __device__ inline int lds_words(int n, int stride) { return n * stride + n + n * (kLut / 4) + n * kLut; }

// the same tables copied into LDS by the whole workgroup: a Tables whose pointers lead there
__device__ inline Tables stage_tables(const Tables& t, uint32_t* lds)
{
    // (the four arrays are one allocation in this order: dcvc_rans_dev_create)
    const int ns = t.n * t.stride, nw = lds_words(t.n, t.stride);
    for (int i = threadIdx.x; i < nw; i += blockDim.x) lds[i] = t.sym[i];
    __syncthreads();
    return Tables{lds, lds + ns, lds + ns + t.n, lds + ns + t.n + t.n * (kLut / 4), t.n, t.stride};
}

// ------------------------------------------------------------------------------------------ encoder
// Bytes go downwards into the lane's slot through a 32-bit accumulator, one aligned word store per four bytes: a global
// store per byte would put a memory wait into nearly every symbol's step (the wave's loads and stores retire in order).
struct Emit {
    uint8_t* slot;                      // 4-byte aligned, a multiple of 4 bytes long
    int pos;                            // bytes still free below the write position
    uint32_t acc;
    bool ovf;
    __device__ inline void byte(uint32_t b)
    {
        if (pos == 0) {
            ovf = true;                 // the slot would overflow: flag instead of writing
            return;
        }
        acc = (acc << 8) | (b & 0xff);
        if ((--pos & 3) == 0) *reinterpret_cast<uint32_t*>(slot + pos) = acc;
    }
    __device__ inline void finish()     // the bytes of a last, partial word (its low bytes lie below the chunk: never read)
    {
        if (pos & 3) *reinterpret_cast<uint32_t*>(slot + (pos & ~3)) = acc << (8 * (pos & 3));
    }
};

__device__ inline void put_bits(uint32_t& x, Emit& e, uint32_t val)
{
    constexpr uint32_t x_max = (1u << (kScaleBits - kBypassBits)) << 15;
    while (x >= x_max && !e.ovf) {
        e.byte(x & 0xff);
        x >>= 8;
    }
    x = (x << kBypassBits) | val;
}

__device__ inline void put_symbol(uint32_t& x, Emit& e, uint32_t entry)
{
    const uint32_t start = entry & kMask, freq = entry >> 16;
    const uint32_t x_max = ((kRansL >> kScaleBits) << 8) * freq;
    while (x >= x_max && !e.ovf) {
        e.byte(x & 0xff);
        x >>= 8;
    }
    x = ((x / freq) << kScaleBits) + (x % freq) + start;
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
    const int64_t S = (int64_t)1 << log2_s, nch = (count + S - 1) >> log2_s;
    if ((int64_t)blockIdx.x * WG >= nch) return;                     // (whole workgroup: before the barrier below)
    const Tables T = stage_tables(t, reinterpret_cast<uint32_t*>(smem));
    const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (c >= nch) return;
    const int64_t a = c << log2_s, b = min(count, a + S);
    Emit e{slots + c * slot, slot, 0, false};
    uint32_t x = kRansL;
    // the symbols come in blocks of 8 (one 16-byte load, the next block fetched while this one is coded: the loads stay off
    // the state's dependency chain); a block that is not whole, aligned and inside the array is read entry by entry
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
    int64_t blk = (b - 1) & ~(int64_t)7;
    uint4 cur = fetch(blk), nxt = fetch(blk - 8);
    for (int64_t i = b - 1; i >= a && !e.ovf; --i) {
        if (i < blk) {
            blk -= 8;
            cur = nxt;
            nxt = fetch(blk - 8);
        }
        const int k = (int)(i - blk);
        const uint32_t word = k < 4 ? (k < 2 ? cur.x : cur.y) : (k < 6 ? cur.z : cur.w);
        const int32_t cs = (int16_t)(word >> ((k & 1) * 16));
        int idx = cs & 0xff;
        if (idx >= T.n) {               // not a table of the group: the host fallback reports it
            e.ovf = true;
            break;
        }
        const uint32_t m = T.meta[idx];
        const int32_t max_value = (int32_t)(m & kMask), offset = (int16_t)(m >> 16);
        const int32_t value = (cs >> 8) - offset;
        const uint32_t* row = T.sym + idx * T.stride;
        if ((uint32_t)value < (uint32_t)max_value) {
            put_symbol(x, e, row[value]);
            continue;
        }
        const uint32_t raw = value < 0 ? (uint32_t)(-2 * value - 1) : (uint32_t)(2 * (value - max_value));
        int n_bypass = 0;
        while ((raw >> (n_bypass * kBypassBits)) != 0) ++n_bypass;
        // pushed in reverse of the decoding order: the raw groups from the top, then the unary count from its last digit
        for (int j = n_bypass - 1; j >= 0; --j) put_bits(x, e, (raw >> (j * kBypassBits)) & kBypassMax);
        const int threes = n_bypass / (int)kBypassMax;
        put_bits(x, e, (uint32_t)(n_bypass - threes * (int)kBypassMax));
        for (int j = 0; j < threes; ++j) put_bits(x, e, kBypassMax);
        put_symbol(x, e, row[max_value]);
    }
    if (e.pos < 4) e.ovf = true;
    if (e.ovf) {
        lens[c] = 0;
        atomicOr(flag, 1);
        return;
    }
    e.byte(x >> 24);                    // the 4-byte flush: the state, little endian, below everything else
    e.byte(x >> 16);
    e.byte(x >> 8);
    e.byte(x >> 0);
    e.finish();
    lens[c] = (uint32_t)(slot - e.pos);
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
    const int64_t nch = (count + ((int64_t)1 << log2_s) - 1) >> log2_s;
    const unsigned long long total = block_scan(nch, [&](int64_t i) { return (unsigned long long)lens[i]; },
                                                [&](int64_t i, unsigned long long o) { offs[i] = (uint32_t)o; }, sh);
    const unsigned long long bytes = 2ull * (unsigned long long)nch + total;
    const bool ovf = flag[0] != 0 || bytes > (unsigned long long)capacity;
    if (!ovf)
        for (int64_t i = threadIdx.x; i < nch; i += SB) {
            unit[2 * i] = (uint8_t)(lens[i] & 0xff);
            unit[2 * i + 1] = (uint8_t)(lens[i] >> 8);
        }
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
    const int64_t nch = e ? 0 : (count + ((int64_t)1 << log2_s) - 1) >> log2_s;
    if (!e && 2 * nch > ubytes) e = DCVC_RANS_DEV_E_COUNT;
    const uint8_t* tab = payload + uoff;                             // (read only when e == 0: 2 * nch bytes lie inside the unit)
    const int64_t n = e ? 0 : nch;
    auto len_of = [&](int64_t i) { return (unsigned long long)tab[2 * i] | ((unsigned long long)tab[2 * i + 1] << 8); };
    const unsigned long long total = block_scan(n, len_of, [&](int64_t i, unsigned long long o) { offs[i] = (uint32_t)o; }, sh);
    if (!e && 2ull * (unsigned long long)nch + total != (unsigned long long)ubytes) e = DCVC_RANS_DEV_E_TABLE;
    // (with the sum equal to the unit's size every offs[i] + len_i lies inside the unit: what dec_chunks_kernel relies on)
    if (threadIdx.x == 0) {
        head[0] = e ? 0 : (int32_t)nch;
        if (e) atomicOr(err, e);
    }
}

// The chunk's bytes through a window of two aligned 32-bit words.  A workgroup stages the bodies of its chunks in LDS with
// coalesced loads (dec_chunks_kernel); a word of the staged range comes from there, any other one (a workgroup whose
// bodies outgrow the staging area: escape-heavy chunks) from the payload itself.  Addresses come from the validated chunk
// start and a running counter only - never from payload content - and stay inside the payload buffer; a byte at or past
// the chunk's end is never USED: next() returns 0 there and marks the overrun (a damaged stream reads zeros).
struct Reader {
    const uint8_t* base;                // payload buffer, 4-byte aligned
    const uint32_t* staged;             // LDS copy of the payload words [lo4, hi4)
    uint32_t lo4, hi4;
    uint32_t cap;                       // size of the payload buffer
    uint32_t pos, end;                  // next byte / end of the chunk, offsets into the payload buffer
    uint32_t w0, w1;
    bool over;
    __device__ inline uint32_t word(uint32_t off) const
    {
        if (off >= lo4 && off < hi4) return staged[(off - lo4) >> 2];
        if (off + 4 <= cap) return *reinterpret_cast<const uint32_t*>(base + off);
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k)
            if (off + k < cap) v |= (uint32_t)base[off + k] << (8 * k);
        return v;
    }
    __device__ inline void open(uint32_t begin, uint32_t len)
    {
        pos = begin, end = begin + len, over = false;
        w0 = word(pos & ~3u);
        w1 = word((pos & ~3u) + 4);
    }
    __device__ inline uint32_t next()
    {
        if (pos >= end) {
            over = true;
            return 0;
        }
        const uint32_t v = (w0 >> (8 * (pos & 3))) & 0xff;
        if ((++pos & 3) == 0) {
            w0 = w1;
            w1 = word(pos + 4);
        }
        return v;
    }
};

__device__ inline uint32_t get_bits(uint32_t& x, Reader& r)
{
    const uint32_t val = x & kBypassMax;
    x >>= kBypassBits;
    if (x < kRansL) x = (x << 8) | r.next();
    return val;
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
    const int tab_bytes = lds_words(t.n, t.stride) * 4;              // (a multiple of 16: dcvc_rans_dev_create)
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
    const uint32_t p_hi = body0 + offs[last] + ((uint32_t)unit[2 * last] | ((uint32_t)unit[2 * last + 1] << 8));
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
        const uint32_t len = (uint32_t)unit[2 * c] | ((uint32_t)unit[2 * c + 1] << 8);
        Reader r;
        r.base = payload, r.staged = pay, r.lo4 = lo4, r.hi4 = hi4, r.cap = payload_capacity;
        r.open(body0 + offs[c], len);
        uint32_t x = r.next();
        x |= r.next() << 8;
        x |= r.next() << 16;
        x |= r.next() << 24;
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
            const uint32_t g = cum >> (kScaleBits - kLutBits);
            uint32_t s = (T.lut[ti * (kLut / 4) + (g >> 2)] >> ((g & 3) * 8)) & 0xff;
            uint32_t ent = T.lute[ti * kLut + g];
            uint32_t d = cum - (ent & kMask);
            while (d >= (ent >> 16) && s < max_value) {       // (s stays inside the row whatever the tables hold)
                ent = row[++s];
                d = cum - (ent & kMask);
            }
            x = (ent >> 16) * (x >> kScaleBits) + d;
            if (x < kRansL) {
                x = (x << 8) | r.next();
                if (x < kRansL) x = (x << 8) | r.next();
            }
            int32_t value = (int32_t)s;
            if (s == max_value) {                             // escape, as DecCursor::decode (saturating count, 16 groups at most)
                uint32_t val = get_bits(x, r);
                uint32_t n_bypass = val;
                while (val == kBypassMax && !r.over) {
                    val = get_bits(x, r);
                    n_bypass = n_bypass < 1024u ? n_bypass + val : n_bypass;
                }
                uint32_t raw = 0;
                for (uint32_t j = 0; j < n_bypass && j < 16; ++j) raw |= get_bits(x, r) << (j * kBypassBits);
                value = (int32_t)(raw >> 1);
                if (raw & 1)
                    value = -value - 1;
                else
                    value += (int32_t)max_value;
            }
            io[i] = (uint8_t)(value + offset);                // in place: index i has been read
        }
        if (r.over || r.pos != r.end || x != kRansL) e |= DCVC_RANS_DEV_E_CHUNK;
        if (e) atomicOr(err, e);
    }
    __syncthreads();
    // ---- the symbols of positions [lo, hi), nothing past the count
    for (int j = threadIdx.x; j < n_vec; j += WG) reinterpret_cast<uint4*>(out + lo)[j] = reinterpret_cast<const uint4*>(io)[j];
    for (int j = (n_vec << 4) + threadIdx.x; j < n_io; j += WG) out[lo + j] = (int8_t)io[j];
}

int64_t chunks_max(int64_t max_symbols, int log2_s) { return (max_symbols + ((int64_t)1 << log2_s) - 1) >> log2_s; }
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
    DCVC_REQUIRE(cdf && sizes && offsets && out && n > 0 && n <= 255 && stride >= 3 && stride <= 34,
                 "dcvc_rans_dev_create: bad table group (n=%d stride=%d)", n, stride);
    // (the decoder keeps the tables, 16 KB of indexes / symbols and 24 KB of chunk bodies in 64 KB of LDS)
    DCVC_REQUIRE(lds_words(n, stride) * 4 + kIoBytes + kPayBytes <= 65536 && lds_words(n, stride) % 4 == 0,
                 "dcvc_rans_dev_create: tables of %d bytes do not fit the decoder's LDS budget (n a multiple of 4, n * (stride + 21) <= 6144)",
                 lds_words(n, stride) * 4);
    std::vector<uint32_t> h((size_t)lds_words(n, stride), 0);
    uint32_t* sym = h.data();
    uint32_t* meta = sym + (size_t)n * stride;
    uint8_t* lut = reinterpret_cast<uint8_t*>(meta + n);
    uint32_t* lute = meta + n + (size_t)n * (kLut / 4);
    for (int t = 0; t < n; ++t) {
        const int32_t* c = cdf + (size_t)t * stride;
        bool ok = sizes[t] >= 3 && sizes[t] <= stride && c[0] == 0 && c[sizes[t] - 1] == (1 << kScaleBits) &&
                  offsets[t] >= -32768 && offsets[t] <= 32767;
        for (int j = 0; ok && j + 1 < sizes[t]; ++j) ok = c[j + 1] > c[j];
        DCVC_REQUIRE(ok, "dcvc_rans_dev_create: table %d is not a strictly increasing 16-bit cdf of 3..%d entries", t, stride);
        const int nsym = sizes[t] - 1;
        for (int v = 0; v < nsym; ++v) sym[(size_t)t * stride + v] = (uint32_t)c[v] | ((uint32_t)(c[v + 1] - c[v]) << 16);
        meta[t] = (uint32_t)(nsym - 1) | ((uint32_t)(uint16_t)(int16_t)offsets[t] << 16);
        int v = 0;
        for (int b = 0; b < kLut; ++b) {
            while (c[v + 1] <= (b << (kScaleBits - kLutBits))) ++v;
            lut[(size_t)t * kLut + b] = (uint8_t)v;
            lute[(size_t)t * kLut + b] = sym[(size_t)t * stride + v];
        }
    }
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
    d->t = Tables{d->dev, d->dev + (size_t)n * stride, d->dev + (size_t)n * stride + n,
                  d->dev + (size_t)n * stride + n + (size_t)n * (kLut / 4), n, stride};
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
    if (max_symbols < 0 || log2_s < 8 || log2_s > 12 || !slot_ok(slot_bytes)) return 0;
    const int64_t nch = chunks_max(max_symbols, log2_s);
    return 2 * up16(nch * 4) + 16 + up16(nch * slot_of(log2_s, slot_bytes));
}

int dcvc_rans_dev_encode_y(const dcvc_rans_dev* d, const int16_t* sym_dev, const int32_t* count_dev, int64_t max_symbols,
                           int log2_s, int slot_bytes, void* workspace, uint8_t* unit_host, int64_t unit_capacity, void* stream)
{
    DCVC_REQUIRE(d && sym_dev && count_dev && workspace && unit_host, "dcvc_rans_dev_encode_y: null pointer");
    DCVC_REQUIRE(log2_s >= 8 && log2_s <= 12, "dcvc_rans_dev_encode_y: log2 of the chunk size is %d (8 .. 12)", log2_s);
    // a slot of at most 65535 bytes is also what keeps every chunk length inside its uint16 field
    DCVC_REQUIRE(slot_ok(slot_bytes), "dcvc_rans_dev_encode_y: slot of %d bytes (a multiple of 4, 0 .. 65532)", slot_bytes);
    DCVC_REQUIRE(max_symbols >= 0 && max_symbols < (1ll << 31) && unit_capacity >= 0 && unit_capacity < (1ll << 31),
                 "dcvc_rans_dev_encode_y: bad sizes");
    DCVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "dcvc_rans_dev_encode_y: workspace must be 16-byte aligned");
    const int64_t nch = chunks_max(max_symbols, log2_s);
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
    if (max_symbols < 0 || log2_s < 8 || log2_s > 12) return 0;
    return 16 + up16(chunks_max(max_symbols, log2_s) * 4);
}

int dcvc_rans_dev_decode_y(const dcvc_rans_dev* d, const uint8_t* payload_dev, int64_t payload_capacity,
                           const int32_t* unit_desc_dev, const uint8_t* idx_dev, const int32_t* count_dev, int64_t max_symbols,
                           int log2_s, void* workspace, int8_t* sym_dev, int32_t* error_host, void* stream)
{
    DCVC_REQUIRE(d && payload_dev && unit_desc_dev && idx_dev && count_dev && workspace && sym_dev && error_host,
                 "dcvc_rans_dev_decode_y: null pointer");
    DCVC_REQUIRE(log2_s >= 8 && log2_s <= 12, "dcvc_rans_dev_decode_y: log2 of the chunk size is %d (8 .. 12)", log2_s);
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
    const int64_t blocks = (chunks_max(max_symbols, log2_s) + lanes - 1) / lanes;
    hipLaunchKernelGGL(dec_scan_kernel, dim3(1), dim3(SB), 0, st, payload_dev, payload_capacity, unit_desc_dev, count_dev,
                       max_symbols, log2_s, head, offs, err_dev);
    if (blocks > 0)
        hipLaunchKernelGGL(dec_chunks_kernel, dim3((unsigned)blocks), dim3(WG), d->lds + kIoBytes + kPayBytes, st, d->t, payload_dev,
                           (uint32_t)payload_capacity, unit_desc_dev, idx_dev, count_dev, log2_s, head, offs, sym_dev, err_dev);
    DCVC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
