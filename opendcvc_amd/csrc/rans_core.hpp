// rans_core.hpp - the entropy stage's stream format, stated once: byte-wise rANS with a 32-bit state from 1 << 23, 16-bit
// probabilities, escape ("bypass") coding of symbols outside their table, the 4-byte flush and the geometry of the chunked
// y units (docs/chunked_stream.md).  For rans_host.cpp (g++), dcvc_rans_dev.hip (through rans_lane.hpp), dcvc_rate.hip and
// rans_fuzz.cpp; table search, the symbol push (reciprocal multiply / division) and byte I/O stay per side.  The arithmetic
// is the reference's (src/cpp/py_rans/rans_byte.h:61-141, rans.cpp:28-58,356-429), which tests/ verify against golden
// streams; oracle/rans_oracle.c and tests/rate_ref.py restate it independently on purpose.
#pragma once
#include <cstdint>

#include "common.hpp"

#define RANS_HD __host__ __device__ inline

namespace rans {

constexpr int kScaleBits = 16;
constexpr uint32_t kRansL = 1u << 23;                        // lower bound of the normalised state
constexpr int kRenormShift = 23 - kScaleBits + 8;
constexpr int kBypassBits = 2;
constexpr uint32_t kBypassMax = (1u << kBypassBits) - 1;
constexpr uint32_t kMask = (1u << kScaleBits) - 1;
// the state is renormalised (low byte out) while it is not below these, before bypass bits / a symbol of `freq` go in
constexpr uint32_t kBitsXMax = (1u << (kScaleBits - kBypassBits)) << kRenormShift;
RANS_HD uint32_t symbol_x_max(uint32_t freq) { return ((kRansL >> kScaleBits) << 8) * freq; }
constexpr int kLog2ChunkMin = 8, kLog2ChunkMax = 12;         // chunk sizes of the chunked y units: 256 .. 4096 symbols

// ---- table entry: a value's (start | freq << 16); a freq of 65536 does not occur (every table has >= 2 values)
RANS_HD uint32_t entry(uint32_t start, uint32_t freq) { return start | (freq << 16); }
RANS_HD uint32_t entry_start(uint32_t e) { return e & kMask; }
RANS_HD uint32_t entry_freq(uint32_t e) { return e >> 16; }

// ---- escapes: value = symbol - offset outside [0, max_value) is coded as the table's symbol max_value, then bypass
// groups of 2 bits: the number n of groups that hold `raw` in unary base 3 (n / 3 threes and one digit below 3), then raw's
// n groups from the lowest.  The encoder pushes everything in reverse of that order.
RANS_HD uint32_t escape_raw(int32_t value, int32_t max_value) { return value < 0 ? -2 * value - 1 : 2 * (value - max_value); }
RANS_HD int32_t escape_value(uint32_t raw, int32_t max_value)
{
    const int32_t v = (int32_t)(raw >> 1);
    return (raw & 1) ? -v - 1 : v + max_value;
}
RANS_HD uint32_t bypass_groups(uint32_t raw)         // 2-bit groups that hold raw
{
#ifdef __HIP_DEVICE_COMPILE__
    return raw ? (uint32_t)(33 - __clz((int)raw)) >> 1 : 0u;
#else
    return raw ? (uint32_t)(33 - __builtin_clz(raw)) >> 1 : 0u;
#endif
}
RANS_HD uint32_t escape_group_count(uint32_t n) { return n / 3u + 1u + n; }      // count digits + raw groups

template <typename PutBits>
RANS_HD void put_escape(uint32_t raw, PutBits put_bits)
{
    const int n = (int)bypass_groups(raw);
    for (int j = n - 1; j >= 0; --j) put_bits((raw >> (j * kBypassBits)) & kBypassMax);
    const int threes = n / (int)kBypassMax;
    put_bits((uint32_t)(n - threes * (int)kBypassMax));
    for (int j = 0; j < threes; ++j) put_bits(kBypassMax);
}

// the 4-byte flush: the state, little endian; the encoder writes downwards, so from the top byte (put_byte: the low 8 bits)
template <typename PutByte>
RANS_HD void put_state(uint32_t x, PutByte put_byte)
{
    put_byte(x >> 24);
    put_byte(x >> 16);
    put_byte(x >> 8);
    put_byte(x);
}

// ---- decode side.  Src: a byte source with next() (0 past its end, which sets the flag) and a bool `overrun`.
template <typename Src>
RANS_HD uint32_t get_state(Src& src)
{
    uint32_t x = src.next();
    x |= src.next() << 8;
    x |= src.next() << 16;
    x |= src.next() << 24;
    return x;
}

template <typename Src>
RANS_HD uint32_t get_bits(uint32_t& x, Src& src)
{
    const uint32_t val = x & kBypassMax;
    x >>= kBypassBits;
    if (x < kRansL) x = (x << 8) | src.next();
    return val;
}

template <typename Src>
RANS_HD void renorm_after_symbol(uint32_t& x, Src& src)
{
    if (x < kRansL) {
        x = (x << 8) | src.next();
        if (x < kRansL) x = (x << 8) | src.next();
    }
}

// the value behind a decoded escape symbol.  A valid stream carries at most 16 groups - 32 bits - per escape; a corrupt one
// may claim any number: the count saturates, the value is assembled without signed overflow, and the source keeps its rules
template <typename Src>
RANS_HD int32_t decode_escape(uint32_t& x, Src& src, int32_t max_value)
{
    uint32_t val = get_bits(x, src);
    uint32_t n = val;
    while (val == kBypassMax && !src.overrun) {
        val = get_bits(x, src);
        n = n < 1024u ? n + val : n;
    }
    uint32_t raw = 0;
    for (uint32_t j = 0; j < n && j < 16; ++j) raw |= get_bits(x, src) << (j * kBypassBits);
    return escape_value(raw, max_value);
}

// ---- chunked y unit: chunks(count) little-endian uint16 chunk byte lengths, then the chunk bodies; a chunk is 1 << log2_s
// kept symbols (the last one fewer) coded as a stream of its own: state kRansL, symbols pushed in reverse, 4-byte flush
RANS_HD bool chunked_args_ok(int log2_s) { return log2_s >= kLog2ChunkMin && log2_s <= kLog2ChunkMax; }
RANS_HD int64_t chunks(int64_t count, int log2_s) { return (count + ((int64_t)1 << log2_s) - 1) >> log2_s; }
template <typename Index>      // (the index arithmetic in the caller's type: dec_chunks_kernel's is 32 bits wide)
RANS_HD uint32_t chunk_len(const uint8_t* unit, Index c) { return (uint32_t)unit[2 * c] | ((uint32_t)unit[2 * c + 1] << 8); }
RANS_HD void put_chunk_len(uint8_t* unit, int64_t c, uint32_t len) { unit[2 * c] = (uint8_t)len, unit[2 * c + 1] = (uint8_t)(len >> 8); }

// ---- table preparation (host).  A cdf group: n rows of `stride` int32, row t a strictly increasing cdf of sizes[t] entries
// from 0 to 65536 (its last value is the escape), offsets[t] the symbol of value 0 - an int16 in every decoder's tables.
inline bool check_cdf_group(const char* who, const int32_t* cdf, int n, int stride, const int32_t* sizes, const int32_t* offsets)
{
    if (!cdf || !sizes || !offsets || n <= 0 || stride < 3 || stride > 34) {
        dcvc::set_error("%s: bad table group (n=%d stride=%d, stride must be 3..34)", who, n, stride);
        return false;
    }
    for (int t = 0; t < n; ++t) {
        const int32_t* c = cdf + (size_t)t * stride;
        const char* bad = sizes[t] < 3 || sizes[t] > stride ? "has a size outside 3..stride" : nullptr;
        if (!bad && (offsets[t] < -32768 || offsets[t] > 32767)) bad = "has an offset outside int16 (no decoder table holds it)";
        if (!bad && (c[0] != 0 || c[sizes[t] - 1] != (1 << kScaleBits))) bad = "is not a 16-bit cdf from 0 to 65536";
        for (int j = 0; !bad && j + 1 < sizes[t]; ++j) bad = c[j + 1] > c[j] ? nullptr : "is not strictly increasing";
        if (!bad) continue;
        dcvc::set_error("%s: table %d (size %d, stride %d, offset %d) %s", who, t, sizes[t], stride, offsets[t], bad);
        return false;
    }
    return true;
}

inline void fill_entries(const int32_t* c, int nsym, uint32_t* out)      // the nsym = size - 1 values of one checked cdf row
{
    for (int v = 0; v < nsym; ++v) out[v] = entry((uint32_t)c[v], (uint32_t)(c[v + 1] - c[v]));
}

// first guess of the table search: set(b, v) per bucket b of the cumulative slot, v the value that owns its lower edge
template <int LUT_BITS, typename Set>
inline void fill_first_guess(const int32_t* c, Set set)
{
    int v = 0;
    for (int b = 0; b < (1 << LUT_BITS); ++b) {
        while (c[v + 1] <= (b << (kScaleBits - LUT_BITS))) ++v;      // the row ends at 65536 > every edge
        set(b, v);
    }
}

}  // namespace rans
