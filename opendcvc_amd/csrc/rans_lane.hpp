// rans_lane.hpp - what ONE LANE of the device coder does with ONE CHUNK of a chunked y unit (dcvc_rans_dev.hip), as
// host-and-device functions: the tables, the byte sink and source and the encoder's walk are plain integer and pointer code,
// so the sanitizer driver (rans_fuzz.cpp) runs exactly these bodies on the CPU (the decoder's walk stays in its kernel).  The format is rans_core.hpp's.  The encoder
// divides by freq where the host coder multiplies by a reciprocal: both are exact.
#pragma once
#include <vector>

#include "rans_core.hpp"

namespace rans {

constexpr int kLaneLutBits = 4;
constexpr int kLaneLut = 1 << kLaneLutBits;

struct Tables {                         // pointers (device memory, its LDS copy, or a host array) + geometry, passed by value
    const uint32_t* sym;                // [n][stride]
    const uint32_t* meta;               // [n] max_value | (uint16)offset << 16
    const uint32_t* lut;                // [n][kLaneLut / 4] first-guess value per bucket, bytes packed in words
    const uint32_t* lute;               // [n][kLaneLut] the guessed value's entry itself: ONE read on the state chain
    int n, stride;
};

// the four arrays are one block of table_words() words in this order (20 KB for the 128 Gaussian tables)
RANS_HD int table_words(int n, int stride) { return n * stride + n + n * (kLaneLut / 4) + n * kLaneLut; }
RANS_HD Tables tables_at(const uint32_t* w, int n, int stride)
{
    return Tables{w, w + n * stride, w + n * stride + n, w + n * stride + n + n * (kLaneLut / 4), n, stride};
}

// that block for a cdf group (host); false with the error text set when the group is not one
inline bool build_tables(const char* who, const int32_t* cdf, int n, int stride, const int32_t* sizes, const int32_t* offsets,
                         std::vector<uint32_t>& words)
{
    if (!check_cdf_group(who, cdf, n, stride, sizes, offsets)) return false;
    words.assign((size_t)table_words(n, stride), 0);
    uint32_t* sym = words.data();
    uint32_t* meta = sym + (size_t)n * stride;
    uint8_t* lut = reinterpret_cast<uint8_t*>(meta + n);
    uint32_t* lute = meta + n + (size_t)n * (kLaneLut / 4);
    for (int t = 0; t < n; ++t) {
        const int32_t* c = cdf + (size_t)t * stride;
        uint32_t* row = sym + (size_t)t * stride;
        fill_entries(c, sizes[t] - 1, row);
        meta[t] = (uint32_t)(sizes[t] - 2) | ((uint32_t)(uint16_t)(int16_t)offsets[t] << 16);
        fill_first_guess<kLaneLutBits>(c, [&](int b, int v) {
            lut[(size_t)t * kLaneLut + b] = (uint8_t)v;
            lute[(size_t)t * kLaneLut + b] = row[v];
        });
    }
    return true;
}

// ------------------------------------------------------------------------------------------ encoder
// Bytes go downwards into the lane's slot through a 32-bit accumulator, one aligned word store per four bytes: a global
// store per byte would put a memory wait into nearly every symbol's step (the wave's loads and stores retire in order).
struct Emit {
    uint8_t* slot;                      // 4-byte aligned, a multiple of 4 bytes long
    int pos;                            // bytes still free below the write position
    uint32_t acc;
    bool ovf;
    RANS_HD void byte(uint32_t b)
    {
        if (pos == 0) {
            ovf = true;                 // the slot would overflow: flag instead of writing
            return;
        }
        acc = (acc << 8) | (b & 0xff);
        if ((--pos & 3) == 0) *reinterpret_cast<uint32_t*>(slot + pos) = acc;
    }
    RANS_HD void finish()     // the bytes of a last, partial word (its low bytes lie below the chunk: never read)
    {
        if (pos & 3) *reinterpret_cast<uint32_t*>(slot + (pos & ~3)) = acc << (8 * (pos & 3));
    }
};

RANS_HD void put_bits(uint32_t& x, Emit& e, uint32_t val)
{
    while (x >= kBitsXMax && !e.ovf) {
        e.byte(x & 0xff);
        x >>= 8;
    }
    x = (x << kBypassBits) | val;
}

RANS_HD void put_symbol(uint32_t& x, Emit& e, uint32_t ent)
{
    const uint32_t start = entry_start(ent), freq = entry_freq(ent);
    const uint32_t x_max = symbol_x_max(freq);
    while (x >= x_max && !e.ovf) {
        e.byte(x & 0xff);
        x >>= 8;
    }
    x = ((x / freq) << kScaleBits) + (x % freq) + start;
}

// Codes the packed symbols [a, b) - (symbol << 8) | table index - downwards into the slot (4-byte aligned, `slot` bytes, a
// multiple of 4), last symbol first, and flushes; the chunk is the slot's last `return value` bytes.  fetch(j0), j0 a multiple
// of 8, returns the entries [j0, j0 + 8) as a uint4 (those outside [a, b) are not looked at): the next block is fetched while
// this one is coded, so the loads stay off the state's dependency chain.  0: the slot is too small or an index names no table
// of the group; nothing outside the slot has been written.  (The Emit as a reference parameter cost enc_chunks_kernel 26 SGPRs.)
template <typename Fetch>
RANS_HD uint32_t encode_chunk(const Tables& T, Fetch fetch, int64_t a, int64_t b, uint8_t* slot_p, int slot)
{
    Emit e{slot_p, slot, 0, false};
    uint32_t x = kRansL;
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
        put_escape(escape_raw(value, max_value), [&](uint32_t v) { put_bits(x, e, v); });
        put_symbol(x, e, row[max_value]);
    }
    if (e.pos < 4) e.ovf = true;
    if (e.ovf) return 0;
    put_state(x, [&](uint32_t v) { e.byte(v); });
    e.finish();
    return (uint32_t)(slot - e.pos);
}

// ------------------------------------------------------------------------------------------ decoder
// The chunk's bytes through a window of two aligned 32-bit words.  A workgroup stages the bodies of its chunks with
// coalesced loads (dec_chunks_kernel: in LDS); a word of the staged range comes from there, any other one (a workgroup whose
// bodies outgrow the staging area: escape-heavy chunks) from the payload itself.  Addresses come from the validated chunk
// start and a running counter only - never from payload content - and stay inside the payload buffer; a byte at or past
// the chunk's end is never USED: next() returns 0 there and marks the overrun (a damaged stream reads zeros).
struct Reader {
    const uint8_t* base;                // payload buffer, 4-byte aligned
    const uint32_t* staged;             // copy of the payload words [lo4, hi4)
    uint32_t lo4, hi4;
    uint32_t cap;                       // size of the payload buffer
    uint32_t pos, end;                  // next byte / end of the chunk, offsets into the payload buffer
    uint32_t w0, w1;
    bool overrun;
    RANS_HD uint32_t word(uint32_t off) const
    {
        if (off >= lo4 && off < hi4) return staged[(off - lo4) >> 2];
        if (off + 4 <= cap) return *reinterpret_cast<const uint32_t*>(base + off);
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k)
            if (off + k < cap) v |= (uint32_t)base[off + k] << (8 * k);
        return v;
    }
    RANS_HD void open(uint32_t begin, uint32_t len)
    {
        pos = begin, end = begin + len, overrun = false;
        w0 = word(pos & ~3u);
        w1 = word((pos & ~3u) + 4);
    }
    RANS_HD uint32_t next()
    {
        if (pos >= end) {
            overrun = true;
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

}  // namespace rans
