"""The chunked y units of the GPU-decodable stream mode (docs/chunked_stream.md) on the host: dcvc_rans_chunked_encode_y /
_decode_y are the format's normative implementation, the device encoder's fallback and what the device kernels are compared
against (tests/test_gpu_rans_dev.py).  All on the CPU, over the real Gaussian tables.

  * round trip for every count around a chunk boundary, every table, both escape signs and the int8 extremes;
  * size condition: a unit costs at most 7 bytes per chunk (+ 8) over the single stream of the existing coder.  An
    independent chunk pays its own 4-byte state flush and its 2-byte length entry; cutting a stream at a symbol boundary
    otherwise moves bits between two byte-granular streams, at most one byte of rounding per cut;
  * a chunk IS the old coder: reset(); encode_y(chunk); flush() of one coder, byte for byte;
  * damaged units (truncated, every byte of the length table, a bit of a body, a table longer than the unit) are refused;
  * the container carries the mode in its NAL type and leaves every other stream byte-identical.
"""
import hashlib
import io
import json
import os
import subprocess

import numpy as np
import pytest

from opendcvc_amd import _lib
from opendcvc_amd import bitstream as B
from opendcvc_amd._lib import DcvcError
from opendcvc_amd.pipeline import FramePacket

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libdcvc_amd.so not built")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = lambda S: (0, 1, S - 1, S, S + 1, 3 * S + 7, 40000)      # noqa: E731
LOG2S = (8, 10)


@pytest.fixture(scope="module")
def coder():
    from opendcvc_amd import entropy
    c = entropy.EntropyCoder()
    assert c.add_cdf(*entropy.gaussian_cdf_tables()) == 0
    c.set_use_two_entropy_coders(False)
    return c


def make_symbols(count, seed=0, escapes=True):
    """`count` kept symbols (sym << 8) | index: the indexes walk through all 128 tables, the values follow each table's
    scale; with `escapes`, every 7th value lies outside its table on either side and the int8 extremes occur"""
    rng = np.random.default_rng(1000 + seed)
    idx = (np.arange(count) * 37 + seed) % 128
    sigma = 0.11 * (16 / 0.11) ** (idx / 127.0)
    sym = np.clip(np.round(rng.standard_normal(count) * sigma), -128, 127).astype(np.int32)
    if escapes and count:
        k = np.arange(count)
        sym = np.where(k % 14 == 3, 20 + k % 100, sym)
        sym = np.where(k % 14 == 10, -20 - k % 100, sym)
        sym[count // 2] = 127
        sym[0] = -128
        sym = np.clip(sym, -128, 127)
    return ((sym << 8) + idx).astype(np.int16), idx.astype(np.uint8), sym.astype(np.int8)


def single_stream(coder, packed):
    """the existing host coder on the same symbols: reset(); encode_y(...); flush() of one coder"""
    coder.reset()
    coder.encode_y(packed, 0)
    coder.flush()
    return coder.get_encoded_stream()


def size_bound(single_bytes, count, log2_s):
    """the size condition (module docstring): 4 flush + 2 length + 1 rounding per chunk, + 8"""
    return single_bytes + 7 * ((count + (1 << log2_s) - 1) >> log2_s) + 8


@pytest.mark.parametrize("log2_s", LOG2S)
def test_round_trip_and_size_condition(coder, log2_s):
    S = 1 << log2_s
    from opendcvc_amd import entropy
    sizes, offsets = entropy.gaussian_cdf_tables()[1:]
    for count in COUNTS(S):
        packed, idx, sym = make_symbols(count, seed=count % 11)
        if count >= 256:
            assert set(idx.tolist()) == set(range(128))
            value = sym.astype(np.int32) - offsets[idx]
            assert (value < 0).any() and (value >= sizes[idx] - 2).any()          # both escape signs
            assert sym.min() == -128 and sym.max() == 127
        unit = coder.chunked_encode_y(packed, 0, log2_s)
        nch = (count + S - 1) // S
        lens = np.frombuffer(unit[:2 * nch], "<u2")
        assert len(unit) == 2 * nch + int(lens.sum()) and (count > 0 or unit == b"")
        out = np.full(count + 3, 77, np.int8)
        assert coder.chunked_decode_y(unit, idx, count, 0, log2_s, out) == count
        assert np.array_equal(out[:count], sym) and (out[count:] == 77).all()
        single = len(single_stream(coder, packed))
        print(f"log2 S {log2_s} count {count}: unit {len(unit)} single stream {single} bound {size_bound(single, count, log2_s)}")
        assert len(unit) <= size_bound(single, count, log2_s)


@pytest.mark.parametrize("log2_s", LOG2S)
def test_a_chunk_is_the_existing_coder(coder, log2_s):
    S = 1 << log2_s
    for count in (1, S - 1, S):
        packed = make_symbols(count, seed=5)[0]
        unit = coder.chunked_encode_y(packed, 0, log2_s)
        body = single_stream(coder, packed)
        assert unit == len(body).to_bytes(2, "little") + body
    # ... and every chunk of a longer unit is the coder's stream of its S symbols
    packed = make_symbols(3 * S + 7, seed=6)[0]
    unit = coder.chunked_encode_y(packed, 0, log2_s)
    lens = np.frombuffer(unit[:8], "<u2")
    pos = 8
    for c in range(4):
        assert unit[pos:pos + lens[c]] == single_stream(coder, packed[c * S:(c + 1) * S])
        pos += int(lens[c])
    assert pos == len(unit)


def test_arguments(coder):
    packed, idx, _ = make_symbols(300)
    for bad in (7, 13):
        with pytest.raises(DcvcError):
            coder.chunked_encode_y(packed, 0, bad)
    with pytest.raises(DcvcError):
        coder.chunked_encode_y(packed, 3, 8)                              # unknown group
    with pytest.raises(DcvcError):
        coder.chunked_encode_y(np.array([0x01FF], np.int16), 0, 8)        # a sentinel is not a kept symbol
    unit = coder.chunked_encode_y(packed, 0, 8)
    with pytest.raises(DcvcError):
        coder.chunked_decode_y(unit, np.full(300, 200, np.uint8), 300, 0, 8, np.zeros(300, np.int8))


def _refused(coder, unit, idx, count, log2_s):
    """decodes an exact-size copy of `unit`; True if it is refused as damaged (-4), never another error"""
    out = np.zeros(count, np.int8)
    try:
        coder.chunked_decode_y(bytes(unit), idx, count, 0, log2_s, out)
    except DcvcError as e:
        assert "(-4)" in str(e), e
        return True
    return False


@pytest.mark.parametrize("log2_s", LOG2S)
def test_damaged_units_are_refused(coder, log2_s):
    S = 1 << log2_s
    count = 3 * S + 7
    # table-coded symbols only: a flipped body bit then cannot hide in an escape's verbatim bits, which no rANS-level
    # check can see (csrc/rans_fuzz.cpp) - the end state is off except by a 2**-23 accident
    from opendcvc_amd import entropy
    packed, idx, _ = make_symbols(2 * count, seed=2, escapes=False)
    sizes, offsets = entropy.gaussian_cdf_tables()[1:]
    value = (packed.astype(np.int32) >> 8) - offsets[idx]
    keep = (value >= 0) & (value < sizes[idx] - 2)
    packed, idx = packed[keep][:count], idx[keep][:count]
    assert packed.size == count
    unit = coder.chunked_encode_y(packed, 0, log2_s)
    nch = (count + S - 1) // S
    assert not _refused(coder, unit, idx, count, log2_s)
    for cut in list(range(0, 2 * nch + 6)) + list(range(2 * nch + 6, len(unit), 37)) + [len(unit) - 1]:
        assert _refused(coder, unit[:cut], idx, count, log2_s), cut
    assert _refused(coder, unit + b"\0", idx, count, log2_s)
    for b in range(2 * nch):                       # each byte of the length table: one bit, then all of them
        for mask in (1 << (b % 8), 0xFF):
            u = bytearray(unit)
            u[b] ^= mask
            assert _refused(coder, u, idx, count, log2_s), (b, mask)
    lens = np.frombuffer(unit[:2 * nch], "<u2")
    starts = 2 * nch + np.concatenate([[0], np.cumsum(lens)[:-1]])
    for c in range(nch):                           # one bit in every chunk body: first, middle and last byte
        for at in (int(starts[c]), int(starts[c]) + int(lens[c]) // 2, int(starts[c]) + int(lens[c]) - 1):
            u = bytearray(unit)
            u[at] ^= 0x10
            assert _refused(coder, u, idx, count, log2_s), (c, at)
    # a length table longer than the unit: the count asks for more entries than there are bytes
    assert _refused(coder, unit[:2 * nch - 1], idx, count, log2_s)
    assert _refused(coder, unit[:3], np.resize(idx, 40000), 40000, log2_s)
    assert _refused(coder, unit, idx, count - S, log2_s) and _refused(coder, unit, np.resize(idx, count + S), count + S, log2_s)


def test_sanitizer_driver_covers_the_chunked_entry_points():
    """the ASan / UBSan fuzz driver (make asan, csrc/rans_fuzz.cpp) round-trips, truncates and flips chunked units too"""
    csrc = os.path.join(REPO, "opendcvc_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "asan"], check=True, capture_output=True, timeout=600)
    p = subprocess.run([os.path.join(REPO, "opendcvc_amd", "rans_fuzz_asan"), "6"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "chunked-unit cases, 0 failures" in p.stdout and " 0 chunked-unit" not in p.stdout


# ------------------------------------------------------------------------------------------ payload + container
def test_payload_header_round_trip_and_validation():
    from opendcvc_amd import entropy
    z, units = b"zzzzz", [b"a" * 300, b"", b"c" * 20000]
    payload = entropy.pack_chunked_payload(9, z, units)
    assert payload[0] == 9
    log2_s, z2, spans = entropy.parse_chunked_payload(payload, 3)
    assert (log2_s, z2) == (9, z) and [payload[o:o + n] for o, n in spans] == units
    for bad in (payload[:-1], payload + b"\0", payload[:1], b"", bytes([7]) + payload[1:], payload[:400]):
        with pytest.raises(DcvcError):
            entropy.parse_chunked_payload(bad, 3)
    with pytest.raises(DcvcError):
        entropy.parse_chunked_payload(payload, 2)
    with pytest.raises(DcvcError):
        entropy.pack_chunked_payload(13, z, units)


def test_container_carries_the_mode(golden_dir):
    assert (B.NalType.NAL_I_CHUNKED, B.NalType.NAL_P_CHUNKED) == (3, 4)
    rng = np.random.default_rng(9)
    pkts = [FramePacket(i == 0, 20 + i, int(i == 1), rng.integers(0, 256, 50 + 300 * i, dtype=np.uint8).tobytes(), chunked=bool(i % 2 == 0))
            for i in range(5)]
    f = io.BytesIO()
    w = B.StreamWriter(f)
    for p in pkts:
        w.write_frame(136, 200, False, p)
    r = B.StreamReader(io.BytesIO(f.getvalue()))
    for p in pkts:
        sps, is_i, qp, payload = r.read_frame()
        assert (is_i, qp, payload, r.chunked, sps["use_ada_i"]) == (p.is_i, p.qp, p.bit_stream, p.chunked, p.use_ada_i)
        assert set(sps) == {"sps_id", "height", "width", "ec_part", "use_ada_i"}
    # the two modes differ in the NAL type nibble only
    a, b = io.BytesIO(), io.BytesIO()
    B.write_ip(a, False, 3, 30, b"payload")
    B.write_ip(b, False, 3, 30, b"payload", chunked=True)
    assert a.getvalue()[0] == 0x23 and b.getvalue()[0] == 0x43 and a.getvalue()[1:] == b.getvalue()[1:]
    assert B.read_sps_remaining(io.BytesIO(bytes([0x80 | 4, 56, 0x80 | 7, 128, 5])), 2) == \
        {"sps_id": 2, "height": 1080, "width": 1920, "ec_part": 1, "use_ada_i": 1}
    # a stream without the new types is the reference's, byte for byte (the golden stream of tests/test_bitstream.py, written
    # here from packets that carry the new attribute switched off)
    s = json.load(open(os.path.join(golden_dir, "container_kat.json")))
    rng = np.random.default_rng(5)
    for c in s["ip"]:
        rng.integers(0, 256, c["payload_len"], dtype=np.uint8)
    f = io.BytesIO()
    w = B.StreamWriter(f)
    for fr in s["stream"]["frames"]:
        w.write_frame(1080, 1920, True, FramePacket(fr["is_i"], fr["qp"], fr["use_ada_i"],
                                                   rng.integers(0, 256, fr["payload_len"], dtype=np.uint8).tobytes(), chunked=False))
    assert hashlib.sha256(f.getvalue()).hexdigest() == s["stream"]["sha256"]
