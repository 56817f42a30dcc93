"""The digest unit of the container (bitstream.NalType.NAL_DIGEST, docs/state_digest.md): written in front of the frame it
describes, read back with it, and absent from a stream written without digests."""
import io

import numpy as np
import pytest

from digest_ref import strip_digest_units
from opendcvc_amd import bitstream as B
from opendcvc_amd.pipeline import FramePacket

H, W = 136, 200


def _packets(digests=True, n=7):
    """I P P P(use_ada_i: a second SPS) P I(chunked) P(chunked) with payloads on both sides of the 1- / 2-byte varint"""
    rng = np.random.default_rng(3)
    out = []
    for k in range(n):
        payload = rng.integers(0, 256, 40 + 60 * k, dtype=np.uint8).tobytes()
        d = int(rng.integers(0, 2 ** 63)) * 2 + (k & 1)          # (drawn either way: the payloads do not depend on `digests`)
        out.append(FramePacket(k in (0, 5), 30 + k, int(k == 3), payload, chunked=k >= 5, digest=d if digests else None))
    out[1].digest = 0 if digests else None                     # (a digest of zero is a digest)
    out[2].digest = 2 ** 64 - 1 if digests else None
    return out


def _write(pkts):
    f = io.BytesIO()
    wr = B.StreamWriter(f)
    sizes = [wr.write_frame(H, W, False, p) for p in pkts]
    return f.getvalue(), sizes


def _read(data, n):
    rd = B.StreamReader(io.BytesIO(data))
    out = []
    for _ in range(n):
        sps, is_i, qp, payload = rd.read_frame()
        out.append(FramePacket(is_i, qp, sps["use_ada_i"], payload, chunked=rd.chunked, digest=rd.digest))
    return out, rd


def test_nal_type_and_packet_field():
    assert B.NalType.NAL_DIGEST == 5 and B.DIGEST_UNIT_BYTES == 9
    p = FramePacket(True, 1, 0, b"x")
    assert p.digest is None and list(p.__dataclass_fields__)[-1] == "digest"


def test_stream_with_digests_reads_back():
    pkts = _packets()
    data, sizes = _write(pkts)
    back, rd = _read(data, len(pkts))
    assert back == pkts
    assert all(isinstance(p.digest, int) for p in back)
    with pytest.raises(EOFError):
        rd.read_frame()
    assert sum(sizes) == len(data)


def test_removing_the_units_gives_the_stream_without_digests():
    on, off = _packets(True), _packets(False)
    data_on, sizes_on = _write(on)
    data_off, sizes_off = _write(off)
    assert [a - b for a, b in zip(sizes_on, sizes_off)] == [9] * len(on)          # write_frame counts the unit
    # (the unit stands directly in front of the frame unit, behind an SPS if the frame brought one)
    stripped, digests = strip_digest_units(data_on, on, sizes_on)
    assert stripped == data_off and digests == [p.digest for p in on]
    back, _ = _read(data_off, len(off))
    assert back == off and all(p.digest is None for p in back)


def test_reader_forgets_the_digest_of_the_frame_before():
    pkts = _packets()
    pkts[2].digest = pkts[4].digest = None
    back, _ = _read(_write(pkts)[0], len(pkts))
    assert [p.digest for p in back] == [p.digest for p in pkts]


def test_truncation_inside_a_digest_unit():
    pkts = _packets()[:2]
    data, sizes = _write(pkts)
    unit = sizes[0] + 0                                        # frame 1 brings no SPS: its digest unit starts the frame
    assert data[unit] >> 4 == 5
    for cut in range(unit + 1, unit + 9):
        rd = B.StreamReader(io.BytesIO(data[:cut]))
        rd.read_frame()
        with pytest.raises(EOFError):
            rd.read_frame()
    # the stream ends directly behind a whole digest unit: the EOFError of an empty read
    rd = B.StreamReader(io.BytesIO(data[:unit + 9]))
    rd.read_frame()
    with pytest.raises(EOFError) as at_unit:
        rd.read_frame()
    with pytest.raises(EOFError) as empty:
        B.StreamReader(io.BytesIO(b"")).read_frame()
    assert str(at_unit.value) == str(empty.value)


def test_a_digest_unit_must_be_followed_by_its_frame():
    data, sizes = _write(_packets()[:2])
    head, frame1 = data[:sizes[0]], data[sizes[0]:]
    unit = frame1[:9]
    sps = io.BytesIO()
    B.write_sps(sps, dict(sps_id=1, height=H, width=W, ec_part=0, use_ada_i=1))
    for middle in (unit, sps.getvalue()):                      # digest digest frame, digest SPS frame
        rd = B.StreamReader(io.BytesIO(head + unit + middle + frame1[9:]))
        rd.read_frame()
        with pytest.raises(ValueError):
            rd.read_frame()
    rd = B.StreamReader(io.BytesIO(head + sps.getvalue() + frame1))          # SPS digest frame is the order written
    rd.read_frame()
    rd.read_frame()
    assert rd.digest == 0


def test_a_digest_outside_64_bits_is_refused():
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            _write([FramePacket(True, 1, 0, b"abc", digest=bad)])
