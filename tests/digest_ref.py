"""numpy restatement of csrc/dcvc_digest.hip (the decoder-state digest), written from the definition in
include/dcvc_amd.h - not from the kernel - so that the two can be compared bit for bit: uint64 arithmetic wraps mod 2^64
and the sum is commutative, so no order of reduction can differ."""
import numpy as np

G = 0x9E3779B97F4A7C15


def mix(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def digest_ref(data):
    """data: bytes (or anything np.frombuffer reads) of n = 8 m bytes, m >= 1 -> the digest as a Python int"""
    w = np.frombuffer(data, dtype="<u8")
    if w.size == 0 or 8 * w.size != len(memoryview(data).cast("B")):
        raise ValueError("the digest is of a positive number of whole 64-bit words")
    with np.errstate(over="ignore"):
        pos = np.arange(1, w.size + 1, dtype=np.uint64) * np.uint64(G)
        total = int(mix(w + pos).sum(dtype=np.uint64)) + int(mix(np.uint64(8 * w.size) * np.uint64(G)))
    return total & (2 ** 64 - 1)


def strip_digest_units(data, pkts, sizes):
    """the container `data` (StreamWriter.write_frame of `pkts`, which returned `sizes`) without its 9-byte digest units:
    each stands directly in front of its frame's I / P unit, whose size follows from the payload's -> (bytes, [digests])"""
    from opendcvc_amd.bitstream import frame_overhead_bytes
    out, digests, pos = b"", [], 0
    for p, n in zip(pkts, sizes):
        frame = data[pos:pos + n]
        at = n - (frame_overhead_bytes(len(p.bit_stream)) + len(p.bit_stream)) - 9
        assert at >= 0 and frame[at] >> 4 == 5 and frame[at] & 15 == frame[at + 9] & 15, "no digest unit in front of the frame unit"
        digests.append(int.from_bytes(frame[at + 1:at + 9], "little"))
        out += frame[:at] + frame[at + 9:]
        pos += n
    assert pos == len(data)
    return out, digests
