"""Host side of the entropy model: CDF table construction (once per model), the C++ rANS coder of
libdcvc_amd.so with its pinned staging buffers, and the device coder's tables (handoff.py moves a
frame's symbols between the GPU and these).

Mirrors, with the same method names, the reference's
  EntropyCoder     src/models/entropy_models.py:11-81   (over MLCodec_extensions_cpp)
  GaussianEncoder  src/models/entropy_models.py:227-341 (scale table, index maths, tables)
  BitEstimator     src/models/entropy_models.py:129-224 (factorized prior of z)
Symbols travel as fixed-size arrays with a sentinel for skipped entries instead of the
reference's boolean-mask compaction (data-dependent size => device sync); the coder drops the
sentinels, so the byte stream is unchanged.
"""
import ctypes
import io
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, bitstream
from ._lib import DcvcError, check

SCALE_MIN, SCALE_MAX, SCALE_LEVELS = 0.11, 16.0, 128

# Chunked payloads (docs/chunked_stream.md; this project's extension, not readable by the reference): the y symbols of a
# frame are coded in independent chunks of 1 << log2_s symbols, so that the GPU codes them with one lane per chunk.
CHUNK_LOG2_MIN, CHUNK_LOG2_MAX = 8, 12
CHUNK_LOG2_DEFAULT = 8          # the fastest decode; the rate overhead is what tools/entropy_time.py reports
DEV_E_COUNT, DEV_E_TABLE, DEV_E_CHUNK, DEV_E_RANGE = 1, 2, 4, 8      # DCVC_RANS_DEV_E_*


def pack_chunked_payload(log2_s, z_part, units):
    """payload of one chunked I / P frame: log2 S, varint len_z + the z part, then varint size + bytes of every y unit"""
    if not CHUNK_LOG2_MIN <= log2_s <= CHUNK_LOG2_MAX:
        raise DcvcError(f"chunked payload: log2 of the chunk size is {log2_s} ({CHUNK_LOG2_MIN} .. {CHUNK_LOG2_MAX})")
    f = io.BytesIO()
    f.write(bytes((log2_s,)))
    for part in [z_part] + list(units):
        bitstream.write_uint_adaptive(f, len(part))
        f.write(part)
    return f.getvalue()


def parse_chunked_payload(payload, n_units):
    """-> (log2_s, z part, [(offset, size) of each y unit inside `payload`]); DcvcError unless the header is well formed and
    the parts add up to the payload exactly"""
    f = io.BytesIO(payload)
    try:
        log2_s = bitstream._byte(f)
        if not CHUNK_LOG2_MIN <= log2_s <= CHUNK_LOG2_MAX:
            raise DcvcError(f"corrupt chunked payload: log2 of the chunk size is {log2_s}")
        nz = bitstream.read_uint_adaptive(f)
        z_part = f.read(nz)
        if len(z_part) != nz:
            raise DcvcError("corrupt or truncated chunked payload: the z part runs past the end")
        units = []
        for _ in range(n_units):
            size = bitstream.read_uint_adaptive(f)
            units.append((f.tell(), size))
            if f.seek(size, io.SEEK_CUR) > len(payload):
                raise DcvcError("corrupt or truncated chunked payload: a y unit runs past the end")
    except EOFError as e:
        raise DcvcError("corrupt or truncated chunked payload: header cut short") from e
    if f.tell() != len(payload):
        raise DcvcError(f"corrupt chunked payload: {len(payload) - f.tell()} bytes behind the last y unit")
    return log2_s, z_part, units


def _ip(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pmf_to_quantized_cdf(pmf, precision=16):
    pmf = np.ascontiguousarray(pmf, np.float32)
    out = np.zeros(pmf.size + 1, np.uint32)
    check(_lib.lib().dcvc_pmf_to_quantized_cdf(_ip(pmf), pmf.size, precision, _ip(out)), "pmf_to_quantized_cdf")
    return out


def _pmf_to_cdf(pmf, tail_mass, pmf_length, max_length):
    cdf = np.zeros((len(pmf_length), max_length + 2), np.int32)
    for i in range(len(pmf_length)):
        prob = np.concatenate([pmf[i, :pmf_length[i]], tail_mass[i]])
        c = pmf_to_quantized_cdf(prob)
        cdf[i, :c.size] = c.astype(np.int32)
    return cdf


def gaussian_cdf_tables():
    """128 quantised zero-mean Gaussian CDFs on the log-spaced scale table (entropy_models.py:244-283).
    Computed on the host CPU in fp32 so encoder and decoder always agree."""
    table = torch.exp(torch.linspace(math.log(SCALE_MIN), math.log(SCALE_MAX), SCALE_LEVELS))
    normal = torch.distributions.normal.Normal
    center = torch.full_like(table, 8.0)
    d = normal(0., table)
    for i in range(8, 1, -1):
        probs = d.cdf(torch.full_like(table, float(i)))
        center = torch.where(probs > 0.9999, torch.full_like(table, float(i)), center)
    center = center.int()
    length = 2 * center + 1
    max_length = int(length.max())
    samples = (torch.arange(max_length) - center[:, None]).float()
    d = normal(0., table[:, None].expand_as(samples))
    upper, lower = d.cdf(samples + 0.5), d.cdf(samples - 0.5)
    cdf = _pmf_to_cdf((upper - lower).numpy(), (2 * lower[:, :1]).numpy(), length.numpy(), max_length)
    return cdf, (length + 2).numpy().astype(np.int32), (-center).numpy().astype(np.int32)


def factorized_cdf_tables(params, qp_num, channel):
    """Per-(qp, channel) CDFs of the factorized z prior (entropy_models.py:152-205).
    params: dict 'f1.h' ... 'f4.b' -> float32 tensors [qp_num, channel, 1, 1] on the CPU."""
    def bitparm(x, f, final):
        x = x * F.softplus(params[f + ".h"]) + params[f + ".b"]
        return x if final else x + torch.tanh(x) * torch.tanh(params[f + ".a"])

    def cdf_of(x):
        for f in ("f1", "f2", "f3"):
            x = bitparm(x, f, False)
        return torch.sigmoid(bitparm(x, "f4", True))

    zero = torch.zeros((qp_num, channel, 1, 1))
    minima, maxima = zero + 8, zero + 8
    for i in range(8, 1, -1):
        minima = torch.where(cdf_of(zero - i) < 0.0001, zero + i, minima)
        maxima = torch.where(cdf_of(zero + i) > 0.9999, zero + i, maxima)
    minima, maxima = minima.int(), maxima.int()
    pmf_length = maxima + minima + 1
    max_length = int(pmf_length.max())
    samples = torch.arange(max_length)[None, None, None, :] + (zero - minima)
    lower, upper = cdf_of(samples - 0.5), cdf_of(samples + 0.5)
    pmf = (upper - lower)[:, :, 0, :]
    top = cdf_of(maxima.to(torch.float32))
    tail = lower[:, :, 0, :1] + (1.0 - top[:, :, 0, -1:])
    cdf = _pmf_to_cdf(pmf.reshape(-1, max_length).numpy(), tail.reshape(-1, 1).numpy(),
                      pmf_length.reshape(-1).numpy(), max_length)
    return cdf, (pmf_length.reshape(-1) + 2).numpy().astype(np.int32), (-minima).reshape(-1).numpy().astype(np.int32)


def cost_table(cdf, cdf_length, offset):
    """Code lengths of one cdf group as the uint32 rows csrc/dcvc_rate.hip reads (rate control's size estimate), from the
    QUANTISED cdfs - the arrays add_cdf receives - in fp64:  row t = [meta, cost[0 .. sizes[t] - 2], 0 ...] with
    meta = (max_value << 16) | (offset & 0xffff), max_value = sizes[t] - 2 (the escape symbol) and
    cost[v] = rint(65536 * (16 - log2(cdf[t][v + 1] - cdf[t][v]))): Q16 bits of a 16-bit-precision rANS step."""
    cdf = np.ascontiguousarray(cdf, np.int64)
    sizes = np.ascontiguousarray(cdf_length, np.int64)
    offset = np.ascontiguousarray(offset, np.int64)
    n, stride = cdf.shape[0], int(sizes.max())
    if sizes.min() < 2 or stride > cdf.shape[1] or np.abs(offset).max() >= 1 << 15 or stride - 2 >= 1 << 15:
        raise DcvcError("cost_table: cdf lengths of 2 .. the row length and 16-bit offsets are needed")
    freq = cdf[:, 1:stride] - cdf[:, :stride - 1]
    valid = np.arange(stride - 1)[None, :] < (sizes - 1)[:, None]
    if (freq[valid] <= 0).any() or (freq[valid] > 1 << 16).any():
        raise DcvcError("cost_table: a symbol of a quantised cdf has no probability mass")
    cost = np.rint(65536.0 * (16.0 - np.log2(np.where(valid, freq, 1).astype(np.float64))))
    out = np.zeros((n, stride), np.uint32)
    out[:, 0] = (((sizes - 2) << 16) | (offset & 0xffff)).astype(np.uint32)
    out[:, 1:] = np.where(valid, cost, 0).astype(np.uint32)
    return out


class PinnedBuffer:
    """hipHostMalloc'ed staging buffer viewed as a numpy array."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = _lib.lib().dcvc_host_alloc(self.nbytes)
        if not self.ptr:
            raise DcvcError("pinned host allocation failed")
        self.u8 = np.ctypeslib.as_array(ctypes.cast(self.ptr, ctypes.POINTER(ctypes.c_uint8)), (self.nbytes,))
        self._dptr = None

    @property
    def dptr(self):
        """device address of the buffer (kernels write the coder's input in place: no copy command)"""
        if self._dptr is None:
            self._dptr = _lib.lib().dcvc_host_device_ptr(ctypes.c_void_p(self.ptr))
            if not self._dptr:
                raise DcvcError("pinned buffer has no device address")
        return self._dptr

    def view(self, dtype, count):
        return self.u8[:count * np.dtype(dtype).itemsize].view(dtype)

    def __del__(self):
        try:
            _lib.lib().dcvc_host_free(ctypes.c_void_p(self.ptr))
        except Exception:
            pass


class EntropyCoder:
    """reference: EntropyCoder (entropy_models.py:11-81) + RansEncoder/RansDecoder (py_rans.cpp)."""

    def __init__(self):
        L = _lib.lib()
        self.enc = ctypes.c_void_p(L.dcvc_rans_enc_create())
        self.dec = ctypes.c_void_p(L.dcvc_rans_dec_create())
        if not self.enc or not self.dec:
            raise DcvcError("cannot create the rANS coder")
        self._pinned = {}
        self.two = False             # set_use_two_entropy_coders: the frame's ec_part split
        self.tables = []             # (cdf, cdf_length, offset) of every group, as add_cdf received them

    def __del__(self):
        try:
            L = _lib.lib()
            L.dcvc_rans_enc_destroy(self.enc)
            L.dcvc_rans_dec_destroy(self.dec)
        except Exception:
            pass

    def pinned(self, key, nbytes):
        """Pinned staging buffer for (key, nbytes).  One buffer per distinct size, never replaced or freed while
        the coder lives: captured HIP graphs (models.GraphCache) keep the raw host pointer in their memcpy
        nodes, so a buffer handed out once must stay valid and keep its meaning for that (key, size)."""
        k = (key, int(nbytes))
        b = self._pinned.get(k)
        if b is None:
            b = self._pinned[k] = PinnedBuffer(nbytes)
        return b

    def adopt_pinned(self, other):
        """takes over another coder's staging buffers (CompressionModel.update() called again: graphs captured
        earlier may still reference them)"""
        if other is not None:
            self._pinned.update(other._pinned)

    def add_cdf(self, cdf, cdf_length, offset):
        L = _lib.lib()
        cdf = np.ascontiguousarray(cdf, np.int32)
        cdf_length = np.ascontiguousarray(cdf_length, np.int32)
        offset = np.ascontiguousarray(offset, np.int32)
        a = check(L.dcvc_rans_enc_add_cdf(self.enc, _ip(cdf), cdf.shape[0], cdf.shape[1], _ip(cdf_length), _ip(offset)), "add_cdf")
        b = check(L.dcvc_rans_dec_add_cdf(self.dec, _ip(cdf), cdf.shape[0], cdf.shape[1], _ip(cdf_length), _ip(offset)), "add_cdf")
        assert a == b == len(self.tables)
        self.tables.append((cdf, cdf_length, offset))
        return a

    def set_use_two_entropy_coders(self, two):
        L = _lib.lib()
        self.two = bool(two)
        L.dcvc_rans_enc_set_use_two(self.enc, int(bool(two)))
        L.dcvc_rans_dec_set_use_two(self.dec, int(bool(two)))

    # ---- encoder
    def reset(self):
        check(_lib.lib().dcvc_rans_enc_reset(self.enc), "rans reset")

    def encode_y(self, symbols, cdf_group_index, borrowed=False):
        """symbols: host int16 array ((sym << 8) + index, index 0xFF = skipped).  borrowed=True skips the
        copy: the array must then stay untouched until get_encoded_stream() has returned."""
        symbols = np.ascontiguousarray(symbols, np.int16)
        f = _lib.lib().dcvc_rans_enc_encode_y_borrowed if borrowed else _lib.lib().dcvc_rans_enc_encode_y
        check(f(self.enc, _ip(symbols), symbols.size, cdf_group_index), "encode_y")

    def encode_z(self, symbols, cdf_group_index, start_offset, per_channel_size):
        symbols = np.ascontiguousarray(symbols, np.int8)
        check(_lib.lib().dcvc_rans_enc_encode_z(self.enc, _ip(symbols), symbols.size, cdf_group_index, start_offset,
                                                per_channel_size), "encode_z")

    def flush(self):
        check(_lib.lib().dcvc_rans_enc_flush(self.enc), "rans flush")

    def get_encoded_stream(self):
        p = ctypes.c_void_p()
        n = check(_lib.lib().dcvc_rans_enc_get_stream(self.enc, ctypes.byref(p)), "get_encoded_stream")
        return ctypes.string_at(p, n) if n else b""

    # ---- decoder
    def set_stream(self, stream):
        buf = np.frombuffer(stream, np.uint8)
        check(_lib.lib().dcvc_rans_dec_set_stream(self.dec, _ip(buf), buf.size), "set_stream")

    def decode_y(self, indexes, cdf_group_index):
        """indexes: host uint8 array, 0xFF = skipped (decodes to 0)."""
        indexes = np.ascontiguousarray(indexes, np.uint8)
        check(_lib.lib().dcvc_rans_dec_decode_y(self.dec, _ip(indexes), indexes.size, cdf_group_index), "decode_y")

    def decode_z(self, total_size, cdf_group_index, start_offset, per_channel_size):
        check(_lib.lib().dcvc_rans_dec_decode_z(self.dec, total_size, cdf_group_index, start_offset, per_channel_size), "decode_z")

    def get_decoded(self, out):
        """Blocks until the queued decode finished and copies the int8 symbols into `out` (host)."""
        n = check(_lib.lib().dcvc_rans_dec_get(self.dec, _ip(out), out.size), "get_decoded")
        return n

    def check_end(self):
        """After the last symbol of a frame: raises DcvcError if the payload was corrupt or truncated (the coder is not
        back in its initial state / has bytes left over).  No reference counterpart (it decodes garbage silently)."""
        check(_lib.lib().dcvc_rans_dec_check_end(self.dec), "corrupt or truncated frame payload")

    def decode_compact(self, indexes, count, cdf_group_index, out):
        """Synchronous: `indexes[:count]` are the KEPT table indexes only (compacted on the device, stream order); decodes one
        symbol each into out[:count]."""
        if indexes.dtype != np.uint8 or out.dtype != np.int8 or count < 0 or indexes.size < count or out.size < count or \
                not indexes.flags.c_contiguous or not out.flags.c_contiguous:
            raise DcvcError("decode_compact: need contiguous uint8 indexes and an int8 output of at least `count` entries")
        check(_lib.lib().dcvc_rans_dec_decode_compact(self.dec, _ip(indexes), int(count), cdf_group_index, _ip(out)),
              "decode_compact")
        return count

    # ---- chunked y units (both directions synchronous, on the calling thread)
    def chunked_encode_y(self, symbols, cdf_group_index, log2_s):
        """symbols: host int16 array of KEPT symbols ((sym << 8) + index, no sentinels) -> the unit's bytes"""
        symbols = np.ascontiguousarray(symbols, np.int16)
        nch = (symbols.size + (1 << log2_s) - 1) >> log2_s if CHUNK_LOG2_MIN <= log2_s <= CHUNK_LOG2_MAX else 0
        out = np.empty(4 * symbols.size + 6 * nch + 16, np.uint8)        # 4 bytes per symbol, flush + length per chunk
        n = check(_lib.lib().dcvc_rans_chunked_encode_y(self.enc, _ip(symbols), symbols.size, cdf_group_index, log2_s, _ip(out),
                                                        out.size), "chunked_encode_y")
        return out[:n].tobytes()

    def chunked_decode_y(self, unit, indexes, count, cdf_group_index, log2_s, out):
        """unit: bytes of one y unit; indexes[:count]: the kept table indexes in stream order; symbols into out[:count].
        DcvcError on a damaged unit."""
        unit = np.frombuffer(unit, np.uint8)
        if indexes.dtype != np.uint8 or out.dtype != np.int8 or count < 0 or indexes.size < count or out.size < count or \
                not indexes.flags.c_contiguous or not out.flags.c_contiguous:
            raise DcvcError("chunked_decode_y: need contiguous uint8 indexes and an int8 output of at least `count` entries")
        check(_lib.lib().dcvc_rans_chunked_decode_y(self.dec, _ip(unit), unit.size, _ip(indexes), int(count), cdf_group_index,
                                                    log2_s, _ip(out)), "corrupt or truncated chunked y unit")
        return count

    def decode_and_get_y(self, indexes, cdf_group_index, out):
        """Synchronous: decodes straight from `indexes` into `out` (both host arrays of the same length)."""
        if indexes.dtype != np.uint8 or out.dtype != np.int8 or out.size < indexes.size or \
                not indexes.flags.c_contiguous or not out.flags.c_contiguous:
            raise DcvcError("decode_and_get_y: need contiguous uint8 indexes and an int8 output of the same length")
        check(_lib.lib().dcvc_rans_dec_decode_and_get_y(self.dec, _ip(indexes), indexes.size, cdf_group_index,
                                                        _ip(out)), "decode_and_get_y")
        return indexes.size


class DeviceCoder:
    """Device tables of one cdf group for the chunked-unit kernels (csrc/dcvc_rans_dev.hip): dcvc_rans_dev_create / _destroy"""

    def __init__(self, cdf, cdf_length, offset):
        cdf = np.ascontiguousarray(cdf, np.int32)
        cdf_length = np.ascontiguousarray(cdf_length, np.int32)
        offset = np.ascontiguousarray(offset, np.int32)
        self.handle = ctypes.c_void_p()
        check(_lib.lib().dcvc_rans_dev_create(_ip(cdf), cdf.shape[0], cdf.shape[1], _ip(cdf_length), _ip(offset),
                                              ctypes.byref(self.handle)), "rans_dev_create")

    def __del__(self):
        try:
            if self.handle:
                _lib.lib().dcvc_rans_dev_destroy(self.handle)
        except Exception:
            pass

    UNIT_INFO_BYTES = 16     # int32 {unit bytes, overflow flag, count, chunks} in front of the unit in its pinned buffer

    @staticmethod
    def enc_ws_bytes(max_symbols, log2_s, slot_bytes=0):
        return int(_lib.lib().dcvc_rans_dev_enc_ws_bytes(max_symbols, log2_s, slot_bytes))

    @staticmethod
    def dec_ws_bytes(max_symbols, log2_s):
        return int(_lib.lib().dcvc_rans_dev_dec_ws_bytes(max_symbols, log2_s))

    @staticmethod
    def unit_buffer_bytes(max_symbols, log2_s):
        """pinned bytes for a unit of up to max_symbols symbols: one byte per symbol (kept y symbols average well under
        that; a unit that needs more raises its overflow flag and is coded on the host) + length table + info"""
        nch = (max_symbols + (1 << log2_s) - 1) >> log2_s
        return (DeviceCoder.UNIT_INFO_BYTES + max_symbols + 2 * nch + 64 + 15) // 16 * 16

    def encode_y(self, sym_dev, count_dev, max_symbols, log2_s, workspace, unit_buf, stream, slot_bytes=0):
        """enqueues the encode of sym_dev[:*count_dev] (device pointers) into the PinnedBuffer unit_buf; unit_info() /
        unit_bytes() read the result once the stream has passed this point"""
        check(_lib.lib().dcvc_rans_dev_encode_y(self.handle, sym_dev, count_dev, max_symbols, log2_s, slot_bytes, workspace,
                                                ctypes.c_void_p(unit_buf.ptr), unit_buf.nbytes - self.UNIT_INFO_BYTES, stream),
              "rans_dev_encode_y")

    @staticmethod
    def unit_info(unit_buf):
        """-> (unit bytes, overflow flag, symbol count, chunks)"""
        return tuple(int(v) for v in unit_buf.view(np.int32, 4))

    @staticmethod
    def unit_bytes(unit_buf):
        n = int(unit_buf.view(np.int32, 1)[0])
        return unit_buf.u8[DeviceCoder.UNIT_INFO_BYTES:DeviceCoder.UNIT_INFO_BYTES + n].tobytes()

    def decode_y(self, payload_dev, payload_capacity, unit_desc_dev, idx_dev, count_dev, max_symbols, log2_s, workspace, sym_dev,
                 error_buf, stream):
        """enqueues the decode of the unit at payload_dev + desc[0] (desc[1] bytes; device int32 pair) into sym_dev; a damaged
        unit ORs DEV_E_* bits into the first int32 of the PinnedBuffer error_buf"""
        check(_lib.lib().dcvc_rans_dev_decode_y(self.handle, payload_dev, payload_capacity, unit_desc_dev, idx_dev, count_dev,
                                                max_symbols, log2_s, workspace, sym_dev, ctypes.c_void_p(error_buf.ptr), stream),
              "rans_dev_decode_y")
