"""The entropy hand-off: everything between "the network produced packed symbols / scales" and "the coder has bytes / the
network has y_hat".  models.py keeps the networks, the captured runs, the DPB and the deferred-output / deferred-stream logic
and calls in here with the model `m` as first argument (its coder, persistent buffers, stream and tables are the model's).

Encoder: stage() puts one frame's symbols where the coder reads them and returns an EncodeJob; code() turns a job into the
frame's payload.  Three forms, chosen once per frame by encoder_form():
  REFERENCE       the reference's stream: kept symbols compacted into pinned memory, coded by the host rANS coder
  CHUNKED_HOST    the chunked payload of docs/chunked_stream.md, the same staging, its y units coded by the host
  CHUNKED_DEVICE  the chunked payload, kept symbols compacted into device memory and coded there, one unit per part

Decoder: open_frame() returns the frame's hand-off object, whose class is chosen once.  Four forms:
  WholeArrayFrame     reference stream, whole index / symbol arrays moved by copy commands (models.DEC_COMPACT false)
  CompactFrame        reference stream, kept indexes / symbols compacted on the device, through pinned memory (the default)
  ChunkedHostFrame    chunked payload through the compacted hand-off, units decoded by the host
  ChunkedDeviceFrame  chunked payload uploaded once, units decoded by kernels: no host step between the runs
"""
import ctypes

import numpy as np
import torch

from . import _lib, entropy
from . import nn as L
from ._lib import DcvcError, check

REFERENCE, CHUNKED_HOST, CHUNKED_DEVICE = "reference", "chunked_host", "chunked_device"


# =============================================================================== encoder

def encoder_form(m, chunked):
    """compress(chunked=...): None -> what the model's entropy attribute implies"""
    if m.entropy not in ("host", "device"):
        raise DcvcError(f"entropy must be 'host' or 'device', not {m.entropy!r}")
    dev = m.entropy == "device"
    chunked = dev if chunked is None else bool(chunked)
    if dev and not chunked:
        raise DcvcError("entropy='device' writes chunked payloads only: the reference's stream format is two serial "
                        "coder chains per frame, which the GPU cannot produce in parallel")
    if chunked and not entropy.CHUNK_LOG2_MIN <= m.chunk_log2 <= entropy.CHUNK_LOG2_MAX:
        raise DcvcError(f"chunk_log2 is {m.chunk_log2} ({entropy.CHUNK_LOG2_MIN} .. {entropy.CHUNK_LOG2_MAX})")
    return CHUNKED_DEVICE if dev else CHUNKED_HOST if chunked else REFERENCE


class EncodeJob:
    """one frame's symbols on their way to the coder; valid for the host once `ready` has passed.
    hz: pinned z symbols (nz int8).  REFERENCE / CHUNKED_HOST: hp, hc = pinned kept symbols [parts, nsym] int16 and their
    counts.  CHUNKED_DEVICE: units = one pinned buffer (info + unit) per part, csym = the compacted symbols on the device.
    est: the pinned words of dcvc_rate_estimate (None unless the model's rate_estimate is set), two: the ec_part split."""
    __slots__ = ("form", "ready", "qp", "hz", "nz", "zhw", "parts", "nsym", "log2_s", "hp", "hc", "units", "csym", "est", "two")


def stage(m, key, form, z8, packed, qp, zhw):
    """Encoder hand-off without a copy command: z (int8) and the KEPT y symbols of each part of `packed`, compacted in order
    on the device, are written by kernels straight into pinned host buffers (dcvc_compact_symbols).  CHUNKED_DEVICE: the kept
    symbols are compacted into DEVICE memory and entropy-coded there, one unit per part, each landing in its own pinned
    buffer; nothing waits for the host.  Records the job's ready event behind the last of these launches."""
    lib, ec = _lib.lib(), m.entropy_coder
    job = EncodeJob()
    job.form, job.qp, job.zhw, job.log2_s = form, qp, zhw, m.chunk_log2
    job.parts, job.nsym = packed.shape
    job.nz = nz = z8.numel()
    job.hp = job.hc = job.units = job.csym = job.est = None
    job.two = ec.two
    parts, nsym, dev = job.parts, job.nsym, packed.device
    job.hz = ec.pinned(key + "_z", (nz + 3) // 4 * 4)
    if nz % 4 == 0:
        check(lib.dcvc_copy_f32(ctypes.c_void_p(job.hz.dptr), L._p(z8), nz // 4, m._stream()), "z to host")
    else:
        check(lib.dcvc_memcpy_d2h(ctypes.c_void_p(job.hz.ptr), L._p(z8), nz, m._stream()), "d2h")
    ws = m._buffer("compact_ws", (256 * parts,), torch.int32, dev)
    if form != CHUNKED_DEVICE:
        job.hp = ec.pinned(key + "_sym", parts * nsym * 2)
        job.hc = ec.pinned(key + "_cnt", 4 * parts)
        check(lib.dcvc_compact_symbols(L._p(packed), nsym, parts, ctypes.c_void_p(job.hp.ptr), ctypes.c_void_p(job.hc.ptr),
                                       L._p(ws), m._stream()), "compact_symbols")
    else:
        log2_s = job.log2_s
        job.csym = m._buffer(key + "_csym", (parts, nsym), torch.int16, dev)
        ccnt = m._buffer(key + "_ccnt", (parts,), torch.int32, dev)               # counts[p] of part p, dense
        check(lib.dcvc_compact_symbols_dev(L._p(packed), nsym, parts, L._p(job.csym), L._p(ccnt), L._p(ws), m._stream()),
              "compact_symbols_dev")
        coder = m._device_coder()
        ews = m._buffer("rans_enc_ws", (coder.enc_ws_bytes(nsym, log2_s, m._slot_bytes),), torch.uint8, dev)
        job.units = []
        for k in range(parts):
            ub = ec.pinned(f"{key}_unit{k}_{log2_s}", coder.unit_buffer_bytes(nsym, log2_s))
            coder.encode_y(L._p(job.csym[k]), ctypes.c_void_p(ccnt.data_ptr() + 4 * k), nsym, log2_s, L._p(ews), ub, m._stream(),
                           slot_bytes=m._slot_bytes)
            job.units.append(ub)
    if m.rate_estimate:
        job.est = _enqueue_estimate(m, key, z8, packed, qp, zhw)
    job.ready = torch.cuda.Event()
    job.ready.record()
    return job


def _rate_tables(m, dev):
    """device copies of the two groups' cost tables (entropy.cost_table), uploaded once per update()"""
    if m._rate_dev is None or m._rate_dev[0].device != dev:
        g, z = (entropy.cost_table(*m.entropy_coder.tables[k]) for k in (m._g_group, m._z_group))
        m._rate_dev = tuple(torch.from_numpy(t.view(np.int32)).to(dev) for t in (g, z))
    return m._rate_dev


def _enqueue_estimate(m, key, z8, packed, qp, zhw):
    """dcvc_rate_estimate on the frame's symbols where the front run left them -> pinned words (per staging set, like the
    symbols: the host may still be reading the other set's)"""
    lib, dev = _lib.lib(), packed.device
    parts, nsym = packed.shape
    nz = z8.numel()
    gcost, zcost = _rate_tables(m, dev)
    out = m.entropy_coder.pinned(key + "_est", 8 * (3 * parts + 2))
    ws = m._buffer("rate_ws", (int(check(lib.dcvc_rate_estimate_ws_bytes(nsym, parts, nz), "rate_estimate_ws_bytes")) // 8,),
                   torch.int64, dev)
    check(lib.dcvc_rate_estimate(L._p(packed), nsym, parts, L._p(gcost), gcost.shape[0], gcost.shape[1], L._p(z8), nz, zhw,
                                 L._p(zcost), zcost.shape[0], zcost.shape[1], qp * m.z_channel, L._p(ws),
                                 ctypes.c_void_p(out.ptr), m._stream()), "rate_estimate")
    return out


FLUSH_BYTES = 4          # rans_host.cpp: the coder's 32-bit state, written once per non-empty coder / per chunk
CHUNK_LEN_BYTES = 2      # the uint16 entry of a chunk in its unit's length table


def _varint_bytes(v):
    """bitstream.write_uint_adaptive"""
    return 1 if v < 1 << 7 else 2 if v < 1 << 14 else 4


def _bytes_of(q16):
    return -(-int(q16) // (8 << 16))


def estimate_words(job):
    """-> ([(Q16 bits, kept, escapes) per part], (Q16 bits, escapes) of z) once the hand-off has landed"""
    if job.est is None:
        raise DcvcError("this frame carries no size estimate: set the model's rate_estimate before compress()")
    job.ready.synchronize()
    w = [int(v) for v in job.est.view(np.uint64, 3 * job.parts + 2)]
    return [tuple(w[3 * p:3 * p + 3]) for p in range(job.parts)], (w[3 * job.parts], w[3 * job.parts + 1])


def coders_of(job, kept):
    """streams that end in a flush: REFERENCE - the non-empty coders of the frame (ec_part = 1 gives the first coder
    kept / 2 of every part's kept symbols and nz / 2 of z, the second one the rest); chunked - those of the z part plus
    one per chunk"""
    nz, halves = job.nz, ((lambda n: (n // 2, n - n // 2)) if job.two else (lambda n: (n,)))
    z = sum(1 for n in halves(nz) if n)
    if job.form == REFERENCE:
        loads = [halves(nz)] + [halves(k) for k in kept]
        return sum(1 for c in range(len(loads[0])) if any(l[c] for l in loads))
    return z + sum((k + (1 << job.log2_s) - 1) >> job.log2_s for k in kept)


def estimated_bytes(m, job):
    """Predicted size of the payload code(m, job) returns, known as soon as job.ready has passed (before the host coder
    has started): ceil(bits / 8) of the device's estimate plus the fixed costs of the job's form.  REFERENCE: FLUSH_BYTES
    per non-empty coder.  Chunked (entropy.pack_chunked_payload): the log2 S byte, the z part (its coders' flushes) and
    every unit - a length entry and a flush per chunk - each behind the varint of its size."""
    ybits, (zbits, _) = estimate_words(job)
    kept = [k for _, k, _ in ybits]
    if job.form == REFERENCE:
        return _bytes_of(zbits + sum(b for b, _, _ in ybits)) + FLUSH_BYTES * coders_of(job, kept)
    zc = coders_of(job, [])
    sizes = [_bytes_of(zbits) + FLUSH_BYTES * zc]
    for b, k, _ in ybits:
        nch = (k + (1 << job.log2_s) - 1) >> job.log2_s
        sizes.append(_bytes_of(b) + (FLUSH_BYTES + CHUNK_LEN_BYTES) * nch)
    return 1 + sum(_varint_bytes(s) + s for s in sizes)


def code(m, job):
    """host: one frame's payload from its job (waits for the hand-off first).  REFERENCE: z and every part through the host
    coder's one stream.  Chunked: the z part is what the host coder writes for reset(); encode_z(...); flush(), then one unit
    per part - coded here by the host implementation of the format or, CHUNKED_DEVICE, coded already: a unit whose overflow
    flag is up (a chunk outgrew its scratch slot, or the unit its buffer) is coded here instead, from the compacted symbols."""
    job.ready.synchronize()
    ec, form, nsym, log2_s = m.entropy_coder, job.form, job.nsym, job.log2_s
    ec.reset()
    ec.encode_z(job.hz.view(np.int8, job.nz), m._z_group, job.qp * m.z_channel, job.zhw)
    if form != REFERENCE:
        ec.flush()
        z_part = ec.get_encoded_stream()
    if form != CHUNKED_DEVICE:
        ps, counts = job.hp.view(np.int16, job.parts * nsym), job.hc.view(np.int32, job.parts)
    units = []
    for k in range(job.parts):
        if form == CHUNKED_DEVICE:
            _, overflow, count, _ = entropy.DeviceCoder.unit_info(job.units[k])
            if not overflow:
                units.append(entropy.DeviceCoder.unit_bytes(job.units[k]))
                continue
            if not 0 <= count <= nsym:
                raise DcvcError("encoder hand-off: %d kept symbols of %d positions" % (count, nsym))
            kept = job.csym[k, :count].cpu().numpy()
            m.dev_fallbacks += 1
        else:
            kept = ps[k * nsym:k * nsym + counts[k]]
        if form == REFERENCE:
            ec.encode_y(kept, m._g_group, borrowed=True)      # pinned staging buffer, untouched until get_encoded_stream()
        else:
            units.append(ec.chunked_encode_y(kept, m._g_group, log2_s))
    if form != REFERENCE:
        return entropy.pack_chunked_payload(log2_s, z_part, units)
    ec.flush()
    return ec.get_encoded_stream()


# =============================================================================== decoder

class Step:
    """One checkerboard decoding step's hand-off buffers: the device-side index array (and, compacted forms, the workspace the
    restore needs again), the kept indexes / their count and the decoded symbols in the memory the frame's form puts them in.

    These records come out of captured runs: GraphCache caches them and hands the SAME object back on every replay, for every
    later frame that shares the run.  A record therefore holds only address-stable things - pinned and device buffers,
    capacities.  Everything that changes per frame (the payload bytes, the unit spans, the kept count) is read from the
    current frame's object, never through a reference stored here."""
    __slots__ = ("n", "cap", "idx", "ws", "kept", "cnt", "sym")

    def __init__(self, n, cap, idx, ws, kept, cnt, sym):
        self.n, self.cap, self.idx, self.ws, self.kept, self.cnt, self.sym = n, cap, idx, ws, kept, cnt, sym


class _Frame:
    """The hand-off of the frame being decoded.  index() and restore() launch inside captured runs (so they read only their
    arguments, the Step and what the graph key pins down); decode() runs on the host between two runs, for unit 0 .. units-1
    in order; end_z() follows the z symbols, close() the frame's last launch."""
    suffix = ()                 # graph-key suffix of the runs that contain index() / restore()
    host_waits = True           # the host decodes between the runs: it waits for index() to have landed before decode()

    def __init__(self, m, prefix, units):
        self.m, self.prefix, self.units = m, prefix, units

    def _pinned(self, unit, name, nbytes):
        return self.m.entropy_coder.pinned(f"{self.prefix}{unit}{name}", nbytes)

    def end_z(self):
        pass

    def _end_of_stream(self, unit):
        if unit == self.units - 1:
            self.m.entropy_coder.check_end()      # corrupt / truncated payload: DcvcError here, not a garbage picture

    def close(self):
        pass


class WholeArrayFrame(_Frame):
    """Pinned host buffers filled / read by stream-ordered copies.
    Measured in round 4 (profiles/r04_dec_inplace.txt): the kernel writing the indexes straight into the pinned buffer takes
    39 us instead of 5.4 us + a ~10 us copy command, and the restore kernel reading the symbols in place 108 us instead
    of 7.7 us + copy - a channel's run of 16 pixels is 16 bytes, one bus transaction per lane, where the copy moves
    whole lines; only z (read coalesced, 65 KB) is taken in place."""

    def index(self, groups, unit, scales, H, W, C):
        m, lib = self.m, _lib.lib()
        n = (C // groups) * H * W
        idx = torch.empty(n, dtype=torch.uint8, device=scales.device)
        check(lib.dcvc_prior_dec_index(L.dtype_code(scales.dtype), groups, unit, *L.map_args(scales),
                                       H, W, C, m._thres(), L._p(idx), m._stream()), "prior_dec_index")
        buf = self._pinned(unit, "_idx", n)
        check(lib.dcvc_memcpy_d2h(ctypes.c_void_p(buf.ptr), L._p(idx), n, m._stream()), "d2h")
        return Step(n, n, idx, None, buf, None, self._pinned(unit, "_sym", n))

    def decode(self, unit, st):
        self.m.entropy_coder.decode_and_get_y(st.kept.view(np.uint8, st.n), self.m._g_group, st.sym.view(np.int8, st.n))
        self._end_of_stream(unit)

    def restore(self, st, groups, unit, means, yhat, H, W, C, out):
        m, lib = self.m, _lib.lib()
        sym = torch.empty(st.n, dtype=torch.int8, device=yhat.device)
        check(lib.dcvc_memcpy_h2d(L._p(sym), ctypes.c_void_p(st.sym.ptr), st.n, m._stream()), "h2d")
        check(lib.dcvc_prior_dec_restore(L.dtype_code(means.dtype), groups, unit, L._p(sym), *L.map_args(means),
                                         H, W, C, *L.map_args(yhat), *L.map_args(out), m._stream()),
              "prior_dec_restore")


class CompactFrame(_Frame):
    """The KEPT indexes only, compacted in stream order by a kernel that writes them (and their count) straight into pinned
    buffers; the decoded symbols are read back from pinned memory by the restore the same way."""

    def index(self, groups, unit, scales, H, W, C):
        m, lib = self.m, _lib.lib()
        n = (C // groups) * H * W
        cap = (n + 15) // 16 * 16
        idx = torch.empty(n, dtype=torch.uint8, device=scales.device)
        ws = torch.empty(int(lib.dcvc_prior_dec_compact_ws_bytes(H, W, C, groups)), dtype=torch.uint8, device=scales.device)
        buf, cnt = self._pinned(unit, "_cidx", cap), self._pinned(unit, "_ccnt", 16)
        check(lib.dcvc_prior_dec_index_compact(L.dtype_code(scales.dtype), groups, unit, *L.map_args(scales),
                                               H, W, C, m._thres(), L._p(idx), L._p(ws), ctypes.c_void_p(buf.ptr),
                                               ctypes.c_void_p(cnt.ptr), m._stream()), "prior_dec_index_compact")
        return Step(n, cap, idx, ws, buf, cnt, self._pinned(unit, "_csym", cap))

    def decode(self, unit, st):
        count = int(st.cnt.view(np.int32, 1)[0])
        if not 0 <= count <= st.n:
            raise DcvcError("decoder hand-off: %d kept symbols of %d positions" % (count, st.n))
        self._decode_kept(unit, st.kept.view(np.uint8, st.cap), count, st.sym.view(np.int8, st.cap))

    def _decode_kept(self, unit, kept, count, out):
        self.m.entropy_coder.decode_compact(kept, count, self.m._g_group, out)
        self._end_of_stream(unit)

    def restore(self, st, groups, unit, means, yhat, H, W, C, out):
        check(_lib.lib().dcvc_prior_dec_restore_compact(
            L.dtype_code(means.dtype), groups, unit, ctypes.c_void_p(st.sym.ptr), L._p(st.idx), L._p(st.ws),
            *L.map_args(means), H, W, C, *L.map_args(yhat), *L.map_args(out), self.m._stream()),
            "prior_dec_restore_compact")


class ChunkedHostFrame(CompactFrame):
    """A chunked payload on the host: the compacted hand-off (and its captured runs), each step's unit through the host
    implementation of the format.  Every unit checks its own end; the z part is a stream of its own."""

    def __init__(self, m, prefix, log2_s, payload, spans):
        super().__init__(m, prefix, len(spans))
        self.log2_s, self.payload, self.spans = log2_s, payload, spans

    def end_z(self):
        self.m.entropy_coder.check_end()          # exactly consumed, or the payload is damaged

    def _decode_kept(self, unit, kept, count, out):
        off, size = self.spans[unit]
        self.m.entropy_coder.chunked_decode_y(self.payload[off:off + size], kept, count, self.m._g_group, self.log2_s, out)


class ChunkedDeviceFrame(_Frame):
    """A chunked payload on the device.  open uploads [unit (offset, size) int32 pairs: DESC_BYTES][payload] with one
    stream-ordered copy, so that a captured launch finds every frame's units through fixed addresses; kept indexes and their
    count stay in device memory, the step's unit is decoded right behind them on the stream and the restore reads the device
    symbols - no host step, no event wait.  The chunk size and the buffer's capacity are baked into the runs: `suffix`."""
    DESC_BYTES = 64
    host_waits = False

    def __init__(self, m, prefix, log2_s, payload, spans):
        super().__init__(m, prefix, len(spans))
        ec, D, n = m.entropy_coder, self.DESC_BYTES, len(payload)
        cap = 1 << 16
        while cap < n:
            cap *= 2
        stage = ec.pinned("dev_payload", D + cap)
        desc = stage.view(np.int32, D // 4)
        desc[:] = 0
        desc[:2 * len(spans)] = np.asarray(spans, np.int32).reshape(-1)
        stage.u8[D:D + n] = np.frombuffer(payload, np.uint8)
        self.log2_s, self.cap, self.suffix = log2_s, cap, ("dev", log2_s, cap)
        self.blob = m._buffer("dev_payload", (D + cap,), torch.uint8, m._dtype_device()[1])
        self.err = ec.pinned("dev_err", 16)
        self.err.view(np.int32, 4)[:] = 0
        check(_lib.lib().dcvc_memcpy_h2d(L._p(self.blob), ctypes.c_void_p(stage.ptr), (D + n + 15) // 16 * 16, m._stream()), "h2d")

    def end_z(self):
        self.m.entropy_coder.check_end()          # the z part is a stream of its own

    def index(self, groups, unit, scales, H, W, C):
        m, lib, dev = self.m, _lib.lib(), scales.device
        n = (C // groups) * H * W
        cap = (n + 15) // 16 * 16
        idx = torch.empty(n, dtype=torch.uint8, device=dev)
        ws = torch.empty(int(lib.dcvc_prior_dec_compact_ws_bytes(H, W, C, groups)), dtype=torch.uint8, device=dev)
        cidx = torch.empty(cap, dtype=torch.uint8, device=dev)
        cnt = torch.empty(4, dtype=torch.int32, device=dev)
        dsym = torch.empty(cap, dtype=torch.int8, device=dev)
        check(lib.dcvc_prior_dec_index_compact_dev(L.dtype_code(scales.dtype), groups, unit, *L.map_args(scales),
                                                   H, W, C, m._thres(), L._p(idx), L._p(ws), L._p(cidx), L._p(cnt),
                                                   m._stream()), "prior_dec_index_compact_dev")
        coder = m._device_coder()
        dws = torch.empty(coder.dec_ws_bytes(n, self.log2_s), dtype=torch.uint8, device=dev)
        blob = self.blob.data_ptr()
        coder.decode_y(ctypes.c_void_p(blob + self.DESC_BYTES), self.cap, ctypes.c_void_p(blob + 8 * unit), L._p(cidx), L._p(cnt),
                       n, self.log2_s, L._p(dws), L._p(dsym), self.err, m._stream())
        return Step(n, cap, idx, ws, cidx, cnt, dsym)

    def decode(self, unit, st):
        pass                                      # decoded on the stream already

    def restore(self, st, groups, unit, means, yhat, H, W, C, out):
        check(_lib.lib().dcvc_prior_dec_restore_compact_dev(
            L.dtype_code(means.dtype), groups, unit, L._p(st.sym), L._p(st.idx), L._p(st.ws), *L.map_args(means),
            H, W, C, *L.map_args(yhat), *L.map_args(out), self.m._stream()),
            "prior_dec_restore_compact_dev")

    def close(self):
        """waits for the frame's last kernel and reads the error word once"""
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        bits = int(self.err.view(np.int32, 1)[0])
        if bits:
            raise DcvcError("corrupt or truncated frame payload: the device entropy decoder reports error bits 0x%x "
                            "(1: symbol count vs length table, 2: length table vs unit size, 4: a chunk does not end in its "
                            "initial state on its last byte, 8: range)" % bits)


def open_frame(m, bit_stream, sps, units, prefix, chunked, compact):
    """decoder: hands the frame's stream (a chunked payload: its z part, after parsing and validating the header) to the host
    coder and returns the frame's hand-off object.  `units`: y units / checkerboard steps of the frame; `prefix` names the
    model's pinned step buffers; `compact`: models.DEC_COMPACT, read per frame."""
    ec = m.entropy_coder
    if not chunked:
        ec.set_use_two_entropy_coders(sps["ec_part"] == 1)
        ec.set_stream(bit_stream)
        return (CompactFrame if compact else WholeArrayFrame)(m, prefix, units)
    if not compact:       # (checked for every frame: the captured runs of the whole-array hand-off must never serve one)
        raise DcvcError("chunked payloads are decoded through the compacted hand-off (DCVC_DEC_COMPACT=0 is set)")
    log2_s, z_part, spans = entropy.parse_chunked_payload(bit_stream, units)
    ec.set_use_two_entropy_coders(sps["ec_part"] == 1)
    ec.set_stream(z_part)
    return (ChunkedDeviceFrame if m.entropy == "device" else ChunkedHostFrame)(m, prefix, log2_s, bit_stream, spans)
