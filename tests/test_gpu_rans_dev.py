"""The device entropy coder of the chunked stream mode (csrc/dcvc_rans_dev.hip, docs/chunked_stream.md) on the GPU:
the kernels against the host implementation of the same format (tests/test_rans_chunked_host.py), the overflow fallback,
a damaged payload, and DMCI / DMC with entropy="device" end to end against the default host mode.

Payload size condition used below (per frame, against host mode's payload of the same frame): every y unit may cost
7 bytes per chunk + 8 over its share of the single stream (the unit condition of test_rans_chunked_host.py); the z part is
one more independent stream (+ 8, like a unit's); the header is 1 byte + one varint (<= 4 bytes) per part.
"""
import ctypes
import io

import numpy as np
import pytest
import torch

from opendcvc_amd import weights
from test_gpu_codec import hip_codecs
from test_rans_chunked_host import COUNTS, make_symbols

pytestmark = pytest.mark.gpu

E_COUNT, E_TABLE, E_CHUNK, E_RANGE = 1, 2, 4, 8


# ------------------------------------------------------------------------------------------ kernels
@pytest.fixture(scope="module")
def coders():
    from opendcvc_amd import entropy
    t = entropy.gaussian_cdf_tables()
    host = entropy.EntropyCoder()
    assert host.add_cdf(*t) == 0
    host.set_use_two_entropy_coders(False)
    return host, entropy.DeviceCoder(*t)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def dev_encode(dev, packed, max_symbols, log2_s, slot=0, capacity=None):
    """-> (info, unit bytes, guard bytes intact): the unit buffer is told `capacity` bytes and followed by a canary, the
    workspace likewise"""
    from opendcvc_amd import _lib, entropy
    count = packed.size
    sym = torch.zeros(max(max_symbols, 1), dtype=torch.int16, device="cuda")
    sym[:count] = torch.from_numpy(packed).cuda()
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    ws_bytes = dev.enc_ws_bytes(max_symbols, log2_s, slot)
    ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    capacity = 4 * count + 6 * ((count >> log2_s) + 1) + 16 if capacity is None else capacity
    buf = entropy.PinnedBuffer(16 + capacity + 256)
    buf.u8[:] = 0x5A
    _lib.check(_lib.lib().dcvc_rans_dev_encode_y(dev.handle, _p(sym), _p(cnt), max_symbols, log2_s, slot, _p(ws),
                                                 ctypes.c_void_p(buf.ptr), capacity, _stream()), "rans_dev_encode_y")
    torch.cuda.synchronize()
    info = dev.unit_info(buf)
    intact = bool((buf.u8[16 + capacity:] == 0x5A).all()) and bool((ws[ws_bytes:] == 0xA5).all().item())
    return info, dev.unit_bytes(buf), intact


def dev_decode(dev, unit, idx, count, max_symbols, log2_s, at=5):
    """decodes `unit`, placed at byte `at` of a payload buffer -> (symbols, error word)"""
    from opendcvc_amd import entropy
    cap = at + len(unit) + 3
    payload = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    if len(unit):
        payload[at:at + len(unit)] = torch.from_numpy(np.frombuffer(bytes(unit), np.uint8).copy()).cuda()
    desc = torch.tensor([at, len(unit)], dtype=torch.int32, device="cuda")
    didx = torch.zeros(max(max_symbols, 1), dtype=torch.uint8, device="cuda")
    didx[:min(count, idx.size)] = torch.from_numpy(idx[:count]).cuda()
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    ws = torch.empty(dev.dec_ws_bytes(max_symbols, log2_s), dtype=torch.uint8, device="cuda")
    out = torch.full((max(max_symbols, 1),), 77, dtype=torch.int8, device="cuda")
    err = entropy.PinnedBuffer(16)
    err.view(np.int32, 4)[:] = 0
    dev.decode_y(_p(payload), cap, _p(desc), _p(didx), _p(cnt), max_symbols, log2_s, _p(ws), _p(out), err, _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(err.view(np.int32, 1)[0])


@pytest.mark.parametrize("log2_s", (8, 10))
def test_kernels_write_and_read_the_host_units(coders, log2_s):
    host, dev = coders
    S = 1 << log2_s
    # (count, positions): the counts of the host test; 40 000 kept of 130 560 = (128 / 2) * 34 * 60 positions spans
    # several workgroups of 64 chunks at S = 256
    for count, positions in [(c, c + 100) for c in COUNTS(S)[:-1]] + [(40000, 130560)]:
        packed, idx, sym = make_symbols(count, seed=count % 11)
        unit = host.chunked_encode_y(packed, 0, log2_s)
        info, got, intact = dev_encode(dev, packed, positions, log2_s)
        assert info == (len(unit), 0, count, (count + S - 1) // S), (count, info)
        assert got == unit and intact, f"count {count}: the device unit differs from the host's"
        out, err = dev_decode(dev, unit, idx, count, positions, log2_s)
        assert err == 0 and np.array_equal(out[:count], sym) and (out[count:] == 77).all(), count


def test_overflow_raises_the_flag_and_stays_in_range(coders):
    """escapes only (about 30 bits each against the 16 the slot allows per symbol): the chunks outgrow their slots"""
    host, dev = coders
    count = 600
    sym = np.where(np.arange(count) % 2 == 0, 120 + np.arange(count) % 8, -120 - np.arange(count) % 8)
    packed = ((sym << 8) + 0).astype(np.int16)                       # table 0: the narrowest one
    unit = host.chunked_encode_y(packed, 0, 8)
    lens = np.frombuffer(unit[:6], "<u2")
    assert lens[0] > 2 * 256 + 64 and lens[2] <= 2 * 256 + 64        # full chunks exceed the default slot, the last one fits
    info, _, intact = dev_encode(dev, packed, count + 50, 8)
    assert info[1] == 1 and info[0] == 0 and info[2:] == (count, 3) and intact
    # ... a slot that is large enough codes the same symbols, byte for byte
    info, got, intact = dev_encode(dev, packed, count + 50, 8, slot=4 * 256 + 16)
    assert info == (len(unit), 0, count, 3) and got == unit and intact
    # a unit that does not fit the pinned buffer raises the flag as well, and nothing lands behind the buffer
    packed, _, _ = make_symbols(3000, seed=1)
    unit = host.chunked_encode_y(packed, 0, 8)
    info, _, intact = dev_encode(dev, packed, 3000, 8, capacity=len(unit) - 1)
    assert info[:2] == (0, 1) and intact
    info, got, intact = dev_encode(dev, packed, 3000, 8, capacity=len(unit))
    assert info[:2] == (len(unit), 0) and got == unit and intact


def test_damaged_units_set_the_error_word(coders):
    host, dev = coders
    from opendcvc_amd import entropy
    sizes, offsets = entropy.gaussian_cdf_tables()[1:]
    packed, idx, _ = make_symbols(2000, seed=2, escapes=False)
    value = (packed.astype(np.int32) >> 8) - offsets[idx]
    keep = (value >= 0) & (value < sizes[idx] - 2)                   # table-coded symbols only (see the host test)
    packed, idx = packed[keep][:775], idx[keep][:775]
    unit = host.chunked_encode_y(packed, 0, 8)
    nch = 4
    assert dev_decode(dev, unit, idx, 775, 900, 8)[1] == 0
    assert dev_decode(dev, unit[:-1], idx, 775, 900, 8)[1] == E_TABLE
    assert dev_decode(dev, unit + b"\0", idx, 775, 900, 8)[1] == E_TABLE
    assert dev_decode(dev, unit[:2 * nch - 1], idx, 775, 900, 8)[1] == E_COUNT      # a length table longer than the unit
    assert dev_decode(dev, unit, idx, 775 - 256, 900, 8)[1] == E_TABLE
    for b in range(2 * nch):
        u = bytearray(unit)
        u[b] ^= 1 << (b % 8)
        assert dev_decode(dev, u, idx, 775, 900, 8)[1] == E_TABLE, b
    # two length entries traded against each other: the sum still fits the unit, two chunks end in the wrong place
    lens = np.frombuffer(unit[:2 * nch], "<u2").astype(np.int64)
    assert lens[0] < 0xFFFF and lens[1] > 4
    traded = lens.copy()
    traded[0] += 1
    traded[1] -= 1
    u = bytearray(traded.astype("<u2").tobytes() + unit[2 * nch:])
    assert len(u) == len(unit) and dev_decode(dev, u, idx, 775, 900, 8)[1] == E_CHUNK
    for at in (2 * nch + 1, 2 * nch + 40, len(unit) - 1):
        u = bytearray(unit)
        u[at] ^= 0x10
        assert dev_decode(dev, u, idx, 775, 900, 8)[1] == E_CHUNK, at
    assert dev_decode(dev, unit, idx, 901, 900, 8)[1] == E_RANGE     # more symbols than positions


# ------------------------------------------------------------------------------------------ models
QP = 32
SIZES = {"64x64": (64, 64, 64, 64), "136x200": (200, 136, 208, 144)}     # picture h, w -> padded model input H, W


def unit_spans(payload, n_units):
    from opendcvc_amd import entropy
    return entropy.parse_chunked_payload(payload, n_units)


def unit_chunks(unit):
    """chunks of a valid unit: the (smallest) n whose first n length entries + 2 n add up to the unit's size"""
    for n in range(len(unit) // 6 + 1):
        if 2 * n + int(np.frombuffer(unit[:2 * n], "<u2").sum()) == len(unit):
            return n
    raise AssertionError("not a chunked unit")


def payload_bound(host_bytes, payload, is_i):
    n_units = 4 if is_i else 2
    _, _, spans = unit_spans(payload, n_units)
    return host_bytes + sum(7 * unit_chunks(payload[o:o + n]) + 8 for o, n in spans) + 8 + 1 + 4 * (1 + n_units)


def make_frames(dtype, size, n, seed=11):
    _, _, H, W = SIZES[size]
    return [torch.from_numpy(weights.synthetic_frame_yuv444(H, W, fi, seed)).to("cuda", dtype) for fi in range(n)]


_POOL = {}


def nets(dtype, entropy, log2=None, role="enc"):
    """one (DMCI, DMC) pair per (dtype, role), built once for the module and switched between the modes - the mode is an
    attribute, the captured runs of each mode live side by side; every sequence below starts with an I frame"""
    from opendcvc_amd.entropy import CHUNK_LOG2_DEFAULT
    if (dtype, role) not in _POOL:
        _POOL[(dtype, role)] = hip_codecs(1234, 0.12, dtype)
    i_net, p_net = _POOL[(dtype, role)]
    for m in (i_net, p_net):
        m.set_use_two_entropy_coders(False)
        m.entropy = entropy
        m.chunk_log2 = CHUNK_LOG2_DEFAULT if log2 is None else log2
        m._slot_bytes = 0
        m.dev_fallbacks = 0
    return i_net, p_net


@pytest.fixture(scope="module", autouse=True)
def _drop_pool():
    yield
    _POOL.clear()


def encode(dtype, frames, entropy, defer=False, log2=None, intra_period=-1, hook=None):
    """-> (packets, the encoder's reference feature after every frame)"""
    from opendcvc_amd.pipeline import SequenceEncoder
    ie, pe = nets(dtype, entropy, log2)
    if hook:
        hook(ie, pe)
    enc = SequenceEncoder(ie, pe, QP, intra_period=intra_period, reset_interval=2, defer_stream=defer)
    pkts, feats = [], []
    for x in frames:
        r = enc.encode(x)
        pkts += r if defer else [r]
        f = pe.dpb[0].feature
        feats.append(None if f is None else f.float().cpu().numpy())
    pkts += enc.flush()
    return pkts, feats, (ie, pe)


def decode(dtype, pkts, dims, entropy, defer=False):
    """dims: per packet (h, w) of the picture -> (pictures, the decoder's reference feature after every frame)"""
    from opendcvc_amd.pipeline import SequenceDecoder
    idc, pdc = nets(dtype, entropy, role="dec")
    dec = SequenceDecoder(idc, pdc, dims[0][0], dims[0][1], False, defer_output=defer)
    out, feats = [], []
    for pkt, (h, w) in zip(pkts, dims):
        dec.h, dec.w = h, w
        r = dec.decode(pkt)
        out += [t.float().cpu().numpy() for t in (r if defer else [r])]
        f = pdc.dpb[0].feature
        feats.append(None if f is None else f.float().cpu().numpy())
    out += [t.float().cpu().numpy() for t in dec.flush()]
    return out, feats


@pytest.fixture(scope="module")
def host_runs():
    """host mode (the default) once per (dtype, size): packets, pictures, features - shared, never modified"""
    cache = {}

    def get(dtype, size):
        k = (dtype, size)
        if k not in cache:
            h, w, _, _ = SIZES[size]
            frames = make_frames(dtype, size, 4)
            pkts, efeat, _ = encode(dtype, frames, "host")
            pics, dfeat = decode(dtype, pkts, [(h, w)] * 4, "host")
            cache[k] = dict(frames=frames, pkts=pkts, pics=pics, efeat=efeat, dims=[(h, w)] * 4)
        return cache[k]
    return get


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_device_mode_end_to_end(host_runs, dtype, size):
    ref = host_runs(dtype, size)
    assert not any(p.chunked for p in ref["pkts"])
    pkts, efeat, _ = encode(dtype, ref["frames"], "device")
    assert all(p.chunked for p in pkts) and [p.is_i for p in pkts] == [True, False, False, False]
    # 1. device encode -> device decode: the pictures of host mode, bit for bit, and no encoder / decoder drift
    pics, dfeat = decode(dtype, pkts, ref["dims"], "device")
    for fi in range(4):
        assert np.array_equal(pics[fi], ref["pics"][fi]), f"frame {fi}: picture differs from host mode's"
        if fi:
            assert np.array_equal(efeat[fi], ref["efeat"][fi]) and np.array_equal(dfeat[fi], efeat[fi]), f"frame {fi}: feature"
    # 2. the device-written payload through the host implementation of the format (device decoder off)
    pics_h, dfeat_h = decode(dtype, pkts, ref["dims"], "host")
    for fi in range(4):
        assert np.array_equal(pics_h[fi], ref["pics"][fi]), f"frame {fi}: host decode of the device payload"
        assert fi == 0 or np.array_equal(dfeat_h[fi], efeat[fi])
    # 4. payload size condition, frame by frame, against host mode's payload
    for fi, (p, q) in enumerate(zip(pkts, ref["pkts"])):
        bound = payload_bound(len(q.bit_stream), p.bit_stream, p.is_i)
        print(f"{size} {dtype} frame {fi}: device payload {len(p.bit_stream)} host payload {len(q.bit_stream)} bound {bound}")
        assert len(q.bit_stream) < len(p.bit_stream) <= bound, fi


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_host_written_chunked_stream_decodes_on_the_device(host_runs, dtype):
    """3. compress(chunked=True) of a host-mode model writes the same format (the same bytes as the device coder) ..."""
    from opendcvc_amd.pipeline import INDEX_MAP, FramePacket
    ref = host_runs(dtype, "136x200")
    ie, pe = nets(dtype, "host", log2=9)
    pkts = []
    for fi, x in enumerate(ref["frames"]):
        if fi == 0:
            enc = ie.compress(x, QP, chunked=True)
            pe.clear_dpb()
            pe.add_ref_frame(None, enc["x_hat"])
            pkts.append(FramePacket(True, QP, 0, enc["bit_stream"], chunked=enc["chunked"]))
            continue
        ada = int(fi % 2 == 1)
        if ada:
            pe.prepare_feature_adaptor_i(pkts[-1].qp if fi > 1 else 0)
        qp = pe.shift_qp(QP, INDEX_MAP[fi % 8])
        enc = pe.compress(x, qp, chunked=True)
        pkts.append(FramePacket(False, qp, ada, enc["bit_stream"], chunked=enc["chunked"]))
    dev_pkts, _, _ = encode(dtype, ref["frames"], "device", log2=9)
    assert [p.bit_stream for p in pkts] == [p.bit_stream for p in dev_pkts] and all(p.bit_stream[0] == 9 for p in pkts)
    # ... which the device decodes, through the container
    from opendcvc_amd import bitstream as B
    f = io.BytesIO()
    w = B.StreamWriter(f)
    for p in pkts:
        w.write_frame(200, 136, False, p)
    r = B.StreamReader(io.BytesIO(f.getvalue()))
    back = []
    for _ in pkts:
        sps, is_i, qp, payload = r.read_frame()
        back.append(FramePacket(is_i, qp, sps["use_ada_i"], payload, chunked=r.chunked))
    assert all(p.chunked for p in back)
    pics, _ = decode(dtype, back, ref["dims"], "device")
    for fi in range(4):
        assert np.array_equal(pics[fi], ref["pics"][fi]), fi


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_deferred_modes_and_a_resolution_change_on_the_device(dtype):
    """5. defer_stream / defer_output and 64x64 -> 136x200 -> 64x64 (an I frame at every change) under device mode: the
    packets of the immediate device encoder, the pictures of host mode"""
    order = ["64x64"] * 3 + ["136x200"] * 3 + ["64x64"] * 3
    frames = [make_frames(dtype, s, 9, seed=4)[fi] for fi, s in enumerate(order)]
    dims = [SIZES[s][:2] for s in order]
    host_pkts, _, _ = encode(dtype, frames, "host", intra_period=3)
    host_pics, _ = decode(dtype, host_pkts, dims, "host")
    pkts, _, _ = encode(dtype, frames, "device", intra_period=3)
    dpkts, _, _ = encode(dtype, frames, "device", defer=True, intra_period=3)
    assert [(p.is_i, p.qp, p.use_ada_i, p.chunked, p.bit_stream) for p in dpkts] == \
        [(p.is_i, p.qp, p.use_ada_i, True, p.bit_stream) for p in pkts]
    for defer in (False, True):
        pics, _ = decode(dtype, dpkts, dims, "device", defer=defer)
        assert len(pics) == 9
        for fi in range(9):
            assert np.array_equal(pics[fi], host_pics[fi]), (defer, fi)


def test_overflow_falls_back_to_the_host_encoder(host_runs):
    """a slot of 16 bytes holds no chunk: every unit raises its flag and the model codes it on the host - the same payload"""
    ref = host_runs(torch.float16, "136x200")
    pkts, _, _ = encode(torch.float16, ref["frames"], "device")

    def tiny_slots(ie, pe):
        ie._slot_bytes = pe._slot_bytes = 16
    fb, _, (ie, pe) = encode(torch.float16, ref["frames"], "device", hook=tiny_slots)
    assert [p.bit_stream for p in fb] == [p.bit_stream for p in pkts]
    assert getattr(ie, "dev_fallbacks", 0) >= 1 and getattr(pe, "dev_fallbacks", 0) >= 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_a_damaged_body_is_reported_and_kept_out_of_the_dpb(host_runs, dtype):
    from opendcvc_amd._lib import DcvcError
    from opendcvc_amd.pipeline import FramePacket
    ref = host_runs(dtype, "136x200")
    pkts, _, _ = encode(dtype, ref["frames"], "device")
    idc, pdc = nets(dtype, "device", role="dec")
    h, w = ref["dims"][0]
    sps = dict(height=h, width=w, ec_part=0, use_ada_i=0)
    dec = idc.decompress(pkts[0].bit_stream, sps, pkts[0].qp, chunked=True)
    pdc.clear_dpb()
    pdc.add_ref_frame(None, dec["x_hat"])
    pdc.reset_ref_feature()
    pdc.decompress(pkts[1].bit_stream, dict(sps, use_ada_i=1), pkts[1].qp, chunked=True)
    ref_entry, poc = pdc.dpb[0], pdc.curr_poc
    good = pkts[2].bit_stream
    _, _, spans = unit_spans(good, 2)
    off, n = spans[1]
    bad = bytearray(good)
    bad[off + 2 * unit_chunks(good[off:off + n]) + 6] ^= 0x04        # one bit in the first chunk body of the second unit
    with pytest.raises(DcvcError):
        pdc.decompress(bytes(bad), sps, pkts[2].qp, chunked=True)
    assert len(pdc.dpb) == 1 and pdc.dpb[0] is ref_entry and pdc.curr_poc == poc
    with pytest.raises(DcvcError):                                    # the same on an I frame
        bad_i = bytearray(pkts[0].bit_stream)
        o, n = unit_spans(pkts[0].bit_stream, 4)[2][0]
        bad_i[o + 2 * unit_chunks(pkts[0].bit_stream[o:o + n]) + 6] ^= 0x04
        idc.decompress(bytes(bad_i), sps, pkts[0].qp, chunked=True)
    with pytest.raises(DcvcError):                                    # a header that does not add up never reaches the GPU
        pdc.decompress(good[:-1], sps, pkts[2].qp, chunked=True)


# ------------------------------------------------------------------------------------------ harness
def test_harness_sweep_in_device_mode(tmp_path, golden_dir):
    import sys
    sys.path.insert(0, golden_dir)
    from make_golden_sweep import write_yuv420
    from opendcvc_amd import bitstream as B
    from opendcvc_amd import harness
    W, H, N = 136, 200, 4
    src = str(tmp_path / "seq.yuv")
    write_yuv420(src, W, H, N, 5)
    logs = {}
    for mode in ("host", "device"):
        logs[mode] = harness.run_sweep(lambda: nets(torch.float16, "host"), src, W, H, N, qp_i=[21, 42], verbose_json=True,
                                       entropy=mode, bin_prefix=str(tmp_path / mode))
    for q in (21, 42):
        a, b = logs["host"][q], logs["device"][q]
        assert list(a) == list(b)                                     # the logs gain nothing but other byte counts
        assert a["frame_psnr"] == b["frame_psnr"] and a["frame_type"] == b["frame_type"]
        rd = [B.StreamReader(io.BytesIO(open(tmp_path / f"{m}_q{q}.bin", "rb").read())) for m in ("host", "device")]
        for fi in range(N):
            (_, is_i, _, hp), (_, _, _, dp) = rd[0].read_frame(), rd[1].read_frame()
            assert (rd[0].chunked, rd[1].chunked) == (False, True)
            # (a longer payload may need a longer length varint in its NAL unit: 3 bytes at most)
            extra_bits = 8 * (payload_bound(len(hp), dp, is_i) - len(hp) + 3)
            assert a["frame_bpp"][fi] < b["frame_bpp"][fi] <= a["frame_bpp"][fi] + extra_bits / (W * H), (q, fi)
