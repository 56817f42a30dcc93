"""Active-area coding on the GPU (docs/active_area.md): the envelope, the extent rule and the window / paste copies of
csrc/dcvc_bars.hip against the numpy restatement (tests/bars_ref.py) bit for bit, in fp16 and fp32, and the option end to end
through the harness, the container's active-area unit and pipeline.StreamDecoder."""
import ctypes
import io

import numpy as np
import pytest
import torch

import bars_ref as R
from opendcvc_amd import _lib, bars, harness, weights
from opendcvc_amd.bars import ActiveArea, BarDetector
from opendcvc_amd.bitstream import StreamReader
from opendcvc_amd.grain import GrainParams

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.float32, np.float32, id="fp32"), pytest.param(torch.float16, np.float16, id="fp16")]
STW, STH = 64, 128                 # the scan kernel's tile (csrc/dcvc_bars.hip)


def _pad(n, to=16):
    return n + (-n) % to


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _dev(host, offset=0):
    """the host frame [3][Hp][Wp] on the device as [1, 3, Hp, Wp]; offset: that many elements into a larger allocation"""
    t = torch.from_numpy(np.array(host))
    if not offset:
        return t[None].cuda()
    flat = torch.empty(host.size + 16, dtype=t.dtype, device="cuda")
    dev = flat[offset:offset + host.size].view(1, *host.shape)
    dev.copy_(t[None])
    assert dev.data_ptr() % 16 == (offset * host.itemsize) % 16 and dev.is_contiguous()
    return dev


def _frame(ndt, H, W, Hp, Wp, seed, poison=(np.nan, 6e4)):
    """uniform content in [0, 1) in a frame whose padding holds the poison values, alternating"""
    host = np.empty((3, Hp, Wp), ndt)
    host[:, ::2], host[:, 1::2] = poison
    host[:, :H, :W] = np.random.default_rng(seed).random((3, H, W), dtype=np.float32).astype(ndt)
    return host


def _keys(det):
    torch.cuda.synchronize()
    return det.keys().cpu().numpy().view(np.uint32)


def _check_scan(frames, H, W, offset=0):
    det = BarDetector("cuda:0")
    det.reset((H, W))
    env = R.empty(H, W)
    for host in frames:
        det.scan(_dev(host, offset), (H, W))
        env = R.scan(env, host, H, W)
    got, want = _keys(det), R.flat_words(env)
    diff = int((got != want).sum())
    print(f"{H}x{W} in {frames[0].shape[1]}x{frames[0].shape[2]} {frames[0].dtype} offset {offset}: {diff} of {want.size} words differ")
    assert got.size == want.size == 6 * (H + W) and diff == 0
    return det, env


# ---------------------------------------------------------------------------------- scan
SCAN_SHAPES = [(70, 98, 80, 112),                         # padding with NaN and 6e4 on both sides
               (16, 8, 16, 8),                            # smaller than any tile
               (1, 1, 1, 1),
               (STH - 1, STW - 1, STH, STW), (STH, STW, STH, STW),          # tile size - 1, the tile
               (STH + 1, STW + 1, STH + 8, STW + 8), (STH + 8, STW + 8, STH + 8, STW + 8),   # + 1 and + 8: a second tile each way
               (2 * STH + 3, 3 * STW + 5, 2 * STH + 8, 3 * STW + 8)]


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("H,W,Hp,Wp", SCAN_SHAPES)
def test_scan_equals_the_restatement(H, W, Hp, Wp, tdt, ndt):
    _check_scan([_frame(ndt, H, W, Hp, Wp, H * 1000 + W)], H, W)


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_scan_orders_negative_values_and_both_zeros(tdt, ndt):
    H, W = 40, 72
    host = _frame(ndt, H, W, 48, 80, 3)
    host[:, :H, :W] = np.random.default_rng(4).standard_normal((3, H, W)).astype(ndt) * ndt(100.0)
    host[0, 5, :W] = 0.0
    host[0, 5, 7] = -0.0                                   # a row of zeros whose min is -0
    host[1, :H, 9] = -0.0
    host[1, 11, 9] = 0.0                                   # a column of -0 whose max is +0
    host[2, 6, :W] = -np.abs(host[2, 6, :W]) - ndt(1.0)    # an all-negative row
    det, env = _check_scan([host], H, W)
    assert env[0][0, 5] == 0x7FFFFFFF and env[2][0, 5] == 0x80000000
    assert env[1][1, 9] == 0x7FFFFFFF and env[3][1, 9] == 0x80000000 and env[2][2, 6] < 0x7FFFFFFF


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_scan_accumulates_frames_and_reset_empties(tdt, ndt):
    H, W = 70, 98
    det, env = _check_scan([_frame(ndt, H, W, 80, 112, s) for s in (11, 12, 13)], H, W)
    one = R.scan(R.empty(H, W), _frame(ndt, H, W, 80, 112, 11), H, W)
    assert (R.flat_words(env) != R.flat_words(one)).any()                     # the later frames did widen it
    det.reset((H, W))
    assert np.array_equal(_keys(det), R.flat_words(R.empty(H, W)))
    det.scan(_dev(_frame(ndt, H, W, 80, 112, 11)), (H, W))
    assert np.array_equal(_keys(det), R.flat_words(one))


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_scan_from_an_unaligned_base_takes_the_narrow_form(tdt, ndt):
    H, W = 70, 98
    _check_scan([_frame(ndt, H, W, 80, 112, 21)], H, W, offset=1)
    _check_scan([_frame(ndt, H, W, 72, 100, 22)], H, W)                      # rows of 100: 16-byte rows in fp32 only


# ---------------------------------------------------------------------------------- extent
EH, EW = 48, 80
GREY = (0.5, 0.25, 0.75)
BLACK = (16 / 255, 128 / 255, 128 / 255)


def _barred(ndt, top, bottom, left, right, colour=BLACK, seed=0, noise=0.0):
    """content in [0.3, 0.9) between bars of `colour` (+- noise on the bars)"""
    rng = np.random.default_rng(seed)
    x = np.empty((3, EH, EW), np.float32)
    x[:] = np.asarray(colour, np.float32)[:, None, None]
    if noise:
        x += (rng.random((3, EH, EW), dtype=np.float32) - 0.5) * np.float32(2 * noise)
    x[:, top:EH - bottom, left:EW - right] = rng.random((3, EH - top - bottom, EW - left - right), dtype=np.float32) * 0.6 + 0.3
    return x.astype(ndt)


def _flat_picture(ndt):
    x = np.empty((3, EH, EW), ndt)
    x[:] = np.asarray(GREY, ndt)[:, None, None]
    return [x]


def _intrusion(ndt):
    frames = [_barred(ndt, 8, 8, 0, 0, seed=s) for s in range(5)]
    frames[3][:, 5:8, 30:34] = ndt(0.8)                    # a subtitle reaches 3 rows into the top bar in one frame
    return frames


NOISE = 2.0 / 255
EXTENT_CASES = {
    "letterbox": (lambda ndt: [_barred(ndt, 8, 6, 0, 0)], 0.0, (8, 6, 0, 0)),
    "pillarbox": (lambda ndt: [_barred(ndt, 0, 0, 10, 12)], 0.0, (0, 0, 10, 12)),
    "windowbox": (lambda ndt: [_barred(ndt, 4, 2, 6, 8)], 0.0, (4, 2, 6, 8)),
    "no_bars": (lambda ndt: [_barred(ndt, 0, 0, 0, 0)], 0.0, None),
    "bottom_only": (lambda ndt: [_barred(ndt, 0, 7, 0, 0)], 0.0, (0, 7, 0, 0)),
    "flat_picture": (_flat_picture, 0.0, (EH, EH, EW, EW)),
    "grey_bars": (lambda ndt: [_barred(ndt, 8, 8, 0, 0, GREY)], 0.0, (8, 8, 0, 0)),
    "noisy_bars_tol_0": (lambda ndt: [_barred(ndt, 8, 8, 0, 0, noise=NOISE)], 0.0, None),
    "noisy_bars_tol_above": (lambda ndt: [_barred(ndt, 8, 8, 0, 0, noise=NOISE)], 2.5 * NOISE, (8, 8, 0, 0)),
    "intrusion": (_intrusion, 0.0, (5, 8, 0, 0)),
}


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("case", list(EXTENT_CASES))
def test_extent_equals_the_restatement(case, tdt, ndt):
    make, tol, expect = EXTENT_CASES[case]
    frames = make(ndt)
    det, env = _check_scan(frames, EH, EW)
    tol = float(np.float32(tol))
    want = R.extent(env, tol)
    got = det.extents(tol)
    words = np.array(det._out)
    print(f"{case} {ndt.__name__}: kernel {words.tolist()}, restatement {want.tolist()}")
    assert np.array_equal(words, want)
    if expect is None:
        assert got is None and not want.any()
    else:
        assert got[:4] == expect and want[0] == 1
        assert np.array_equal(np.asarray(got[4], np.float32).view(np.int32), want[5:8])
        if case not in ("noisy_bars_tol_above",):
            colour = GREY if case in ("flat_picture", "grey_bars") else BLACK
            assert got[4] == tuple(float(np.float32(ndt(np.float32(c)))) for c in colour)
    assert det.extents(tol) == got                          # reading the extents leaves the envelope as it was


# ---------------------------------------------------------------------------------- window and paste
GUARD = 64
COLOUR = (16 / 255, 128 / 255, 0.7)
# (full H, W, Hp, Wp) -> (window HO, WO)
COPY_SHAPES = [((44, 70, 48, 80), (30, 52)),              # a pad of the output in both directions, a partial 8-pixel group
               ((20, 330, 24, 336), (16, 300))]           # two tiles of columns


def _guarded(shape, tdt):
    """an output tensor [1, 3, Hp, Wp] inside a larger allocation filled with a sentinel -> (tensor, check of the guards)"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), -7.0, dtype=tdt, device="cuda")
    out = flat[GUARD:GUARD + n].view(shape)
    out.fill_(float("nan"))
    assert out.data_ptr() % 16 == 0

    def intact():
        return bool((flat[:GUARD] == -7.0).all() and (flat[GUARD + n:] == -7.0).all())
    return out, intact


def _args(x, size):
    return (0 if x.dtype == torch.float16 else 1, ctypes.c_void_p(x.data_ptr()), x.shape[2], x.shape[3], *size)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("top", [0, 2])
@pytest.mark.parametrize("left", [0, 2, 4, 6, 8])             # (4: the 8-byte loads of fp16)
@pytest.mark.parametrize("full,win", COPY_SHAPES)
def test_window_and_paste_equal_the_restatement(full, win, left, top, offset, tdt, ndt):
    (H, W, Hp, Wp), (HO, WO) = full, win
    host = _frame(ndt, H, W, Hp, Wp, H + left + top)
    x = _dev(host, offset)
    out, intact = _guarded((1, 3, _pad(HO), _pad(WO)), tdt)
    rc = _lib.lib().dcvc_frame_window(*_args(x, (H, W)), top, left, ctypes.c_void_p(out.data_ptr()), out.shape[2], out.shape[3],
                                      HO, WO, _st())
    torch.cuda.synchronize()
    assert rc == 0 and intact()
    got = out[0].cpu().numpy()
    want = R.window(host, top, left, HO, WO, _pad(HO), _pad(WO))
    assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want))      # all written, no poison of the pad read

    # the window, in a frame with poisoned padding of its own, back into a full picture
    wh = _frame(ndt, HO, WO, _pad(HO), _pad(WO), 1)
    wh[:, :HO, :WO] = want[:, :HO, :WO]
    back, intact = _guarded((1, 3, Hp, Wp), tdt)
    colour = (ctypes.c_float * 3)(*COLOUR)
    rc = _lib.lib().dcvc_frame_paste(*_args(_dev(wh, offset), (HO, WO)), ctypes.c_void_p(back.data_ptr()), Hp, Wp, H, W, top, left,
                                     colour, _st())
    torch.cuda.synchronize()
    assert rc == 0 and intact()
    got = back[0].cpu().numpy()
    want = R.paste(wh, HO, WO, top, left, H, W, Hp, Wp, np.asarray(COLOUR, np.float32))
    assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[:, top:top + HO, left:left + WO]), _bits(host[:, top:top + HO, left:left + WO]))


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("top,bottom,left,right", [(8, 6, 0, 0), (0, 0, 10, 12), (4, 2, 6, 8), (0, 2, 2, 0)])
def test_paste_of_window_is_the_frame_bit_for_bit(top, bottom, left, right, tdt, ndt):
    host = _barred(ndt, top, bottom, left, right, GREY)
    x = _dev(host)
    det = BarDetector("cuda:0")
    det.reset((EH, EW))
    det.scan(x, (EH, EW))
    area = ActiveArea.from_extents(EH, EW, det.extents(), min_size=16)
    assert area.extents == [top, bottom, left, right]
    w = bars.window(x, (EH, EW), area)
    assert w.shape == (1, 3, _pad(EH - top - bottom), _pad(EW - left - right))
    back = bars.paste(w, area)
    assert back.shape == x.shape and torch.equal(back.view(torch.uint8), x.view(torch.uint8))


# ---------------------------------------------------------------------------------- end to end
H, W, N = 128, 160, 4
BAR = 32
PARAMS = GrainParams(4242, 1, (8, 40, 72, 104, 136, 168, 200, 255), 90, 160)


@pytest.fixture(scope="module")
def nets():
    from opendcvc_amd.models import DMC, DMCI
    out = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to("cuda").eval()
        m.update(0.12)
        out.append(m)
    return out


def _make_clips(d, side):
    """N frames of 128 x 160: synthetic content under 32-row bars of (16, 128, 128), and `side` columns of them at the left
    and right (0: 64 x 160 of content, 16: 64 x 128) -> (barred path, the content alone, barred bytes, the directory)"""
    barred, cropped = d / "barred.yuv", d / "cropped.yuv"
    with open(barred, "wb") as fb, open(cropped, "wb") as fc:
        for i in range(N):
            for k, plane in enumerate(weights.synthetic_frame_yuv420(H - 2 * BAR, W - 2 * side, i, 3)):
                b, c = (BAR, side) if k == 0 else (BAR // 2, side // 2)
                full = np.full((plane.shape[0] + 2 * b, plane.shape[1] + 2 * c), 16 if k == 0 else 128, np.uint8)
                full[b:b + plane.shape[0], c:c + plane.shape[1]] = plane
                fb.write(full.tobytes())
                fc.write(plane.tobytes())
    return str(barred), str(cropped), open(barred, "rb").read(), d


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    return _make_clips(tmp_path_factory.mktemp("bars"), 0)


def _planes(data, h, w):
    """the frames of a planar 4:2:0 file -> per frame (y, u, v)"""
    n = h * w * 3 // 2
    a = np.frombuffer(data, np.uint8).reshape(-1, n)
    return [(f[:h * w].reshape(h, w), f[h * w:h * w * 5 // 4].reshape(h // 2, w // 2), f[h * w * 5 // 4:].reshape(h // 2, w // 2))
            for f in a]


def _frames_of(data, n):
    rd = StreamReader(io.BytesIO(data))
    out = []
    for _ in range(n):
        sps, is_i, qp, payload = rd.read_frame()
        out.append((sps["height"], sps["width"], is_i, qp, payload, rd.active, rd.display, sps["sps_id"]))
    return out


# side 0: 64 x 160 of content under the 32-row bars, active_area [32, 32, 0, 0]; side 16: 64 x 128 of content, the SPS
# says 64 x 128, and the window starts 16 columns in
@pytest.mark.parametrize("side", [0, 16])
def test_crop_auto_end_to_end(nets, clips, side, tmp_path):
    from opendcvc_amd.bitstream import write_active
    from opendcvc_amd.pipeline import StreamDecoder, store_yuv420_frame
    barred, cropped, src_bytes, d = clips if side == 0 else _make_clips(tmp_path, side)
    CH, CW = H - 2 * BAR, W - 2 * side
    kw = dict(intra_period=2, verbose_json=True)
    log = harness.run_one_point(*nets, barred, W, H, N, 32, 32, crop="auto", bin_path=str(d / "auto.bin"),
                                rec_path=str(d / "auto.yuv"), **kw)
    plain = harness.run_one_point(*nets, cropped, CW, CH, N, 32, 32, bin_path=str(d / "plain.bin"),
                                  rec_path=str(d / "plain.yuv"), **kw)
    assert log["active_area"] == [BAR, BAR, side, side] and list(log)[-2:] == ["active_area", "bar_colour"]
    assert log["bar_colour"] == [float(np.float32(c) / np.float32(255)) for c in (16, 128, 128)]
    assert list(log)[:-2] == list(plain) and "active_area" not in plain
    assert log["frame_pixel_num"] == H * W and plain["frame_pixel_num"] == CH * CW         # per SOURCE pixel

    data, plain_data = open(d / "auto.bin", "rb").read(), open(d / "plain.bin", "rb").read()
    area = ActiveArea(H, W, BAR, side, CH, CW, tuple(log["bar_colour"]))
    got, want = _frames_of(data, N), _frames_of(plain_data, N)
    for g, p in zip(got, want):
        assert g[:2] == (CH, CW) and g[:5] == p[:5] and g[5] == area and p[5] is None and g[6] is None     # the SPS: the window
    n_sps = len({g[7] for g in got})                        # (use_ada_i 0 and 1: a unit behind each SPS, nothing else is new)
    assert len(data) == len(plain_data) + n_sps * write_active(io.BytesIO(), 0, area)
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data)

    rec, plain_rec = open(d / "auto.yuv", "rb").read(), open(d / "plain.yuv", "rb").read()
    assert len(rec) == len(src_bytes)
    for (y, u, v), (sy, su, sv), (py, pu, pv) in zip(_planes(rec, H, W), _planes(src_bytes, H, W), _planes(plain_rec, CH, CW)):
        for r, s, p, b, c in ((y, sy, py, BAR, side), (u, su, pu, BAR // 2, side // 2), (v, sv, pv, BAR // 2, side // 2)):
            assert np.array_equal(r[:b], s[:b]) and np.array_equal(r[-b:], s[-b:])          # the bars: the source's bytes
            assert np.array_equal(r[:, :c], s[:, :c]) and np.array_equal(r[:, r.shape[1] - c:], s[:, r.shape[1] - c:])
            assert np.array_equal(r[b:-b, c:r.shape[1] - c], p)                              # the window: the plain run's
    assert log["ave_all_frame_psnr"] > plain["ave_all_frame_psnr"]                          # (the bars are exact)

    # the container through the decode-side entry point alone
    decoder = StreamDecoder(io.BytesIO(data), *nets, "cuda:0")
    shown = b""
    for _ in range(N):
        frame = decoder.next()
        assert frame.active == area and frame.shown is frame.x_hat and frame.x_hat.shape == (1, 3, H, W)
        assert (frame.sps["height"], frame.sps["width"]) == (CH, CW)
        for plane in store_yuv420_frame(frame.shown, H, W):
            shown += plane.cpu().numpy().tobytes()
    decoder.flush()
    assert shown == rec


def test_crop_with_the_other_extensions(nets, clips):
    from opendcvc_amd.pipeline import StreamDecoder, store_yuv420_frame
    barred, _, src_bytes, d = clips
    log = harness.run_one_point(*nets, barred, W, H, N, 32, 32, intra_period=2, crop="auto", coded_size=(48, 96), film_grain=PARAMS,
                                digest=True, entropy="device", bin_path=str(d / "all.bin"), rec_path=str(d / "all.yuv"))
    assert log["digests_checked"] == N and (log["coded_height"], log["coded_width"]) == (48, 96)
    assert log["active_area"] == [BAR, BAR, 0, 0] and list(log)[-2:] == ["active_area", "bar_colour"]
    rec = open(d / "all.yuv", "rb").read()
    for (y, u, v), (sy, su, sv) in zip(_planes(rec, H, W), _planes(src_bytes, H, W)):
        for r, s, b in ((y, sy, BAR), (u, su, BAR // 2), (v, sv, BAR // 2)):
            assert np.array_equal(r[:b], s[:b]) and np.array_equal(r[-b:], s[-b:])          # no grain on the bars
    with open(d / "all.bin", "rb") as f:
        decoder = StreamDecoder(f, *nets, "cuda:0")
        shown = b""
        for _ in range(N):
            frame = decoder.next()
            assert (frame.sps["height"], frame.sps["width"]) == (48, 96) and frame.display == (H - 2 * BAR, W, "lanczos3")
            assert frame.active.extents == [BAR, BAR, 0, 0] and frame.grain == PARAMS
            assert frame.shown is not frame.x_hat and frame.x_hat.shape == frame.shown.shape == (1, 3, H, W)
            for plane in store_yuv420_frame(frame.shown, H, W):
                shown += plane.cpu().numpy().tobytes()
        decoder.flush()
        assert decoder.digests_checked == N
    assert shown == rec


def test_crop_none_is_the_stream_of_before_and_makes_no_detector(nets, clips, monkeypatch):
    barred, _, _, d = clips

    def refuse(*a, **k):
        raise AssertionError("constructed on the off path")
    monkeypatch.setattr(bars, "BarDetector", refuse)
    monkeypatch.setattr(bars, "window", refuse)
    monkeypatch.setattr(bars, "paste", refuse)
    a = harness.run_one_point(*nets, barred, W, H, N, 32, 32, intra_period=2, bin_path=str(d / "off_a.bin"))
    b = harness.run_one_point(*nets, barred, W, H, N, 32, 32, intra_period=2, crop=None, crop_tol=0.0, bin_path=str(d / "off_b.bin"))
    data = open(d / "off_a.bin", "rb").read()
    assert data == open(d / "off_b.bin", "rb").read()
    assert list(a) == list(b) and "active_area" not in a and "bar_colour" not in b
    assert all(f[5] is None and f[:2] == (H, W) for f in _frames_of(data, N))
    # nothing to find: the keys say so, no unit is written, the stream is the one of the option off
    monkeypatch.undo()
    clean = str(d / "clean.yuv")
    with open(clean, "wb") as f:
        for i in range(N):
            for plane in weights.synthetic_frame_yuv420(H, W, i, 3):
                f.write(plane.tobytes())
    off = harness.run_one_point(*nets, clean, W, H, N, 32, 32, intra_period=2, bin_path=str(d / "clean_off.bin"))
    on = harness.run_one_point(*nets, clean, W, H, N, 32, 32, intra_period=2, crop="auto", bin_path=str(d / "clean_on.bin"))
    assert open(d / "clean_off.bin", "rb").read() == open(d / "clean_on.bin", "rb").read()
    assert on["active_area"] == [0, 0, 0, 0] and on["bar_colour"] is None and list(on)[:-2] == list(off)
