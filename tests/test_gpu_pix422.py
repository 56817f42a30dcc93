"""4:2:2 frame I/O on the device (csrc/dcvc_pix422.hip) against the numpy restatement of tests/pix422_ref.py, bit for bit:
every format, both storage types, widths around one macropixel, one v210 group and one v210 unit of 24 pixels, pitched and
offset surfaces between canaries, the metric planes, and the harness with 4:2:2 sources."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import frame_io_place as P
import pix422_ref as R2
from opendcvc_amd import _lib, harness, pix422, weights
from opendcvc_amd import nn as L
from opendcvc_amd.metrics import DeviceMetrics
from opendcvc_amd.pipeline import load_frame

pytestmark = pytest.mark.gpu

# one macropixel, one group, W % 6 in {0, 2, 4}, W % 8 in {0, 2, 4, 6}, one v210 unit (24) exactly, just under and just over,
# two units and their neighbours
WIDTHS = (2, 4, 6, 8, 10, 22, 24, 26, 46, 48, 50)
HEIGHTS = (1, 2, 3)
DTYPES = {"f16": (np.float16, torch.float16), "f32": (np.float32, torch.float32)}
NAMES = sorted(R2.FORMATS)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def raw_load(name, tdt, ptrs, ys, cs, h, w, pb, pr):
    """dcvc_yuv422_to_frame on plain addresses -> the frame [1, 3, h + pb, w + pr] on the host"""
    out = torch.empty((1, 3, h + pb, w + pr), dtype=tdt, device="cuda")
    ptrs = [ctypes.c_void_p(p) if p is not None else None for p in ptrs] + [None] * (3 - len(ptrs))
    _lib.check(_lib.lib().dcvc_yuv422_to_frame(L.dtype_code(tdt), R2.LAYOUT[R2.packing_of(name)], R2.bits_of(name), *ptrs, ys, cs,
                                               h, w, pb, pr, L._p(out), L._stream()), "dcvc_yuv422_to_frame")
    return host(out)


def raw_store(name, x, h, w, ptrs, ys, cs):
    ptrs = [ctypes.c_void_p(p) if p is not None else None for p in ptrs] + [None] * (3 - len(ptrs))
    code, *frame = L.frame_args(x, (h, w))
    _lib.check(_lib.lib().dcvc_frame_to_yuv422(code, R2.LAYOUT[R2.packing_of(name)], R2.bits_of(name), *frame, *ptrs, ys, cs,
                                               L._stream()), "dcvc_frame_to_yuv422")
    torch.cuda.synchronize()


def tight_strides(name, w):
    return (w, w // 2) if R2.packing_of(name) == "planar" else (R2.row_bytes(name, w), 0)


def same(a, b):
    """bit identity, NaN patterns included"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- tight frames, every size
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", NAMES)
def test_load_is_the_restatement(name, dt):
    ndt, tdt = DTYPES[dt]
    bits = R2.bits_of(name)
    rng = np.random.default_rng(100 + bits + len(name))
    for h in HEIGHTS:
        for w in WIDTHS:
            frame = R2.pack(R2.random_planes(rng, h, w, bits), name)
            on_dev = [dev(p) for p in frame]
            got = host(pix422.load_frame_422(on_dev, name, tdt, pad_to=16, width=w))
            assert same(got, R2.load_ref(frame, name, ndt, w, pad_to=16)), (h, w)
            # an explicit pad of 0 rows and 8 columns past the next multiple of 8: with W = 24 the frame is 32 wide and the
            # second v210 thread of a row owns nothing but padding
            pr = (-w) % 8 + 8
            got = raw_load(name, tdt, [t.data_ptr() for t in on_dev], *tight_strides(name, w), h, w, 0, pr)
            assert same(got, R2.load_ref(frame, name, ndt, w, pad=(0, pr))), (h, w, pr)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", NAMES)
def test_store_is_the_restatement(name, dt):
    ndt, tdt = DTYPES[dt]
    bits = R2.bits_of(name)
    rng = np.random.default_rng(200 + bits + len(name))
    for h in HEIGHTS:
        for w in WIDTHS:
            pic = P.random_picture(rng, h, w, ndt, (1 << bits) - 1)
            for hp, wp in ((h + (-h) % 16, w + (-w) % 16), (h, w + (-w) % 8 + 8)):
                x = P.poisoned_frame(pic, hp, wp)                      # NaN everywhere outside the picture
                got = pix422.store_frame_422(dev(x), h, w, name)
                want = R2.store_ref(x, h, w, name)
                assert len(got) == len(want)
                for g, wnt in zip(got, want):
                    assert same(host(g), np.ascontiguousarray(wnt)), (h, w, hp, wp)
                if name == "v210":                                     # the filler inside row_bytes is zero, bits 30 and 31 too
                    s = host(got[0])
                    assert s.shape == (h, R2.row_bytes(name, w))
                    words = s.view("<u4")
                    assert not (words >> 30).any() and not words[:, 4 * ((w + 5) // 6):].any()


# ------------------------------------------------------------------------------------------- placement
PLANAR_PLACEMENTS = [P.PLANAR_PLACEMENTS[k] for k in (0, 1, 2, 3, 4, 6, 8, 10, 11, 14)]
PACKED_PLACEMENTS = [(extra, off) for extra in (0, 4, 8, 16) for off in (0, 4, 8, 16)]          # bytes
V210_PLACEMENTS = [(extra, off) for extra in (0, 16, 128) for off in (0, 16, 128)]
PLACED_SIZES = ((3, 26), (2, 48), (1, 6), (2, 10))


def packed_class(pitch, offset):
    """docs/pixel_formats_422.md: the widest of 16, 8 and 4 bytes that divides the surface's address and its pitch"""
    return next(b for b in (16, 8, 4) if pitch % b == 0 and offset % b == 0)


def placements(name):
    packing = R2.packing_of(name)
    return PLANAR_PLACEMENTS if packing == "planar" else (V210_PLACEMENTS if packing == "v210" else PACKED_PLACEMENTS)


def test_the_tables_reach_every_access_class():
    """on the CPU: every class of the planar rule (restated in frame_io_place.expected_class: 4:2:2 planes follow the planar
    4:2:0 rule, luma in 8-sample and chroma in 4-sample pieces) and of the packed rule is reached by a picture wider than the
    8 pixels of one thread"""
    wide = [(h, w) for h, w in PLACED_SIZES if w > 8]
    for es in (1, 2):
        reached = set()
        for h, w in wide:
            for ey, ec, oy, ou, ov in PLANAR_PLACEMENTS:
                reached.add(P.expected_class("420p", es, [oy * es, ou * es, ov * es], w + ey, w // 2 + ec))
        assert reached == {8, 4, 2, 1}, (es, reached)
    reached = {packed_class(2 * w + extra, off) for h, w in wide for extra, off in PACKED_PLACEMENTS}
    assert reached == {16, 8, 4}
    assert all((R2.row_bytes("v210", w) + extra) % 16 == 0 and off % 16 == 0 for _, w in wide for extra, off in V210_PLACEMENTS)


def geometry(name, h, w, placement):
    """[(rows, row bytes, pitch bytes, offset bytes)] of every plane / of the surface"""
    if R2.packing_of(name) == "planar":
        es = R2.sample_dtype(R2.bits_of(name)).itemsize
        ey, ec, oy, ou, ov = placement
        return [(h, w * es, (w + ey) * es, oy * es), (h, w // 2 * es, (w // 2 + ec) * es, ou * es),
                (h, w // 2 * es, (w // 2 + ec) * es, ov * es)]
    extra, off = placement
    rb = R2.row_bytes(name, w)
    return [(h, rb, rb + extra, off)]


def entry_strides(name, geo):
    if R2.packing_of(name) == "planar":
        es = R2.sample_dtype(R2.bits_of(name)).itemsize
        return geo[0][2] // es, geo[1][2] // es
    return geo[0][2], 0


@pytest.mark.parametrize("name", NAMES)
def test_load_reads_pitched_and_offset_surfaces(name):
    bits = R2.bits_of(name)
    rng = np.random.default_rng(300 + bits + len(name))
    for h, w in PLACED_SIZES:
        frame = R2.pack(R2.random_planes(rng, h, w, bits), name)
        for placement in placements(name):
            geo = geometry(name, h, w, placement)
            es = frame[0].dtype.itemsize
            placed = [P.Placed(P.pitched_image(p, pitch // es, rng), off, rng) for p, (_, _, pitch, off) in zip(frame, geo)]
            for ndt, tdt in DTYPES.values():
                got = raw_load(name, tdt, [pl.ptr for pl in placed], *entry_strides(name, geo), h, w, 2, (-w) % 8)
                assert same(got, R2.load_ref(frame, name, ndt, w, pad=(2, (-w) % 8))), (h, w, placement)


@pytest.mark.parametrize("name", NAMES)
def test_store_touches_nothing_but_its_samples(name):
    bits = R2.bits_of(name)
    rng = np.random.default_rng(400 + bits + len(name))
    for h, w in PLACED_SIZES:
        for k, placement in enumerate(placements(name)):
            geo = geometry(name, h, w, placement)
            ndt, tdt = list(DTYPES.values())[k % 2]
            x = P.poisoned_frame(P.random_picture(rng, h, w, ndt, (1 << bits) - 1), h + 1, w + (-w) % 8)
            want = R2.store_ref(x, h, w, name)
            for fill in P.FILLS:
                bufs = [P.guarded(P.plane_nbytes(rows, rb, pitch), off, fill) for rows, rb, pitch, off in geo]
                raw_store(name, dev(x), h, w, [b.ptr for b in bufs], *entry_strides(name, geo))
                for b, wnt, (rows, rb, pitch, _) in zip(bufs, want, geo):
                    b.check(P.plane_mask(rows, rb, pitch))             # canaries and pitch gaps intact
                    assert same(P.plane_rows(b.read(), rows, rb, pitch, wnt.dtype), np.ascontiguousarray(wnt)), (h, w, placement)


# ------------------------------------------------------------------------------------------- one picture, several formats
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("family,ref444", [(("yuv422p", "uyvy422", "yuyv422"), "yuv444p"), (("yuv422p10le", "v210"), "yuv444p10le")])
def test_formats_of_the_same_samples_load_alike(family, ref444, dt):
    _, tdt = DTYPES[dt]
    bits = R2.bits_of(family[0])
    rng = np.random.default_rng(bits)
    for h, w in ((3, 50), (2, 24), (5, 70)):
        planes = R2.random_planes(rng, h, w, bits)
        doubled = [planes[0], np.repeat(planes[1], 2, axis=1), np.repeat(planes[2], 2, axis=1)]
        want = host(load_frame([dev(p) for p in doubled], ref444, tdt))
        for name in family:
            got = host(pix422.load_frame_422([dev(p) for p in R2.pack(planes, name)], name, tdt, width=w))
            assert same(got, want), (name, h, w)


# ------------------------------------------------------------------------------------------- metrics
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_metric_planes_are_the_restatement(dt):
    ndt, tdt = DTYPES[dt]
    rng = np.random.default_rng(7)
    dm = DeviceMetrics("cuda:0")
    for name in ("yuv422p", "v210", "yuv422p16le"):
        fmt = pix422.Format422.parse(name)
        for h, w in ((3, 26), (1, 2), (37, 50), (2, 48)):
            x = P.poisoned_frame(P.random_picture(rng, h, w, ndt, fmt.max_val), h + 3, w + (-w) % 8)
            got = dm.metric_planes(dev(x), h, w, fmt)
            torch.cuda.synchronize()
            for g, want in zip(got, R2.metric_planes_ref(x, h, w, fmt.bit_depth)):
                assert g.dtype == torch.float32 and same(host(g), want), (name, h, w)


def test_device_metrics_of_a_v210_surface_equal_the_planar_ones():
    rng = np.random.default_rng(11)
    h, w = 90, 182                                   # (chroma planes of 90 x 91: MS-SSIM takes 88 and up)
    planes = R2.random_planes(rng, h, w, 10)
    x = torch.from_numpy(R2.load_ref(planes, "yuv422p10le", np.float32))
    noisy = (x + torch.from_numpy(rng.normal(0, 0.01, tuple(x.shape)).astype(np.float32))).half().cuda()
    dm = DeviceMetrics("cuda:0")
    planar = dm.yuv(noisy, [dev(p) for p in planes], pix422.Format422.parse("yuv422p10le"), True, w)
    packed = dm.yuv(noisy, [dev(R2.pack(planes, "v210")[0])], pix422.Format422.parse("v210"), True, w)
    assert planar == packed and 30 < planar[0][1] < 50 and 0 < planar[1][1] <= 1
    on_host = harness.pixfmt_distortion(noisy, [dev(R2.pack(planes, "v210")[0])], pix422.Format422.parse("v210"), True, w)
    # (the bounds tests/test_gpu_pixfmt.py holds the two paths to: both compare the same fp32 planes)
    assert all(abs(a - b) <= 1e-9 for a, b in zip(planar[0], on_host[0])), (planar, on_host)
    assert all(abs(a - b) <= 1e-12 for a, b in zip(planar[1], on_host[1])), (planar, on_host)


# ------------------------------------------------------------------------------------------- the harness
H, W, N = 96, 128, 4


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


def clip_planes(h, w, i, bits):
    """frame i of a synthetic clip as low-aligned planar 4:2:2 samples"""
    y, u, v = weights.synthetic_frame_yuv420(h, w, i, 3)
    shift = bits - 8
    return [(p.astype(np.uint16) << shift).astype(R2.sample_dtype(bits)) for p in (y, np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0))]


def write_clip(path, frames):
    with open(path, "wb") as f:
        for frame in frames:
            for p in frame:
                f.write(np.ascontiguousarray(p).tobytes())


def test_a_uyvy_clip_codes_like_the_444_clip_with_doubled_chroma(nets, tmp_path):
    clip = [clip_planes(H, W, i, 8) for i in range(N)]
    write_clip(tmp_path / "a.uyvy", [R2.pack(p, "uyvy422") for p in clip])
    write_clip(tmp_path / "a.444", [[y, np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1)] for y, u, v in clip])
    logs = {}
    for src_type, ext in (("uyvy422", "uyvy"), ("yuv444p", "444")):
        logs[src_type] = harness.run_one_point(nets[0], nets[1], str(tmp_path / f"a.{ext}"), W, H, N, 32, 32, intra_period=2,
                                               src_type=src_type, metrics="device", verbose_json=True,
                                               bin_path=str(tmp_path / f"{ext}.bin"))
    assert open(tmp_path / "uyvy.bin", "rb").read() == open(tmp_path / "444.bin", "rb").read()
    assert logs["uyvy422"]["frame_bpp"] == logs["yuv444p"]["frame_bpp"] and list(logs["uyvy422"]) == list(logs["yuv444p"])
    assert logs["uyvy422"]["frame_psnr"] != logs["yuv444p"]["frame_psnr"]          # (4:2:2 chroma planes are what is measured)
    assert all(math.isfinite(v) and 0 < v < 99 for v in logs["uyvy422"]["frame_psnr"])       # (synthetic weights: a few dB)


def test_a_v210_run_saves_its_reconstruction_as_v210(nets, tmp_path):
    clip = [clip_planes(H, W, i, 10) for i in range(N)]
    write_clip(tmp_path / "a.v210", [R2.pack(p, "v210") for p in clip])
    rec = str(tmp_path / "rec.v210")
    log = harness.run_one_point(nets[0], nets[1], str(tmp_path / "a.v210"), W, H, N, 32, 32, src_type="v210", metrics="device",
                                bin_path=str(tmp_path / "a.bin"), rec_path=rec)
    rb = R2.row_bytes("v210", W)
    assert os.path.getsize(rec) == N * H * rb
    reader = pix422.Raw422Reader(rec, W, H, "v210")
    for i in range(N):
        (s,) = reader.read()
        assert s.shape == (H, rb) and not (s.view("<u4") >> 30).any() and not s[:, 16 * ((W + 5) // 6):].any()
        assert [p.shape for p in R2.unpack([s], "v210", W)] == [(H, W), (H, W // 2), (H, W // 2)]
    with pytest.raises(EOFError):
        reader.read()
    reader.close()
    assert math.isfinite(log["ave_all_frame_psnr"])


def test_a_uyvy_clip_deinterlaces_at_a_height_that_is_no_multiple_of_4(nets, tmp_path):
    h = 98
    write_clip(tmp_path / "i.uyvy", [R2.pack(clip_planes(h, W, i, 8), "uyvy422") for i in range(N)])
    log = harness.run_one_point(nets[0], nets[1], str(tmp_path / "i.uyvy"), W, h, N, 32, 32, src_type="uyvy422", metrics="device",
                                deinterlace="on")
    assert log["deinterlace"] == "on" and math.isfinite(log["ave_all_frame_psnr"]) and 0 < log["ave_all_frame_psnr"] < 99
    with pytest.raises(ValueError, match="multiple of 4"):
        harness.run_one_point(nets[0], nets[1], str(tmp_path / "i.uyvy"), W, h, N, 32, 32, src_type="yuv420p10le", deinterlace="on")
