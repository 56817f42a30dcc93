"""Deinterlacing on the GPU (docs/deinterlace.md): dcvc_deinterlace and dcvc_comb_detect of csrc/dcvc_deint.hip against the
numpy restatement (tests/deint_ref.py) bit for bit, in fp16 and fp32, deinterlace.Deinterlacer's state, and the option end to
end through the harness."""
import ctypes

import numpy as np
import pytest
import torch

import deint_ref as R
from opendcvc_amd import _lib, bars, deinterlace, harness, weights
from opendcvc_amd.deinterlace import Deinterlacer
from opendcvc_amd.pipeline import store_yuv420_frame

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.float32, np.float32, id="fp32"), pytest.param(torch.float16, np.float16, id="fp16")]
# (H, W, Hp, Wp): one missing chroma line, every row offset reflects or collapses; narrower than the +-3 column reach; padding
# both ways; a cut last tile and rows that are 16-byte aligned in fp32 only; many workgroups, no padding
SHAPES = [(4, 8, 16, 8), (8, 3, 16, 8), (40, 72, 48, 80), (68, 100, 80, 104), (272, 480, 272, 480)]
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


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
    """a smooth texture plus a little noise in a frame whose padding holds the poison values, alternating"""
    host = np.empty((3, Hp, Wp), ndt)
    host[:, ::2], host[:, 1::2] = poison
    rng = np.random.default_rng(seed)
    pic = np.stack([R.texture(H, W, seed * 3 + p, 1) for p in range(3)]) + rng.normal(0.0, 0.02, (3, H, W))
    host[:, :H, :W] = pic.astype(ndt)
    return host


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(cur, prev, H, W, parity, lines, decision=None):
    """dcvc_deinterlace into an output full of poison -> numpy [3, Hp, Wp]"""
    out = torch.full(cur.shape, float("nan"), dtype=cur.dtype, device="cuda")
    rc = _lib.lib().dcvc_deinterlace(0 if cur.dtype == torch.float16 else 1, P(cur), P(prev), cur.shape[2], cur.shape[3], H, W,
                                     parity, lines, P(decision), P(out), _stream())
    assert rc == 0, _lib.lib().dcvc_last_error()
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


# ---------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("H,W,Hp,Wp", SHAPES)
def test_deinterlace_equals_the_restatement(H, W, Hp, Wp, tdt, ndt):
    seed = H * 1000 + W
    # the two frames' padding holds NaN where the other's holds 6e4: a padding sample read would show in the picture
    cur, prev = _frame(ndt, H, W, Hp, Wp, seed), _frame(ndt, H, W, Hp, Wp, seed + 1, poison=(6e4, np.nan))
    words = torch.tensor([0, 1, 7], dtype=torch.int32, device="cuda")            # decision words: pass, filter, filter
    word = lambda k: words[k:k + 1]
    passed = R.deinterlace(cur, None, H, W, 0, 1, decision=0)
    assert np.array_equal(_bits(passed[:, :H, :W]), _bits(cur[:, :H, :W]))
    for offset in (0, 1):
        dc, dp = _dev(cur, offset), _dev(prev, offset)
        for parity in (0, 1):
            for lines in (1, 2):
                for p_host, p_dev in ((None, None), (prev, dp)):
                    want = R.deinterlace(cur, p_host, H, W, parity, lines)
                    assert np.isfinite(want.astype(np.float32)).all() and want.shape == (3, Hp, Wp)
                    what = f"offset {offset} parity {parity} chroma_lines {lines} prev {p_host is not None}"
                    for decision in ((None, word(1), word(2)) if not offset else (None,)):
                        got = _run(dc, p_dev, H, W, parity, lines, decision)
                        bad = int((_bits(got) != _bits(want)).sum())
                        print(f"{what} decision {None if decision is None else int(decision)}: {bad} samples differ")
                        assert bad == 0, what
                    kept = [y for y in range(H) if (y // 1) % 2 == parity]
                    assert np.array_equal(_bits(want[0, kept, :W]), _bits(cur[0, kept, :W]))       # the first field's bits
                got = _run(dc, dp, H, W, parity, 2, word(0))                     # found progressive: cur and its pad
                assert np.array_equal(_bits(got), _bits(passed)), f"offset {offset} parity {parity}: pass through"
        if offset:                                         # one aligned address does not allow the 16-byte form
            want = R.deinterlace(cur, prev, H, W, 0, 2)
            assert np.array_equal(_bits(_run(_dev(cur), dp, H, W, 0, 2)), _bits(want)), "only prev off"
            assert np.array_equal(_bits(_run(dc, _dev(prev), H, W, 0, 2)), _bits(want)), "only cur off"


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_a_static_monotone_picture_is_a_copy_and_alternating_lines_are_flattened(tdt, ndt):
    H, W, Hp, Wp = 40, 72, 48, 80
    ramp = np.cumsum(np.random.default_rng(3).random((3, H, W)) + 0.05, axis=1)
    ramp = (ramp / ramp.max()).astype(ndt)
    ramp[1:] = np.repeat(ramp[1:, ::2], 2, 1)                # chroma as a 4:2:0 loader leaves it: rows in pairs
    x = R.replicate_pad(ramp, Hp, Wp)
    for lines in (1, 2):
        got = _run(_dev(x), _dev(x), H, W, 0, lines)
        assert np.array_equal(_bits(got), _bits(x)), lines
    comb = np.zeros((3, Hp, Wp), ndt)
    comb[:, 0::2], comb[:, 1::2] = 0.25, 0.75                # the known limit: a static comb cannot be told from a moving one
    got = _run(_dev(comb), _dev(comb), H, W, 0, 1)
    assert np.array_equal(_bits(got), _bits(R.deinterlace(comb, comb, H, W, 0, 1))) and (got == ndt(0.25)).all()


# ---------------------------------------------------------------------------------- the decision
class _Detect:
    def __init__(self):
        self.lib = _lib.lib()
        assert self.lib.dcvc_comb_ws_bytes() == 64
        self.ws = torch.zeros(8, dtype=torch.int64, device="cuda")
        self.words = torch.full((8,), 0x55, dtype=torch.int32, device="cuda")

    def call(self, cur, prev, H, W, parity, slot=0):
        rc = self.lib.dcvc_comb_detect(0 if cur.dtype == torch.float16 else 1, P(cur), P(prev), cur.shape[2], cur.shape[3], H, W,
                                       parity, P(self.ws), ctypes.c_void_p(self.words.data_ptr() + 4 * slot), _stream())
        assert rc == 0, self.lib.dcvc_last_error()

    def read(self):
        torch.cuda.synchronize()
        return self.words.cpu().tolist(), self.ws.cpu().tolist()


def _clip_frames(kinds, H, W, Hp, Wp, ndt, parity=0, lines=1, speed=3):
    """one moving scene, frame t of kind kinds[t], as model frames with NaN padding"""
    clips = {k: R.make_clip(k, len(kinds), H, W, speed=speed, seed=5, parity=parity, chroma_lines=lines, blur=1)[0] for k in set(kinds)}
    return [R.to_frame(clips[k][t], ndt, Hp, Wp, pad=np.nan) for t, k in enumerate(kinds)]


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("H,W,Hp,Wp", SHAPES[2:])
def test_comb_detect_equals_the_restatement(H, W, Hp, Wp, tdt, ndt):
    kinds = ["progressive", "progressive", "interlaced", "interlaced", "interlaced"]
    for parity in (0, 1):
        frames = _clip_frames(kinds, H, W, Hp, Wp, ndt, parity)
        for offset in (0, 1):
            det = _Detect()
            dev = [_dev(f, offset) for f in frames]
            want, judged, found = [], 0, 0
            for t in range(5):
                prev = frames[t - 1] if t else None
                want.append(R.comb_decision(frames[t], prev, H, W, parity))
                det.call(dev[t], dev[t - 1] if t else None, H, W, parity, slot=t)
                words, ws = det.read()
                judged, found = judged + 1, found + want[-1]
                print(f"frame {t} ({kinds[t]}): sums {R.comb_sums(frames[t], prev, H, W, parity)}, decision {words[t]}, want {want[-1]}")
                assert words[t] == want[-1] and ws == [0, 0, 0, judged, found, 0, 0, 0], (t, words, ws)
            assert want[1] == 0 and want[3:] == [1, 1]                           # both classes occur
            # two calls back to back, nothing in between: the first one left the sums zero
            det.call(dev[1], dev[0], H, W, parity, slot=5)
            det.call(dev[4], dev[3], H, W, parity, slot=6)
            words, ws = det.read()
            assert words[5:7] == [want[1], want[4]] and ws == [0, 0, 0, 7, found + want[1] + want[4], 0, 0, 0]


# ---------------------------------------------------------------------------------- the object
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("mode", ["on", "auto"])
def test_deinterlacer_follows_the_restatement(mode, tdt, ndt):
    H, W, Hp, Wp = 40, 72, 48, 80
    kinds = ["progressive", "progressive", "interlaced", "interlaced", "progressive", "interlaced"]
    frames = _clip_frames(kinds, H, W, Hp, Wp, ndt, parity=1, lines=2)
    small = _clip_frames(kinds[:2], 36, 64, Hp, Wp, ndt, parity=1, lines=2)
    dev, ref = Deinterlacer("cuda:0", mode, "bff", 2), R.Deinterlacer(mode, "bff", 2)

    def step(x, size, what):
        got = dev.filter(_dev(x), size)
        assert got.shape == (1, 3, Hp, Wp) and got.dtype == tdt
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(ref.filter(x, size))), what

    for t in range(4):
        step(frames[t], (H, W), f"frame {t}")
    dev.reset()
    ref.reset()
    step(frames[4], (H, W), "after reset(): no previous frame")
    step(frames[5], (H, W), "frame 5")
    step(small[0], (36, 64), "another size: no previous frame")
    step(small[1], (36, 64), "the second frame of that size")
    assert dev.frames == 8 and dev.counts() == (ref.counts() if mode == "auto" else (0, 0))
    assert dev.filtered() == (ref.counts()[1] if mode == "auto" else 8)
    with pytest.raises(ValueError, match="multiple of 4"):
        dev.filter(_dev(frames[0]), (38, W))


# ---------------------------------------------------------------------------------- end to end
H, W = 128, 160


def _make_nets():
    from opendcvc_amd.models import DMC, DMCI
    out = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to("cuda").eval()
        m.update(0.12)
        out.append(m)
    return out


@pytest.fixture(scope="module")
def nets():
    return _make_nets()


def _write(path, frames):
    with open(path, "wb") as f:
        for planes in frames:
            for plane in planes:
                f.write(np.ascontiguousarray(plane, np.uint8).tobytes())
    return str(path)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("deint")
    return {kind: _write(d / f"{kind}.yuv", R.make_clip(kind, 4, H, W, speed=4, seed=11, chroma_lines=2, blur=1)[0])
            for kind in ("interlaced", "progressive")}


class _Spy:
    """what the passes saw: the model frames of the loader, the front end's inputs and the planes the metrics were held against"""

    def __init__(self, monkeypatch):
        self.loaded, self.fed, self.measured = [], [], []
        make_source, front_input = harness.make_source, harness._front_input

        def spy_source(*a):
            src = make_source(*a)
            to_input, distortion = src.to_input, src.distortion
            src.to_input = lambda planes, dt: self.loaded.append(to_input(planes, dt)) or self.loaded[-1]
            src.distortion = lambda x, p, ssim, dm: self.measured.append([t.cpu().numpy() for t in p]) or distortion(x, p, ssim, dm)
            return src

        def spy_input(*a):
            self.fed.append(front_input(*a))
            return self.fed[-1]

        monkeypatch.setattr(harness, "make_source", spy_source)
        monkeypatch.setattr(harness, "_front_input", spy_input)


def _stored(pic):
    """the model frame pic [3, H, W] (numpy) as a planar 8-bit 4:2:0 file holds it"""
    return [p.cpu().numpy() for p in store_yuv420_frame(torch.from_numpy(pic[None]).cuda(), H, W)]


@pytest.mark.parametrize("mode", ["on", "auto"])
def test_run_one_point_codes_the_restatements_pictures(nets, clips, tmp_path, monkeypatch, mode):
    spy = _Spy(monkeypatch)
    log = harness.run_one_point(*nets, clips["interlaced"], W, H, 4, 32, 32, deinterlace=mode, field_order="tff", verbose_json=True,
                                bin_path=str(tmp_path / "d.bin"))
    assert list(log)[-3:] == ["deinterlace", "field_order", "deint_frames"] and (log["deinterlace"], log["field_order"]) == (mode, "tff")
    assert len(log["frame_psnr"]) == 4 and all(np.isfinite(p) and p > 0.0 for p in log["frame_psnr"])       # the stream decodes
    assert len(spy.loaded) == 8 and len(spy.fed) == 4 and len(spy.measured) == 4                # both passes load every frame
    ref = R.Deinterlacer(mode, "tff", 2)
    for t in range(4):
        x = spy.loaded[t][0].cpu().numpy()
        assert np.array_equal(x, spy.loaded[4 + t][0].cpu().numpy())
        want = ref.filter(x, (H, W))
        assert np.array_equal(_bits(spy.fed[t][0].cpu().numpy()), _bits(want)), t                # what the encoder was fed
        for got, plane in zip(spy.measured[t], _stored(want)):                                  # what the metrics compared
            assert got.dtype == np.uint8 and np.array_equal(got, plane), t
    assert log["deint_frames"] == (4 if mode == "on" else ref.counts()[1])
    print(f"{mode}: deint_frames {log['deint_frames']}, the restatement's decisions {ref.counts()}")
    if mode == "auto":                                      # (the first-frame rule and the rule with a previous frame both say so)
        assert ref.counts() == (4, 4)


def test_off_is_off_and_auto_passes_a_progressive_clip(nets, clips, tmp_path, monkeypatch):
    kw = dict(intra_period=2, verbose_json=True)
    auto = harness.run_one_point(*nets, clips["progressive"], W, H, 4, 32, 32, deinterlace="auto", bin_path=str(tmp_path / "auto.bin"), **kw)

    def refuse(*a, **k):
        raise AssertionError("constructed on the off path")
    monkeypatch.setattr(deinterlace, "Deinterlacer", refuse)
    a = harness.run_one_point(*nets, clips["progressive"], W, H, 4, 32, 32, bin_path=str(tmp_path / "a.bin"), **kw)
    b = harness.run_one_point(*nets, clips["progressive"], W, H, 4, 32, 32, deinterlace=None, field_order="tff",
                              bin_path=str(tmp_path / "b.bin"), **kw)
    data = open(tmp_path / "a.bin", "rb").read()
    assert data == open(tmp_path / "b.bin", "rb").read()
    assert list(a) == list(b) and not {"deinterlace", "field_order", "deint_frames"} & set(a)
    assert {k: v for k, v in a.items() if k != "test_time"} == {k: v for k, v in b.items() if k != "test_time"}
    # a progressive clip under auto: the first-frame rule (dc > ds) finds frame 0 progressive too - its lines are smoother one
    # row apart than two rows apart - so no frame is filtered and the WHOLE stream is the one of the option off
    assert auto["deint_frames"] == 0 and list(auto)[:-3] == list(a)
    assert open(tmp_path / "auto.bin", "rb").read() == data
    assert auto["frame_psnr"] == a["frame_psnr"] and auto["frame_bpp"] == a["frame_bpp"]


def test_deinterlace_with_a_crop_the_temporal_filter_and_frame_dup(nets, tmp_path, monkeypatch):
    frames = R.make_clip("interlaced", 3, H - 12, W, speed=4, seed=12, chroma_lines=2, blur=1)[0]
    barred = []
    for planes in [frames[0], frames[0], frames[1], frames[2]]:                 # a repeated source frame; bars of 6 and 6 rows
        full = [np.full((H // s, W // s), c, np.uint8) for s, c in ((1, 16), (2, 128), (2, 128))]
        for dst, src, s in zip(full, planes, (1, 2, 2)):
            dst[6 // s:6 // s + src.shape[0]] = src
        barred.append(full)
    clip = _write(tmp_path / "barred.yuv", barred)
    spy = _Spy(monkeypatch)
    # top offset 6: three chroma lines - a window cut first would flip the chroma planes' field parity
    log = harness.run_one_point(*nets, clip, W, H, 4, 32, 32, deinterlace="on", crop=(6, 6, 0, 0, (16, 128, 128)), temporal_filter=3,
                                frame_dup=True, verbose_json=True)
    assert log["deint_frames"] == 4 and log["active_area"] == [6, 6, 0, 0] and log["tf_level"] == 3
    assert len(log["frame_psnr"]) == 4 and all(np.isfinite(p) and p > 0.0 for p in log["frame_psnr"])
    area = bars.ActiveArea.from_manual(H, W, (6, 6, 0, 0), [float(np.float32(c) / np.float32(255.0)) for c in (16, 128, 128)])
    ref = R.Deinterlacer("on", "tff", 2)
    for t in range(4):
        want = ref.filter(spy.loaded[t][0].cpu().numpy(), (H, W))
        got = spy.fed[t][0, :, :H - 12, :W].cpu().numpy()
        assert spy.fed[t].shape[-2:] == (H - 12 + (-(H - 12)) % 16, W)
        assert np.array_equal(_bits(got), _bits(want[:, 6:H - 6, :W])), t        # the window of the FULL frame's filter
    # frame 1 repeats frame 0 in the source, but its previous frame differs from frame 0's (none): no bit repeat behind the
    # filter (docs/deinterlace.md), and the detector, which sees the filtered pictures, says so
    same = np.array_equal(spy.fed[0].cpu().numpy(), spy.fed[1].cpu().numpy())
    assert log["frame_repeat"] == [0, int(same), 0, 0] and area.size == (H - 12, W)
