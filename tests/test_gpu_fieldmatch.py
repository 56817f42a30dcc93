"""The deinterlacer's film mode on the GPU (docs/deinterlace.md, "Film mode"): dcvc_field_match and dcvc_field_weave of
csrc/dcvc_fieldmatch.hip against the numpy restatement (tests/fieldmatch_ref.py) bit for bit, in fp16 and fp32,
deinterlace.Deinterlacer("film") on clips whose class is known, and the mode end to end through the harness, where with
frame_dup it is an inverse telecine."""
import ctypes

import numpy as np
import pytest
import torch

import deint_ref as R
import fieldmatch_ref as M
from opendcvc_amd import _lib, deinterlace, harness, weights
from opendcvc_amd.deinterlace import Deinterlacer

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.float32, np.float32, id="fp32"), pytest.param(torch.float16, np.float16, id="fp16")]
# test_gpu_deint's (H, W, Hp, Wp): no judged row; narrower than a block; cut edge blocks both ways, padded; rows that are
# 16-byte aligned in fp32 only; many workgroups, no padding
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


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(tdt):
    return _lib.F16 if tdt == torch.float16 else _lib.F32


def _framed(pic, ndt, Hp, Wp, poison):
    """the picture [3, H, W] in a frame whose padding holds the two poison values, alternating by row"""
    host = np.empty((3, Hp, Wp), ndt)
    host[:, ::2], host[:, 1::2] = poison
    host[:, :pic.shape[1], :pic.shape[2]] = pic.astype(ndt)
    return host


def _texture(H, W, seed):
    rng = np.random.default_rng(seed)
    return np.stack([R.texture(H, W, seed * 3 + p, 1) for p in range(3)]) + rng.normal(0.0, 0.004, (3, H, W))


def _woven(first, second, parity):
    out = np.array(first)
    rows = np.arange(out.shape[1]) % 2 != parity
    out[:, rows] = second[:, rows]
    return out


# ---------------------------------------------------------------------------------- the measure and the rule
class _Match:
    def __init__(self):
        self.lib = _lib.lib()
        assert self.lib.dcvc_field_match_ws_bytes() == 64
        self.ws = torch.zeros(16, dtype=torch.int32, device="cuda")
        self.words = torch.full((16,), 0x55, dtype=torch.int32, device="cuda")
        self.counters = [0, 0, 0, 0]                       # judged, passed, woven, filtered: what the calls so far should have left

    def call(self, cur, prev, H, W, parity, slot=0):
        rc = self.lib.dcvc_field_match(_code(cur.dtype), P(cur), P(prev), cur.shape[2], cur.shape[3], H, W, parity, P(self.ws),
                                       ctypes.c_void_p(self.words.data_ptr() + 8 * slot), _stream())
        assert rc == 0, self.lib.dcvc_last_error()

    def expect(self, want):
        _, _, filt, weave = want
        self.counters[0] += 1
        self.counters[3 if filt else 2 if weave else 1] += 1

    def read(self):
        torch.cuda.synchronize()
        return self.words.cpu().tolist(), self.ws.cpu().tolist()


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("H,W,Hp,Wp", SHAPES)
def test_field_match_equals_the_restatement(H, W, Hp, Wp, tdt, ndt):
    seed = H * 1000 + W
    a, b, c = (_texture(H, W, seed + k) for k in range(3))
    outcomes = set()
    for parity in (0, 1):
        # a whole picture; the same with the other field from elsewhere; a previous frame that holds the field that fits; one
        # that does not.  The two frames' padding holds NaN where the other's holds 6e4: a padding sample read would show
        clean, comb = _framed(a, ndt, Hp, Wp, (np.nan, 6e4)), _framed(_woven(a, b, parity), ndt, Hp, Wp, (np.nan, 6e4))
        fits, unrelated = _framed(_woven(c, a, parity), ndt, Hp, Wp, (6e4, np.nan)), _framed(c, ndt, Hp, Wp, (6e4, np.nan))
        cases = [(clean, None), (comb, None), (comb, fits), (comb, unrelated), (clean, unrelated), (clean, fits)]
        want = [M.field_match(cur, prev, H, W, parity) for cur, prev in cases]
        outcomes |= {w[2:] for w in want}
        for offset in (0, 1):                              # 1: no address is 16-byte aligned, the element-wise path
            m = _Match()
            dev = {id(f): _dev(f, offset) for f in (clean, comb, fits, unrelated)}
            for k, ((cur, prev), w) in enumerate(zip(cases, want)):
                m.call(dev[id(cur)], dev[id(prev)] if prev is not None else None, H, W, parity, slot=k)
                m.expect(w)
                words, ws = m.read()
                print(f"parity {parity} offset {offset} case {k}: want {w}, got words {words[2 * k:2 * k + 2]} ws {ws[:10]}")
                assert ws == [0, 0, 0, 0] + m.counters + [w[0], w[1]] + [0] * 6, (parity, offset, k)
                assert words[2 * k:2 * k + 2] == list(w[2:]) and words[2 * k + 2:] == [0x55] * (14 - 2 * k), (parity, offset, k)
            # three calls in a row, nothing in between: each one left the scratch words zero for the next
            for k, slot in ((2, 6), (3, 7), (0, 6)):
                m.call(dev[id(cases[k][0])], dev[id(cases[k][1])] if cases[k][1] is not None else None, H, W, parity, slot=slot)
                m.expect(want[k])
            words, ws = m.read()
            assert ws == [0, 0, 0, 0] + m.counters + list(want[0][:2]) + [0] * 6 and m.counters[0] == 9
            assert words[12:16] == list(want[0][2:]) + list(want[3][2:])
    if H >= 40:
        assert outcomes == {(0, 0), (0, 1), (1, 0)}, outcomes      # pass, weave and filter all occur
    else:
        assert outcomes == {(0, 0)}                        # too small to hold more than MI combed samples: everything passes


# ---------------------------------------------------------------------------------- the weave
def _weave(prev, out, H, W, parity, lines, word):
    rc = _lib.lib().dcvc_field_weave(_code(prev.dtype), P(prev), prev.shape[2], prev.shape[3], H, W, parity, lines, P(word), P(out),
                                     _stream())
    assert rc == 0, _lib.lib().dcvc_last_error()
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("H,W,Hp,Wp", SHAPES)
def test_field_weave_equals_the_restatement(H, W, Hp, Wp, tdt, ndt):
    rng = np.random.default_rng(H * 1000 + W)
    prev = _framed(rng.random((3, H, W)), ndt, Hp, Wp, (6e4, np.nan))
    prev[:, 1::3, ::5] = np.nan                            # NaNs inside the picture, on rows of both fields
    prev_bits = _bits(prev)
    prev_bits[0, 1, 0] |= 1                                # (a NaN with a payload of its own)
    start = rng.random((3, Hp, Wp)).astype(ndt)            # every sample of out differs from what could replace it
    poison = np.full((3, Hp, Wp), np.nan, ndt)
    words = torch.tensor([0, 1, 7], dtype=torch.int32, device="cuda")
    for offset_prev, offset_out in ((0, 0), (1, 1), (0, 1), (1, 0)):
        dp = _dev(prev, offset_prev)
        for parity in (0, 1):
            for lines in (1, 2):
                what = f"offsets {offset_prev} {offset_out} parity {parity} chroma_lines {lines}"
                got = _weave(dp, _dev(poison, offset_out), H, W, parity, lines, words[0:1])
                assert np.array_equal(_bits(got), _bits(poison)), what + ": weave 0 wrote"
                want = M.field_weave(start, prev, H, W, parity, lines, 1)
                for k in (1, 2) if not (offset_prev or offset_out) else (1,):
                    got = _weave(dp, _dev(start, offset_out), H, W, parity, lines, words[k:k + 1])
                    bad = int((_bits(got) != _bits(want)).sum())
                    print(f"{what} word {int(words[k])}: {bad} samples differ")
                    assert bad == 0, what
                kept = [y for y in range(H) if y % 2 == parity]
                assert np.array_equal(_bits(want[0, kept]), _bits(start[0, kept]))               # the first field's rows stay
                if parity == 0:                            # the last row is not kept: the pad below follows it
                    assert np.array_equal(_bits(want[:, H:, :W]), np.broadcast_to(_bits(prev[:, H - 1:H, :W]), (3, Hp - H, W)))


# ---------------------------------------------------------------------------------- the object
H0, W0 = 96, 128
CLIP = dict(speed=4, sigma=0.0, seed=5, blur=2)


def _clip(kind, parity, lines):
    if kind == "telecined":
        return M.telecine(R.make_clip("progressive", 6, H0, W0, parity=parity, chroma_lines=lines, **CLIP)[0], M.PULLDOWN, parity)
    return R.make_clip(kind, 7, H0, W0, parity=parity, chroma_lines=lines, **CLIP)[0]


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("kind,order,lines,matches", [("telecined", "tff", 1, (4, 3, 0)), ("telecined", "bff", 2, (4, 3, 0)),
                                                      ("interlaced", "tff", 2, (0, 0, 7)), ("progressive", "tff", 1, (7, 0, 0)),
                                                      ("static", "bff", 1, (7, 0, 0))])
def test_the_film_deinterlacer_follows_the_restatement_and_waits_for_nothing(kind, order, lines, matches, tdt, ndt, monkeypatch):
    Hp, Wp = H0 + 16, W0 + 8
    frames = [R.to_frame(f, ndt, Hp, Wp, pad=np.nan) for f in _clip(kind, deinterlace.ORDERS.index(order), lines)]
    inputs = [_dev(f) for f in frames]
    dev, ref = Deinterlacer("cuda:0", "film", order, lines), M.Deinterlacer(order, lines)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("filter() waited for the device")

    with monkeypatch.context() as m:                       # no synchronisation and no read-back inside filter()
        m.setattr(torch.cuda, "synchronize", refuse)
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, refuse)
        outs = [dev.filter(x, (H0, W0)) for x in inputs[:4]]
        dev.reset()                                        # (frame 4 has no previous frame: it cannot be woven)
        outs += [dev.filter(x, (H0, W0)) for x in inputs[4:]]
    torch.cuda.synchronize()
    for t, (x, got) in enumerate(zip(frames, outs)):
        if t == 4:
            ref.reset()
        want = ref.filter(x, (H0, W0))
        assert got.shape == (1, 3, Hp, Wp) and got.dtype == tdt
        assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(want)), (kind, t)
    print(f"{kind} {order} chroma_lines {lines}: maxima {ref.maxima}, matches {ref.matches()}")
    assert dev.matches() == ref.matches() == matches and dev.counts() == ref.counts() == (7, matches[2])
    assert dev.filtered() == matches[2] and dev.frames == 7
    if kind == "telecined":                                # the film frames 0 0 1 2 | 3 4 4, bit for bit
        film = R.make_clip("progressive", 6, H0, W0, parity=deinterlace.ORDERS.index(order), chroma_lines=lines, **CLIP)[0]
        for t, k in enumerate((0, 0, 1, 2, 3, 4, 4)):
            assert np.array_equal(_bits(outs[t][0].cpu().numpy()), _bits(R.to_frame(film[k], ndt, Hp, Wp))), t
    with pytest.raises(ValueError, match="multiple of"):
        dev.filter(inputs[0], (H0 - 2 * lines + 1, W0))


def test_the_other_modes_make_the_launches_they_made(monkeypatch):
    lib, seen = _lib.lib(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            return (lambda *a: seen.append(name) or fn(*a)) if name.startswith("dcvc_") else fn

    x = _dev(R.to_frame(_clip("interlaced", 0, 1)[0], np.float16))
    for mode, calls in (("on", ["dcvc_deinterlace"]), ("auto", ["dcvc_comb_detect", "dcvc_deinterlace"]),
                        ("film", ["dcvc_field_match", "dcvc_deinterlace", "dcvc_field_weave"])):
        d = Deinterlacer("cuda:0", mode)
        d._lib = Spy()
        d.filter(x, (H0, W0))
        del seen[:]
        d.filter(x, (H0, W0))
        assert seen == calls, (mode, seen)
        d.reset()
        del seen[:]
        d.filter(x, (H0, W0))                              # without a previous frame there is nothing to weave from
        assert seen == calls[:2], (mode, seen)
    torch.cuda.synchronize()


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
    """8-bit 4:2:0: five film frames, and the seven frames a 3:2 pulldown makes of them (the second field of the last one comes
    from a sixth picture, which no output shows)"""
    d = tmp_path_factory.mktemp("film")
    film = R.make_clip("progressive", 6, H, W, chroma_lines=2, **CLIP)[0]
    return {"film": _write(d / "film.yuv", film[:5]), "telecined": _write(d / "telecined.yuv", M.telecine(film, M.PULLDOWN)),
            "frames": film}


class _Spy:
    """what the passes saw: the model frames of the loader and the front end's inputs (test_gpu_deint's)"""

    def __init__(self, monkeypatch):
        self.loaded, self.fed = [], []
        make_source, front_input = harness.make_source, harness._front_input

        def spy_source(*a):
            src = make_source(*a)
            to_input = src.to_input
            src.to_input = lambda planes, dt: self.loaded.append(to_input(planes, dt)) or self.loaded[-1]
            return src

        def spy_input(*a):
            self.fed.append(front_input(*a))
            return self.fed[-1]

        monkeypatch.setattr(harness, "make_source", spy_source)
        monkeypatch.setattr(harness, "_front_input", spy_input)


def test_film_with_frame_dup_is_an_inverse_telecine(nets, clips, tmp_path, monkeypatch):
    spy = _Spy(monkeypatch)
    log = harness.run_one_point(*nets, clips["telecined"], W, H, 7, 32, 32, deinterlace="film", frame_dup=True, verbose_json=True,
                                bin_path=str(tmp_path / "t.bin"))
    plain = harness.run_one_point(*nets, clips["film"], W, H, 5, 32, 32, verbose_json=True, bin_path=str(tmp_path / "f.bin"))
    assert len(spy.fed) == 12 and len(spy.loaded) == 7 + 7 + 5           # both passes of the first run load every frame
    ref = M.Deinterlacer("tff", 2)
    shown = (0, 0, 1, 2, 3, 4, 4)
    for t, k in enumerate(shown):                          # the front end was fed the film frames, bit for bit
        x = spy.fed[t].cpu().numpy()
        assert np.array_equal(_bits(x), _bits(spy.fed[7 + k].cpu().numpy())), t
        assert np.array_equal(_bits(x[0]), _bits(ref.filter(spy.loaded[t][0].cpu().numpy(), (H, W)))), t
    assert ref.matches() == (4, 3, 0)
    assert log["frame_repeat"] == [0, 1, 0, 0, 0, 0, 1] and log["repeat_frames"] == 2
    assert log["field_matches"] == {"pass": 4, "weave": 3} and log["deint_frames"] == 0
    assert (log["deinterlace"], log["field_order"]) == ("film", "tff")
    assert list(log)[-4:] == ["deinterlace", "field_order", "deint_frames", "field_matches"]
    assert list(log)[:-4] == list(plain) + ["repeat_frames", "dup_tol", "frame_repeat"]
    coded = [t for t in range(7) if not log["frame_repeat"][t]]
    print("bpp", log["frame_bpp"], plain["frame_bpp"], "psnr", log["frame_psnr"], plain["frame_psnr"])
    for key in ("frame_bpp", "frame_psnr"):                # the five coded frames: those of the film clip coded on its own
        assert [log[key][t] for t in coded] == plain[key], key
    assert [log["frame_psnr"][t] for t in (1, 6)] == [plain["frame_psnr"][k] for k in (0, 4)]         # a repeat shows the picture again


def test_a_progressive_clip_codes_as_with_the_option_off_and_on_keeps_its_log(nets, clips, tmp_path):
    kw = dict(intra_period=2, verbose_json=True)
    off = harness.run_one_point(*nets, clips["film"], W, H, 5, 32, 32, bin_path=str(tmp_path / "off.bin"), **kw)
    film = harness.run_one_point(*nets, clips["film"], W, H, 5, 32, 32, deinterlace="film", bin_path=str(tmp_path / "film.bin"), **kw)
    assert open(tmp_path / "film.bin", "rb").read() == open(tmp_path / "off.bin", "rb").read()
    assert film["field_matches"] == {"pass": 5, "weave": 0} and film["deint_frames"] == 0 and list(film)[:-4] == list(off)
    assert film["frame_psnr"] == off["frame_psnr"] and film["frame_bpp"] == off["frame_bpp"]
    on = harness.run_one_point(*nets, clips["film"], W, H, 5, 32, 32, deinterlace="on", **kw)
    assert list(on)[-3:] == ["deinterlace", "field_order", "deint_frames"] and list(on)[:-3] == list(off)
    assert (on["deinterlace"], on["field_order"], on["deint_frames"]) == ("on", "tff", 5)
