"""Field-rate deinterlacing on the GPU (docs/deinterlace.md, "Field-rate output"): dcvc_deinterlace_field of
csrc/dcvc_deint_field.hip against the numpy restatement (tests/deint_field_ref.py) bit for bit, in fp16 and fp32, where it
writes and what it reads, deinterlace.Deinterlacer's fields() / drain() against the frame-rate object on woven frames, and
--deint-rate field end to end through the harness."""
import ctypes
import os

import numpy as np
import pytest
import torch

import deint_field_ref as FR
import deint_ref as R
from opendcvc_amd import _lib, deinterlace, harness, weights
from opendcvc_amd.deinterlace import Deinterlacer

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.float32, np.float32, id="fp32"), pytest.param(torch.float16, np.float16, id="fp16")]
# (H, W, Hp, Wp): smaller than every halo, every row offset reflected; one tile with padding both ways; across a tile edge both
# ways with one tile row of four rows; three tile columns and a reflected bottom edge in the third tile row
SHAPES = [(4, 8, 16, 16), (8, 24, 16, 32), (36, 136, 48, 144), (68, 264, 80, 272)]
GUARD = 64                                                  # elements of poison either side of out
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _dev(host, offset=0):
    """the host frame [3][Hp][Wp] on the device as [1, 3, Hp, Wp], `offset` elements into a 16-byte aligned allocation"""
    t = torch.from_numpy(np.array(host))
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


def _run(before, cur, after, H, W, parity, lines, offset=0):
    """dcvc_deinterlace_field into an out carved `GUARD + offset` elements into a buffer of poison -> numpy [3, Hp, Wp]; nothing
    outside out's [3, Hp, Wp] may change.  offset 0: out is 16-byte aligned"""
    n = cur.numel()
    poison = 0x7BCD if cur.dtype == torch.float16 else 0x7FABCDEF                 # a NaN pattern no arithmetic makes
    ints = torch.full((n + 2 * GUARD + 16,), poison, dtype=torch.int16 if cur.dtype == torch.float16 else torch.int32, device="cuda")
    buf = ints.view(cur.dtype)
    out = buf[GUARD + offset:GUARD + offset + n].view(cur.shape)
    rc = _lib.lib().dcvc_deinterlace_field(0 if cur.dtype == torch.float16 else 1, P(before), P(cur), P(after), cur.shape[2],
                                           cur.shape[3], H, W, parity, lines, P(out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().dcvc_last_error()
    torch.cuda.synchronize()
    host = ints.cpu().numpy()
    assert (host[:GUARD + offset] == poison).all() and (host[GUARD + offset + n:] == poison).all(), "written outside out"
    return out[0].cpu().numpy()


def _unread(before, after, H, W, parity, lines):
    """before and after with NaN in every sample the entry must not read: outside H x W, and the rows of the field that is not
    taken - before's first field, after's second"""
    b, a = np.full_like(before, np.nan), np.full_like(after, np.nan)
    for p in range(3):
        L = 1 if p == 0 else lines
        first = np.array([(y // L) % 2 == parity for y in range(H)])
        b[p, :H, :W][~first] = before[p, :H, :W][~first]
        a[p, :H, :W][first] = after[p, :H, :W][first]
    return b, a


# ---------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("H,W,Hp,Wp", SHAPES)
def test_the_second_picture_equals_the_restatement(H, W, Hp, Wp, tdt, ndt):
    """offset 0: every frame and out are 16-byte aligned and Wp is a multiple of 8 - the 16-byte staging path (every shape; the
    pieces that cross W and the 4 x 8 picture's halo take the element-wise branch inside it).  offset 1: every address is one
    element off - the scalar path, in every shape too"""
    seed = H * 1000 + W
    # the frames' padding holds NaN where the next one's holds 6e4: a padding sample read would show in the picture
    before, cur, after = (_frame(ndt, H, W, Hp, Wp, seed + k, poison=(np.nan, 6e4) if k != 1 else (6e4, np.nan)) for k in range(3))
    for parity in (0, 1):
        for lines in (1, 2):
            want = {True: FR.field_picture(before, cur, after, H, W, parity, lines),
                    False: FR.field_picture(None, cur, None, H, W, parity, lines)}
            assert all(np.isfinite(w.astype(np.float32)).all() and w.shape == (3, Hp, Wp) for w in want.values())
            assert not np.array_equal(want[True], want[False])
            second = [y for y in range(H) if y % 2 != parity]                    # luma: cur's second field arrives bit for bit
            assert np.array_equal(_bits(want[True][0, second, :W]), _bits(cur[0, second, :W]))
            nb, na = _unread(before, after, H, W, parity, lines)
            for offset in (0, 1):
                db, dc, da = _dev(before, offset), _dev(cur, offset), _dev(after, offset)
                for b, a, name in ((db, da, "both"), (None, da, "no before"), (db, None, "no after"), (None, None, "neither"),
                                   (_dev(nb, offset), _dev(na, offset), "both, what is not read is NaN")):
                    got = _run(b, dc, a, H, W, parity, lines, offset)
                    bad = int((_bits(got) != _bits(want[b is not None and a is not None])).sum())
                    what = f"offset {offset} parity {parity} chroma_lines {lines} neighbours: {name}"
                    print(f"{what}: {bad} samples differ")
                    assert bad == 0, what
            # one address off is enough to leave the 16-byte form
            assert np.array_equal(_bits(_run(_dev(before), _dev(cur), _dev(after, 1), H, W, parity, lines)), _bits(want[True]))
            assert np.array_equal(_bits(_run(_dev(before), _dev(cur), _dev(after), H, W, parity, lines, 1)), _bits(want[True]))


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_special_values_arrive_as_the_restatement_has_them(tdt, ndt):
    H, W, Hp, Wp = 36, 136, 48, 144
    frames = [_frame(ndt, H, W, Hp, Wp, 70 + k) for k in range(3)]
    rng = np.random.default_rng(9)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, -3.5, 7.25, 6e4, -6e4, 1e-7], np.float32).astype(ndt)
    for f in frames:                                        # a tenth of every picture, anywhere
        at = rng.random((3, H, W)) < 0.1
        f[:, :H, :W][at] = rng.choice(special, int(at.sum()))
    canon = lambda x: np.where(np.isnan(x), ndt(np.nan), x)
    for parity, lines in ((0, 2), (1, 1)):
        with np.errstate(all="ignore"):
            want = FR.field_picture(*frames, H, W, parity, lines)
        assert np.isnan(want.astype(np.float32)).any() and np.isinf(want.astype(np.float32)).any()
        for offset in (0, 1):
            got = _run(*(_dev(f, offset) for f in frames), H, W, parity, lines, offset)
            # Bit for bit on integer views, with ONE exception the document states ("Field-rate output"): the sign and payload
            # of a NaN in a sample the filter COMPUTES are the machine's (inf - inf is the negative default NaN on a CPU, the
            # positive one on the GPU).  So: a computed sample compares with one pattern for every NaN - where a NaN stands,
            # every zero's sign, every infinity and every other bit are the restatement's - and every sample that is a copy
            # (the second field's rows and their replicate pad, to the right and below) compares exactly, NaNs included
            copied = np.zeros((3, Hp, Wp), bool)
            for plane, L in ((0, 1), (1, lines), (2, lines)):
                copied[plane] = np.array([(min(y, H - 1) // L) % 2 != parity for y in range(Hp)])[:, None]
            raw = _bits(got) != _bits(want)
            print(f"parity {parity} chroma_lines {lines} offset {offset}: {int(raw.sum())} samples differ as they stand "
                  f"({int(raw[copied].sum())} of them copies), {int((_bits(canon(got)) != _bits(canon(want))).sum())} with one "
                  f"pattern for every NaN")
            assert not raw[copied].any(), (parity, lines, offset)
            assert np.array_equal(_bits(canon(got))[~copied], _bits(canon(want))[~copied]), (parity, lines, offset)
            for plane, L in ((0, 1), (1, lines), (2, lines)):           # the second field's rows are cur's, NaNs included
                rows = [y for y in range(H) if (y // L) % 2 != parity]
                assert np.array_equal(_bits(got[plane, rows, :W]), _bits(frames[1][plane, rows, :W])), (parity, lines, offset, plane)


# ---------------------------------------------------------------------------------- the object, on the device alone
def _woven(a, b, H, parity, lines):
    """S of two device frames [1, 3, Hp, Wp]: the rows of the picture with (y / L) % 2 == parity from b, all others from a"""
    out = a.clone()
    y = torch.arange(H, device=a.device)
    for p in range(3):
        rows = y[(y // (1 if p == 0 else lines)) % 2 == parity]
        out[0, p, rows] = b[0, p, rows]
    return out


def _same(a, b):
    """two device tensors hold the same bits"""
    view = torch.int16 if a.dtype == torch.float16 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("order,lines", [("tff", 2), ("bff", 1)])
def test_fields_and_drain_are_the_frame_rate_filter_on_woven_frames(order, lines, tdt, ndt):
    H, W, Hp, Wp, n = 36, 136, 48, 144, 6
    parity, other = deinterlace.ORDERS.index(order), deinterlace.ORDERS[1 - deinterlace.ORDERS.index(order)]
    clip = R.make_clip("interlaced", n, H, W, speed=3, seed=5, parity=parity, chroma_lines=lines, blur=1)[0]
    F = [_dev(R.to_frame(c, ndt, Hp, Wp, pad=np.nan)) for c in clip]
    dev = Deinterlacer("cuda:0", "on", order, lines, rate="field")
    got = [dev.fields(x, (H, W)) for x in F] + [dev.drain()]
    assert [len(g) for g in got] == [1] + [2] * (n - 1) + [1] and dev.drain() == []
    assert (dev.frames, dev.pictures, dev.filtered()) == (n, 2 * n, 2 * n)
    first = [got[0][0]] + [g[1] for g in got[1:n]]
    second = [g[0] for g in got[1:]]
    a, b = Deinterlacer("cuda:0", "on", order, lines), Deinterlacer("cuda:0", "on", other, lines)
    for t in range(n):
        assert _same(first[t], a.filter(F[t], (H, W))), f"A_{t}"
        want = b.filter(_woven(F[t], F[t + 1], H, parity, lines), (H, W)) if t < n - 1 else \
            Deinterlacer("cuda:0", "on", other, lines).filter(F[t], (H, W))
        assert _same(second[t], want), f"B_{t}"
        assert second[t].data_ptr() not in [x.data_ptr() for x in F + first]     # new tensors
    # another size: still two pictures, both from the spatial predictor alone; reset() drops what is pending
    small = _dev(R.to_frame(clip[0], ndt, Hp, Wp, pad=np.nan))
    dev.fields(F[0], (H, W))
    dev.fields(F[1], (H, W))
    pair = dev.fields(small, (H - 4, W))
    fresh = lambda o, x, size: Deinterlacer("cuda:0", "on", o, lines).filter(x, size)
    assert len(pair) == 2 and _same(pair[0], fresh(other, F[1], (H, W))) and _same(pair[1], fresh(order, small, (H - 4, W)))
    dev.reset()
    assert dev.drain() == [] and len(dev.fields(F[2], (H, W))) == 1
    with pytest.raises(ValueError, match="field-rate"):
        dev.filter(F[0], (H, W))
    with pytest.raises(ValueError, match="rate='field'"):
        a.fields(F[0], (H, W))
    with pytest.raises(ValueError, match="rate='field'"):
        a.drain()


# ---------------------------------------------------------------------------------- end to end
H0, W0, N0 = 64, 64, 4


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


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    path = tmp_path_factory.mktemp("deint_field") / "interlaced.yuv"
    with open(path, "wb") as f:
        for planes in R.make_clip("interlaced", N0, H0, W0, speed=4, seed=11, chroma_lines=2, blur=1)[0]:
            for plane in planes:
                f.write(np.ascontiguousarray(plane, np.uint8).tobytes())
    return str(path)


def test_run_one_point_codes_two_pictures_per_frame(nets, clip, tmp_path, monkeypatch):
    fed, loaded = [], []
    windowed, make_source = harness._windowed, harness.make_source

    def spy_source(*a):
        src = make_source(*a)
        to_input = src.to_input
        src.to_input = lambda planes, dt: loaded.append(to_input(planes, dt)) or loaded[-1]
        return src

    monkeypatch.setattr(harness, "make_source", spy_source)
    monkeypatch.setattr(harness, "_windowed", lambda src, x, area: fed.append(x) or windowed(src, x, area))
    rec = str(tmp_path / "rec.yuv")
    log = harness.run_one_point(*nets, clip, W0, H0, N0, 32, 32, deinterlace="on", deint_rate="field", verbose_json=True,
                                rec_path=rec, bin_path=str(tmp_path / "f.bin"))
    assert list(log)[-4:] == ["deinterlace", "field_order", "deint_rate", "deint_frames"]
    assert (log["deinterlace"], log["field_order"], log["deint_rate"], log["deint_frames"]) == ("on", "tff", "field", 2 * N0)
    assert log["i_frame_num"] + log["p_frame_num"] == 2 * N0 == len(log["frame_psnr"]) == len(log["frame_bpp"])
    assert all(np.isfinite(p) and p > 0.0 for p in log["frame_psnr"])                           # the stream decodes
    assert os.path.getsize(rec) == 2 * N0 * H0 * W0 * 3 // 2                                     # eight pictures in display order
    # what the encoder was fed: the restatement's pictures, in order
    assert len(loaded) == 2 * N0 and len(fed) == 2 * N0
    ref = FR.FieldRate("tff", 2)
    want = [p for x in loaded[:N0] for p in ref.fields(x[0].cpu().numpy(), (H0, W0))] + ref.drain()
    for t in range(2 * N0):
        assert np.array_equal(_bits(fed[t][0].cpu().numpy()), _bits(want[t])), t
    monkeypatch.undo()
    for kw in (dict(frame_dup=True), dict(temporal_filter=3)):
        other = harness.run_one_point(*nets, clip, W0, H0, N0, 32, 32, deinterlace="on", deint_rate="field", verbose_json=True, **kw)
        assert other["i_frame_num"] + other["p_frame_num"] == 2 * N0 == len(other["frame_psnr"]) == other["deint_frames"]
        assert all(np.isfinite(p) and p > 0.0 for p in other["frame_psnr"]), kw


def test_frame_rate_is_what_it_was(nets, clip, tmp_path):
    logs, streams = [], []
    for k, kw in enumerate(({}, dict(deint_rate=None), dict(deint_rate="frame"))):
        logs.append(harness.run_one_point(*nets, clip, W0, H0, N0, 32, 32, deinterlace="on", verbose_json=True,
                                          bin_path=str(tmp_path / f"{k}.bin"), **kw))
        streams.append(open(tmp_path / f"{k}.bin", "rb").read())
    assert streams[0] == streams[1] == streams[2]
    drop = lambda log: {k: v for k, v in log.items() if k != "test_time"}
    assert list(logs[0]) == list(logs[1]) == list(logs[2]) and drop(logs[0]) == drop(logs[1]) == drop(logs[2])
    assert "deint_rate" not in logs[0] and logs[0]["deint_frames"] == N0 == logs[0]["i_frame_num"] + logs[0]["p_frame_num"]
