"""The temporal pre-filter on the GPU (docs/temporal_filter.md): dcvc_tf_pyramid, dcvc_tf_motion and dcvc_tf_blend against the
numpy restatement (tests/tf_ref.py, held against the document's figures on the CPU by tests/test_tf_host.py) bit for bit,
prefilter.TemporalFilter's sequence interface, and --temporal-filter end to end through the harness against a loop of the
test's own."""
import ctypes
import io

import numpy as np
import pytest
import torch

import tf_ref as R
from opendcvc_amd import _lib, harness
from opendcvc_amd.prefilter import TemporalFilter, window
from tf_utils import _bits, _padded_shape, _to_device, clip_fixture, tex  # noqa: F401 (tex: a fixture)

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float32, np.float32), (torch.float16, np.float16)]
SIZES = [(16, 16),                 # every search window and every gather clamps
         (33, 40),                 # a 48 x 48 tensor, NaN around the picture, carved one element into a larger allocation
         (70, 118),                # partial blocks on both edges, odd pyramid sizes (35 x 59, 18 x 30)
         (136, 200)]               # the document's texture: many blocks, vectors up to (4, 6)
SHIFTS = {-2: (-4, 6), -1: (-2, 3), 0: (0, 0), 1: (2, -3), 2: (4, -6)}
REF_SETS = {1: [1], 2: [1, 2], 3: [-1, 1, 2], 4: [-1, 1, -2, 2]}          # the windows at a sequence's start, and a full one


@pytest.fixture(scope="module")
def frames(tex):
    """per (size, numpy dtype): five frames by distance -2 .. 2 - the texture moving (2, -3) per frame under noise of
    2 / 255, each in a NaN-filled padded tensor - host (read-only) and device, and the restatement's (mv, err) per distance"""
    cache = {}

    def get(size, ndt):
        if (size, ndt) not in cache:
            h, w = size
            rng = np.random.default_rng(h * 1000 + w)
            host, dev = {}, {}
            for d, s in SHIFTS.items():
                f = np.full((3,) + _padded_shape(size), np.nan, ndt)
                f[:, :h, :w] = (R.shift(tex, *s, h, w) * 1.1 - 0.05 + rng.standard_normal((3, h, w)) * (2.0 / 255.0)).astype(ndt)
                if d == 0:
                    f[0, 0, 0] = -0.0
                f.setflags(write=False)
                host[d], dev[d] = f, _to_device(f, size == (33, 40))
            pyr = {d: R.pyramid(host[d], size) for d in host}
            motions = {d: R.motion(pyr[0], pyr[d]) for d in host if d}
            cache[(size, ndt)] = (host, dev, motions)
        return cache[(size, ndt)]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def filters():
    made = {}

    def get(level, radius=2):
        if (level, radius) not in made:
            made[(level, radius)] = TemporalFilter("cuda:0", level, radius)
        return made[(level, radius)]
    yield get
    made.clear()


# ---------------------------------------------------------------------------------- pyramid, motion
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_pyramid_and_motion_equal_the_restatement(frames, filters, size, tdt, ndt):
    host, dev, motions = frames(size, ndt)
    tf = filters(3)
    got = tf.pyramid(dev[0], size).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, R.pyramid_flat(host[0], size))
    gh, gw = R.grid(*size)
    for d in (-2, -1, 1, 2):
        mv, err = tf.motion(dev[0], dev[d], size)
        mv, err = mv.cpu().numpy(), err.cpu().numpy()
        want_mv, want_err = motions[d]
        assert mv.shape == (gh, gw, 2) and mv.dtype == np.int16 and err.shape == (gh, gw)
        wrong = int((mv != want_mv).any(axis=2).sum())
        print(f"{size} {ndt.__name__} distance {d}: {wrong} of {gh * gw} vectors differ, largest {np.abs(mv).max()}")
        assert wrong == 0 and np.array_equal(err.astype(np.uint32), want_err)
    if size == (136, 200):
        inner = motions[2][0][3:-3, 3:-3]
        assert (inner[..., 0] == -4).all() and (inner[..., 1] == 6).all()          # the kernels were asked something


# ---------------------------------------------------------------------------------- blend
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("nref", [1, 2, 3, 4])
@pytest.mark.parametrize("level", [1, 3, 5])
@pytest.mark.parametrize("size", SIZES)
def test_blend_equals_the_restatement(frames, filters, size, level, nref, tdt, ndt):
    host, dev, motions = frames(size, ndt)
    dists = REF_SETS[nref]
    want, want_total, _ = R.filter_frame(host[0], [host[d] for d in dists], dists, size, level, [motions[d] for d in dists])
    tf = filters(level)
    tf.reset()
    out = torch.full_like(dev[0], 7.0)
    assert tf.filter(dev[0], [dev[d] for d in dists], dists, size, out=out) is out and out.dtype == tdt
    total = tf.weight_sum()
    got = out[0].cpu().numpy()
    H, W = size
    diff = int((_bits(got) != _bits(want)).sum())
    print(f"{size} level {level} {nref} refs {ndt.__name__}: {diff} of {got.size} elements differ, weight sum {total}")
    assert diff == 0 and total == want_total
    assert np.isfinite(got).all()
    rows, cols = np.minimum(np.arange(got.shape[1]), H - 1), np.minimum(np.arange(got.shape[2]), W - 1)
    assert np.array_equal(_bits(got), _bits(got[:, :H, :W][:, rows][:, :, cols]))          # the pad: the filtered picture's replicate
    if level >= 3:
        assert total > 0 and (_bits(got[:, :H, :W]) != _bits(host[0][:, :H, :W])).mean() > 0.5      # not the identity
    for d in [0] + dists:
        assert np.array_equal(_bits(dev[d][0].cpu().numpy()), _bits(host[d]))                      # the inputs are untouched


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_a_cut_is_a_bit_copy(filters, tdt, ndt):
    size, rng = (70, 118), np.random.default_rng(5)
    pics = []
    for _ in range(5):
        f = np.full((3, 80, 128), np.nan, ndt)
        f[:, :70, :118] = rng.random((3, 70, 118)).astype(ndt)
        pics.append(f)
    dev = [_to_device(f, False) for f in pics]
    tf = filters(3)
    tf.reset()
    got = tf.filter(dev[0], dev[1:], [-1, 1, -2, 2], size)[0].cpu().numpy()
    assert tf.weight_sum() == 0
    assert np.array_equal(_bits(got[:, :70, :118]), _bits(pics[0][:, :70, :118]))
    assert np.array_equal(_bits(got), _bits(R.filter_frame(pics[0], pics[1:], [-1, 1, -2, 2], size, 3)[0]))


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_blend_does_not_depend_on_where_the_frames_lie(tex, filters, tdt, ndt):
    """a 45 x 77 picture in frames [3, 48, Wp], Wp 80 and 84, each once on a 16-byte boundary and once one element into a
    larger allocation (the current frame, the references and out alike): Wp 80 on the boundary takes the wide accesses in
    fp16 and fp32, Wp 84 only in fp32, the view never"""
    size, dists, rng = (45, 77), [-1, 1], np.random.default_rng(4577)
    pics = [(R.shift(tex, *SHIFTS[d], 45, 77) * 1.1 - 0.05 + rng.standard_normal((3, 45, 77)) * (2.0 / 255.0)).astype(ndt)
            for d in [0] + dists]
    tf = filters(3)
    got, totals = [], []
    for wp in (80, 84):
        hosts = [np.full((3, 48, wp), np.nan, ndt) for _ in pics]
        for f, pic in zip(hosts, pics):
            f[:, :45, :77] = pic
        want, want_total, _ = R.filter_frame(hosts[0], hosts[1:], dists, size, 3)
        for mis in (False, True):
            dev = [_to_device(f, mis) for f in hosts]
            out = _to_device(np.full_like(hosts[0], 7.0), mis)
            assert mis or all(t.data_ptr() % 16 == 0 for t in dev + [out])
            tf.reset()
            tf.filter(dev[0], dev[1:], dists, size, out=out)
            totals.append(tf.weight_sum())
            got.append(out[0].cpu().numpy())
            assert np.array_equal(_bits(got[-1]), _bits(want)) and totals[-1] == want_total > 0
    assert all(np.array_equal(_bits(g[:, :45, :77]), _bits(got[0][:, :45, :77])) for g in got) and len(set(totals)) == 1
    assert (_bits(got[0][:, :45, :77]) != _bits(pics[0])).mean() > 0.5


def test_refused_calls_leave_out_untouched(frames, filters):
    _, dev, _ = frames((70, 118), np.float16)
    tf = TemporalFilter("cuda:0", 3, 2)
    refs, dists = [dev[-1], dev[1]], [-1, 1]
    with pytest.raises(_lib.DcvcError, match="overlaps"):                 # out is the current frame
        work = dev[0].clone()
        tf.filter(work, refs, dists, (70, 118), out=work)
    torch.cuda.synchronize()
    assert torch.equal(work.view(torch.int16), dev[0].view(torch.int16))
    with pytest.raises(_lib.DcvcError, match="overlaps"):                 # out is a reference
        work = dev[1].clone()
        tf.filter(dev[0], [dev[-1], work], dists, (70, 118), out=work)
    torch.cuda.synchronize()
    assert torch.equal(work.view(torch.int16), dev[1].view(torch.int16))
    keep = torch.full_like(dev[0], 7.0)
    with pytest.raises(ValueError, match="does not lie"):                 # the picture is larger than the tensor
        tf.filter(dev[0], refs, dists, (81, 118), out=keep)
    with pytest.raises(ValueError):
        tf.filter(dev[0], refs, [-1, 3], (70, 118), out=keep)
    with pytest.raises(ValueError):
        tf.filter(dev[0], [dev[0]] * 5, [1] * 5, (70, 118), out=keep)
    with pytest.raises(ValueError):
        TemporalFilter("cuda:0", 6, 2)
    tf.level = 6                                                          # past the constructor: the entry point refuses
    with pytest.raises(_lib.DcvcError, match="level 6"):
        tf.filter(dev[0], refs, dists, (70, 118), out=keep)
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())
    L, p = _lib.lib(), lambda t: t.data_ptr()
    assert L.dcvc_tf_blend(0, p(dev[0]), None, None, 0, 80, 128, 81, 118, None, None, 3, p(keep), p(tf._total), None) < 0
    assert b"does not hold the picture" in L.dcvc_last_error()
    assert L.dcvc_tf_pyramid(5, p(dev[0]), 80, 128, 70, 118, p(tf._pyr), None) < 0
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())


# ---------------------------------------------------------------------------------- the three blend entries, one host check
# (entry, has a level word): dcvc_tf_blend_subpel is both forms
BLEND_FORMS = [("dcvc_tf_blend", False), ("dcvc_tf_blend_auto", True), ("dcvc_tf_blend_subpel", False), ("dcvc_tf_blend_subpel", True)]


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size", [(33, 40), (16, 16)])          # the element-wise path (one element into an allocation); the vector path
def test_blend_entries_refuse_alike_and_agree(frames, size, tdt, ndt):
    """every refused call of every entry returns -1 with the entry's name first in the error text and launches nothing; the
    accepted calls - at level 3 and through a device word of 3, dcvc_tf_blend_subpel with the whole-pel vectors times four -
    give the restatement's bits and weight sum"""
    from opendcvc_amd import nn as NN
    host, dev, motions = frames(size, ndt)
    L, (H, W), dists = _lib.lib(), size, [-1, 1]
    gh, gw = R.grid(H, W)
    code, _, Hp, Wp, _, _ = NN.frame_args(dev[0], size)
    cur_p = dev[0].data_ptr()
    assert (cur_p % 16 == 0) == (size == (16, 16))
    mv = torch.zeros((4, gh, gw, 2), dtype=torch.int16, device="cuda")
    err = torch.zeros((4 * gh * gw + 2,), dtype=torch.int32, device="cuda")
    for i, d in enumerate(dists):
        mv[i].copy_(torch.from_numpy(motions[d][0]))
        err[i * gh * gw:(i + 1) * gh * gw].copy_(torch.from_numpy(motions[d][1].astype(np.int32).ravel()))
    mvq = 4 * mv
    word = torch.full((2,), 3, dtype=torch.int32, device="cuda")
    total = torch.zeros(2, dtype=torch.int64, device="cuda")
    keep = _to_device(np.full_like(host[0], 7.0), size == (33, 40))
    ptrs = (ctypes.c_void_p * 4)(dev[-1].data_ptr(), dev[1].data_ptr(), 0, 0)
    d4, bad = (ctypes.c_int * 4)(-1, 1, -2, 2), (ctypes.c_int * 4)(-1, 3, -2, 2)

    def blend(entry, worded, **kw):
        a = dict(dtype=code, cur=cur_p, refs=ptrs, dists=d4, nref=2, hp=Hp, h=H, mv=(mvq if "subpel" in entry else mv).data_ptr(),
                 err=err.data_ptr(), level=3 if not worded else 0, level_dev=word.data_ptr() if worded else None,
                 out=keep.data_ptr(), total=total.data_ptr())
        a.update(kw)
        head = (a["dtype"], a["cur"], a["refs"], a["dists"], a["nref"], a["hp"], Wp, a["h"], W, a["mv"], a["err"])
        levels = {"dcvc_tf_blend": (a["level"],), "dcvc_tf_blend_auto": (a["level_dev"],)}.get(entry, (a["level"], a["level_dev"]))
        return getattr(L, entry)(*head, *levels, a["out"], a["total"], None)

    common = [dict(cur=None), dict(refs=None), dict(dists=None), dict(mv=None), dict(err=None), dict(out=None), dict(total=None),
              dict(mv=mv.data_ptr() + 1), dict(err=err.data_ptr() + 2), dict(total=total.data_ptr() + 4),
              dict(nref=-1), dict(nref=5), dict(nref=3), dict(dists=bad), dict(h=Hp + 1), dict(dtype=5), dict(out=cur_p),
              dict(out=dev[1].data_ptr())]
    for entry, worded in BLEND_FORMS:
        own = [dict(level_dev=word.data_ptr() + 2)] if entry != "dcvc_tf_blend" else []
        own += [dict(level_dev=None)] if entry == "dcvc_tf_blend_auto" else []
        own += [dict(level=0), dict(level=6)] if not worded else []
        for kw in common + own:
            assert blend(entry, worded, **kw) == -1 and L.dcvc_last_error().startswith(entry.encode() + b":"), (entry, worded, kw)
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all()) and int(total[0]) == 0
    assert np.array_equal(_bits(dev[1][0].cpu().numpy()), _bits(host[1])) and np.array_equal(_bits(dev[0][0].cpu().numpy()), _bits(host[0]))
    want, want_total, _ = R.filter_frame(host[0], [host[d] for d in dists], dists, size, 3, [motions[d] for d in dists])
    for entry, worded in BLEND_FORMS:
        out = _to_device(np.full_like(host[0], 7.0), size == (33, 40))
        total.zero_()
        assert blend(entry, worded, out=out.data_ptr()) == 0, L.dcvc_last_error()
        got = out[0].cpu().numpy()
        print(f"{entry} {'word' if worded else 'level'} {size} {ndt.__name__}: {int((_bits(got) != _bits(want)).sum())} differ, sum {int(total[0])}")
        assert np.array_equal(_bits(got), _bits(want)) and int(total[0]) == want_total > 0 and int(total[1]) == 0


# ---------------------------------------------------------------------------------- a sequence
@pytest.mark.parametrize("n,radius", [(7, 2), (7, 1), (1, 2), (2, 2), (2, 1)])
def test_push_and_flush_equal_filter_on_the_window(tex, filters, n, radius):
    size, rng = (70, 118), np.random.default_rng(n * 10 + radius)
    seq = []
    for t in range(n):
        f = np.full((3, 80, 128), np.nan, np.float16)
        f[:, :70, :118] = (R.shift(tex, 2 * t, -3 * t, 70, 118) + rng.standard_normal((3, 70, 118)) * (2.0 / 255.0)).astype(np.float16)
        seq.append(_to_device(f, False))
    ref_tf = filters(3, radius)
    ref_tf.reset()
    want = [ref_tf.filter(seq[t], [seq[i] for i, _ in refs], [d for _, d in refs], size) for t, refs in enumerate(window(n, radius))]
    want_total = ref_tf.weight_sum()
    tf = TemporalFilter("cuda:0", 3, radius)
    got, counts = [], []
    for x in seq:
        out = tf.push(x, size)
        counts.append(len(out))
        got += [o.clone() for o in out]
    rest = tf.flush()
    got += [o.clone() for o in rest]
    assert counts == [0] * min(radius, n) + [1] * max(n - radius, 0) and len(rest) == min(radius, n) and tf.flush() == []
    assert len(got) == n and tf.weight_sum() == want_total
    for t in range(n):
        assert torch.equal(got[t].view(torch.int16), want[t].view(torch.int16)), f"frame {t}"
    if n == 7:                                   # a second sequence through the same object: the ring starts over
        again = [o.clone() for x in seq[:3] for o in tf.push(x, size)] + [o.clone() for o in tf.flush()]
        want3 = [ref_tf.filter(seq[t], [seq[i] for i, _ in refs], [d for _, d in refs], size) for t, refs in enumerate(window(3, radius))]
        assert len(again) == 3 and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(again, want3))
        tf.reset()
        assert tf.weight_sum() == 0


# ---------------------------------------------------------------------------------- end to end
H, W, N = 96, 128, 8


clip = clip_fixture(H, W, N, "tf")          # the 96 x 128, 8-frame clip of test_gpu_harness_options.py


def _run(clip, name, **kw):
    nets, folder = clip
    path = str(folder / f"{name}.bin")
    log = harness.run_one_point(nets[0], nets[1], str(folder / "clip.yuv"), W, H, N, 32, 32, intra_period=4, reset_interval=32,
                                verbose_json=True, bin_path=path, **kw)
    return log, open(path, "rb").read()


def test_the_harness_codes_what_the_restatement_filters(clip):
    from opendcvc_amd.bitstream import StreamWriter
    from opendcvc_amd.pipeline import SequenceEncoder, use_two_entropy_coders
    nets, folder = clip
    log, data = _run(clip, "tf3", temporal_filter=3)
    assert list(log)[-3:] == ["tf_level", "tf_radius", "tf_mean_weight"] and (log["tf_level"], log["tf_radius"]) == (3, 2)
    # the test's own loop: loader -> the restatement on the host -> upload -> SequenceEncoder -> StreamWriter
    src = harness.make_source("yuv420", str(folder / "clip.yuv"), W, H)
    reader = src.reader()
    host = [src.to_input(harness._to_device(reader.read(), "cuda:0"), torch.float32)[0].cpu().numpy() for _ in range(N)]
    reader.close()
    enc = SequenceEncoder(nets[0], nets[1], qp_i=32, qp_p=32, intra_period=4, reset_interval=32)
    out = io.BytesIO()
    writer, two, total = StreamWriter(out), use_two_entropy_coders(H, W), 0
    for t, refs in enumerate(window(N, 2)):
        x, s, _ = R.filter_frame(host[t], [host[i] for i, _ in refs], [d for _, d in refs], (H, W), 3)
        total += s
        writer.write_frame(H, W, two, enc.encode(torch.from_numpy(x)[None].cuda()))
    assert out.getvalue() == data
    assert total > 0 and log["tf_mean_weight"] == total / (256.0 * H * W * N)
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data)


def test_level_0_is_the_run_of_today(clip):
    log0, data0 = _run(clip, "plain")
    log, data = _run(clip, "off", temporal_filter=0, tf_radius=1)
    assert data == data0 and list(log) == list(log0) and not [k for k in log if k.startswith("tf_")]
    assert {k: v for k, v in log.items() if k != "test_time"} == {k: v for k, v in log0.items() if k != "test_time"}
    _, data3 = _run(clip, "on", temporal_filter=3, tf_radius=1)
    assert data3 != data0


def test_with_the_other_extensions(clip):
    log, data = _run(clip, "all", temporal_filter=3, coded_size=(64, 80), film_grain="auto", scenecut=150, digest=True)
    assert log["digests_checked"] == N
    assert list(log)[-9:] == ["coded_height", "coded_width", "scale_filter", "grain_units", "grain_scale_y", "grain_corr",
                              "tf_level", "tf_radius", "tf_mean_weight"]
    assert 0.0 <= log["tf_mean_weight"] <= 358.0 / 256.0
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data)
