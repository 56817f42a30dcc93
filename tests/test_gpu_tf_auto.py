"""The temporal pre-filter's automatic level on the GPU (docs/temporal_filter.md, "Choosing the level from the picture"):
dcvc_tf_noise and dcvc_tf_blend_auto against the numpy restatement (tests/tf_auto_ref.py, held against the document's table on
the CPU by tests/test_tf_auto_host.py) - the four integers exactly, the filtered frames bit for bit - TemporalFilter's
sequence interface at level "auto", and --temporal-filter auto end to end through the harness against a loop of the test's own."""
import ctypes
import io

import numpy as np
import pytest
import torch

import tf_auto_ref as A
import tf_ref as R
from opendcvc_amd import _lib, harness
from opendcvc_amd.prefilter import TemporalFilter, window
from tf_utils import _bits, _to_device, clip_fixture, tex  # noqa: F401 (tex: a fixture)

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float32, np.float32), (torch.float16, np.float16)]
SIZES = {(136, 200): (144, 208),   # the document's texture: 17 x 25 blocks, 5 x 4 tiles of the spatial pass, partial on both edges
         (33, 41): (48, 48),       # partial blocks, an odd pyramid, one tile cut on both sides; carved one element into an allocation
         (8, 8): (16, 16),         # one block
         (1, 1): (16, 16)}         # one sample: every fetch clamps
SHIFTS = {-2: (-4, 6), -1: (-2, 3), 0: (0, 0), 1: (2, -3), 2: (4, -6)}
REF_SETS = [[], [1], [-1, 1], [-2, 2], [-1, 1, -2, 2]]          # none, a sequence's start, radius 1, no distance of one, a full window
MATERIALS = ["noise 1", "noise 3", "static", "band", "cut"]


def pictures(tex, material, size, seed):
    """distance -> picture [3, H, W] (float64): the texture moving (2, -3) per frame under noise of 1 / 255 or 3 / 255; one
    clean picture five times; the moving noisy texture under a clean black band over the top third; five unrelated pictures"""
    h, w = size
    rng = np.random.default_rng(seed)
    if material == "cut":
        return {d: rng.random((3, h, w)) for d in SHIFTS}
    if material == "static":
        return {d: R.shift(tex, 0, 0, h, w) * 1.0 for d in SHIFTS}
    sigma = {"noise 1": 1.0, "noise 3": 3.0, "band": 2.0}[material] / 255.0
    pics = {d: R.shift(tex, *s, h, w) * 0.9 + 0.05 + rng.standard_normal((3, h, w)) * sigma for d, s in SHIFTS.items()}
    if material == "band":
        for p in pics.values():
            p[:, :(h + 2) // 3] = 0.0
    return pics


def host_frames(pics, size, ndt):
    """the pictures in NaN-filled padded frames (read-only)"""
    h, w = size
    out = {}
    for d, p in pics.items():
        f = np.full((3,) + SIZES[size], np.nan, ndt)
        f[:, :h, :w] = p.astype(ndt)
        f.setflags(write=False)
        out[d] = f
    return out


def expected(host, size):
    """per reference set: (the four integers or None, the filtered frame, its weight sum) of the restatement"""
    pyr = {d: R.pyramid(f, size) for d, f in host.items()}
    motions = {d: R.motion(pyr[0], pyr[d]) for d in host if d}
    want = []
    for dists in REF_SETS:
        refs = [host[d] for d in dists]
        if not dists:
            want.append((None,) + R.filter_frame(host[0], [], [], size, 3)[:2])
            continue
        four = A.noise(pyr[0][0], [motions[d][1] for d in dists], dists)
        out, total, _ = R.filter_frame(host[0], refs if four[0] else [], dists if four[0] else [], size, four[0] or 3,
                                       [motions[d] for d in dists] if four[0] else None)
        want.append((four, out, total))
    return want


@pytest.fixture(scope="module")
def cases(tex):
    """(material, size, numpy dtype) -> (host frames, device frames, expected(...)), made once"""
    cache = {}

    def get(material, size, ndt):
        key = (material, size, ndt)
        if key not in cache:
            host = host_frames(pictures(tex, material, size, size[0] * 1000 + size[1]), size, ndt)
            dev = {d: _to_device(f, size == (33, 41)) for d, f in host.items()}
            cache[key] = (host, dev, expected(host, size))
        return cache[key]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def auto():
    return TemporalFilter("cuda:0", "auto", 2)


# ---------------------------------------------------------------------------------- the estimate and the blend at its level
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("material", MATERIALS)
def test_noise_and_filter_equal_the_restatement(cases, auto, material, size, tdt, ndt):
    host, dev, want = cases(material, size, ndt)
    H, W = size
    fixed = TemporalFilter("cuda:0", 3, 2)                                     # noise() is the same on a fixed-level object
    levels = []
    for dists, (four, want_out, want_total) in zip(REF_SETS, want):
        refs = [dev[d] for d in dists]
        got4 = auto.noise(dev[0], refs, dists, size)
        spatial_only = A.noise(R.pyramid(host[0], size)[0], [], [])
        print(f"{material} {size} {ndt.__name__} refs {dists}: noise() {got4}, restated {four}")
        assert all(type(v) is int for v in got4) and got4 == (four if four is not None else spatial_only)
        assert fixed.noise(dev[0], refs, dists, size) == got4
        auto.reset()
        out = torch.full_like(dev[0], 7.0)
        assert auto.filter(dev[0], refs, dists, size, out=out) is out
        got = out[0].cpu().numpy()
        diff = int((_bits(got) != _bits(want_out)).sum())
        totals = auto.levels()
        print(f"    filter(): {diff} of {got.size} elements differ, weight sum {auto.weight_sum()}, totals {totals}")
        assert diff == 0 and auto.weight_sum() == want_total
        assert totals == A.totals([four])                                      # (no reference: not estimated, all zero)
        if four is not None and four[0] == 0:
            rows, cols = np.minimum(np.arange(got.shape[1]), H - 1), np.minimum(np.arange(got.shape[2]), W - 1)
            assert want_total == 0 and np.array_equal(_bits(got), _bits(host[0][:, :H, :W][:, rows][:, :, cols]))      # a bit copy + pad
        if four is not None:
            levels.append(four[0])
        for d in [0] + dists:
            assert np.array_equal(_bits(dev[d][0].cpu().numpy()), _bits(host[d]))                                     # inputs untouched
    if size == (136, 200):                                                     # the kernels were asked something
        full = want[-1][0]
        if material in ("noise 1", "noise 3", "band"):
            assert full[0] >= 2 and full[2] > 0 and want[-1][2] > 0
            assert (_bits(got[:, :H, :W]) != _bits(host[0][:, :H, :W])).mean() > 0.4
        if material == "static":
            assert full[:3] == (0, 0, 0) and want[3][0][2] == -1 and want[3][0][1] == full[3] > 0
        if material == "cut":
            assert full[0] == 5 and want[-1][2] == 0                           # "heavy noise" is chosen, and every block stands aside
    if material == "noise 3" and size == (136, 200):
        assert levels[-1] > cases("noise 1", size, ndt)[2][-1][0][0]           # the level follows the noise


# ---------------------------------------------------------------------------------- more tiles than workgroups
WIDE = (40, 33001)                 # 2 x 516 tiles of the spatial pass on at most 512 workgroups: every one walks two, eight three


def wide_frames():
    """distance -> frame [3, 48, 33008] fp16 (NaN outside the picture): a smooth pattern moving (1, -2) per frame under noise
    whose strength grows along the picture, so that the tiles a workgroup walks hold different values, and a clean black
    stretch of columns (exact zeros in every table)"""
    h, w = WIDE
    rng = np.random.default_rng(4033001)
    y, x = np.arange(h + 8)[:, None], np.arange(w + 16)[None, :]
    base = 0.5 + 0.25 * np.sin(x * 0.013) * np.cos(y * 0.21) + 0.1 * np.sin(x * 0.0007 + y * 0.05)
    sigma = (0.5 + 3.5 * np.arange(w) / w)[None, None, :] / 255.0
    out = {}
    for d in (-1, 0, 1):
        pic = np.broadcast_to(base[4 + d:4 + d + h, 8 - 2 * d:8 - 2 * d + w], (3, h, w)) + rng.standard_normal((3, h, w)) * sigma
        pic[:, :, 9000:12000] = 0.0
        f = np.full((3, 48, 33008), np.nan, np.float16)
        f[:, :h, :w] = pic.astype(np.float16)
        f.setflags(write=False)
        out[d] = f
    return out


def test_a_workgroup_that_walks_several_tiles(auto):
    host = wide_frames()
    dev = {d: _to_device(f) for d, f in host.items()}
    dists = [-1, 1]
    pyr = {d: R.pyramid(f, WIDE) for d, f in host.items()}
    motions = [R.motion(pyr[0], pyr[d]) for d in dists]
    want = A.noise(pyr[0][0], [m[1] for m in motions], dists)
    want_spatial = A.noise(pyr[0][0], [], [])
    tables = [A.spatial_table(pyr[0][0])] + [A.temporal_table(m[1]) for m in motions]
    print(f"{WIDE}: restated {want}, spatial alone {want_spatial}; zeros per table {[int((t == 0).sum()) for t in tables]} of {tables[0].size}")
    assert want[0] >= 1 and all((t == 0).sum() > 1000 for t in tables) and len(np.unique(tables[0])) > 300      # something to get wrong
    refs = [dev[d] for d in dists]
    for _ in range(2):                                                         # (the histograms are cleared per call)
        assert auto.noise(dev[0], refs, dists, WIDE) == want
        assert auto.noise(dev[0], [], [], WIDE) == want_spatial
    L = _lib.lib()                                                             # more tiles per workgroup still: 344 and 1032 each
    built_in = L.dcvc_tf_noise_workgroups(3)
    try:
        assert built_in == 512 and auto.noise(dev[0], refs, dists, WIDE) == want
        assert L.dcvc_tf_noise_workgroups(1) == 3 and auto.noise(dev[0], refs, dists, WIDE) == want
        assert L.dcvc_tf_noise_workgroups(0) == 1 and L.dcvc_tf_noise_workgroups(-5) == 1                  # neither changes anything
    finally:
        L.dcvc_tf_noise_workgroups(built_in)
    assert L.dcvc_tf_noise_workgroups(0) == built_in
    auto.reset()
    out = auto.filter(dev[0], refs, dists, WIDE)
    want_out, want_total, _ = R.filter_frame(host[0], [host[d] for d in dists], dists, WIDE, want[0], motions)
    assert int((_bits(out[0].cpu().numpy()) != _bits(want_out)).sum()) == 0
    assert auto.weight_sum() == want_total > 0 and auto.levels() == A.totals([want])


# ---------------------------------------------------------------------------------- blend_auto beside blend
def _blend_args(tf, dev, dists, size, out):
    from opendcvc_amd import nn as L
    code, cur_p, Hp, Wp, H, W = L.frame_args(dev[0], size)
    ptrs = (ctypes.c_void_p * 4)(*[dev[d].data_ptr() for d in dists])
    return (code, cur_p, ptrs, (ctypes.c_int * 4)(*dists), len(dists), Hp, Wp, H, W, tf._mv.data_ptr(), tf._err.data_ptr()), \
           (out.data_ptr(), tf._total.data_ptr(), None)


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_blend_auto_with_a_word_equals_blend_at_that_level(cases, tdt, ndt):
    size, dists = (136, 200), [-1, 1, -2, 2]
    host, dev, _ = cases("noise 1", size, ndt)
    tf = TemporalFilter("cuda:0", 3, 2)
    tf.filter(dev[0], [dev[d] for d in dists], dists, size)                    # leaves the vectors and errors in the object
    L = _lib.lib()
    word = torch.zeros(2, dtype=torch.int32, device="cuda")
    copy = torch.full_like(dev[0], 7.0)
    head, tail = _blend_args(tf, dev, [], size, copy)
    assert L.dcvc_tf_blend(*head, 3, *tail) == 0                               # no reference: the copy level 0 has to equal
    for level in (3, 1, 5, 0, 6, -1, 1 << 20):
        a, b = torch.full_like(dev[0], 7.0), torch.full_like(dev[0], 7.0)
        word[0] = level
        tf._total.zero_()
        head, tail = _blend_args(tf, dev, dists, size, a)
        assert L.dcvc_tf_blend_auto(*head, word.data_ptr(), *tail) == 0, L.dcvc_last_error()
        total_auto = tf.weight_sum()
        if 1 <= level <= 5:
            tf._total.zero_()
            head, tail = _blend_args(tf, dev, dists, size, b)
            assert L.dcvc_tf_blend(*head, level, *tail) == 0
            assert tf.weight_sum() == total_auto > 0
        else:
            b = copy
            assert total_auto == 0
        torch.cuda.synchronize()
        view = torch.int16 if tdt == torch.float16 else torch.int32
        assert torch.equal(a.view(view), b.view(view)), f"level word {level}"


def test_refused_calls_leave_result_and_out_untouched(cases):
    size = (33, 41)
    host, dev, _ = cases("noise 1", size, np.float16)
    tf = TemporalFilter("cuda:0", "auto", 2)
    dists = [-1, 1]
    tf.filter(dev[0], [dev[d] for d in dists], dists, size)
    L, n = _lib.lib(), 2 * tf.radius + 1
    assert L.dcvc_tf_noise_ws_bytes() == 3 * 4096 * 4
    result = torch.full((6,), -77, dtype=torch.int32, device="cuda")
    totals = torch.full((9,), -77, dtype=torch.int64, device="cuda")
    pyr, err, ws = tf._pyr[n].data_ptr(), tf._err.data_ptr(), tf._noise_ws.data_ptr()
    d2, bad = (ctypes.c_int * 4)(-1, 1, 0, 0), (ctypes.c_int * 4)(-1, 3, 0, 0)
    H, W = size
    calls = [(None, err, d2, 2, H, W, ws, result.data_ptr(), totals.data_ptr()),          # NULL pointers
             (pyr, None, d2, 2, H, W, ws, result.data_ptr(), totals.data_ptr()),
             (pyr, err, None, 2, H, W, ws, result.data_ptr(), totals.data_ptr()),
             (pyr, err, d2, 2, H, W, None, result.data_ptr(), totals.data_ptr()),
             (pyr, err, d2, 2, H, W, ws, None, totals.data_ptr()),
             (pyr + 1, err, d2, 2, H, W, ws, result.data_ptr(), totals.data_ptr()),       # misaligned
             (pyr, err + 2, d2, 2, H, W, ws, result.data_ptr(), totals.data_ptr()),
             (pyr, err, d2, 2, H, W, ws + 2, result.data_ptr(), totals.data_ptr()),
             (pyr, err, d2, 2, H, W, ws, result.data_ptr() + 2, totals.data_ptr()),
             (pyr, err, d2, 2, H, W, ws, result.data_ptr(), totals.data_ptr() + 4),
             (pyr, err, d2, 2, 0, W, ws, result.data_ptr(), totals.data_ptr()),           # sizes
             (pyr, err, d2, 2, H, -1, ws, result.data_ptr(), totals.data_ptr()),
             (pyr, err, d2, 5, H, W, ws, result.data_ptr(), totals.data_ptr()),           # nref
             (pyr, err, d2, -1, H, W, ws, result.data_ptr(), totals.data_ptr()),
             (pyr, err, bad, 2, H, W, ws, result.data_ptr(), totals.data_ptr())]          # a distance
    for args in calls:
        assert L.dcvc_tf_noise(*args, None) == -1 and L.dcvc_last_error().startswith(b"dcvc_tf_noise"), args
    torch.cuda.synchronize()
    assert bool((result == -77).all()) and bool((totals == -77).all())
    assert L.dcvc_tf_noise(pyr, err, d2, 2, H, W, ws, result.data_ptr(), totals.data_ptr() + 8, None) == 0      # and the call goes through
    torch.cuda.synchronize()
    assert result[4:].tolist() == [-77, -77] and totals[0].item() == -77
    assert tuple(result[:4].tolist()) == tf.noise(dev[0], [dev[d] for d in dists], dists, size)
    assert L.dcvc_tf_noise(pyr, None, None, 0, H, W, ws, result.data_ptr(), None, None) == 0                    # no reference, no totals
    with pytest.raises(ValueError):
        TemporalFilter("cuda:0", "Auto", 2)
    with pytest.raises(ValueError):
        tf.noise(dev[0], [dev[1]], [3], size)


# ---------------------------------------------------------------------------------- a sequence
@pytest.mark.parametrize("radius", [2, 1])
def test_push_and_flush_follow_the_noise(tex, radius):
    size, n, rng = (70, 118), 7, np.random.default_rng(70 + radius)
    host = []
    for t in range(n):
        sigma = (0.75 if t < 3 else 4.0) / 255.0                               # the noise changes in the middle
        f = np.full((3, 80, 128), np.nan, np.float16)
        f[:, :70, :118] = (R.shift(tex, 2 * t, -3 * t, 70, 118) * 0.9 + 0.05 + rng.standard_normal((3, 70, 118)) * sigma).astype(np.float16)
        host.append(f)
    want = [A.filter_auto(host[t], [host[i] for i, _ in refs], [d for _, d in refs], size) for t, refs in enumerate(R.window(n, radius))]
    chosen = [four[0] for _, _, four in want]
    print(f"radius {radius}: levels {chosen}, N {[four[1] for _, _, four in want]}")
    assert len(set(chosen)) >= 2
    tf = TemporalFilter("cuda:0", "auto", radius)
    got = []
    for f in host:
        got += [o.clone() for o in tf.push(_to_device(f), size)]
    got += [o.clone() for o in tf.flush()]
    assert len(got) == n
    for t in range(n):
        assert np.array_equal(_bits(got[t][0].cpu().numpy()), _bits(want[t][0])), f"frame {t}"
    assert tf.levels() == A.totals([four for _, _, four in want]) and tf.levels()[7] == n
    assert tf.weight_sum() == sum(total for _, total, _ in want)
    single = [o for o in tf.push(_to_device(host[0]), size)] + tf.flush()      # a frame without references: a copy, no total
    assert len(single) == 1 and tf.levels()[7] == n
    assert np.array_equal(_bits(single[0][0].cpu().numpy()), _bits(R.filter_frame(host[0], [], [], size, 3)[0]))
    tf.reset()
    assert tf.levels() == [0] * 8 and tf.weight_sum() == 0


# ---------------------------------------------------------------------------------- end to end
H, W, N = 96, 128, 8


clip = clip_fixture(H, W, N, "tf_auto")     # the 96 x 128, 8-frame clip of test_gpu_tf.py


def test_the_harness_codes_what_the_restatement_filters(clip):
    from opendcvc_amd.bitstream import StreamWriter
    from opendcvc_amd.pipeline import SequenceEncoder, use_two_entropy_coders
    nets, folder = clip
    path = str(folder / "auto.bin")
    log = harness.run_one_point(nets[0], nets[1], str(folder / "clip.yuv"), W, H, N, 32, 32, intra_period=4, reset_interval=32,
                                verbose_json=True, bin_path=path, temporal_filter="auto")
    data = open(path, "rb").read()
    assert list(log)[-5:] == ["tf_level", "tf_radius", "tf_mean_weight", "tf_levels", "tf_noise"]
    assert (log["tf_level"], log["tf_radius"]) == ("auto", 2)
    src = harness.make_source("yuv420", str(folder / "clip.yuv"), W, H)
    reader = src.reader()
    host = [src.to_input(harness._to_device(reader.read(), "cuda:0"), torch.float32)[0].cpu().numpy() for _ in range(N)]
    reader.close()
    enc = SequenceEncoder(nets[0], nets[1], qp_i=32, qp_p=32, intra_period=4, reset_interval=32)
    out = io.BytesIO()
    writer, two, total, fours = StreamWriter(out), use_two_entropy_coders(H, W), 0, []
    for t, refs in enumerate(window(N, 2)):
        x, s, four = A.filter_auto(host[t], [host[i] for i, _ in refs], [d for _, d in refs], (H, W))
        total += s
        fours.append(four)
        writer.write_frame(H, W, two, enc.encode(torch.from_numpy(x)[None].cuda()))
    totals = A.totals(fours)
    print(f"levels {[f[0] for f in fours]}, N {[f[1] for f in fours]}, log {log['tf_levels']} {log['tf_noise']}")
    assert out.getvalue() == data
    assert log["tf_levels"] == totals[:6] and sum(log["tf_levels"]) == N
    assert log["tf_noise"] == totals[6] / N * (255.0 / (68.0 * 1023.0))
    assert log["tf_mean_weight"] == total / (256.0 * H * W * N)
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data)
