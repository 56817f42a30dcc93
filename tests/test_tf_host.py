"""The temporal pre-filter on the host (docs/temporal_filter.md): the numpy restatement tests/tf_ref.py against hand-sized
cases and against the figures the document quotes (motion recovery, noise reduction, cut, identical references), the pure
prefilter.window, and the harness's two options.  No GPU."""
import inspect

import numpy as np
import pytest

import tf_ref as R
from opendcvc_amd import harness, prefilter

SIZE = (136, 200)


@pytest.fixture(scope="module")
def tex():
    t = R.texture()
    t.setflags(write=False)
    return t


def _frame(pic, ndt):
    """a picture [3, H, W] in a padded NaN-filled frame"""
    _, h, w = pic.shape
    f = np.full((3, h + (-h) % 16, w + (-w) % 16), np.nan, ndt)
    f[:, :h, :w] = pic.astype(ndt)
    return f


# ---------------------------------------------------------------------------------- hand-sized cases
def test_quantiser():
    one = np.float32(1.0) / np.float32(1023.0)
    v = np.array([np.nan, -0.0, 0.0, -1.0, 2.0, 1.0, 0.5 * one, 1.5 * one, 2.5 * one, np.inf, -np.inf], np.float32)
    # (ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, where the fp32 product lands on the tie)
    prod = v[6:9] * np.float32(1023.0)
    want_ties = [int(np.rint(p)) for p in prod]
    assert R.quant(v).tolist() == [0, 0, 0, 0, 1023, 1023] + want_ties + [1023, 0]
    exact = np.array([0.5, 1.5, 2.5, 3.5], np.float64)                       # rint itself: ties to even
    assert np.rint(exact).tolist() == [0.0, 2.0, 2.0, 4.0]
    h = np.array([0.25, 0.5, 1.0], np.float16)                               # fp16 is widened first, one fp32 multiply
    assert R.quant(h).tolist() == [256, 512, 1023] and R.quant(h).tolist() == R.quant(h.astype(np.float32)).tolist()


def test_pyramid_at_odd_sizes():
    q0 = np.arange(15, dtype=np.int32).reshape(3, 5) * 10
    q1 = R.half(q0)
    assert q1.shape == (2, 3)
    assert q1.tolist() == [[(0 + 10 + 50 + 60 + 2) >> 2, (20 + 30 + 70 + 80 + 2) >> 2, (40 + 40 + 90 + 90 + 2) >> 2],
                           [(100 + 110 + 100 + 110 + 2) >> 2, (120 + 130 + 120 + 130 + 2) >> 2, (140 * 4 + 2) >> 2]]
    q2 = R.half(q1)
    assert q2.shape == (1, 2) and q2[0, 1] == (q1[0, 2] * 2 + q1[1, 2] * 2 + 2) >> 2
    assert R.half(np.array([[7]], np.int32)).tolist() == [[7]]
    frame = _frame(np.random.default_rng(1).random((3, 33, 41)), np.float32)
    p = R.pyramid(frame, (33, 41))
    assert [q.shape for q in p] == [(33, 41), (17, 21), (9, 11)]
    assert R.pyramid_flat(frame, (33, 41)).shape == (33 * 41 + 17 * 21 + 9 * 11,)


def test_tie_break_key_is_the_documents_total_order():
    cands = [(s, dy, dx) for s in (0, 5) for dy in range(-4, 5) for dx in range(-4, 5)]
    by_key = sorted(cands, key=lambda c: int(R.key(*c)))
    by_tuple = sorted(cands, key=lambda c: (c[0], abs(c[1]) + abs(c[2]), c[1], c[2]))
    assert by_key == by_tuple and len({int(R.key(*c)) for c in cands}) == len(cands)
    # a flat picture: every candidate has SAD 0, the centre wins; so does it over a reference that differs everywhere alike
    flat = np.full((16, 16), 100, np.int32)
    mv, sad = R.search_level(flat, flat + 3, np.zeros((2, 2, 2), np.int32), 4)
    assert not mv.any() and (sad == 64 * 3).all()
    # columns alternate, the reference one column out of phase, rows alike: SAD 0 at every odd dx and any dy.  Of those
    # (0, -1) and (0, 1) have the smallest |dy| + |dx| and the same dy: the smaller dx wins
    cur = np.tile(np.array([100, 900], np.int32), (8, 12))
    ref = np.tile(np.array([900, 100], np.int32), (8, 12))
    mv, sad = R.search_level(cur, ref, np.zeros((1, 3, 2), np.int32), 2)
    assert mv[0, 1].tolist() == [0, -1] and sad[0, 1] == 0
    mv, _ = R.search_level(cur.T.copy(), ref.T.copy(), np.zeros((3, 1, 2), np.int32), 2)
    assert mv[1, 0].tolist() == [-1, 0]


def test_parent_clamp_and_centres():
    parent = np.arange(12, dtype=np.int32).reshape(2, 3, 2)
    c = R.parent_centre(parent, 5, 7)                        # rows 4 and columns 6 have no parent of their own: clamped
    assert c.shape == (5, 7, 2)
    assert c[0, 0].tolist() == [0, 2] and c[3, 5].tolist() == (2 * parent[1, 2]).tolist()
    assert c[4, 6].tolist() == (2 * parent[1, 2]).tolist() and c[4, 0].tolist() == (2 * parent[1, 0]).tolist()


def test_weights_by_hand():
    # level 3: T = 32, A = 2048, P = 64
    assert int(R.block_weight(0, 1, 3)) == 102 and int(R.block_weight(0, -2, 3)) == 77
    assert int(R.block_weight(2047, 1, 3)) == (102 * (2048 ** 2 - 2047 ** 2)) >> 22 and int(R.block_weight(2048, 1, 3)) == 0
    assert int(R.block_weight(65472, 2, 5)) == 0
    assert int(R.block_weight(8191, 1, 5)) == (102 * (8192 ** 2 - 8191 ** 2)) >> 26
    assert R.sample_weight(np.int64(102), np.array([0, 1, 63, 64, 1023]), 3).tolist() == [102, (102 * 4095) >> 12, (102 * 127) >> 12, 0, 0]
    n = np.arange(256, 615)
    assert np.array_equal(R.rcp(n), (1.0 / n.astype(np.float64)).astype(np.float32)) and R.rcp(n).dtype == np.float32


# ---------------------------------------------------------------------------------- motion recovery
@pytest.mark.parametrize("ndt", [np.float32, np.float16])
@pytest.mark.parametrize("sigma", [0.0, 2.0 / 255.0])
@pytest.mark.parametrize("shift", [(5, -9), (-13, 18), (16, -16), (1, 1), (0, 0)])
def test_motion_recovery(tex, shift, sigma, ndt):
    rng = np.random.default_rng(11)
    noisy = lambda pic: pic + sigma * rng.standard_normal(pic.shape)
    cur, ref = _frame(noisy(R.shift(tex, 0, 0)), ndt), _frame(noisy(R.shift(tex, *shift)), ndt)
    mv, err = R.motion(R.pyramid(cur, SIZE), R.pyramid(ref, SIZE))
    assert mv.shape == (17, 25, 2) and mv.dtype == np.int16 and err.dtype == np.uint32
    hit = (mv[..., 0] == -shift[0]) & (mv[..., 1] == -shift[1])
    print(f"shift {shift} sigma {sigma:.4f} {ndt.__name__}: inner {hit[3:-3, 3:-3].mean():.3f}, all {hit.mean():.3f}")
    assert hit[3:-3, 3:-3].all()
    if sigma == 0.0:
        assert not err[3:-3, 3:-3].any()
    assert np.abs(mv).max() <= 22


# ---------------------------------------------------------------------------------- noise reduction
SHIFTS5 = [(-4, 6), (-2, 3), (0, 0), (2, -3), (4, -6)]


def _five(tex, sigma, ndt=np.float32):
    rng = np.random.default_rng(23)
    clean = [R.shift(tex, *s) for s in SHIFTS5]
    return clean[2], [_frame(c + sigma * rng.standard_normal(c.shape), ndt) for c in clean]


def _filter_middle(frames, level):
    refs = [(frames[2 + d], d) for d in (-1, 1, -2, 2)]
    return R.filter_frame(frames[2], [r for r, _ in refs], [d for _, d in refs], SIZE, level)


def _ratios(clean, noisy, out):
    h, w = SIZE
    mse = lambda a: np.mean(np.square(a[:, :h, :w].astype(np.float64) - clean), axis=(1, 2))
    return mse(out) / mse(noisy)


@pytest.mark.parametrize("sigma,level", [(1, 3), (2, 3), (2, 4), (4, 4)])
def test_noise_reduction(tex, sigma, level):
    clean, frames = _five(tex, sigma / 255.0)
    out, total, _ = _filter_middle(frames, level)
    ratio = _ratios(clean, frames[2], out)
    print(f"sigma {sigma}/255 level {level}: MSE ratio per plane {ratio}, mean weight {total / (256.0 * SIZE[0] * SIZE[1]):.3f}")
    assert (ratio <= 0.40).all()


def test_a_weak_filter_stands_aside(tex):
    clean, frames = _five(tex, 4.0 / 255.0)
    out, total, _ = _filter_middle(frames, 1)
    ratio = _ratios(clean, frames[2], out)
    print(f"sigma 4/255 level 1: MSE ratio per plane {ratio}")
    assert (ratio >= 0.99).all()


def test_mean_weight_rises_with_the_level(tex):
    """(1/255, 5) over-smooths - ratios above 1, stated in the document, not asserted; the weight must rise with L"""
    clean, frames = _five(tex, 1.0 / 255.0)
    weights = []
    for level in (1, 2, 3, 4, 5):
        out, total, _ = _filter_middle(frames, level)
        weights.append(total / (256.0 * SIZE[0] * SIZE[1]))
        print(f"sigma 1/255 level {level}: mean weight {weights[-1]:.4f}, MSE ratio {_ratios(clean, frames[2], out)}")
    assert all(a < b for a, b in zip(weights, weights[1:]))


# ---------------------------------------------------------------------------------- cut, identical references
@pytest.mark.parametrize("ndt", [np.float32, np.float16])
def test_cut_is_a_bit_copy(ndt):
    rng = np.random.default_rng(5)
    frames = [_frame(rng.random((3,) + SIZE), ndt) for _ in range(5)]
    frames[0][0, 0, 0] = -0.0
    out, total, wsum = R.filter_frame(frames[0], frames[1:], [-1, 1, -2, 2], SIZE, 3)
    h, w = SIZE
    bits = lambda a: a.view(np.uint16 if ndt == np.float16 else np.uint32)
    assert total == 0 and (wsum == 256).all()
    assert np.array_equal(bits(out[:, :h, :w]), bits(np.ascontiguousarray(frames[0][:, :h, :w])))
    assert np.array_equal(bits(out[:, h:, :w]), bits(np.repeat(out[:, h - 1:h, :w], out.shape[1] - h, axis=1)))      # replicate pad


@pytest.mark.parametrize("ndt", [np.float32, np.float16])
def test_identical_references(tex, ndt):
    cur = _frame(R.shift(tex, 0, 0), ndt)
    out, total, wsum = R.filter_frame(cur, [cur.copy() for _ in range(4)], [-1, 1, -2, 2], SIZE, 3)
    h, w = SIZE
    assert (wsum == 614).all() and total == 358 * h * w
    a, b = out[:, :h, :w].astype(np.float64), cur[:, :h, :w].astype(np.float64)
    print(f"{ndt.__name__}: max |out - in| {np.abs(a - b).max():.3e}")
    if ndt == np.float16:
        assert np.array_equal(out[:, :h, :w], cur[:, :h, :w])
    else:
        assert np.abs(a - b).max() <= 1.2e-7


# ---------------------------------------------------------------------------------- window
def test_window():
    w = prefilter.window
    assert w(1, 1) == [[]] and w(1, 2) == [[]] and w(0, 2) == []
    assert w(2, 1) == w(2, 2) == [[(1, 1)], [(0, -1)]]
    assert w(5, 1) == [[(1, 1)], [(0, -1), (2, 1)], [(1, -1), (3, 1)], [(2, -1), (4, 1)], [(3, -1)]]
    assert w(5, 2) == [[(1, 1), (2, 2)], [(0, -1), (2, 1), (3, 2)], [(1, -1), (3, 1), (0, -2), (4, 2)],
                       [(2, -1), (4, 1), (1, -2)], [(3, -1), (2, -2)]]
    for n in (1, 2, 5):
        for r in (1, 2):
            assert w(n, r) == R.window(n, r)
    with pytest.raises(ValueError):
        w(5, 3)


# ---------------------------------------------------------------------------------- harness
def test_the_command_line_has_both_options():
    ap = harness.build_parser()
    assert ap.get_default("temporal_filter") == 0 and ap.get_default("tf_radius") == 2
    args = ap.parse_args("--src a.yuv --width 64 --height 64 --frames 1".split())
    assert harness.prefilter_kwargs(vars(args)) == {"temporal_filter": 0, "tf_radius": 2}
    args = ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0 --temporal-filter 3 --tf-radius 1".split())
    assert harness.prefilter_kwargs(vars(args)) == {"temporal_filter": 3, "tf_radius": 1}
    opts, _ = harness.manifest_options(args, ap)
    assert (opts["temporal_filter"], opts["tf_radius"]) == (3, 1)             # the pool's options carry them
    with pytest.raises(SystemExit):
        ap.parse_args("--src a.yuv --temporal-filter 6".split())
    with pytest.raises(SystemExit):
        ap.parse_args("--src a.yuv --tf-radius 3".split())


def test_prefilter_kwargs_normalises():
    off = {"temporal_filter": 0, "tf_radius": 2}
    assert harness.prefilter_kwargs({}) == off and harness.prefilter_kwargs({"temporal_filter": None, "tf_radius": None}) == off
    assert harness.prefilter_kwargs({"temporal_filter": 4, "tf_radius": 1, "x": 3}) == {"temporal_filter": 4, "tf_radius": 1}
    params = inspect.signature(harness.run_one_point).parameters
    assert {k: params[k].default for k in off} == off


def test_the_option_table_is_unchanged():
    assert [name for name, _, _ in harness.POINT_OPTIONS] == ["verbose", "verbose_json", "calc_ssim", "metrics", "entropy", "scenecut",
                                                             "min_keyint", "digest", "coded_size", "scale_filter", "film_grain"]
    assert not {"temporal_filter", "tf_radius"} & set(harness.point_kwargs({}))
    assert not {"temporal_filter", "tf_radius"} & set(harness.point_kwargs({"temporal_filter": 3, "tf_radius": 1}))


def test_run_job_and_main_hand_the_options_on(monkeypatch):
    import os
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw) or {})
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    harness.run_job(("i", "p"), job, {})
    harness.run_job(("i", "p"), job, {"temporal_filter": 2, "tf_radius": 1})
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --temporal-filter 5 --out {os.devnull}".split())
    assert [(kw["temporal_filter"], kw["tf_radius"]) for kw in seen] == [(0, 2), (2, 1), (5, 2)]


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"a net was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(temporal_filter=6), dict(temporal_filter=-1), dict(temporal_filter=True), dict(tf_radius=3),
                                dict(temporal_filter=3, tf_radius=0)])
def test_bad_values_are_refused_before_anything_is_touched(tmp_path, kw):
    with pytest.raises(ValueError, match="temporal filter"):
        harness.run_one_point(_Untouchable(), _Untouchable(), str(tmp_path / "missing.yuv"), 64, 64, 2, 32, device="cuda:7", **kw)
