"""Quarter-pel motion of the temporal pre-filter on the host (docs/temporal_filter.md, "Quarter-pel motion"): the numpy
restatement tests/tf_subpel_ref.py against hand-computed samples and constructed blocks, its effect on the document's texture
(the figures of the document's table are printed here), and the harness's option.  No GPU."""
import inspect
import os

import numpy as np
import pytest

import tf_ref as R
import tf_subpel_ref as S
from opendcvc_amd import harness, prefilter

SIZE = (136, 200)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _frame(pic, ndt=np.float32):
    _, h, w = pic.shape
    f = np.full((3, h + (-h) % 16, w + (-w) % 16), np.nan, ndt)
    f[:, :h, :w] = pic.astype(ndt)
    return f


# ---------------------------------------------------------------------------------- taps, vectors, hand-computed samples
def test_taps_and_the_split_of_a_component():
    assert S.TAPS.shape == (4, 8) and (S.TAPS.sum(axis=1) == 64).all()
    assert S.TAPS[0].tolist() == [0, 0, 0, 64, 0, 0, 0, 0] and S.TAPS[3].tolist() == S.TAPS[1][::-1].tolist()
    assert [tuple(int(v) for v in S.split(m)) for m in (-5, -4, -1, 0, 3, 4, 91, -91)] == \
        [(-2, 3), (-1, 0), (-1, 3), (0, 0), (0, 3), (1, 0), (22, 3), (-23, 1)]
    assert all(4 * int(i) + int(f) == m for m in range(-91, 92) for i, f in [S.split(m)])
    assert np.iinfo(np.int16).max >= 4 * 22 + 3


def test_phase_zero_is_the_sample_itself():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 1024, (11, 13)).astype(np.int32)
    yc, xc = np.arange(11)[:, None], np.arange(13)[None, :]
    for my, mx in [(0, 0), (8, -12), (-88, 88)]:
        want = q[np.clip(yc + my // 4, 0, 10), np.clip(xc + mx // 4, 0, 12)]
        assert np.array_equal(S.interp_int(q, yc, xc, my, mx), want)
    ref = rng.random((3, 16, 16)).astype(np.float32)
    ref[0, 0, 0], ref[1, 2, 3], ref[2, 10, 12] = -0.0, np.nan, np.inf
    ref[:, 11:], ref[:, :, 13:] = np.nan, np.nan                       # the padding, which nothing reads
    mvq = np.zeros((2, 2, 2), np.int16)
    mvq[0, 1], mvq[1, 0], mvq[1, 1] = (4, -8), (-12, 0), (88, 88)
    got = S.interp_f32(ref, (11, 13), mvq)
    ys, xs = np.arange(11)[:, None], np.arange(13)[None, :]
    mv = mvq.astype(np.int32) // 4
    want = ref[:, np.clip(ys + mv[ys >> 3, xs >> 3, 0], 0, 10), np.clip(xs + mv[ys >> 3, xs >> 3, 1], 0, 12)]
    assert np.array_equal(_bits(got), _bits(want))                     # -0, NaN and Inf included


def test_hand_computed_samples_at_an_edge():
    q = np.array([[100, 900, 500, 300], [200, 100, 300, 800]], np.int32)
    # position (0, 0), vector (0, -5): ix = -2, fx = 3; columns clamp(k - 5): taps 0 .. 5 on column 0, tap 6 on 1, tap 7 on 2;
    # every row is row 0 and fy = 0: v = 64 h
    h = (0 + 1 - 5 + 17 + 58 - 10) * 100 + 4 * 900 - 1 * 500
    assert h == 9200 and int(S.interp_int(q, 0, 0, 0, -5)) == (64 * h + 2048) >> 12 == 144
    # position (1, 3), vector (6, 1): iy = 1, fy = 2: rows clamp(j - 1): taps 0, 1 on row 0, the rest on row 1;
    # ix = 0, fx = 1: columns clamp(k): taps 0, 1, 2 on columns 0, 1, 2, taps 3 .. 7 (58 + 17 - 5 + 1 + 0 = 71) on column 3
    h0 = -100 + 4 * 900 - 10 * 500 + 71 * 300
    h1 = -200 + 4 * 100 - 10 * 300 + 71 * 800
    v = (-1 + 4) * h0 + (-11 + 40 + 40 - 11 + 4 - 1) * h1
    assert (h0, h1, v) == (19800, 54000, 3353400) and int(S.interp_int(q, 1, 3, 6, 1)) == (v + 2048) >> 12 == 819
    # a sample that leaves 0 .. 1023 is clamped: a step edge overshoots at the half-pel position
    step = np.array([[0, 0, 0, 0, 1023, 1023, 1023, 1023]], np.int32)
    assert int(S.interp_int(step, 0, 4, 0, 2)) == 1023 and (40 + 40 - 11 + 4 - 1) * 64 > 4096          # taps 3 .. 7 on the step
    assert int(S.interp_int(step, 0, 2, 0, 2)) == 0 and -11 + 4 - 1 < 0                                # taps 5 .. 7
    # the same geometry in fp32 on eighths, where every product and sum is exact: r = (3 g0 + 61 g1) / 64,
    # g0 = (-1 + 4 * 7 - 10 * 4 + 71 * 2) / 8 / 64, g1 = (-2 + 4 * 1 - 10 * 3 + 71 * 6) / 8 / 64
    ref = np.zeros((3, 16, 16), np.float32)
    ref[:, :2, :4] = np.array([[1, 7, 4, 2], [2, 1, 3, 6]], np.float32) / 8
    ref[:, 2:], ref[:, :, 4:] = np.nan, np.nan
    r = S.interp_f32(ref, (2, 4), np.array([[[6, 1]]], np.int16))
    assert (3 * 129 + 61 * 398) == 24665 and r.dtype == np.float32
    assert all(float(r[p, 1, 3]) == 24665 / 32768 for p in range(3)) and np.isfinite(r).all()
    # r is not clamped: the same step edge in fp32 overshoots 1
    edge = np.zeros((3, 16, 16), np.float32)
    edge[:, :1, 4:8] = 1.0
    r = S.interp_f32(edge, (1, 8), np.array([[[0, 2]]], np.int16))
    assert float(r[0, 0, 4]) == (40 + 40 - 11 + 4 - 1) / 64 > 1.0 and float(r[0, 0, 2]) == (-11 + 4 - 1) / 64 < 0.0


# ---------------------------------------------------------------------------------- the ranking
def _ramp_block(a):
    """24 x 24 Q0 planes: the reference a ramp of 8 codes per column, the current one that ramp half a pel to the right plus a.
    For block (1, 1), whose taps stay inside the picture, the half-pel filter is exact on a ramp: the candidate (0, +2) has
    SAD 64 a, the centre 64 (4 + a), (0, -2) 64 (8 + a), and no row offset changes a SAD"""
    ref = np.tile(100 + 8 * np.arange(24, dtype=np.int32), (24, 1))
    return ref + 4 + a, ref


def test_the_penalty_keeps_a_centre_that_is_less_than_an_eighth_worse():
    zero = np.zeros((3, 3, 2), np.int16)
    for a, want_mv, want_err in [(40, (0, 0), 64 * 44),       # 2560 against 2816: 9 % lower; R = 2880 loses
                                 (32, (0, 0), 64 * 36),       # 2048 against 2304: R = 2304 ties; the centre's |dy| + |dx| wins
                                 (31, (0, 2), 64 * 31),       # 1984 against 2240: R = 2232 wins
                                 (10, (0, 2), 64 * 10)]:      # errq is the winner's own SAD, 640, not its rank 720
        cur, ref = _ramp_block(a)
        mvq, errq = S.refine(cur, ref, zero, 1)
        assert mvq.dtype == np.int16 and errq.dtype == np.uint32 and mvq.shape == (3, 3, 2)
        assert tuple(mvq[1, 1]) == want_mv and int(errq[1, 1]) == want_err, a
        assert int(S.sad_q(cur, ref, mvq.astype(np.int32))[1, 1]) == want_err
    # stage Q goes on from stage H's winner: the quarter filters move a ramp by 15 / 64 and 49 / 64 of a pel - 2 and 6 codes
    cur, ref = _ramp_block(10)
    mvq, errq = S.refine(cur, ref, zero, 2)
    assert tuple(mvq[1, 1]) == (0, 3) and int(errq[1, 1]) == 64 * (14 - 6)          # R = 576 against the centre's 640
    cur, ref = _ramp_block(3)
    mvq, errq = S.refine(cur, ref, zero, 2)                   # (0, 3): 64 * 1 = 64, R = 72, against the centre (0, 2): 192
    assert tuple(mvq[1, 1]) == (0, 3) and int(errq[1, 1]) == 64
    with pytest.raises(ValueError):
        S.refine(cur, ref, zero, 0)
    # a flat block: every SAD alike, the centre of both stages stays
    flat = np.full((24, 24), 500, np.int32)
    mvq, errq = S.refine(flat, flat + 3, zero + np.int16(2), 2)
    assert (mvq == 8).all() and (errq == 192).all()


def test_whole_vectors_give_the_whole_pel_filter(tex):
    """at vectors 4 * mv the interpolating blend is tf_ref's blend bit for bit"""
    rng = np.random.default_rng(41)
    frames = [_frame(R.shift(tex, 2 * d, -3 * d, 45, 77) + rng.standard_normal((3, 45, 77)) * (2.0 / 255.0), np.float16) for d in (0, -1, 1)]
    pyr = R.pyramid(frames[0], (45, 77))
    motions = [R.motion(pyr, R.pyramid(f, (45, 77))) for f in frames[1:]]
    want, want_total, _ = R.filter_frame(frames[0], frames[1:], [-1, 1], (45, 77), 3, motions)
    got, total, _ = S.filter_frame(frames[0], frames[1:], [-1, 1], (45, 77), 3, 2, [((4 * mv).astype(np.int16), err) for mv, err in motions])
    assert np.array_equal(_bits(got), _bits(want)) and total == want_total > 0


# ---------------------------------------------------------------------------------- the effect
@pytest.fixture(scope="module")
def tex():
    t = R.texture()
    t.setflags(write=False)
    return t


def _effect(tex, per_frame, sigma):
    """five frames of the texture moving per_frame, noise of sigma / 255 (seed as in test_tf_host.py), the middle one filtered
    at level 3 -> (MSE ratio at subpel 0, at subpel 2 - means over the planes -, the fraction of blocks whose refined vector
    is fractional)"""
    rng = np.random.default_rng(23)
    clean = [S.moving(tex, t, per_frame) for t in (-2, -1, 0, 1, 2)] if isinstance(per_frame, tuple) else per_frame
    frames = [_frame(c + (sigma / 255.0) * rng.standard_normal(c.shape)) for c in clean]
    refs, dists = [frames[2 + d] for d in (-1, 1, -2, 2)], [-1, 1, -2, 2]
    h, w = SIZE
    mse = lambda a: np.mean(np.square(a[:, :h, :w].astype(np.float64) - clean[2]), axis=(1, 2))
    pyr = R.pyramid(frames[2], SIZE)
    whole = [R.motion(pyr, R.pyramid(r, SIZE)) for r in refs]
    fine = [S.refine(pyr[0], R.pyramid(r, SIZE)[0], mv, 2) for r, (mv, _) in zip(refs, whole)]
    half = [S.refine(pyr[0], R.pyramid(r, SIZE)[0], mv, 1) for r, (mv, _) in zip(refs, whole)]
    ratio1 = float(np.mean(mse(S.filter_frame(frames[2], refs, dists, SIZE, 3, 1, half)[0]) / mse(frames[2])))
    out0, _, _ = R.filter_frame(frames[2], refs, dists, SIZE, 3, whole)
    out2, _, _ = S.filter_frame(frames[2], refs, dists, SIZE, 3, 2, fine)
    ratio0, ratio2 = float(np.mean(mse(out0) / mse(frames[2]))), float(np.mean(mse(out2) / mse(frames[2])))
    fractional = float(np.mean([((mvq & 3) != 0).any(axis=2).mean() for mvq, _ in fine]))
    sad0, sad2 = float(np.median([e for _, e in whole])), float(np.median([e for _, e in fine]))
    print(f"motion {per_frame if isinstance(per_frame, tuple) else 'as given'} sigma {sigma}/255 level 3: MSE ratio subpel 0 {ratio0:.3f}, "
          f"subpel 1 {ratio1:.3f}, subpel 2 {ratio2:.3f}; "
          f"{100 * fractional:.1f} % of the blocks fractional; median level-0 SAD {sad0:.0f} -> {sad2:.0f}")
    return ratio0, ratio2, fractional


def test_fractional_motion_is_filtered_at_half_the_error_or_less(tex):
    ratio0, ratio2, fractional = _effect(tex, (0.75, -1.25), 1)
    assert ratio2 <= 0.5 * ratio0
    assert fractional > 0.9                                   # nearly every block of this material is fractional


@pytest.mark.parametrize("sigma", [1, 2])
def test_integer_motion_is_left_as_it_was(tex, sigma):
    """a condition on the penalty: without it the design's prototype saw a fifth of the blocks go fractional on noise alone"""
    ratio0, ratio2, fractional = _effect(tex, (-2, 3), sigma)          # (tf_ref.shift(tex, 2 t, -3 t): test_tf_host.py's material)
    assert abs(ratio2 - ratio0) <= 0.05 * ratio0
    assert fractional <= 0.05


def _half_pel(tex, t):
    """docs/temporal_filter.md's half-pel material (tests/test_tf_auto_host.py): (1, 1/2) per frame, every second frame the
    two-tap average of its two integer positions"""
    k = t - 2
    if k % 2 == 0:
        return R.shift(tex, k, k // 2)
    return 0.5 * (R.shift(tex, k, (k - 1) // 2) + R.shift(tex, k, (k - 1) // 2 + 1))


@pytest.mark.parametrize("material,sigma", [("static", 2), ("half-pel", 1), ((0.5, 0.5), 1), ((0.75, -1.25), 2)])
def test_the_documents_other_rows(tex, material, sigma):
    """the rows of the document's table that no condition above covers: never worse than whole-pel vectors by more than 5 %"""
    clean = {"static": [R.shift(tex, 0, 0)] * 5, "half-pel": [_half_pel(tex, t) for t in range(5)]}.get(material, material)
    ratio0, ratio2, _ = _effect(tex, clean, sigma)
    assert ratio2 <= 1.05 * ratio0 and (material == "static" or ratio2 <= 0.6 * ratio0)


@pytest.mark.parametrize("sigma", [0, 1])
def test_the_half_pel_rows_of_the_auto_table(tex, sigma):
    """the document's two half-pel rows of "What it chooses", estimated and filtered with subpel 2: the temporal figure no
    longer reads the motion as noise"""
    import tf_auto_ref as A
    rng = np.random.default_rng(23)
    clean = [_half_pel(tex, t) for t in range(5)]
    frames = [_frame(c + sigma / 255.0 * rng.standard_normal(c.shape)) for c in clean]
    refs, dists = [frames[2 + d] for d in (-1, 1, -2, 2)], [-1, 1, -2, 2]
    whole, _ = A.estimate(frames[2], refs, dists, SIZE)
    four, motions = S.estimate(frames[2], refs, dists, SIZE, 2)
    h, w = SIZE
    mse = lambda a: np.mean(np.square(a[:, :h, :w].astype(np.float64) - clean[2]), axis=(1, 2))
    ratios = [float(np.mean(mse(S.filter_frame(frames[2], refs, dists, SIZE, level, 2, motions)[0]) / mse(frames[2])))
              for level in (1, 2, 3, 4, 5)] if sigma else []
    print(f"half-pel sigma {sigma}/255 subpel 2: level {four[0]}, N {four[1]}, temporal {four[2]} (whole-pel vectors: {whole[2]}), "
          f"spatial {four[3]}; MSE ratios at levels 1 .. 5 {[round(r, 2) for r in ratios]}")
    assert four[2] < whole[2] // 2 and four[3] == whole[3]
    if sigma:
        assert 1 <= four[0] <= 5 and ratios[four[0] - 1] <= 1.25 * min(ratios) and max(ratios) < 1.0


def test_the_material_of_the_effect_tests(tex):
    assert np.allclose(S.moving(tex, 1, (-2, 3)), R.shift(tex, 2, -3), atol=1e-12)
    assert np.allclose(S.moving(tex, -2, (-2, 3)), R.shift(tex, -4, 6), atol=1e-12)
    half = S.moving(tex, 1, (0.0, 0.5))                       # half a pel: between its two integer neighbours, not either
    a, b = R.shift(tex, 0, 0), R.shift(tex, 0, -1)
    assert np.abs(half - 0.5 * (a + b)).max() < 0.25 * np.abs(a - b).max()


# ---------------------------------------------------------------------------------- prefilter and harness
def test_the_filter_object_checks_subpel():
    assert prefilter.SUBPELS == (0, 1, 2) and [prefilter.check_subpel(v) for v in (0, 1, 2)] == [0, 1, 2]
    for bad in (3, -1, True, None, "2", 1.5):
        with pytest.raises(ValueError, match="subpel"):
            prefilter.check_subpel(bad)
    params = inspect.signature(prefilter.TemporalFilter.__init__).parameters
    assert list(params)[1:] == ["device", "level", "radius", "subpel"] and params["subpel"].default == 0
    assert prefilter.check_options(3, 2) == (3, 2) and len(inspect.signature(prefilter.check_options).parameters) == 2
    assert inspect.signature(prefilter.TemporalFilter.filter).parameters["motions"].default is None


def test_the_command_line_has_the_option():
    ap = harness.build_parser()
    assert ap.get_default("tf_subpel") == 0
    base = "--src a.yuv --width 64 --height 64 --frames 1"
    args = ap.parse_args(base.split())
    assert harness.prefilter_kwargs(vars(args)) == {"temporal_filter": 0, "tf_radius": 2}
    args = ap.parse_args((base + " --temporal-filter 3 --tf-subpel 0").split())
    assert harness.prefilter_kwargs(vars(args)) == {"temporal_filter": 3, "tf_radius": 2}
    for spelling in ("--tf-subpel", "--tf_subpel"):
        args = ap.parse_args((base + f" --temporal-filter 3 {spelling} 2").split())
        assert harness.prefilter_kwargs(vars(args)) == {"temporal_filter": 3, "tf_radius": 2, "tf_subpel": 2}
    args = ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0 --temporal-filter auto --tf-subpel 1".split())
    opts, _ = harness.manifest_options(args, ap)
    assert opts["tf_subpel"] == 1 and harness.prefilter_kwargs(opts)["tf_subpel"] == 1       # the pool's options carry it
    for bad in ("3", "-1", "auto"):
        with pytest.raises(SystemExit):
            ap.parse_args((base + f" --tf-subpel {bad}").split())


def test_prefilter_kwargs_with_and_without_the_key():
    two = {"temporal_filter": 4, "tf_radius": 1}
    assert harness.prefilter_kwargs(dict(two)) == two
    assert harness.prefilter_kwargs(dict(two, tf_subpel=None)) == two and harness.prefilter_kwargs(dict(two, tf_subpel=0)) == two
    assert harness.prefilter_kwargs(dict(two, tf_subpel=2, x=1)) == dict(two, tf_subpel=2)
    assert harness.prefilter_kwargs({"tf_subpel": 1}) == {"temporal_filter": 0, "tf_radius": 2, "tf_subpel": 1}
    assert inspect.signature(harness.run_one_point).parameters["tf_subpel"].default == 0
    assert "tf_subpel" not in [name for name, _, _ in harness.POINT_OPTIONS] and "tf_subpel" not in harness.point_kwargs({"tf_subpel": 2})


def test_run_job_and_main_hand_the_option_on(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw) or {})
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    harness.run_job(("i", "p"), job, {"temporal_filter": 2})
    harness.run_job(("i", "p"), job, {"temporal_filter": 2, "tf_radius": 1, "tf_subpel": 2})
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --temporal-filter 5 --tf-subpel 1 --out {os.devnull}".split())
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --temporal-filter 5 --out {os.devnull}".split())
    assert [kw.get("tf_subpel") for kw in seen] == [None, 2, 1, None]


def test_run_one_point_hands_the_option_to_the_encode_pass(monkeypatch, tmp_path):
    class Stop(Exception):
        pass

    seen = []

    def encode_pass(*a, **kw):
        seen.append((a[8:], kw))
        raise Stop

    class Net:
        rate_estimate = entropy = None

        def set_use_two_entropy_coders(self, two):
            pass

    assert inspect.signature(harness._encode_pass).parameters["tf_subpel"].default == 0
    monkeypatch.setattr(harness, "_encode_pass", encode_pass)
    for kw in (dict(tf_subpel=2), dict(tf_subpel=0), {}):
        with pytest.raises(Stop):
            harness.run_one_point(Net(), Net(), str(tmp_path / "clip.yuv"), 64, 64, 2, 32, temporal_filter=3, **kw)
    assert seen == [((3, 2), {"tf_subpel": 2}), ((3, 2), {}), ((3, 2), {})]          # off: the call of before the option


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"a net was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("bad", [3, -1, True, "2", None])
def test_a_bad_value_is_refused_before_anything_is_touched(tmp_path, bad):
    with pytest.raises(ValueError, match="temporal filter subpel"):
        harness.run_one_point(_Untouchable(), _Untouchable(), str(tmp_path / "missing.yuv"), 64, 64, 2, 32, device="cuda:7",
                              temporal_filter=3, tf_subpel=bad)
