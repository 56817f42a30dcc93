"""The temporal pre-filter's automatic level on the host (docs/temporal_filter.md, "Choosing the level from the picture"): the
numpy restatement tests/tf_auto_ref.py against hand-sized cases and against the table the document quotes, and the harness's
option with the value "auto".  No GPU."""
import os

import numpy as np
import pytest

import tf_auto_ref as A
import tf_ref as R
from opendcvc_amd import harness, prefilter

SIZE = (136, 200)
DISTS = [-1, 1, -2, 2]


@pytest.fixture(scope="module")
def tex():
    t = R.texture()
    t.setflags(write=False)
    return t


def _frame(pic, ndt=np.float32):
    _, h, w = pic.shape
    f = np.full((3, h + (-h) % 16, w + (-w) % 16), np.nan, ndt)
    f[:, :h, :w] = pic.astype(ndt)
    return f


# ---------------------------------------------------------------------------------- hand-sized cases
def test_figure_is_the_lower_quartile_of_the_positive_values():
    assert A.figure([5, 9, 1, 7, 3, 11, 13, 15]) == 5                      # 8 positive: rank 2 of 1 3 5 7 ...
    assert A.figure([0, 0, 0, 9, 7, 5, 3, 0]) == 5                         # 4 positive of 8: rank 1 of 3 5 7 9; the zeros do not count
    assert A.figure([0, 0, 6, 0, 0, 0, 0, 0]) == 6                         # 1 * 8 >= 8: rank 0
    assert A.figure(np.array([[4, 4], [4, 2]])) == 4                       # rank 1 of 2 4 4 4
    assert A.figure([8, 3, 5]) == 3                                        # 3 >> 2 = 0: the smallest


def test_figure_cut_where_little_of_the_picture_carries_anything():
    assert A.figure([0] * 8 + [9]) == 0                                    # 1 * 8 < 9
    assert A.figure([0] * 7 + [9]) == 9                                    # 1 * 8 >= 8
    assert A.figure([0] * 15 + [4, 9]) == 0 and A.figure([0] * 14 + [4, 9]) == 4
    assert A.figure([0] * 12) == 0 and A.figure(np.zeros((3, 4), np.int64)) == 0


def test_tables_clip_at_4095():
    assert A.temporal_table(np.array([[0, 4095, 4096, 65472]], np.uint32)).tolist() == [[0, 4095, 4095, 4095]]
    assert A.figure(A.temporal_table(np.array([65472] * 4, np.uint32))) == 4095
    q0 = np.zeros((8, 16), np.int32)
    q0[::2, ::2] = 1023                                                    # S far above 4 * 4095 in both blocks
    assert (A.laplacian_sums(q0) > 4 * 4095).all() and A.spatial_table(q0).tolist() == [[4095, 4095]]


def test_level_rule_at_its_edges():
    assert [A.level_of(n) for n in (0, 39, 40, 160, 161, 320, 321, 640, 641, 1280, 1281, 2560, 2561, 4095)] == \
        [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 5, 5]


def test_laplacian_sum_by_hand():
    q0 = np.array([[1, 2, 4, 8, 16], [3, 9, 27, 81, 243], [5, 25, 125, 625, 1]], np.int64)
    pad = np.pad(q0, 1, mode="edge")
    resp = np.zeros((3, 5), np.int64)
    mask = [[1, -2, 1], [-2, 4, -2], [1, -2, 1]]
    for y in range(3):
        for x in range(5):
            resp[y, x] = sum(mask[i][j] * pad[y + i, x + j] for i in range(3) for j in range(3))
    assert resp[0, 0] == 4 * 1 - 2 * (1 + 2 + 1 + 3) + (1 + 2 + 3 + 9)      # the clamped corner, written out
    # one block: rows 3 .. 7 are row 2, columns 5 .. 7 column 4
    want = sum(abs(int(resp[min(y, 2), min(x, 4)])) for y in range(8) for x in range(8))
    assert A.laplacian_sums(q0).tolist() == [[want]] and A.spatial_table(q0).tolist() == [[min(want >> 2, 4095)]]
    # a ramp has no second difference away from the clamped border; a constant has none anywhere
    ramp = np.arange(24)[None, :] * 3 + np.arange(24)[:, None] * 5
    assert A.laplacian_sums(ramp)[1, 1] == 0 and not A.laplacian_sums(np.full((9, 9), 700)).any()


def test_noise_takes_the_minimum_and_only_distance_one():
    q0 = np.zeros((16, 16), np.int32)
    errs = [np.full((2, 2), 500), np.full((2, 2), 300), np.full((2, 2), 50)]
    assert A.noise(q0, errs, [-1, 1, 2]) == (0, 0, 300, 0)                  # spatial 0 wins; the distance-2 table is not one
    assert A.noise(q0, errs[2:], [2]) == (0, 0, -1, 0) and A.noise(q0, [], []) == (0, 0, -1, 0)
    rng = np.random.default_rng(3)
    q0 = rng.integers(0, 1024, (16, 16)).astype(np.int32)                   # spatial 4095
    assert A.noise(q0, errs, [-1, 1, 2]) == (2, 300, 300, 4095) and A.noise(q0, errs[2:], [-2]) == (5, 4095, -1, 4095)


# ---------------------------------------------------------------------------------- the document's table
MOVING = [(-4, 6), (-2, 3), (0, 0), (2, -3), (4, -6)]


def _half_pel(tex, t):
    """frame t of a sequence moving (1, 1/2) per frame: every second frame is the two-tap average of its two neighbours' columns"""
    k = t - 2
    if k % 2 == 0:
        return R.shift(tex, k, k // 2)
    return 0.5 * (R.shift(tex, k, (k - 1) // 2) + R.shift(tex, k, (k - 1) // 2 + 1))


def _case(clean, sigma):
    """five clean pictures under noise of sigma / 255 -> (the four integers of the middle frame, the MSE ratio of the middle
    frame filtered at levels 1 .. 5, mean over the planes)"""
    rng = np.random.default_rng(23)
    frames = [_frame(c + sigma / 255.0 * rng.standard_normal(c.shape)) for c in clean]
    refs = [frames[2 + d] for d in DISTS]
    four, motions = A.estimate(frames[2], refs, DISTS, SIZE)
    h, w = SIZE
    mse = lambda a: np.mean(np.square(a[:, :h, :w].astype(np.float64) - clean[2]), axis=(1, 2))
    ratios = []
    if sigma:
        ratios = [float(np.mean(mse(R.filter_frame(frames[2], refs, DISTS, SIZE, level, motions)[0]) / mse(frames[2])))
                  for level in (1, 2, 3, 4, 5)]
    return four, ratios


@pytest.mark.parametrize("material,sigma,level", [("moving", 0, 0), ("moving", 0.75, 2), ("moving", 1.5, 3), ("moving", 3, 4),
                                                  ("moving", 6, 5), ("half-pel", 0, 0), ("half-pel", 1, None), ("flat", 2, None)])
def test_the_documents_table(tex, material, sigma, level):
    clean = {"moving": lambda: [R.shift(tex, *s) for s in MOVING], "half-pel": lambda: [_half_pel(tex, t) for t in range(5)],
             "flat": lambda: [np.full((3,) + SIZE, 0.5) for _ in range(5)]}[material]()
    four, ratios = _case(clean, sigma)
    print(f"{material} sigma {sigma}/255: level {four[0]}, N {four[1]}, temporal {four[2]}, spatial {four[3]}; "
          f"MSE ratio at levels 1 .. 5 {[round(r, 3) for r in ratios]}")
    if level is not None:
        assert four[0] == level
    if material == "half-pel" and not sigma:
        assert four[2] >= 40 > four[1] == four[3]                          # the temporal figure alone would have filtered
    if sigma:
        assert 1 <= four[0] <= 5 and ratios[four[0] - 1] <= 1.25 * min(ratios)
    else:
        frame = _frame(clean[2])
        out, total, got = A.filter_auto(frame, [_frame(clean[2 + d]) for d in DISTS], DISTS, SIZE)
        assert got == four and total == 0 and np.array_equal(out[:, :SIZE[0], :SIZE[1]], frame[:, :SIZE[0], :SIZE[1]])


# ---------------------------------------------------------------------------------- options
def test_check_options_takes_auto():
    assert prefilter.check_options("auto", 2) == ("auto", 2) and prefilter.check_options(3, 1) == (3, 1)
    for bad in ("Auto", "3", "", None, 6, True, 2.0):
        with pytest.raises(ValueError, match="temporal filter level .*: 0 \\(off\\) .. 5"):
            prefilter.check_options(bad, 2)
    with pytest.raises(ValueError, match="temporal filter radius"):
        prefilter.check_options("auto", 3)


def test_the_parser_takes_auto_and_keeps_ints():
    ap = harness.build_parser()
    assert ap.get_default("temporal_filter") == 0 and isinstance(ap.get_default("temporal_filter"), int)
    base = "--src a.yuv --width 64 --height 64 --frames 1"
    args = ap.parse_args(f"{base} --temporal-filter auto --tf-radius 1".split())
    assert harness.prefilter_kwargs(vars(args)) == {"temporal_filter": "auto", "tf_radius": 1}
    args = ap.parse_args(f"{base} --temporal_filter 4".split())
    assert args.temporal_filter == 4 and type(args.temporal_filter) is int
    assert ap.parse_args(f"{base} --temporal-filter 0".split()).temporal_filter == 0
    for bad in ("6", "-1", "Auto", "3.0", "on"):
        with pytest.raises(SystemExit):
            ap.parse_args(f"{base} --temporal-filter {bad}".split())
    args = ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0 --temporal-filter auto".split())
    opts, _ = harness.manifest_options(args, ap)
    assert (opts["temporal_filter"], opts["tf_radius"]) == ("auto", 2)
    assert "temporal_filter" not in [name for name, _, _ in harness.POINT_OPTIONS]


def test_run_job_main_and_run_one_point_hand_auto_on(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw) or {})
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    harness.run_job(("i", "p"), job, {"temporal_filter": "auto", "tf_radius": 1})
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --temporal-filter auto --out {os.devnull}".split())
    assert [(kw["temporal_filter"], kw["tf_radius"]) for kw in seen] == [("auto", 1), ("auto", 2)]


def test_run_one_point_hands_auto_to_the_encode_pass(monkeypatch, tmp_path):
    class Stop(Exception):
        pass

    seen = []

    def encode_pass(nets, src, frame_num, dev, coded, scale_filter, grain, enc_kw, tf_level=0, tf_radius=2):
        seen.append((tf_level, tf_radius))
        raise Stop

    class Net:
        rate_estimate = entropy = None

        def set_use_two_entropy_coders(self, two):
            pass

    monkeypatch.setattr(harness, "_encode_pass", encode_pass)
    with pytest.raises(Stop):
        harness.run_one_point(Net(), Net(), str(tmp_path / "clip.yuv"), 64, 64, 2, 32, temporal_filter="auto", tf_radius=1)
    assert seen == [("auto", 1)]


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"a net was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("value", ["Auto", "3", "AUTO", ""])
def test_other_strings_are_refused_before_a_net_is_touched(tmp_path, value):
    with pytest.raises(ValueError, match="temporal filter level"):
        harness.run_one_point(_Untouchable(), _Untouchable(), str(tmp_path / "missing.yuv"), 64, 64, 2, 32, device="cuda:7",
                              temporal_filter=value)
