"""tests/frame_io_ref.py, the numpy restatement the GPU tests of tests/test_gpu_frame_io_placement.py compare the 8-bit
planar and RGB frame I/O kernels with, pinned bit for bit to what the reference harness's own functions produced
(tests/golden/frame_io.npz: make_golden_frameio.py, tests/golden/frame_io_rgb.npz: make_golden_rgb.py): every tag, both
storage types, the pad rows and columns.  No GPU."""
import os

import numpy as np
import pytest

import frame_io_ref as R

DTYPES = [(np.float32, "f32"), (np.float16, "f16")]
TAGS = ["a", "b", "c"]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "frame_io.npz"))


@pytest.fixture(scope="module")
def gold_rgb(golden_dir):
    return np.load(os.path.join(golden_dir, "frame_io_rgb.npz"))


@pytest.mark.parametrize("dtype,name", DTYPES)
@pytest.mark.parametrize("tag", TAGS)
def test_yuv420_to_frame(gold, tag, dtype, name):
    y, u, v = (gold[f"src_{tag}_{k}"] for k in "yuv")
    want = gold[f"src_{tag}_{name}"]
    h, w = y.shape
    got = R.yuv420_to_frame(y, u, v, dtype, want.shape[2] - h, want.shape[3] - w)
    assert want.dtype == dtype and (tag == "b" or want.shape[2:] != (h, w))        # (a and c have pad rows and columns)
    assert same_bits(got, want)


@pytest.mark.parametrize("dtype,name", DTYPES)
@pytest.mark.parametrize("tag", TAGS)
def test_frame_to_yuv420_and_its_unrounded_planes(gold, tag, dtype, name):
    x = gold[f"rec_{tag}_{name}_x"]
    want = [gold[f"rec_{tag}_{name}_{k}"] for k in "yuv"]
    h, w = want[0].shape
    assert x.dtype == dtype
    got = R.frame_to_yuv420(x, h, w, round_uv=False)
    for g, t, k in zip(got, want, "yuv"):
        assert same_bits(g, t), k
    # the restatement reads the picture only: whatever lies in the frame's pad changes nothing
    poisoned = x.copy()
    poisoned[:, :, h:, :] = np.nan
    poisoned[:, :, :, w:] = np.nan
    for g, t in zip(R.frame_to_yuv420(poisoned, h, w, round_uv=False), want):
        assert same_bits(g, t)
    # the planes the metrics compare are these samples before the rounding / truncation, in the storage type
    planes = R.yuv420_planes(x, h, w)
    assert all(p.dtype == dtype for p in planes) and planes[0].shape == (h, w) and planes[1].shape == (h // 2, w // 2)
    assert same_bits(np.rint(planes[0].astype(np.float32)).astype(np.uint8), want[0])
    for p, t in zip(planes[1:], want[1:]):
        assert same_bits(p.astype(np.float32).astype(np.uint8), t)
        assert float(p.min()) >= 0 and float(p.max()) <= 255
    # round_uv differs from truncation exactly where the fraction says so
    ru = R.frame_to_yuv420(x, h, w, round_uv=True)
    assert same_bits(ru[0], want[0])
    for p, r in zip(planes[1:], ru[1:]):
        assert same_bits(r, np.rint(p.astype(np.float64)).astype(np.uint8))
    assert any((r != t).any() for r, t in zip(ru[1:], want[1:]))


@pytest.mark.parametrize("dtype,name", DTYPES)
@pytest.mark.parametrize("tag", TAGS)
def test_rgb_to_frame(gold_rgb, tag, dtype, name):
    rgb = gold_rgb[f"src_{tag}_rgb"]
    want = gold_rgb[f"src_{tag}_{name}"]
    _, h, w = rgb.shape
    assert want.dtype == dtype
    assert same_bits(R.rgb_to_frame(rgb, dtype, want.shape[2] - h, want.shape[3] - w), want)


@pytest.mark.parametrize("dtype,name", DTYPES)
@pytest.mark.parametrize("tag", TAGS)
def test_frame_to_rgb(gold_rgb, tag, dtype, name):
    x = gold_rgb[f"rec_{tag}_{name}_x"]
    want = gold_rgb[f"rec_{tag}_{name}_rgb"]
    _, h, w = want.shape
    assert x.dtype == dtype and want.dtype == dtype
    assert same_bits(R.frame_to_rgb(x, h, w), want)
