"""The one frame check of the picture-side entries (csrc/frame_host.hpp, check_frame) as far as a GPU-less host can see it:
every entry that takes a model frame [3][Hp][Wp] refuses a bad one before anything is launched, names itself in the error, and
words the bound failure alike.  Only refusals are exercised: no call here would be valid with its null stream."""
import ctypes

import pytest

from opendcvc_amd import _lib

# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(65536 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63
_A, _B, _C, _D = _PTR, _PTR + 16384, _PTR + 32768, _PTR + 49152        # frames of 3 * 32 * 48 fp16 elements do not overlap

BASE = dict(dtype=_lib.F16, Hp=32, Wp=48, H=30, W=40)


def _grain_apply(dtype, Hp, Wp, H, W, x=_A, out=_B):
    p = _lib.GrainParamsC(1, 1, (ctypes.c_uint8 * 8)(*([16] * 8)), 8, 8)
    return _lib.lib().dcvc_grain_apply(dtype, x, Hp, Wp, H, W, out, p, 0, None)


def _grain_stats(dtype, Hp, Wp, H, W, noisy=_A, clean=_B):
    return _lib.lib().dcvc_grain_stats(dtype, noisy, clean, Hp, Wp, H, W, _C, None)


def _tf_pyramid(dtype, Hp, Wp, H, W, x=_A):
    return _lib.lib().dcvc_tf_pyramid(dtype, x, Hp, Wp, H, W, _B, None)


def _tf_blend(dtype, Hp, Wp, H, W, cur=_A, out=_B, ref=_C):
    refs, dists = (ctypes.c_void_p * 1)(ref), (ctypes.c_int * 1)(1)
    return _lib.lib().dcvc_tf_blend(dtype, cur, refs, dists, 1, Hp, Wp, H, W, _D, _D + 4096, 3, out, _D + 8192, None)


def _resize(dtype, Hp, Wp, H, W, x=_A):
    return _lib.lib().dcvc_resize_frame(dtype, x, Hp, Wp, H, W, _B, 16, 32, 15, 20, _C, _C, 6, _C, _C, 6, None)


def _to_planes(dtype, Hp, Wp, H, W, x=_A):
    return _lib.lib().dcvc_frame_to_planes(dtype, 420, 10, 0, 0, x, Hp, Wp, H, W, _B, _C, _D, W, W // 2, None)


def _to_metric_planes(dtype, Hp, Wp, H, W, x=_A):
    return _lib.lib().dcvc_frame_to_metric_planes(dtype, 420, 1023, x, Hp, Wp, H, W, _B, _C, _D, None)


def _to_yuv420(dtype, Hp, Wp, H, W, x=_A):
    return _lib.lib().dcvc_frame_to_yuv420(dtype, x, Hp, Wp, H, W, 0, _B, _C, _D, None)


def _to_rgb(dtype, Hp, Wp, H, W, x=_A):
    return _lib.lib().dcvc_frame_to_rgb(dtype, x, Hp, Wp, H, W, _B, None)


def _to_yuv420_planes(dtype, Hp, Wp, H, W, x=_A):
    return _lib.lib().dcvc_frame_to_yuv420_planes(dtype, x, Hp, Wp, H, W, _B, _C, _D, None)


# (entry, call, the keyword of each of its frame arguments)
ENTRIES = [("dcvc_grain_apply", _grain_apply, ("x", "out")),
           ("dcvc_grain_stats", _grain_stats, ("noisy", "clean")),
           ("dcvc_tf_pyramid", _tf_pyramid, ("x",)),
           ("dcvc_tf_blend", _tf_blend, ("cur", "out", "ref")),
           ("dcvc_resize_frame", _resize, ("x",)),
           ("dcvc_frame_to_planes", _to_planes, ("x",)),
           ("dcvc_frame_to_metric_planes", _to_metric_planes, ("x",)),
           ("dcvc_frame_to_yuv420", _to_yuv420, ("x",)),
           ("dcvc_frame_to_rgb", _to_rgb, ("x",)),
           ("dcvc_frame_to_yuv420_planes", _to_yuv420_planes, ("x",))]
FRAME_PTR = dict(x=_A, noisy=_A, cur=_A, out=_B, clean=_B, ref=_C)             # the calls' defaults
SLOTS = [pytest.param(name, call, slot, id=f"{name}-{slot}") for name, call, slots in ENTRIES for slot in slots]

# case -> (the arguments it changes; `frame` stands for the slot's keyword, given the pointer's offset), bound failure?
CASES = {"bad_dtype": (dict(dtype=_lib.U8), False),
         "null_frame": (dict(frame=None), False),
         "H_0": (dict(H=0), False),
         "Hp_below_H": (dict(Hp=28), True),
         "Wp_below_W": (dict(Wp=32), True),
         "off_by_one_byte": (dict(frame=1), False),
         "too_large": (dict(Hp=1 << 20, Wp=1 << 20), False)}          # 3 * Hp * Wp = 3 * 2^40


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name, call, slot", SLOTS)
def test_a_bad_frame_is_refused_by_name_before_any_launch(name, call, slot, case):
    change, bound = CASES[case]
    kw = dict(BASE, **{k: v for k, v in change.items() if k != "frame"})
    if "frame" in change:
        kw[slot] = None if change["frame"] is None else FRAME_PTR[slot] + change["frame"]
    before = bytes(_BUF)
    assert call(**kw) == -1, (name, slot, case)
    err = _lib.lib().dcvc_last_error()
    assert name.encode() in err, err
    if bound:
        assert b"hold the picture" in err, err
    assert bytes(_BUF) == before
