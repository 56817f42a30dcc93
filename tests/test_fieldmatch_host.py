"""The deinterlacer's film mode without a device (docs/deinterlace.md, "Film mode"): every argument error of the two C entries
of csrc/dcvc_fieldmatch.hip, the exports, the option's spellings, and the decisions of the numpy restatement
(tests/fieldmatch_ref.py) on clips whose class is known."""
import ctypes
import os

import numpy as np
import pytest

import deint_ref as R
import fieldmatch_ref as M
from opendcvc_amd import _lib, deinterlace, harness

# ---------------------------------------------------------------------------------- the C entries' argument errors
# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(3 * 24576 + 256)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63
_CUR, _PREV, _WS = _PTR, _PTR + 24576, _PTR + 2 * 24576          # frames of 3 * 32 * 48 fp32 elements: 18432 bytes
_OUT = _CUR
_WORDS = _WS + 64


def _match(dtype=_lib.F16, cur=_CUR, prev=_PREV, Hp=32, Wp=48, H=28, W=40, parity=0, ws=_WS, words=_WORDS):
    return _lib.lib().dcvc_field_match(dtype, cur, prev, Hp, Wp, H, W, parity, ws, words, None)


def _weave(dtype=_lib.F16, prev=_PREV, Hp=32, Wp=48, H=28, W=40, parity=0, lines=2, word=_WORDS + 4, out=_OUT):
    return _lib.lib().dcvc_field_weave(dtype, prev, Hp, Wp, H, W, parity, lines, word, out, None)


BAD_FRAME = [dict(dtype=_lib.U8), dict(dtype=-1), dict(prev=_PREV + 1), dict(H=0), dict(W=0), dict(H=-4), dict(W=-1), dict(Hp=8),
             dict(Wp=8), dict(Hp=1 << 20, Wp=1 << 20), dict(parity=2), dict(parity=-1), dict(dtype=_lib.F32, prev=_PREV + 2)]
BAD_MATCH = BAD_FRAME + [dict(cur=None), dict(cur=_CUR + 1), dict(dtype=_lib.F32, cur=_CUR + 2), dict(H=27), dict(H=1), dict(ws=None),
                         dict(ws=_WS + 4), dict(words=None), dict(words=_WORDS + 2)]
BAD_WEAVE = BAD_FRAME + [dict(prev=None), dict(out=None), dict(out=_OUT + 1), dict(dtype=_lib.F32, out=_OUT + 2), dict(lines=0),
                         dict(lines=3), dict(H=27), dict(H=26), dict(H=30, lines=2), dict(H=27, lines=1), dict(word=None),
                         dict(word=_WORDS + 6), dict(out=_PREV), dict(out=_PREV - 9216 + 2), dict(out=_PREV + 9216 - 2),
                         dict(dtype=_lib.F32, out=_PREV - 18428)]


@pytest.mark.parametrize("kw", BAD_MATCH, ids=lambda kw: "-".join(kw))
def test_field_match_refuses_a_bad_argument_by_name_before_any_launch(kw):
    before = bytes(_BUF)
    assert _match(**kw) == -1, kw
    err = _lib.lib().dcvc_last_error()
    assert b"dcvc_field_match" in err, err
    assert bytes(_BUF) == before


@pytest.mark.parametrize("kw", BAD_WEAVE, ids=lambda kw: "-".join(kw))
def test_field_weave_refuses_a_bad_argument_by_name_before_any_launch(kw):
    before = bytes(_BUF)
    assert _weave(**kw) == -1, kw
    err = _lib.lib().dcvc_last_error()
    assert b"dcvc_field_weave" in err, err
    assert bytes(_BUF) == before


def test_the_messages_name_what_is_wrong_and_the_exports_are_there():
    L = _lib.lib()
    for call, kw, word in ((_match, dict(H=27), b"even"), (_match, dict(parity=2), b"keep_parity"), (_match, dict(ws=None), b"workspace"),
                           (_match, dict(ws=_WS + 4), b"8-byte"), (_match, dict(words=None), b"decision words"),
                           (_match, dict(cur=None), b"the current frame is a null"), (_match, dict(Hp=8), b"does not hold the picture"),
                           (_match, dict(dtype=-1), b"bad dtype"), (_match, dict(H=0), b"bad picture size"),
                           (_match, dict(prev=_PREV + 1), b"the previous frame is not aligned"),
                           (_weave, dict(prev=None), b"the previous frame is a null"), (_weave, dict(out=None), b"out is a null"),
                           (_weave, dict(H=26), b"multiple of 4"), (_weave, dict(H=27, lines=1), b"multiple of 2"),
                           (_weave, dict(lines=3), b"chroma_lines"), (_weave, dict(parity=-1), b"keep_parity"),
                           (_weave, dict(word=None), b"weave word"), (_weave, dict(out=_PREV), b"overlaps the previous"),
                           (_weave, dict(Wp=8), b"does not hold the picture")):
        assert call(**kw) == -1 and word in L.dcvc_last_error(), (kw, L.dcvc_last_error())
    assert L.dcvc_field_match_ws_bytes() == 64
    for name in ("dcvc_field_match_ws_bytes", "dcvc_field_match", "dcvc_field_weave"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    make = open(os.path.join(root, "opendcvc_amd", "csrc", "Makefile")).read()
    assert make.count("dcvc_fieldmatch.o") >= 3


# ---------------------------------------------------------------------------------- the option
BASE = "--src a.yuv --width 64 --height 64 --frames 1".split()


def test_film_is_a_mode_of_the_option_all_the_way_down(monkeypatch):
    assert deinterlace.MODES == ("on", "auto", "film")
    assert deinterlace.check_deinterlace("film", "bff") == ("film", 1) and deinterlace.check_deinterlace("film") == ("film", 0)
    ap = harness.build_parser()
    assert harness.deint_kwargs(vars(ap.parse_args(BASE + "--deinterlace film".split()))) == {"deinterlace": "film"}
    assert harness.deint_kwargs(vars(ap.parse_args(BASE + "--deinterlace film --field-order bff".split()))) == \
        {"deinterlace": "film", "field_order": "bff"}
    for bad in ("--deinterlace yes", "--deinterlace Film", "--deinterlace"):
        with pytest.raises(SystemExit):
            ap.parse_args(BASE + bad.split())
    assert harness.deint_kwargs(dict(deinterlace="film", field_order=None, other=1)) == {"deinterlace": "film"}
    seen = []
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    harness.main(BASE + ["--out", os.devnull, "--deinterlace", "film"])
    assert seen[0]["deinterlace"] == "film" and "field_order" not in seen[0]
    with pytest.raises(ValueError, match="multiple of 4"):                     # the height rule holds for the mode as for the others
        harness.run_one_point(None, None, "nowhere.yuv", 64, 66, 2, 32, deinterlace="film")


def test_run_one_point_makes_a_film_deinterlacer_for_each_pass(monkeypatch):
    made = []

    class Stop(Exception):
        pass

    class Stub:
        def __init__(self, *a):
            made.append(a[1:])

    class Net:
        rate_estimate = entropy = None

        def set_use_two_entropy_coders(self, two):
            pass

    def encode_pass(*a, **kw):
        raise Stop

    monkeypatch.setattr(deinterlace, "Deinterlacer", Stub)
    monkeypatch.setattr(harness, "_encode_pass", encode_pass)
    with pytest.raises(Stop):
        harness.run_one_point(Net(), Net(), "nowhere.yuv", 64, 64, 2, 32, deinterlace="film", field_order="bff")
    assert made == [("film", "bff", 2)] * 2


# ---------------------------------------------------------------------------------- the restatement's decisions
H0, W0 = 96, 128
CLIP = dict(speed=4, sigma=0.0, seed=5, blur=2)


def _frames(kind, n=7, **kw):
    return [R.to_frame(f) for f in R.make_clip(kind, n, H0, W0, **dict(CLIP, **kw))[0]]


@pytest.fixture(scope="module")
def film():
    return R.make_clip("progressive", 6, H0, W0, **CLIP)[0]


def _decide(frames, parity=0):
    out = []
    for t, x in enumerate(frames):
        out.append(M.field_match(x, frames[t - 1] if t else None, H0, W0, parity))
        print(t, out[-1])
    return out


def test_a_telecined_clip_passes_and_weaves_and_never_filters(film):
    got = _decide([R.to_frame(f) for f in M.telecine(film, M.PULLDOWN)])
    assert [(f, w) for _, _, f, w in got] == [(0, 0), (0, 1), (0, 1), (0, 0), (0, 0), (0, 0), (0, 1)]
    clean = [mc for t, (mc, _, _, _) in enumerate(got) if t in (0, 3, 4, 5)] + [mp for t, (_, mp, _, _) in enumerate(got) if t in (1, 2, 3, 6)]
    wrong = [mc for t, (mc, _, _, _) in enumerate(got) if t in (1, 2, 6)] + [mp for t, (_, mp, _, _) in enumerate(got) if t in (4, 5)]
    assert max(clean) <= 1 and 99 <= min(wrong) and max(wrong) <= 108, (clean, wrong)      # as measured for the issue
    assert got[0][1] == 0                                                      # no previous frame: no candidate p


@pytest.mark.parametrize("kind,want", [("interlaced", (1, 0)), ("progressive", (0, 0)), ("static", (0, 0))])
def test_video_is_filtered_and_progressive_and_static_material_passes(kind, want):
    got = _decide(_frames(kind))
    assert [(f, w) for _, _, f, w in got] == [want] * 7
    if kind == "interlaced":
        both = [m for mc, mp, _, _ in got[1:] for m in (mc, mp)] + [got[0][0]]
        assert min(both) >= 44, both                                           # the document's table: this class, not a near miss
    if kind == "static":
        assert all(mc == 0 and mp == 0 for mc, mp, _, _ in got)


@pytest.mark.parametrize("lines", [1, 2])
@pytest.mark.parametrize("parity", [0, 1])
def test_the_film_deinterlacer_gives_back_the_film_frames_bit_for_bit(parity, lines):
    film = R.make_clip("progressive", 6, H0, W0, parity=parity, chroma_lines=lines, **CLIP)[0]
    clip = M.telecine(film, M.PULLDOWN, parity)
    d = M.Deinterlacer("bff" if parity else "tff", lines)
    for t, k in enumerate((0, 0, 1, 2, 3, 4, 4)):
        x = R.to_frame(clip[t], np.float32, H0 + 16, W0 + 8, pad=np.nan)       # nothing of the pad reaches the picture or its new pad
        got = d.filter(x, (H0, W0))
        want = R.to_frame(film[k], np.float32, H0 + 16, W0 + 8)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), t
    assert d.matches() == (4, 3, 0) and d.counts() == (7, 0)


def test_a_frame_too_low_to_judge_passes_and_an_orphan_field_is_filtered(film):
    tiny = np.zeros((3, 4, 8), np.float32)
    tiny[:, 1::2] = 1.0                                                        # the worst comb, but H < 5: no judged row
    assert M.field_match(tiny, tiny, 4, 8, 0) == (0, 0, 0, 0)
    # a cut in the middle of a frame: the kept field's partner is in neither frame
    other = R.make_clip("progressive", 2, H0, W0, speed=4, seed=9, blur=2)[0]
    prev, orphan = R.to_frame(other[0]), R.to_frame(M.telecine([film[0], other[1]], [(0, 1)])[0])
    mc, mp, filt, weave = M.field_match(orphan, prev, H0, W0, 0)
    assert (filt, weave) == (1, 0) and mc > M.MI and mp > M.MI
    # the first frame of a clip, combed: there is no previous frame to weave from
    assert M.field_match(orphan, None, H0, W0, 0)[1:] == (0, 1, 0)
    d = M.Deinterlacer("tff", 1)
    got = d.filter(orphan, (H0, W0))
    assert np.array_equal(got, R.deinterlace(orphan, None, H0, W0, 0, 1)) and d.matches() == (0, 0, 1)


def test_the_weave_is_a_copy_of_bits_with_its_pad():
    H, W, Hp, Wp = 8, 6, 12, 8
    rng = np.random.default_rng(1)
    out, prev = rng.random((3, Hp, Wp), dtype=np.float32), rng.random((3, Hp, Wp), dtype=np.float32)
    prev[:, 3, 2] = np.nan
    assert np.array_equal(M.field_weave(out, prev, H, W, 0, 2, 0), out)
    for parity in (0, 1):
        got = M.field_weave(out, prev, H, W, parity, 2, 1)
        for p, L in ((0, 1), (1, 2), (2, 2)):
            for y in range(Hp):
                sy = min(y, H - 1)
                kept = (sy // L) % 2 == parity
                src = out if kept else prev
                row = src[p, y] if kept else src[p, sy, np.minimum(np.arange(Wp), W - 1)]
                assert np.array_equal(got[p, y].view(np.uint32), row.view(np.uint32)), (parity, p, y)
