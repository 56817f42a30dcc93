"""Scene-cut detection without a GPU: the numpy restatement of the analysis on hand-computable planes, the decision on
the project's synthetic material, and the I-frame policy of pipeline.SequenceEncoder with stub codecs and a scripted
analyzer."""
import numpy as np
import pytest

import analysis_ref as R
from opendcvc_amd import analysis
from opendcvc_amd.pipeline import INDEX_MAP, SequenceEncoder


# ---------------------------------------------------------------------------------- hand-computable planes
def _blocks(values, dtype=np.float32):
    """16 x 16 plane of four constant 8 x 8 blocks: values = ((top left, top right), (bottom left, bottom right))"""
    return np.kron(np.asarray(values, np.float64), np.ones((8, 8))).astype(dtype)


def _product_tie(target):
    """a float32 v whose float32 product v * 1023 is exactly `target` (an x.5 value) although the real product is not"""
    v = np.float32(target / 1023.0)
    for _ in range(64):
        if np.float32(v * np.float32(1023.0)) == np.float32(target):
            return v
        v = np.nextafter(v, np.float32(2.0), dtype=np.float32)
    raise AssertionError("no float32 with that product nearby")


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_constant_plane_has_no_activity(dtype):
    x = np.full((16, 16), 0.25, dtype)              # 0.25 * 1023 = 255.75 -> 256
    L, (inter, intra, total, blocks) = R.analyze(x)
    assert L.tolist() == [[64 * 256] * 2] * 2
    assert (inter, intra, total, blocks) == (0, 0, 4 * 64 * 256, 4)
    assert R.analyze(x, L)[1] == (0, 0, 4 * 64 * 256, 4)


def test_four_distinct_blocks():
    # q: 0, 1023, 256 (255.75 up), 128 (127.875 up) -> L = 64 q
    x = _blocks(((0.0, 1.0), (0.25, 0.125)))
    L, (inter, intra, total, blocks) = R.analyze(x)
    assert L.tolist() == [[0, 64 * 1023], [64 * 256, 64 * 128]]
    # first row: |65472 - 0|; first column: |16384 - 0|; block (1, 1): min(|8192 - 16384|, |8192 - 65472|)
    assert intra == 65472 + 16384 + 8192
    assert (inter, total, blocks) == (0, 65472 + 16384 + 8192, 4)
    prev = np.asarray([[100, 65472], [0, 9000]])
    assert R.stats(L, prev)[0] == 100 + 0 + 16384 + 808


def test_clamping_ties_and_nan():
    tie_dn = _product_tie(510.5)                    # float32 product exactly 510.5 -> 510 (ties go to even, not up)
    x = _blocks(((1.5, -0.25), (0.5, float(tie_dn))))
    assert R.quantise(x)[::8, ::8].tolist() == [[1023, 0], [512, 510]]      # 0.5 * 1023 = 511.5 -> 512
    L, (inter, intra, total, _) = R.analyze(x)
    assert intra == 64 * (1023 + (1023 - 512) + min(2, 510)) and total == 64 * (1023 + 512 + 510)
    y = x.copy()
    y[3, 5] = np.nan                                # in the block of 1.5 -> 1023: that sample counts as 0
    y[12, 1] = np.inf                               # in the block of 0.5 -> 512: clamps to 1023
    L2 = R.lowres(y)
    assert L2.tolist() == [[64 * 1023 - 1023, 0], [64 * 512 + 511, 64 * 510]]
    assert R.stats(L2, L)[0] == 1023 + 511
    h = _blocks(((1.5, -0.25), (0.5, 0.125)), np.float16)
    assert R.lowres(h).tolist() == [[64 * 1023, 0], [64 * 512, 64 * 128]]


def test_is_cut_definition():
    S = analysis.FrameStats
    assert not analysis.is_cut(S(10 ** 9, 1, 5, 4, False), 150)            # no previous plane: never a cut
    assert analysis.is_cut(S(150, 100, 5, 4, True), 150) and not analysis.is_cut(S(149, 100, 5, 4, True), 150)
    assert analysis.is_cut(S(2, 0, 5, 4, True), 150) and not analysis.is_cut(S(1, 0, 5, 4, True), 150)    # max(intra, 1)
    big = S(2 ** 62, 2 ** 61, 0, 1, True)                                  # Python integers: no overflow
    assert analysis.is_cut(big, 150) and not analysis.is_cut(big, 250)
    for s in (S(150, 100, 5, 4, True), S(149, 100, 5, 4, True), S(7, 0, 0, 1, False)):
        assert analysis.is_cut(s, 150) == R.is_cut(s.inter, s.intra, s.has_prev, 150)


# ---------------------------------------------------------------------------------- the decision on synthetic material
_SCRIPTS = {}


def _script(h, w, dtype=np.float32):
    """FrameStats of the 12-frame two-scene sequence, frame by frame (computed once per size and dtype)"""
    key = (h, w, np.dtype(dtype).name)
    if key not in _SCRIPTS:
        prev, out = None, []
        for x in R.two_scene_frames(h, w):
            L, (inter, intra, total, blocks) = R.analyze(x[0, 0].astype(dtype), prev)
            out.append(analysis.FrameStats(inter, intra, total, blocks, prev is not None))
            prev = L
        _SCRIPTS[key] = out
    return _SCRIPTS[key]


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("hw", [(64, 64), (136, 200)])
def test_cuts_of_the_two_scene_sequence(hw, dtype):
    """the seed change at frame 5 and the wrap of the generator's shift at frame 8 stand clear of every moving frame"""
    stats = _script(*hw, dtype)
    ratio = [s.inter / max(s.intra, 1) for s in stats]
    print("inter / intra per frame:", [round(r, 3) for r in ratio])
    for fi, r in enumerate(ratio):
        if fi == 0:
            assert not stats[0].has_prev and stats[0].inter == 0
        elif fi == 5:
            assert 3.0 < r < 3.5
        elif fi == 8:
            assert 2.6 < r < 3.0
        else:
            assert 0.3 < r < 0.65
    assert [fi for fi, s in enumerate(stats) if analysis.is_cut(s, 150)] == [5, 8]


# ---------------------------------------------------------------------------------- the policy, pure Python
class _Stubs:
    """stub intra / inter codecs that record every call in one list"""

    def __init__(self):
        self.calls = []
        outer = self

        class I:
            def compress(self, x, qp):
                outer.calls.append(("i.compress", x, qp))
                return dict(bit_stream=b"I%d" % x, x_hat="rec%d" % x)

        class P:
            def set_curr_poc(self, poc):
                outer.calls.append(("set_curr_poc", poc))

            def clear_dpb(self):
                outer.calls.append(("clear_dpb",))

            def add_ref_frame(self, feature, frame):
                outer.calls.append(("add_ref_frame", feature, frame))

            def prepare_feature_adaptor_i(self, last_qp):
                outer.calls.append(("prepare_feature_adaptor_i", last_qp))

            def shift_qp(self, qp, fa_idx):
                return qp + 3 * fa_idx

            def compress(self, x, qp, defer_stream=False):
                outer.calls.append(("p.compress", x, qp, defer_stream))
                return dict(bit_stream=b"P%d" % x)

        self.i, self.p = I(), P()


class _Scripted:
    """an analyzer that replays a list of FrameStats and records what it was given"""

    def __init__(self, stats):
        self.stats, self.seen = list(stats), []

    def analyze(self, x, ready=None):
        self.seen.append((x, ready))
        return self.stats[x]


def _run(n=12, **kw):
    st = _Stubs()
    an = _Scripted(_script(64, 64))
    enc = SequenceEncoder(st.i, st.p, 20, 30, analyzer=an, **kw)
    pkts = [enc.encode(fi, ready="ev%d" % fi) for fi in range(n)]
    return enc, pkts, st, an


def _check_p_frames(pkts, reset_interval):
    """qp and use_ada_i of every P frame follow g, the distance to the most recent I frame"""
    g = 0
    for fi, p in enumerate(pkts):
        g = 0 if p.is_i else g + 1
        if p.is_i:
            assert (p.qp, p.use_ada_i) == (20, 0), fi
        else:
            assert p.qp == 30 + 3 * INDEX_MAP[g % 8], fi
            assert p.use_ada_i == int(reset_interval > 0 and g % reset_interval == 1), fi


@pytest.mark.parametrize("min_keyint,want_i", [(4, [0, 5]), (3, [0, 5, 8])])
def test_cut_frames_become_i_frames_unless_too_close(min_keyint, want_i):
    enc, pkts, st, an = _run(intra_period=-1, reset_interval=3, scenecut=150, min_keyint=min_keyint)
    assert [fi for fi, p in enumerate(pkts) if p.is_i] == want_i         # frame 8 has g = 3
    assert enc.scene_cuts == want_i[1:]
    _check_p_frames(pkts, 3)
    assert an.seen == [(fi, "ev%d" % fi) for fi in range(12)]            # every frame analysed, the event passed through
    assert [p.bit_stream for p in pkts] == [(b"I%d" if fi in want_i else b"P%d") % fi for fi in range(12)]
    # after a cut the references are dropped and the intra picture becomes the reference, as at frame 0
    k = st.calls.index(("i.compress", 5, 20))
    assert st.calls[k + 1:k + 3] == [("clear_dpb",), ("add_ref_frame", None, "rec5")]


def test_default_min_keyint_is_four():
    enc, pkts, _, _ = _run(intra_period=-1, scenecut=150)
    assert [fi for fi, p in enumerate(pkts) if p.is_i] == [0, 5] and enc.scene_cuts == [5]
    _check_p_frames(pkts, 32)


def test_intra_period_counts_from_the_cut():
    # cuts at 5 and 8 honoured (min_keyint 1): the period restarts there - fi % 4 would have put I frames at 4, 8
    enc, pkts, _, _ = _run(intra_period=4, reset_interval=2, scenecut=150, min_keyint=1)
    assert [fi for fi, p in enumerate(pkts) if p.is_i] == [0, 4, 5, 8] and enc.scene_cuts == [5, 8]
    _check_p_frames(pkts, 2)
    # min_keyint 2: the cut at 5 (g = 1) is refused, the cut at 8 falls on a periodic I frame (g = 4) and is listed
    enc, pkts, _, _ = _run(intra_period=4, reset_interval=2, scenecut=150, min_keyint=2)
    assert [fi for fi, p in enumerate(pkts) if p.is_i] == [0, 4, 8] and enc.scene_cuts == [8]
    # only the cut at 5 (threshold between the two ratios): 9 = 5 + 4 is periodic, 8 is not
    enc, pkts, _, _ = _run(intra_period=4, reset_interval=0, scenecut=300, min_keyint=1)
    assert [fi for fi, p in enumerate(pkts) if p.is_i] == [0, 4, 5, 9] and enc.scene_cuts == [5]
    _check_p_frames(pkts, 0)


def test_no_cut_and_g_equal_to_fi_gives_the_plain_sequence_of_calls():
    """a threshold above every ratio: with intra_period -1, and with a period that is a multiple of 8 and of the reset
    interval, the codecs are called exactly as without scenecut"""
    for kw in (dict(intra_period=-1, reset_interval=3), dict(intra_period=8, reset_interval=4)):
        _, pkts, st, _ = _run(scenecut=1000, **kw)
        plain = _Stubs()
        enc = SequenceEncoder(plain.i, plain.p, 20, 30, **kw)
        want = [enc.encode(fi) for fi in range(12)]
        assert st.calls == plain.calls and pkts == want


@pytest.mark.parametrize("scenecut", [None, 0])
@pytest.mark.parametrize("defer", [False, True])
def test_off_is_the_reference_policy_and_builds_no_analyzer(monkeypatch, scenecut, defer):
    def boom(*a, **k):
        raise AssertionError("an analyzer was constructed with scenecut off")

    monkeypatch.setattr(analysis, "FrameAnalyzer", boom)
    st = _Stubs()
    st.p.finish_stream = lambda: st.calls.append(("finish_stream",))
    an = _Scripted(_script(64, 64))
    enc = SequenceEncoder(st.i, st.p, 20, 30, intra_period=5, reset_interval=3, defer_stream=defer, scenecut=scenecut,
                          analyzer=an)
    for fi in range(12):
        enc.encode(fi)
    assert an.seen == [] and enc.scene_cuts == []
    # the reference harness's loop, restated: everything counts the frame index
    want = [("set_curr_poc", 0)]
    last_qp = 0
    for fi in range(12):
        if fi % 5 == 0:
            want += ([("finish_stream",)] if defer else []) + [("i.compress", fi, 20), ("clear_dpb",),
                                                               ("add_ref_frame", None, "rec%d" % fi)]
            continue
        if fi % 3 == 1:
            want.append(("prepare_feature_adaptor_i", last_qp))
        last_qp = 30 + 3 * INDEX_MAP[fi % 8]
        want.append(("p.compress", fi, last_qp, defer))
    assert st.calls == want


def test_bad_arguments():
    st = _Stubs()
    with pytest.raises(ValueError):
        SequenceEncoder(st.i, st.p, 20, scenecut=-5)
    with pytest.raises(ValueError):
        SequenceEncoder(st.i, st.p, 20, scenecut=150, min_keyint=0)


def test_harness_options():
    from opendcvc_amd import harness
    ap = harness.build_parser()
    a = ap.parse_args("--test-config m.json".split())
    assert (a.scenecut, a.min_keyint) == (0, 4)
    a = ap.parse_args("--test-config m.json --scenecut 150 --min-keyint 6".split())
    opts, _ = harness.manifest_options(a, ap)
    assert (opts["scenecut"], opts["min_keyint"]) == (150, 6)
