"""The frame lookahead without a GPU (docs/lookahead.md): the policy of opendcvc_amd.lookahead on the numpy restatement's costs
(tests/lookahead_ref.py) over the document's materials, the margin those materials keep from the threshold, depth and flush,
the weight / offset arithmetic at its edges, the new entries' refusals, SequenceEncoder.encode(cut=...) with stub codecs and
the command line."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import analysis_ref as A
import lookahead_ref as R
from opendcvc_amd import _lib, harness, lookahead
from opendcvc_amd.pipeline import SequenceEncoder

H, W, SCENECUT, DEPTH = 136, 200, 150, 4
MARGIN = 1.3                           # every deciding ratio lies at least this factor from SCENECUT
CUT_SEEDS = ((3, 11), (11, 5), (5, 7), (1, 2))


def _materials():
    m = {"steady": R.steady(H, W), "flash": R.flash(H, W), "flash_left_half": R.flash(H, W, left_half_only=True),
         "dissolve": R.dissolve(H, W)}
    for seeds in CUT_SEEDS:
        m["cut_%d_%d" % seeds] = R.real_cut(H, W, seeds=seeds)
    for name, target in (("fade_black", 0.0), ("fade_white", 1.0)):
        m[name] = R.fade(H, W, target)[0]
    for px in (8, 16, 24):
        m["pan_%d" % px] = R.pan(H, W, px)
    return m


_CACHE = {}


def material(name):
    """(the PlaneCosts of a material, its planes): made once, shared, never changed"""
    if not _CACHE:
        for k, frames in _materials().items():
            planes = R.planes_of(frames)
            _CACHE[k] = (R.PlaneCosts(planes), planes)
    return _CACHE[name]


def run_policy(costs, n, depth=DEPTH, scenecut=SCENECUT, flush_at=None):
    """opendcvc_amd.lookahead.CutPolicy driven the way Lookahead.push / flush drive it -> (cuts, flashes, fades)"""
    pol = lookahead.CutPolicy(costs, depth, scenecut)
    cuts, emitted = [], 0
    n = n if flush_at is None else flush_at
    for pushed in range(1, n + 1):
        if pushed > depth:
            if pol.decide(emitted, pushed):
                cuts.append(emitted)
            emitted += 1
    while emitted < n:                                  # flush: decided from what is there
        if pol.decide(emitted, n):
            cuts.append(emitted)
        emitted += 1
    return cuts, pol.flashes, pol.fades


def both(name, **kw):
    """the library's policy and the restatement's agree -> (cuts, flashes, fades)"""
    costs, planes = material(name)
    got = run_policy(costs, len(planes), **kw)
    want = R.decide(costs, len(planes), kw.get("depth", DEPTH), SCENECUT)[:3]
    assert got == tuple(want), (name, got, want)
    return got


# ---------------------------------------------------------------------------------- the policy on the document's materials
def test_steady_scene_has_no_cut_although_today_sees_one_at_its_jump():
    assert both("steady") == ([], [], [])
    assert R.today(material("steady")[1], SCENECUT)[0] == [8]


@pytest.mark.parametrize("seeds", CUT_SEEDS)
def test_a_real_cut_stays_a_cut(seeds):
    assert both("cut_%d_%d" % seeds) == ([5], [], [])


@pytest.mark.parametrize("name", ["fade_black", "fade_white"])
def test_a_fade_costs_no_i_frame_and_every_fading_frame_is_labelled(name):
    fading = R.fade(8, 8, 0.0)[1]
    assert fading == list(range(3, 10))
    assert both(name) == ([], [], fading)
    assert R.today(material(name)[1], SCENECUT)[0] == fading            # the gap: today every fading frame is a cut


def test_a_two_frame_flash_is_one_flash():
    assert both("flash") == ([], [4], [])
    assert R.today(material("flash")[1], SCENECUT)[0][:3] == [4, 5, 6]  # today: into the flash, inside it, out of it


def test_a_flash_the_weights_cannot_explain_is_still_a_flash():
    assert both("flash_left_half") == ([], [4], [])
    costs, planes = material("flash_left_half")
    mc, wp = costs.costs(4, 3)
    assert lookahead.cutlike(wp, costs.intra(4), SCENECUT)              # not a fade: only the look ahead saves it


@pytest.mark.parametrize("px", [8, 16, 24])
def test_a_pan_is_no_cut(px):
    assert both("pan_%d" % px) == ([], [], [])
    if px == 8:
        assert R.today(material("pan_8")[1], SCENECUT)[0] == [1, 2, 3, 4, 5]


def test_a_dissolve_is_no_cut():
    assert both("dissolve") == ([], [], [])


def test_the_materials_keep_their_margin_from_the_threshold():
    """a condition on the inputs, not on the code: every figure a decision hung on is a factor 1.3 away from 150"""
    for name in _materials():
        costs, planes = material(name)
        ratios = R.deciding(R.decide(costs, len(planes), DEPTH, SCENECUT)[3])
        print(name, [round(r, 1) for r in ratios])
        for r in ratios:
            assert r <= SCENECUT / MARGIN or r >= SCENECUT * MARGIN, (name, r)


# ---------------------------------------------------------------------------------- depth and flush
def test_with_depth_one_the_flash_is_not_seen_to_end():
    cuts, flashes, fades = both("flash", depth=1)
    assert flashes == [] and 4 not in cuts and fades[:1] == [4]         # a uniform flash still passes as a fade ..
    cuts, flashes, fades = both("flash_left_half", depth=1)
    assert cuts[:1] == [4] and flashes == []                            # .. one the weights cannot explain is a cut at frame 4


def test_flush_decides_from_what_is_there():
    costs, planes = material("flash")
    # 6 frames: frame 4 has one frame ahead (the second flash frame): not seen to end, so it falls to rule 3
    assert run_policy(costs, len(planes), flush_at=6) == ([], [], [4, 5])
    # 7 frames: frame 6, back to the scene, is in view
    assert run_policy(costs, len(planes), flush_at=7) == ([], [4], [])
    costs, planes = material("flash_left_half")
    assert run_policy(costs, len(planes), flush_at=6)[0][:1] == [4]
    assert run_policy(costs, len(planes), flush_at=7) == ([], [4], [])
    assert run_policy(material("cut_3_11")[0], 10, flush_at=6) == ([5], [], [])       # the last frame: nothing ahead


def test_pair_costs_beyond_the_predecessor_are_asked_for_only_at_candidates():
    planes = material("steady")[1]
    fresh = R.PlaneCosts(planes)
    run_policy(fresh, len(planes))
    assert fresh.asked == [(t, t - 1) for t in range(1, len(planes))]
    fresh = R.PlaneCosts(material("flash")[1])
    run_policy(fresh, 10)
    assert fresh.asked == [(1, 0), (2, 1), (3, 2), (4, 3), (5, 3), (6, 3), (7, 6), (8, 7), (9, 8)]


def test_policy_arguments():
    costs = material("steady")[0]
    for bad in (-1, 17, True, "4", None):
        with pytest.raises(ValueError, match="lookahead depth"):
            lookahead.CutPolicy(costs, bad, 150)
    with pytest.raises(ValueError, match="scenecut"):
        lookahead.CutPolicy(costs, 4, 0)
    pol = lookahead.CutPolicy(costs, 4, 150)
    with pytest.raises(ValueError, match="in order"):
        pol.decide(1, 5)
    with pytest.raises(ValueError, match="in order"):
        pol.decide(0, 0)


# ---------------------------------------------------------------------------------- arithmetic
def test_cost_of_hand_computable_planes():
    cur = np.full((9, 17), 1000, np.int64)
    assert R.cost(cur, cur) == (0, 0, 64, 0, 1000, 0, 1000, 0)
    ref = cur.copy()
    ref[4, 8] = 1400                       # mean (153000 + 400 + 76) // 153 = 1003, ac = 152 * 3 + 397
    mc, wp, w, o, mean_cur, ac_cur, mean_ref, ac_ref = R.cost(cur, ref)
    assert (mean_ref, ac_ref, mean_cur, ac_cur) == (1003, 853, 1000, 0)
    assert (w, o) == (0, 1000) and wp == 0                      # a flat current plane: weight 0, the offset is its mean
    assert mc == 0                                              # every tile finds a candidate that avoids the one sample
    # a shift by (2, -3) samples is found exactly away from the edges; clamped coordinates repeat the border
    rng = np.random.default_rng(5)
    big = rng.integers(0, 65473, (30, 40))
    cur, ref = big[3:27, 3:35], big[5:29, 0:32]
    assert R._search(cur[8:16, 8:24], cur[8:16, 8:24]) == 0
    inner = np.abs(cur - np.roll(np.roll(ref, 2, 0), -3, 1))[8:16, 8:24].sum()
    assert inner == 0 and R.cost(cur, ref)[0] < R.cost(cur, cur[::-1])[0]


def test_weight_and_offset_at_the_edges():
    flat = lambda v: np.full((3, 5), v, np.int64)
    tex = np.arange(15, dtype=np.int64).reshape(3, 5) * 4000
    m, a = R.moments(tex)
    assert (m, a) == (28000, 224000)
    assert R.weight_offset(*R.moments(tex), *R.moments(flat(500))) == (64, m - 500)         # flat reference: weight 64
    assert R.weight_offset(*R.moments(flat(500)), *R.moments(tex)) == (0, 500)              # flat current plane
    assert R.cost(flat(0), flat(0)) == (0, 0, 64, 0, 0, 0, 0, 0)
    assert R.cost(flat(65472), flat(65472)) == (0, 0, 64, 0, 65472, 0, 65472, 0)
    assert R.cost(flat(65472), flat(0))[:4] == (15 * 65472, 0, 64, 65472)
    assert R.cost(flat(0), flat(65472))[:4] == (15 * 65472, 0, 64, -65472)
    # the weight clamps at 255 and nothing leaves 32 bits before the clamp (weighted() asserts it)
    small = (tex // 4000) * 4 + 65000
    w, o = R.weight_offset(*R.moments(tex), *R.moments(small))
    assert w == 255 and o == 28000 - ((R.moments(small)[0] * 255 + 32) >> 6) and o < -200000
    out = R.weighted(np.asarray([0, 65000, 65472, 65535]), w, o)
    assert out.min() >= 0 and out.max() <= 65535 and out[0] == 0
    assert (65535 * 255 + 32) < 2 ** 31 and abs(-65535 * 255 // 64) + 65535 < 2 ** 31
    assert R.weighted(np.asarray([65535]), 255, 65535)[0] == 65535 and R.weighted(np.asarray([0]), 0, -65535)[0] == 0


def test_cutlike_is_the_scene_cut_comparison():
    assert lookahead.cutlike(150, 100, 150) and not lookahead.cutlike(149, 100, 150)
    assert lookahead.cutlike(2, 0, 150) and not lookahead.cutlike(1, 0, 150)                # max(intra, 1)
    assert lookahead.cutlike(2 ** 62, 2 ** 61, 150) and not lookahead.cutlike(2 ** 62, 2 ** 61, 250)
    for c, i in ((150, 100), (149, 100), (7, 0)):
        assert lookahead.cutlike(c, i, 150) == R.cutlike(c, i, 150) == A.is_cut(c, i, True, 150)


# ---------------------------------------------------------------------------------- the entries' refusals
_BUF = ctypes.create_string_buffer(4096 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63
_GOOD = dict(cur=_PTR, ref=_PTR + 1024, bh=9, bw=17, workspace=_PTR + 2048, out_host=_PTR + 3072)
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libdcvc_amd.so not built")


def _cost(**kw):
    a = dict(_GOOD, **kw)
    return _lib.lib().dcvc_lookahead_cost(a["cur"], a["ref"], a["bh"], a["bw"], a["workspace"], a["out_host"], None)


@needs_lib
@pytest.mark.parametrize("change, names", [(dict(cur=None), b"cur"), (dict(ref=None), b"ref"), (dict(workspace=None), b"workspace"),
                                           (dict(out_host=None), b"out_host"), (dict(cur=_PTR + 1), b"cur"),
                                           (dict(ref=_PTR + 1025), b"ref"), (dict(workspace=_PTR + 2052), b"workspace"),
                                           (dict(out_host=_PTR + 3076), b"out_host"), (dict(bh=0), b"bh x bw"),
                                           (dict(bw=-3), b"bh x bw"), (dict(bh=1 << 13, bw=(1 << 11) + 1), b"bh x bw")])
def test_a_bad_argument_is_refused_by_name_before_any_launch(change, names):
    before = bytes(_BUF)
    assert _cost(**change) == -1
    err = _lib.lib().dcvc_last_error()
    assert b"dcvc_lookahead_cost" in err and names in err, err
    assert bytes(_BUF) == before


@needs_lib
def test_workspace_query():
    L = _lib.lib()
    assert L.dcvc_lookahead_ws_bytes(1, 1) == 8 * (4 + 2)                   # the moments, one workgroup's partials
    assert L.dcvc_lookahead_ws_bytes(135, 240) == 8 * (4 + 2 * 128)         # 17 x 30 = 510 tiles, four per workgroup
    assert L.dcvc_lookahead_ws_bytes(4096, 4096) == 8 * (4 + 2 * 1024)      # capped: the waves stride over the tiles
    for bad in ((0, 5), (5, 0), (-1, -1), (4097, 4096)):
        assert L.dcvc_lookahead_ws_bytes(*bad) == -1
        assert b"dcvc_lookahead_ws_bytes" in L.dcvc_last_error()


# ---------------------------------------------------------------------------------- SequenceEncoder.encode(cut=...)
class _Stubs:
    def __init__(self):
        self.calls = []
        outer = self

        class I:
            def compress(self, x, qp):
                outer.calls.append(("i", x))
                return dict(bit_stream=b"I", x_hat="rec")

        class P:
            def set_curr_poc(self, poc):
                pass

            def clear_dpb(self):
                pass

            def add_ref_frame(self, feature, frame):
                pass

            def prepare_feature_adaptor_i(self, last_qp):
                pass

            def shift_qp(self, qp, fa_idx):
                return qp

            def compress(self, x, qp, defer_stream=False):
                outer.calls.append(("p", x))
                return dict(bit_stream=b"P")

        self.i, self.p = I(), P()


@pytest.mark.parametrize("scenecut", [None, 0])
def test_encode_cut_is_refused_without_scenecut(scenecut):
    st = _Stubs()
    enc = SequenceEncoder(st.i, st.p, 20, 30, scenecut=scenecut)
    for cut in (True, False):
        with pytest.raises(ValueError, match="scenecut"):
            enc.encode(0, cut=cut)
    assert st.calls == [] and enc.frame_idx == 0
    assert enc.encode(0).is_i and enc.encode(1, cut=None).is_i is False     # None: today's call


def test_encode_cut_takes_the_callers_word_and_keeps_the_encoders_rules():
    class NoAnalyzer:
        def analyze(self, x, ready=None):
            raise AssertionError("the analyzer ran although the caller gave the decision")

    st = _Stubs()
    enc = SequenceEncoder(st.i, st.p, 20, 30, scenecut=150, min_keyint=3, intra_period=8, analyzer=NoAnalyzer())
    word = {0: True, 2: True, 5: True, 6: True, 9: True}                 # frame 0 is an I frame anyway; 2, 6: too close
    pkts = [enc.encode(fi, cut=word.get(fi, False)) for fi in range(20)]
    assert [fi for fi, p in enumerate(pkts) if p.is_i] == [0, 5, 9, 17]  # 17: the period, counted from the cut at 9
    assert enc.scene_cuts == [5, 9]
    assert inspect.signature(SequenceEncoder.encode).parameters["cut"].default is None


# ---------------------------------------------------------------------------------- the command line
def test_lookahead_kwargs_and_the_command_line():
    assert harness.lookahead_kwargs({}) == {"lookahead": 0} == harness.lookahead_kwargs({"lookahead": None})
    assert harness.lookahead_kwargs({"lookahead": 4, "x": 1}) == {"lookahead": 4}
    assert inspect.signature(harness.run_one_point).parameters["lookahead"].default == 0
    assert inspect.signature(harness._encode_pass).parameters["lookahead"].default == 0
    assert "lookahead" not in [name for name, _, _ in harness.POINT_OPTIONS]
    ap = harness.build_parser()
    base = "--src a.yuv --width 64 --height 64 --frames 1"
    assert ap.get_default("lookahead") == 0
    args = ap.parse_args((base + " --scenecut 150 --lookahead 4").split())
    assert harness.lookahead_kwargs(vars(args)) == {"lookahead": 4}
    for bad in ("-1", "17", "auto"):
        with pytest.raises(SystemExit):
            ap.parse_args((base + f" --scenecut 150 --lookahead {bad}").split())
    args = ap.parse_args("--test-config m.json --gpus 1 --gpu-ids 0 --scenecut 150 --lookahead 2".split())
    opts, _ = harness.manifest_options(args, ap)
    assert opts["lookahead"] == 2 and harness.lookahead_kwargs(opts) == {"lookahead": 2}    # the pool's options carry it


def test_lookahead_without_scenecut_is_refused(capsys, tmp_path):
    with pytest.raises(SystemExit):
        harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --lookahead 4 --out {os.devnull}".split())
    assert "--scenecut" in capsys.readouterr().err

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"a net was touched ({name}) before the arguments were checked")

    with pytest.raises(ValueError, match="scenecut"):
        harness.run_one_point(Untouchable(), Untouchable(), str(tmp_path / "missing.yuv"), 64, 64, 2, 32, device="cuda:7",
                              lookahead=4)
    for bad in (17, -1, True, "4", None):
        with pytest.raises(ValueError, match="lookahead depth"):
            harness.run_one_point(Untouchable(), Untouchable(), str(tmp_path / "missing.yuv"), 64, 64, 2, 32, device="cuda:7",
                                  scenecut=150, lookahead=bad)


def test_run_job_and_main_hand_on_the_same_keyword(monkeypatch):
    seen = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: seen.append(kw) or {})
    monkeypatch.setattr(harness, "run_sweep", lambda *a, **kw: seen.append(kw) or {})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    harness.run_job(("i", "p"), job, {})
    harness.run_job(("i", "p"), job, {"scenecut": 150, "lookahead": 3})
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --scenecut 150 --lookahead 3 --out {os.devnull}".split())
    harness.main(f"--src a.yuv --width 64 --height 64 --frames 1 --scenecut 150 --out {os.devnull}".split())
    assert [kw["lookahead"] for kw in seen] == [0, 3, 3, 0]
    assert [kw["scenecut"] for kw in seen] == [0, 150, 150, 150]


def test_run_one_point_hands_the_option_to_the_encode_pass(monkeypatch, tmp_path):
    class Stop(Exception):
        pass

    seen = []

    def encode_pass(*a, **kw):
        seen.append(kw)
        raise Stop

    class Net:
        rate_estimate = entropy = None

        def set_use_two_entropy_coders(self, two):
            pass

    monkeypatch.setattr(harness, "_encode_pass", encode_pass)
    for kw in (dict(lookahead=4), dict(lookahead=0), {}):
        with pytest.raises(Stop):
            harness.run_one_point(Net(), Net(), str(tmp_path / "clip.yuv"), 64, 64, 2, 32, scenecut=150, **kw)
    assert seen == [{"lookahead": 4}, {}, {}]                            # off: the call of before the option
