"""The frame lookahead on the device (docs/lookahead.md): dcvc_lookahead_cost against the numpy restatement
(tests/lookahead_ref.py) word for word, lookahead.Lookahead against the policy on restated costs, SequenceEncoder.encode(cut=...)
and the harness option end to end."""
import ctypes

import numpy as np
import pytest
import torch

import analysis_ref as A
import lookahead_ref as R
from opendcvc_amd import weights

pytestmark = pytest.mark.gpu

_NP = {torch.float16: np.float16, torch.float32: np.float32}


# ---------------------------------------------------------------------------------- the pair cost
class _Entries:
    """the buffers dcvc_frame_analyze and dcvc_lookahead_cost need, allocated per case"""

    def __init__(self, bh, bw):
        from opendcvc_amd import _lib
        from opendcvc_amd.entropy import PinnedBuffer
        self.lib, self.check = _lib.lib(), _lib.check
        self.bh, self.bw = bh, bw
        self.pinned = PinnedBuffer(8 * 8)
        self.words = self.pinned.view(np.uint64, 8)
        self.ws = torch.empty(int(self.check(self.lib.dcvc_lookahead_ws_bytes(bh, bw), "dcvc_lookahead_ws_bytes")),
                              dtype=torch.uint8, device="cuda")
        self.ws_an = torch.empty(int(self.check(self.lib.dcvc_frame_analysis_ws_bytes(8 * bh, 8 * bw), "ws")), dtype=torch.uint8,
                                 device="cuda")

    def _st(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def plane(self, luma):
        """the low-resolution plane dcvc_frame_analyze makes of a [8 bh, 8 bw] device picture"""
        from opendcvc_amd import nn as L
        out = torch.zeros((self.bh, self.bw), dtype=torch.uint16, device="cuda")
        self.check(self.lib.dcvc_frame_analyze(L.dtype_code(luma.dtype), L._p(luma), luma.stride(0), 8 * self.bh, 8 * self.bw, None,
                                               L._p(out), L._p(self.ws_an), ctypes.c_void_p(self.pinned.ptr), self._st()),
                   "dcvc_frame_analyze")
        return out

    def cost(self, cur_ptr, ref_ptr):
        self.words[:] = 0xDEAD
        self.check(self.lib.dcvc_lookahead_cost(ctypes.c_void_p(cur_ptr), ctypes.c_void_p(ref_ptr), self.bh, self.bw,
                                                ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_void_p(self.pinned.ptr), self._st()),
                   "dcvc_lookahead_cost")
        self.check(self.lib.dcvc_stream_sync(self._st()), "dcvc_stream_sync")
        v = [int(x) for x in self.words]
        v[3] -= (v[3] >> 63) << 64
        return tuple(v)


def _u16_to_numpy(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int64)


def _u16_from_numpy(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda().view(torch.uint16)


def _check_pair(ent, cur, ref):
    """cur, ref: int64 numpy planes -> the entry's words, equal to the restatement's both ways round"""
    dc, dr = _u16_from_numpy(cur), _u16_from_numpy(ref)
    got = ent.cost(dc.data_ptr(), dr.data_ptr())
    assert got == R.cost(cur, ref), (cur.shape, got, R.cost(cur, ref))
    assert ent.cost(dr.data_ptr(), dc.data_ptr()) == R.cost(ref, cur)
    assert ent.cost(dc.data_ptr(), dc.data_ptr())[:4] == (0, 0, 64, 0)           # a plane against itself
    return got


# 8 x 8: a 1 x 1 plane; 64 x 64: one full tile; 72 x 136: a 9 x 17 plane, partial tiles both ways; 136 x 200: 17 x 25
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("h,w", [(8, 8), (64, 64), (72, 136), (136, 200)])
def test_pair_cost_of_analysed_pictures_equals_the_restatement_word_for_word(h, w, dtype):
    ent = _Entries(h // 8, w // 8)
    flash = R.flash(h, w, n=6)                            # frames 3 (the scene), 4 and 5 (flashed)
    other = weights.synthetic_frame_yuv444(h, w, 4, 11)
    pics = [flash[3], flash[4], flash[5], other]
    planes = []
    for x in pics:
        luma = torch.from_numpy(x[0, 0]).to("cuda", dtype)
        p = ent.plane(luma)
        want = A.lowres(x[0, 0].astype(_NP[dtype]))
        assert np.array_equal(_u16_to_numpy(p), want)
        planes.append((p, want))
    words = {}
    for i, j in ((1, 0), (2, 0), (3, 0), (2, 1), (0, 3)):
        words[i, j] = ent.cost(planes[i][0].data_ptr(), planes[j][0].data_ptr())
        assert words[i, j] == R.cost(planes[i][1], planes[j][1]), (i, j)
    if h > 8:
        assert 4 * words[1, 0][1] < words[1, 0][0]           # the weights explain the flash: wp far below mc


# 1 x 1; one tile; partial tiles; the 1080p plane with its full grid (510 tiles, 128 workgroups); more tiles than the
# search's 1024 workgroups of four waves take in one pass (65 x 66 = 4290), so the waves' stride over the tiles runs
@pytest.mark.parametrize("bh,bw", [(1, 1), (8, 8), (9, 17), (3, 29), (135, 240), (520, 521)])
def test_pair_cost_of_random_planes_with_the_extreme_values(bh, bw):
    rng = np.random.default_rng(bh * 1000 + bw)
    ent = _Entries(bh, bw)
    cur, ref = rng.integers(0, 65473, (bh, bw)), rng.integers(0, 65473, (bh, bw))
    cur.reshape(-1)[::5] = 65472
    cur.reshape(-1)[1::7] = 0
    ref.reshape(-1)[::3] = 0
    ref.reshape(-1)[2::11] = 65472
    _check_pair(ent, cur, ref)
    if bh * bw > 1:
        smooth = (np.add.outer(np.arange(bh) * 37, np.arange(bw) * 91) % 60000).astype(np.int64)
        moved = np.roll(np.roll(smooth, 2, 0), -3, 1) // 2 + 700             # a shift inside the range, a gain and an offset
        got = _check_pair(ent, moved, smooth)
        assert got[2] != 64 and got[3] != 0


def test_flat_planes_and_full_scale():
    bh, bw = 9, 17
    ent = _Entries(bh, bw)
    rng = np.random.default_rng(3)
    tex = rng.integers(0, 65473, (bh, bw))
    flat = lambda v: np.full((bh, bw), v, np.int64)
    assert _check_pair(ent, tex, flat(500))[2] == 64                          # a flat reference: weight 64
    assert _check_pair(ent, flat(500), tex)[1:3] == (0, 0)                    # a flat current plane: weight 0, wp cost 0
    assert _check_pair(ent, flat(0), flat(0)) == (0, 0, 64, 0, 0, 0, 0, 0)
    assert _check_pair(ent, flat(65472), flat(65472)) == (0, 0, 64, 0, 65472, 0, 65472, 0)
    assert _check_pair(ent, flat(65472), flat(0))[:4] == (bh * bw * 65472, 0, 64, 65472)
    assert _check_pair(ent, flat(0), flat(65535))[:4] == (bh * bw * 65535, 0, 64, -65535)
    small = (tex // 4000) * 4 + 65000                                         # the weight clamps at 255
    assert _check_pair(ent, tex, small)[2] == 255


def test_planes_inside_a_larger_buffer_at_odd_sample_offsets():
    """the kernels read single samples: any 2-byte-aligned plane is taken, and what lies around it is not read as one"""
    bh, bw = 9, 17
    ent = _Entries(bh, bw)
    rng = np.random.default_rng(11)
    cur, ref = rng.integers(0, 65473, (bh, bw)), rng.integers(0, 65473, (bh, bw))
    buf = np.full(2 * bh * bw + 16, 40000, np.int64)
    buf[3:3 + bh * bw] = cur.reshape(-1)
    buf[3 + bh * bw + 4:3 + 2 * bh * bw + 4] = ref.reshape(-1)
    dev = _u16_from_numpy(buf)
    got = ent.cost(dev.data_ptr() + 2 * 3, dev.data_ptr() + 2 * (3 + bh * bw + 4))
    assert got == R.cost(cur, ref)


# ---------------------------------------------------------------------------------- Lookahead against the policy
H, W, SCENECUT, DEPTH = 136, 200, 150, 4


def _run_lookahead(frames, dtype, depth=DEPTH):
    from opendcvc_amd.lookahead import Lookahead
    la = Lookahead("cuda:0", depth, SCENECUT)
    xs = [torch.from_numpy(f).to("cuda", dtype) for f in frames]
    out = []
    for i, x in enumerate(xs):
        done = la.push(x)
        assert len(done) == (1 if i >= depth else 0)
        out += done
    out += la.flush()
    assert len(out) == len(xs) and all(a is b for (a, _), b in zip(out, xs))          # the frames themselves, in order
    return la, [i for i, (_, cut) in enumerate(out) if cut]


@pytest.mark.parametrize("name,dtype,want", [("flash", torch.float32, ([], [4], [])), ("flash", torch.float16, ([], [4], [])),
                                             ("flash_left_half", torch.float32, ([], [4], [])),
                                             ("fade_black", torch.float32, ([], [], list(range(3, 10)))),
                                             ("pan_24", torch.float16, ([], [], [])), ("cut", torch.float32, ([5], [], []))])
def test_lookahead_on_the_device_decides_like_the_policy_on_restated_costs(name, dtype, want):
    frames = {"flash": lambda: R.flash(H, W), "flash_left_half": lambda: R.flash(H, W, left_half_only=True),
              "fade_black": lambda: R.fade(H, W, 0.0)[0], "pan_24": lambda: R.pan(H, W, 24), "cut": lambda: R.real_cut(H, W)}[name]()
    la, cuts = _run_lookahead(frames, dtype)
    planes = R.planes_of(frames, _NP[dtype])
    costs = R.PlaneCosts(planes)
    ref_cuts, ref_flashes, ref_fades, _ = R.decide(costs, len(planes), DEPTH, SCENECUT)
    assert (cuts, la.flashes, la.fades) == (ref_cuts, ref_flashes, ref_fades) == want
    assert la.pair_costs == len(costs.asked)               # pairs beyond (t, t - 1) only where a frame looked like a cut
    # the object starts another sequence after flush(); depth 1 does not see the flash end
    if name == "flash_left_half":
        la1, cuts1 = _run_lookahead(frames, dtype, depth=1)
        assert (cuts1, la1.flashes, la1.fades) == tuple(R.decide(R.PlaneCosts(planes), len(planes), 1, SCENECUT)[:3])
        assert cuts1[:1] == [4]
        again = [cut for _, cut in sum((la.push(torch.from_numpy(f).cuda()) for f in frames), []) + la.flush()]
        assert [i for i, c in enumerate(again) if c] == [] and la.flashes == [4]


# ---------------------------------------------------------------------------------- the encoder and the harness
S = 64
QP = 30


def _codecs():
    from opendcvc_amd.models import DMC, DMCI
    i_net, p_net = DMCI(), DMC()
    i_net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict("dmci", 1234).items()})
    p_net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict("dmc", 1234).items()})
    for m in (i_net, p_net):
        m.to("cuda").eval()
        m.update(0.12)
        m.set_use_two_entropy_coders(False)
    return i_net, p_net


@pytest.fixture(scope="module")
def nets():
    return _codecs()


def test_encode_with_the_encoders_own_cuts_handed_back_gives_the_same_packets(nets):
    from opendcvc_amd.pipeline import SequenceEncoder
    frames = [torch.from_numpy(f).cuda() for f in A.two_scene_frames(S, S, n=8)]
    own = SequenceEncoder(nets[0], nets[1], QP, intra_period=-1, reset_interval=3, scenecut=150)
    want = [own.encode(x) for x in frames]
    assert own.scene_cuts == [5] and own._analyzer is not None
    told = SequenceEncoder(nets[0], nets[1], QP, intra_period=-1, reset_interval=3, scenecut=150)
    got = [told.encode(x, cut=fi in own.scene_cuts) for fi, x in enumerate(frames)]
    assert told.scene_cuts == [5] and told._analyzer is None
    assert [(p.is_i, p.qp, p.use_ada_i, p.bit_stream) for p in got] == [(p.is_i, p.qp, p.use_ada_i, p.bit_stream) for p in want]
    with pytest.raises(ValueError, match="scenecut"):
        SequenceEncoder(nets[0], nets[1], QP).encode(frames[0], cut=False)


def _write_yuv(path, frames):
    """float [1, 3, h, w] frames as planar 8-bit 4:2:0"""
    with open(path, "wb") as f:
        for x in frames:
            q = np.clip(np.rint(x[0] * np.float32(255.0)), 0, 255).astype(np.uint8)
            for plane in (q[0], q[1, ::2, ::2], q[2, ::2, ::2]):
                f.write(np.ascontiguousarray(plane).tobytes())


@pytest.fixture(scope="module")
def flash_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("lookahead") / "flash.yuv"
    _write_yuv(path, R.flash(S, S))
    return path


def _point(nets, src, tag, frames=10, **kw):
    from opendcvc_amd import harness
    bin_path = src.parent / f"{tag}.bin"
    log = harness.run_one_point(nets[0], nets[1], str(src), S, S, frames, QP, QP, intra_period=-1, verbose_json=True,
                                bin_path=str(bin_path), **kw)
    return log, bin_path.read_bytes()


def test_harness_codes_the_flash_without_an_i_frame(nets, flash_file):
    plain, plain_bin = _point(nets, flash_file, "plain", scenecut=150)
    assert plain["scene_cuts"] and plain["scene_cuts"][0] == 4 and plain["frame_type"][4] == 0       # today: the flash costs an I frame
    log, data = _point(nets, flash_file, "la4", scenecut=150, lookahead=4)
    assert log["frame_type"] == [0] + [1] * 9
    assert (log["lookahead"], log["flashes"], log["fades"], log["scene_cuts"]) == (4, [4], [], [])
    assert list(log) == list(plain) + ["lookahead", "flashes", "fades"]
    assert len(log["frame_psnr"]) == 10 and all(np.isfinite(v) and 0 < v < 99 for v in log["frame_psnr"])
    # off, by 0 and by absence: the stream and the log's keys of before the option
    zero, zero_bin = _point(nets, flash_file, "la0", scenecut=150, lookahead=0)
    assert zero_bin == plain_bin and list(zero) == list(plain) and zero["scene_cuts"] == plain["scene_cuts"]
    assert data != plain_bin


def test_harness_lookahead_behind_the_filter_and_the_resampler(nets, flash_file):
    n = 10
    log, _ = _point(nets, flash_file, "all", frames=n, scenecut=150, lookahead=2, temporal_filter=3, coded_size=(48, 48),
                    digest=True, film_grain="auto", target_bpp=0.5)
    assert log["digests_checked"] == n and log["lookahead"] == 2 and len(log["frame_type"]) == n
    assert log["frame_type"][0] == 0 and (log["coded_height"], log["coded_width"]) == (48, 48)
    assert "grain_units" in log and log["tf_level"] == 3 and "target_bpp" in log
    assert all(np.isfinite(v) for v in log["frame_psnr"])
