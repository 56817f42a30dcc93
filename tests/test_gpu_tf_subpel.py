"""Quarter-pel motion of the temporal pre-filter on the GPU (docs/temporal_filter.md, "Quarter-pel motion"): dcvc_tf_refine and
dcvc_tf_blend_subpel against the numpy restatement (tests/tf_subpel_ref.py, held against hand-computed samples and the
document's figures on the CPU by tests/test_tf_subpel_host.py) bit for bit, TemporalFilter(subpel=...) in all its uses, and
--tf-subpel end to end through the harness against a loop of the test's own."""
import ctypes
import io

import numpy as np
import pytest
import torch

import tf_auto_ref as A
import tf_ref as R
import tf_subpel_ref as S
from opendcvc_amd import _lib, harness
from opendcvc_amd.prefilter import TemporalFilter, window
from tf_utils import _bits, _padded_shape, _to_device, clip_fixture, tex  # noqa: F401 (tex: a fixture)

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float32, np.float32), (torch.float16, np.float16)]
SIZES = [(5, 11),                  # smaller than a block in both directions: one block, every tap of every row and column clamps
         (16, 16),                 # tests/test_gpu_tf.py's sizes: every window clamps
         (33, 40),                 # a 48 x 48 tensor carved one element into a larger allocation
         (70, 118),                # partial blocks on both edges
         (136, 200)]               # the document's texture: many blocks
DISTS = (-1, 1, -2, 2)
REF_SETS = {0: [], 1: [1], 2: [1, 2], 3: [-1, 1, 2], 4: [-1, 1, -2, 2]}


def displacement(i, band):
    """of band `band` (16 rows: two rows of blocks) of reference number i, in quarter pels: over the bands and the references
    every pair of phases, whole parts 0 .. 2, both signs"""
    sign = 1 if i % 2 == 0 else -1
    return sign * (4 * ((band + i) % 3) + band % 4), -sign * (4 * ((2 * band + i) % 3) + (band // 4 + i) % 4)


def material(tex, size, ndt, shifted):
    """distance -> a read-only frame [3, Hp, Wp] (NaN outside the picture): the texture under noise of 2 / 255, in a reference
    displaced band by band (displacement(); the first band of the first reference not at all), so that one picture holds
    whole and fractional motion of every phase.  shifted: a dict that keeps the displaced textures between calls"""
    h, w = size
    rng = np.random.default_rng(h * 1000 + w)
    host = {}
    for d in (0,) + DISTS:
        pic = np.empty((3, h, w))
        for band in range((h + 15) // 16):
            q = (0, 0) if d == 0 else displacement(DISTS.index(d), band)
            if q not in shifted:
                shifted[q] = S.fourier_shift(tex, q[0] / 4.0, q[1] / 4.0)
            pic[:, 16 * band:16 * band + 16] = R.shift(shifted[q], 0, 0, h, w)[:, 16 * band:16 * band + 16]
        f = np.full((3,) + _padded_shape(size), np.nan, ndt)
        f[:, :h, :w] = (pic * 1.1 - 0.05 + rng.standard_normal((3, h, w)) * (2.0 / 255.0)).astype(ndt)
        if d == 0:
            f[0, 0, 0] = -0.0
        f.setflags(write=False)
        host[d] = f
    return host


def restated(host, size):
    """of material(): the whole-pel (mv, err), the refined (mvq, errq) for subpel 1 and 2, and the interpolated samples at the
    subpel 2 vectors, each per distance"""
    pyr = {d: R.pyramid(host[d], size) for d in host}
    whole = {d: R.motion(pyr[0], pyr[d]) for d in host if d}
    fine = {sp: {d: S.refine(pyr[0][0], pyr[d][0], whole[d][0], sp) for d in whole} for sp in (1, 2)}
    samples = {d: S.interp_f32(host[d], size, fine[2][d][0]) for d in whole}
    return whole, fine, samples


@pytest.fixture(scope="module")
def frames(tex):
    """per (size, numpy dtype): material() on the host and on the device ((33, 40): one element into a larger allocation, as
    tests/test_gpu_tf.py has it) and restated() of it"""
    cache, shifted = {}, {}

    def get(size, ndt):
        if (size, ndt) not in cache:
            host = material(tex, size, ndt, shifted)
            dev = {d: _to_device(f, size == (33, 40)) for d, f in host.items()}
            cache[(size, ndt)] = (host, dev) + restated(host, size)
        return cache[(size, ndt)]
    yield get
    cache.clear()
    shifted.clear()


@pytest.fixture(scope="module")
def filters():
    made = {}

    def get(level, radius=2, subpel=2):
        if (level, radius, subpel) not in made:
            made[(level, radius, subpel)] = TemporalFilter("cuda:0", level, radius, subpel)
        return made[(level, radius, subpel)]
    yield get
    made.clear()


# ---------------------------------------------------------------------------------- refinement
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_motion_subpel_equals_the_restatement(frames, filters, size, tdt, ndt):
    host, dev, whole, fine, _ = frames(size, ndt)
    gh, gw = R.grid(*size)
    if gh * gw >= 100:
        # the restatement was asked something: whole and fractional vectors, all 16 phases, both signs of both components
        mvq = np.concatenate([fine[2][d][0].reshape(-1, 2) for d in fine[2]]).astype(np.int32)
        phases = {(int(y) & 3, int(x) & 3) for y, x in mvq}
        print(f"{size} {ndt.__name__}: phases {len(phases)}, whole {int(((mvq & 3) == 0).all(axis=1).sum())} of {len(mvq)}, "
              f"components {mvq.min(axis=0)} .. {mvq.max(axis=0)}")
        assert len(phases) == 16 and ((mvq & 3) == 0).all(axis=1).sum() >= 10
        assert (mvq[:, 0] < 0).any() and (mvq[:, 0] > 0).any() and (mvq[:, 1] < 0).any() and (mvq[:, 1] > 0).any()
        half = np.concatenate([fine[1][d][0].reshape(-1, 2) for d in fine[1]])
        assert not (half & 1).any() and ((half & 3) == 2).any()
    for subpel in (1, 2):
        tf = filters(3, 2, subpel)
        for d in (-2, -1, 1, 2):
            mvq, errq = tf.motion_subpel(dev[0], dev[d], size)
            mvq, errq = mvq.cpu().numpy(), errq.cpu().numpy()
            want_mv, want_err = fine[subpel][d]
            assert mvq.shape == (gh, gw, 2) and mvq.dtype == np.int16 and errq.shape == (gh, gw)
            wrong = int((mvq != want_mv).any(axis=2).sum())
            print(f"{size} {ndt.__name__} subpel {subpel} distance {d}: {wrong} of {gh * gw} vectors differ")
            assert wrong == 0 and np.array_equal(errq.astype(np.uint32), want_err)
            mv, err = tf.motion(dev[0], dev[d], size)                          # the whole-pel outputs are the search's still
            assert np.array_equal(mv.cpu().numpy(), whole[d][0]) and np.array_equal(err.cpu().numpy().astype(np.uint32), whole[d][1])


def test_exact_matches_keep_their_centres(filters):
    """a reference that equals the current frame in its upper part: whole workgroups of level-0 SAD 0 (which leave early)
    beside mixed and noisy ones; and one that equals it everywhere"""
    size, rng = (70, 118), np.random.default_rng(9)
    cur = np.full((3, 80, 128), np.nan, np.float16)
    cur[:, :70, :118] = rng.random((3, 70, 118)).astype(np.float16)
    ref = cur.copy()
    ref[:, 43:70, :118] = (ref[:, 43:70, :118].astype(np.float32) + rng.standard_normal((3, 27, 118)) * (3.0 / 255.0)).astype(np.float16)
    pyr_c = R.pyramid(cur, size)
    tf = filters(3, 2, 2)
    for other in (ref, cur):
        pyr_r = R.pyramid(other, size)
        mv, err = R.motion(pyr_c, pyr_r)
        want_mv, want_err = S.refine(pyr_c[0], pyr_r[0], mv, 2)
        assert (want_err[:5] == 0).all() and (other is cur or (want_err[6:] > 0).all())
        mvq, errq = tf.motion_subpel(_to_device(cur), _to_device(other), size)
        assert np.array_equal(mvq.cpu().numpy(), want_mv) and np.array_equal(errq.cpu().numpy().astype(np.uint32), want_err)


# ---------------------------------------------------------------------------------- blend
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("nref", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("level", [1, 3, 5])
@pytest.mark.parametrize("size", SIZES)
def test_filter_equals_the_restatement(frames, filters, size, level, nref, tdt, ndt):
    host, dev, _, fine, samples = frames(size, ndt)
    dists = REF_SETS[nref]
    want, want_total, _ = S.filter_frame(host[0], [host[d] for d in dists], dists, size, level, 2, [fine[2][d] for d in dists],
                                         [samples[d] for d in dists])
    tf = filters(level)
    tf.reset()
    out = torch.full_like(dev[0], 7.0)
    assert tf.filter(dev[0], [dev[d] for d in dists], dists, size, out=out) is out and out.dtype == tdt
    total = tf.weight_sum()
    got = out[0].cpu().numpy()
    H, W = size
    diff = int((_bits(got) != _bits(want)).sum())
    print(f"{size} level {level} {nref} refs {ndt.__name__}: {diff} of {got.size} elements differ, weight sum {total}")
    assert diff == 0 and total == want_total
    assert np.isfinite(got).all()
    rows, cols = np.minimum(np.arange(got.shape[1]), H - 1), np.minimum(np.arange(got.shape[2]), W - 1)
    assert np.array_equal(_bits(got), _bits(got[:, :H, :W][:, rows][:, :, cols]))          # the pad: the filtered picture's replicate
    if level >= 3 and nref and H * W > 64:
        assert total > 0 and (_bits(got[:, :H, :W]) != _bits(host[0][:, :H, :W])).mean() > 0.5      # not the identity
    for d in [0] + dists:
        assert np.array_equal(_bits(dev[d][0].cpu().numpy()), _bits(host[d]))                      # the inputs are untouched


@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size", [(5, 11), (33, 40), (70, 118)])
def test_given_vectors_that_point_outside_every_edge(frames, filters, size, tdt, ndt):
    """vectors no search would find, through `motions`: every component up to +-91 quarter pels, the extremes forced into the
    corner blocks, so that on every side all the taps clamp; errors small enough for every block to take part"""
    host, dev, _, _, _ = frames(size, ndt)
    gh, gw = R.grid(*size)
    rng = np.random.default_rng(size[0] * 7 + size[1])
    dists = [-1, 1, -2, 2]
    motions = []
    for i in range(4):
        mvq = rng.integers(-91, 92, (gh, gw, 2)).astype(np.int16)
        mvq[0, 0], mvq[-1, -1] = [(-91, -91), (-90, -89), (-91, 91), (-89, -91)][i], [(91, 91), (90, 89), (91, -91), (89, 91)][i]
        mvq[0, -1], mvq[-1, 0] = (-91, 91), (91, -91)
        motions.append((mvq, rng.integers(0, 300, (gh, gw)).astype(np.uint32)))
    want, want_total, _ = S.filter_frame(host[0], [host[d] for d in dists], dists, size, 5, 2, motions)
    tf = filters(5)
    tf.reset()
    given = [(torch.from_numpy(m).cuda(), torch.from_numpy(e.astype(np.int32)).cuda()) for m, e in motions]
    out = tf.filter(dev[0], [dev[d] for d in dists], dists, size, motions=given)
    got = out[0].cpu().numpy()
    assert np.isnan(host[1][:, size[0]:]).all() and np.isnan(host[1][:, :, size[1]:]).all()      # the padding is NaN
    assert np.array_equal(_bits(got), _bits(want)) and tf.weight_sum() == want_total > 0
    assert np.isfinite(got).all()                                                                # the picture and its pad
    with pytest.raises(ValueError):
        tf.filter(dev[0], [dev[d] for d in dists], dists, size, motions=given[:3])


@pytest.mark.parametrize("tdt,ndt", DTYPES)
def test_subpel_0_is_the_filter_of_today(frames, tdt, ndt):
    size, dists = (70, 118), [-1, 1, -2, 2]
    host, dev, whole, _, _ = frames(size, ndt)
    today, off = TemporalFilter("cuda:0", 3, 2), TemporalFilter("cuda:0", 3, 2, subpel=0)
    a = today.filter(dev[0], [dev[d] for d in dists], dists, size)
    b = off.filter(dev[0], [dev[d] for d in dists], dists, size)
    want, want_total, _ = R.filter_frame(host[0], [host[d] for d in dists], dists, size, 3, [whole[d] for d in dists])
    assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(b[0].cpu().numpy())) and np.array_equal(_bits(b[0].cpu().numpy()), _bits(want))
    assert today.weight_sum() == off.weight_sum() == want_total
    assert off.subpel == 0 and off._mvq is None and off._errq is None          # nothing of the option is made
    with pytest.raises(ValueError, match="subpel"):
        off.motion_subpel(dev[0], dev[1], size)
    for bad in (3, -1, True, "2"):
        with pytest.raises(ValueError, match="subpel"):
            TemporalFilter("cuda:0", 3, 2, bad)
    # whole vectors through the interpolating blend: the same bits once more
    fine = TemporalFilter("cuda:0", 3, 2, 2)
    given = [(torch.from_numpy(4 * whole[d][0]).cuda(), torch.from_numpy(whole[d][1].astype(np.int32)).cuda()) for d in dists]
    c = fine.filter(dev[0], [dev[d] for d in dists], dists, size, motions=given)
    assert np.array_equal(_bits(c[0].cpu().numpy()), _bits(want)) and fine.weight_sum() == want_total


# ---------------------------------------------------------------------------------- the level from the picture
@pytest.mark.parametrize("tdt,ndt", DTYPES)
@pytest.mark.parametrize("size", [(33, 40), (136, 200)])
def test_auto_reads_the_refined_errors(frames, size, tdt, ndt):
    host, dev, whole, fine, samples = frames(size, ndt)
    dists = [-1, 1, -2, 2]
    refs_h, refs_d = [host[d] for d in dists], [dev[d] for d in dists]
    pyr = R.pyramid(host[0], size)
    want_four = A.noise(pyr[0], [fine[2][d][1] for d in dists], dists)
    whole_four = A.noise(pyr[0], [whole[d][1] for d in dists], dists)
    print(f"{size} {ndt.__name__}: estimate with errq {want_four}, with err {whole_four}")
    tf = TemporalFilter("cuda:0", "auto", 2, 2)
    assert tf.noise(dev[0], refs_d, dists, size) == want_four
    if size == (136, 200):
        assert want_four[2] < whole_four[2] and want_four[0] >= 1              # the temporal figure no longer reads the motion as noise
    motions, smp = [fine[2][d] for d in dists], [samples[d] for d in dists]
    want, want_total, _ = S.filter_frame(host[0], refs_h, dists, size, want_four[0], 2, motions, smp) if want_four[0] else \
        R.filter_frame(host[0], [], [], size, 3)
    tf.reset()
    out = tf.filter(dev[0], refs_d, dists, size)                               # (enqueues only: estimate and blend with no read-back between)
    # the blend reads the level's word on the device: another word, put there without the host looking at it, another level
    other = 5 if want_four[0] != 5 else 3
    tf._result[0:1].fill_(other)
    again = torch.empty_like(out)
    tf._blend(tf._frame(dev[0]), [tf._frame(r) for r in refs_d], dists, size, again)
    assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(again[0].cpu().numpy()), _bits(S.filter_frame(host[0], refs_h, dists, size, other, 2, motions, smp)[0]))
    assert tf.levels() == A.totals([want_four])
    got_total = tf.weight_sum()
    assert got_total == want_total + S.filter_frame(host[0], refs_h, dists, size, other, 2, motions, smp)[1]
    got = S.filter_auto(host[0], refs_h, dists, size)                          # the restatement from the frames alone agrees with the pieces
    assert got[2] == want_four and np.array_equal(_bits(got[0]), _bits(want))


# ---------------------------------------------------------------------------------- a sequence
@pytest.mark.parametrize("n,radius", [(6, 2), (5, 1), (1, 2), (2, 1)])
def test_push_and_flush_equal_filter_on_the_window(tex, filters, n, radius):
    size, rng = (70, 118), np.random.default_rng(n * 10 + radius)
    seq = []
    for t in range(n):
        f = np.full((3, 80, 128), np.nan, np.float16)
        f[:, :70, :118] = (S.moving(tex, t, (0.75, -1.25), 70, 118) + rng.standard_normal((3, 70, 118)) * (2.0 / 255.0)).astype(np.float16)
        seq.append(_to_device(f))
    ref_tf = filters(3, radius)
    ref_tf.reset()
    want = [ref_tf.filter(seq[t], [seq[i] for i, _ in refs], [d for _, d in refs], size) for t, refs in enumerate(window(n, radius))]
    want_total = ref_tf.weight_sum()
    tf = TemporalFilter("cuda:0", 3, radius, 2)
    got = []
    for x in seq:
        got += [o.clone() for o in tf.push(x, size)]
    got += [o.clone() for o in tf.flush()]
    assert len(got) == n and tf.weight_sum() == want_total
    for t in range(n):
        assert torch.equal(got[t].view(torch.int16), want[t].view(torch.int16)), f"frame {t}"
    if n > 2:                                    # the vectors were fractional, and it is not the whole-pel filter that ran
        assert bool((tf._mvq[0] & 3).ne(0).any()) and want_total > 0
        plain = filters(3, radius, 0)
        other = plain.filter(seq[2], [seq[1], seq[3]], [-1, 1], size)
        mine = ref_tf.filter(seq[2], [seq[1], seq[3]], [-1, 1], size)
        assert not torch.equal(other.view(torch.int16), mine.view(torch.int16))


# ---------------------------------------------------------------------------------- refused calls
def test_refused_calls_leave_the_outputs_untouched(frames):
    size, dists = (33, 40), [-1, 1]
    host, dev, _, _, _ = frames(size, np.float16)
    tf = TemporalFilter("cuda:0", 3, 2, 2)
    keep = torch.full_like(dev[0], 7.0)
    tf.filter(dev[0], [dev[d] for d in dists], dists, size)                    # leaves pyramids, vectors and errors in the object
    L, n, (H, W) = _lib.lib(), 2 * tf.radius + 1, size
    gh, gw = R.grid(H, W)
    pyr = tf._pyr[n].data_ptr()
    pyrs = (ctypes.c_void_p * 4)(tf._pyr[n + 1].data_ptr(), tf._pyr[n + 2].data_ptr(), 0, 0)
    mv, err = tf._mv.data_ptr(), tf._err.data_ptr()
    mvq = torch.full((4, gh, gw, 2), -77, dtype=torch.int16, device="cuda")
    errq = torch.full((4 * gh * gw + 2,), -77, dtype=torch.int32, device="cuda")
    q, e = mvq.data_ptr(), errq.data_ptr()
    calls = [(pyr, pyrs, 2, H, W, 0, mv, err, q, e),                           # subpel
             (pyr, pyrs, 2, H, W, 3, mv, err, q, e),
             (pyr, pyrs, 2, H, W, 2, mv, err, mv, e),                          # outputs that are inputs
             (pyr, pyrs, 2, H, W, 2, mv, err, q, err),
             (pyr, pyrs, 2, H, W, 2, mv, err, q, q),                           # ... or each other
             (pyr, pyrs, 2, H, W, 2, mv, err, q, e + 2),                       # misaligned
             (pyr, pyrs, 2, H, W, 2, mv, err, q + 1, e),
             (None, pyrs, 2, H, W, 2, mv, err, q, e),                          # NULL pointers
             (pyr, None, 2, H, W, 2, mv, err, q, e),
             (pyr, pyrs, 3, H, W, 2, mv, err, q, e),                           # (the third pyramid)
             (pyr, pyrs, 2, H, W, 2, None, err, q, e),
             (pyr, pyrs, 2, H, W, 2, mv, None, q, e),
             (pyr, pyrs, 2, H, W, 2, mv, err, None, e),
             (pyr, pyrs, 2, H, W, 2, mv, err, q, None),
             (pyr, pyrs, 0, H, W, 2, mv, err, q, e),                           # nref, sizes
             (pyr, pyrs, 5, H, W, 2, mv, err, q, e),
             (pyr, pyrs, 2, 0, W, 2, mv, err, q, e)]
    for args in calls:
        assert L.dcvc_tf_refine(*args, None) == -1 and L.dcvc_last_error().startswith(b"dcvc_tf_refine"), args
    torch.cuda.synchronize()
    assert bool((mvq == -77).all()) and bool((errq == -77).all())
    assert L.dcvc_tf_refine(pyr, pyrs, 2, H, W, 2, mv, err, q, e, None) == 0, L.dcvc_last_error()      # and the call goes through
    torch.cuda.synchronize()
    assert torch.equal(mvq[:2], tf._mvq[:2]) and torch.equal(errq[:2 * gh * gw].view(2, gh, gw), tf._errq[:2])
    assert bool((mvq[2:] == -77).all()) and bool((errq[2 * gh * gw:] == -77).all())
    # dcvc_tf_blend_subpel
    from opendcvc_amd import nn as NN
    code, cur_p, Hp, Wp, _, _ = NN.frame_args(dev[0], size)
    ptrs, d2 = (ctypes.c_void_p * 4)(dev[-1].data_ptr(), dev[1].data_ptr(), 0, 0), (ctypes.c_int * 4)(-1, 1, 0, 0)
    word = torch.full((2,), 3, dtype=torch.int32, device="cuda")
    o, tot = keep.data_ptr(), tf._total.data_ptr()

    tf.reset()                                    # (the refused calls: test_gpu_tf.py's table)  With a word the level is not looked at:
    assert L.dcvc_tf_blend_subpel(code, cur_p, ptrs, d2, 2, Hp, Wp, H, W, q, e, 0, word.data_ptr(), o, tot, None) == 0, L.dcvc_last_error()
    once = tf.weight_sum()
    again = tf.filter(dev[0], [dev[d] for d in dists], dists, size)
    assert torch.equal(keep.view(torch.int16), again.view(torch.int16)) and tf.weight_sum() == 2 * once > 0


# ---------------------------------------------------------------------------------- end to end
H, W, N = 136, 200, 4


clip = clip_fixture(H, W, N, "tf_subpel")   # a 136 x 200, 4-frame clip made like test_gpu_tf.py's


def _run(clip, name, **kw):
    nets, folder = clip
    path = str(folder / f"{name}.bin")
    log = harness.run_one_point(nets[0], nets[1], str(folder / "clip.yuv"), W, H, N, 32, 32, intra_period=2, reset_interval=32,
                                verbose_json=True, bin_path=path, **kw)
    return log, open(path, "rb").read()


def test_the_harness_codes_what_the_restatement_filters(clip):
    from opendcvc_amd.bitstream import StreamWriter
    from opendcvc_amd.pipeline import SequenceEncoder, use_two_entropy_coders
    nets, folder = clip
    log, data = _run(clip, "tf3q", temporal_filter=3, tf_subpel=2)
    assert list(log)[-4:] == ["tf_level", "tf_radius", "tf_mean_weight", "tf_subpel"]
    assert (log["tf_level"], log["tf_radius"], log["tf_subpel"]) == (3, 2, 2)
    src = harness.make_source("yuv420", str(folder / "clip.yuv"), W, H)
    reader = src.reader()
    host = [src.to_input(harness._to_device(reader.read(), "cuda:0"), torch.float32)[0].cpu().numpy() for _ in range(N)]
    reader.close()
    enc = SequenceEncoder(nets[0], nets[1], qp_i=32, qp_p=32, intra_period=2, reset_interval=32)
    out = io.BytesIO()
    writer, two, total = StreamWriter(out), use_two_entropy_coders(H, W), 0
    for t, refs in enumerate(window(N, 2)):
        x, s, _ = S.filter_frame(host[t], [host[i] for i, _ in refs], [d for _, d in refs], (H, W), 3, 2)
        total += s
        writer.write_frame(H, W, two, enc.encode(torch.from_numpy(x)[None].cuda()))
    assert out.getvalue() == data                             # (the stream decoded inside run_one_point: the log has its PSNRs)
    assert total > 0 and log["tf_mean_weight"] == total / (256.0 * H * W * N)
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data) and log["i_frame_num"] + log["p_frame_num"] == N
    _, whole = _run(clip, "tf3", temporal_filter=3)
    assert whole != data


def test_subpel_0_and_no_option_are_the_run_of_today(clip):
    log0, data0 = _run(clip, "plain", temporal_filter=3)
    log, data = _run(clip, "zero", temporal_filter=3, tf_subpel=0)
    assert data == data0 and list(log) == list(log0) and "tf_subpel" not in log
    assert {k: v for k, v in log.items() if k != "test_time"} == {k: v for k, v in log0.items() if k != "test_time"}
    off0, plain0 = _run(clip, "off0")
    off, plain = _run(clip, "off", tf_subpel=2)               # without the filter the option does nothing
    assert plain == plain0 and list(off) == list(off0) and not [k for k in off if k.startswith("tf_")]


def test_with_the_other_extensions(clip):
    log, data = _run(clip, "all", temporal_filter="auto", tf_subpel=2, film_grain="auto", digest=True)
    assert log["digests_checked"] == N
    assert list(log)[-9:] == ["grain_units", "grain_scale_y", "grain_corr", "tf_level", "tf_radius", "tf_mean_weight", "tf_levels",
                              "tf_noise", "tf_subpel"]
    assert log["tf_level"] == "auto" and log["tf_subpel"] == 2 and sum(log["tf_levels"]) == N
    assert 0.0 <= log["tf_mean_weight"] <= 358.0 / 256.0
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data)
