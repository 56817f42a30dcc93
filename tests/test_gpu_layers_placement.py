"""The layer kernels (dcvc_nn.hip, dcb_t128.hpp) on the memory the models and the contract allow, not only on the easiest:
every source a channel-slice view (row stride > channels, 16-byte channel offset, another stride for the second source)
inside a NaN-filled buffer with guard bands, the output such a view of a NaN-filled buffer, quant / in_scale vectors of
exactly their documented length between NaNs, and the scratch filled with NaN immediately before the call
(layer_utils.GuardedRun: "a guarded run").  A kernel that used a width where it should use a row stride, a halo or a
ragged tile that read or wrote past the map, or a tail that read a scratch pixel nobody wrote in this run then gives a
non-finite or different output, or changes a guard byte.

Against the CPU oracle (fp32 bit-exact, fp16 within test_gpu_layers' bounds): every small case of test_gpu_layers, and on a
101 x 123 map (12 423 pixels: the large-map kernels, ragged against 8 x 16 and 8 x 8 tiles) its large cases plus four
forms the models reach that had no layer-level comparison.  Bitwise against the same objects on contiguous tensors:
chains, chains ending in a fused conv, the fragment-stream convs, the residual blocks writing into a concat slice.
A positive control per tail / head form shows that a NaN in one source pixel comes out in exactly its 3 x 3
neighbourhood: the receptive field of each form, and the proof that a NaN survives it."""
import functools

import numpy as np
import pytest
import torch

import dcvc_oracle as O
import test_gpu_layers as TL
from layer_utils import GuardedRun, make_conv_weights

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
LARGE = (101, 123)


def _scratch_bytes(blk, H, W):
    from opendcvc_amd import _lib
    return _lib.lib().dcvc_dcb_scratch_bytes(blk.h, H, W)


def _sources(x, cin_p, split, dtype, g):
    """x [H, W, cin] as the layer's one or two sources: contiguous tensors (g None) or guarded views"""
    parts = [(x, cin_p)] if not split else [(x[:, :, :split], split), (x[:, :, split:], cin_p - split)]
    if g is None:
        return [TL.to_dev(np.array(v), cp, dtype) for v, cp in parts]      # (a copy: the cached inputs are read-only)
    return [g.src(v, cp, second=i == 1) for i, (v, cp) in enumerate(parts)]


def _vec(q, g):
    if q is None:
        return None
    return torch.from_numpy(q).cuda() if g is None else g.vec(q)


def _run_block(sd, x, q, dtype, shortcut, split, guard):
    """one DepthConvBlock on x, plain or as a guarded run -> its logical output channels as float32 numpy"""
    from opendcvc_amd import nn
    blk = nn.DepthConvBlock(sd, "m", dtype, shortcut=shortcut)
    H, W = x.shape[:2]
    g = GuardedRun(dtype) if guard else None
    srcs = _sources(x, blk.cin_p, split, dtype, g)
    qd = _vec(q, g)
    out = None
    if g is not None:
        out = g.out(H, W, blk.c_p, blk.c)
        poisoned = g.scratch(_scratch_bytes(blk, H, W))
        # (the buffer the block is about to use, not another stream's or device's)
        assert nn.Scratch.get(_scratch_bytes(blk, H, W), srcs[0].device).data_ptr() == poisoned.data_ptr()
    res = blk(*srcs, quant=qd, out=out)
    torch.cuda.synchronize()
    if g is not None:
        g.check()
    got = res.float().cpu().numpy()
    assert not np.any(got[:, :, blk.c:]), "pad channels must stay zero"
    return got[:, :, :blk.c]


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


# ----------------------------------------------------------------------------- against the oracle, small maps

@functools.lru_cache(maxsize=None)
def _dcb_small(idx, f16):
    """test_gpu_layers.test_depth_conv_block's inputs and oracle result of DCB_CASES[idx]"""
    cin, c, adaptor, shortcut, quant, H, W, split = TL.DCB_CASES[idx]
    rng = TL._rng(100 + idx)
    sd = TL.make_dcb_weights(rng, "m", cin, c, adaptor)
    x = rng.standard_normal((H, W, cin)).astype(np.float32)
    q = rng.uniform(0.5, 1.5, c).astype(np.float32) if quant else None
    if f16:
        x = x.astype(np.float16).astype(np.float32)
    net = O.Net(sd)
    ref = (net.dcb_f16 if f16 else net.dcb)(x, "m", shortcut=shortcut, q=q)
    return (sd,) + _frozen(x, q, ref)


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("idx", range(len(TL.DCB_CASES)), ids=[str(c) for c in TL.DCB_CASES])
def test_depth_conv_block_guarded(idx, dtype):
    case = TL.DCB_CASES[idx]
    sd, x, q, ref = _dcb_small(idx, dtype == F16)
    got = _run_block(sd, x, q, dtype, case[3], case[7], guard=True)
    TL.compare(got, ref, dtype, f"guarded dcb {case}")


@functools.lru_cache(maxsize=None)
def _conv_small(idx, f16):
    """test_gpu_layers.test_conv's inputs and oracle result of CONV_CASES[idx]"""
    cin, cout, k, stride, pad, epi, H, W = TL.CONV_CASES[idx]
    rng = TL._rng(200 + idx)
    sd = {"m.weight": (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32),
          "m.bias": (rng.standard_normal(cout) * 0.1).astype(np.float32)}
    x = rng.standard_normal((H, W, cin)).astype(np.float32)
    if f16:
        x = x.astype(np.float16).astype(np.float32)
    q = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    if f16:
        ref = O.Net(sd).conv_f16(x, "m", stride, pad, epilogue=epi if epi in ("quant", "wsilu") else "bias", q=q)
        if epi == "shuffle":
            ref = O.pixel_shuffle(ref, 2)
    else:
        ref = O.Net(sd).conv(x, "m", stride, pad)
        if epi == "quant":
            ref = ref * q
        elif epi == "shuffle":
            ref = O.pixel_shuffle(ref, 2)
        elif epi == "wsilu":
            ref = O.wsilu(ref)
    return (sd,) + _frozen(x, q, np.ascontiguousarray(ref))


def _run_conv_guarded(conv, c_log, xs, quant=None, in_scale=None):
    """conv as a guarded run on the numpy sources xs = [(values, c_phys), ...] -> the output view"""
    g = GuardedRun(conv.dtype)
    srcs = [g.src(v, cp, second=i == 1) for i, (v, cp) in enumerate(xs)]
    H, W = xs[0][0].shape[:2]
    out = g.out(*conv.out_hw(H, W), conv.cout_p, c_log)
    res = conv(*srcs, quant=g.vec(quant, "quant"), out=out, in_scale=g.vec(in_scale, "in_scale"))
    g.check()
    return res


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("idx", range(len(TL.CONV_CASES)), ids=[str(c) for c in TL.CONV_CASES])
def test_conv_guarded(idx, dtype):
    from opendcvc_amd import nn
    case = TL.CONV_CASES[idx]
    cin, cout, k, stride, pad, epi, H, W = case
    sd, x, q, ref = _conv_small(idx, dtype == F16)
    conv = nn.Conv2d(sd, "m", dtype, stride, pad, TL.EPI[epi])
    c_log = cout // 4 if epi == "shuffle" else cout
    got = _run_conv_guarded(conv, c_log, [(x, conv.cin_p)], quant=q if epi == "quant" else None).float().cpu().numpy()
    assert got.shape[:2] == ref.shape[:2]
    TL.compare(got[:, :, :c_log], ref, dtype, f"guarded conv {case}")


@pytest.mark.parametrize("dtype", [F32, F16])
def test_conv_concat_sources_guarded(dtype):
    """test_gpu_layers.test_conv_concat_sources (a 1x1 conv of 128 + 384 channels), in fp16 too, each source in its own
    guarded buffer with its own row stride"""
    from opendcvc_amd import nn
    rng = TL._rng(9)
    sd = {"m.weight": (rng.standard_normal((128, 512, 1, 1)) / 22).astype(np.float32),
          "m.bias": rng.standard_normal(128).astype(np.float32)}
    x = rng.standard_normal((5, 6, 512)).astype(np.float32)
    if dtype == F16:
        x = x.astype(np.float16).astype(np.float32)
    ref = O.Net(sd).conv_f16(x, "m") if dtype == F16 else O.Net(sd).conv(x, "m")
    conv = nn.Conv2d(sd, "m", dtype)
    got = _run_conv_guarded(conv, 128, [(x[:, :, :128], 128), (x[:, :, 128:], 384)]).float().cpu().numpy()
    TL.compare(got, ref, dtype, "guarded conv concat sources 128+384->128")


# ----------------------------------------------------------------------------- against the oracle, large maps (fp16)

def _adaptor_seed(cin0, cin1, c):
    return 500 + cin0 + 3 * cin1 + 7 * c          # test_gpu_layers._adaptor_block_large's


# name, cin0, cin1, c, adaptor, shortcut, quant, seed: the blocks of test_depth_conv_block_large_map_fp16 and of
# test_adaptor_block_large_map_fp16, on their inputs
LARGE_KNOWN = ([(f"dcb large map c={c}", c, 0, c, False, True, True, 300 + c) for c in (128, 256, 320, 368, 512)] +
               [(f"adaptor block large map {a}+{b}->{c}", a, b, c, True, False, False, _adaptor_seed(a, b, c))
                for a, b, c in TL.ADAPTOR_LARGE])
# forms the models run on large maps (found by walking arch.py through plan_dcb) without a layer-level comparison so far:
# dec.dec_2 (368 -> 192: dcb_head_kernel + the 64-pixel dcb_tail_kernel at three channel tiles per wave),
# DMCI's y_prior_fusion.0 (256 -> 512), y_spatial_prior_adaptor_* (512 wide, two sources), hyper_enc.0 (256 -> 128)
LARGE_NEW = [(f"new form {a}+{b}->{c}", a, b, c, True, False, False, _adaptor_seed(a, b, c))
             for a, b, c in ((368, 0, 192), (256, 0, 512), (256, 256, 512), (256, 0, 128))]
# (case, placement) in an order that lets a plain and a guarded run of one case share its oracle evaluation
LARGE_RUNS = [(c, "guarded") for c in LARGE_KNOWN] + [(c, p) for c in LARGE_NEW for p in ("plain", "guarded")]


@functools.lru_cache(maxsize=2)
def _large(case):
    name, cin0, cin1, c, adaptor, shortcut, quant, seed = case
    H, W = LARGE
    rng = TL._rng(seed)
    sd = TL.make_dcb_weights(rng, "m", cin0 + cin1, c, adaptor)
    x = rng.standard_normal((H, W, cin0 + cin1)).astype(np.float16).astype(np.float32)
    q = rng.uniform(0.5, 1.5, c).astype(np.float32) if quant else None
    ref = O.Net(sd).dcb_f16(x, "m", shortcut=shortcut, q=q)
    return (sd,) + _frozen(x, q, ref)


@pytest.mark.parametrize("case,placement", LARGE_RUNS, ids=[f"{c[0]} {p}" for c, p in LARGE_RUNS])
def test_large_map_fp16(case, placement):
    name, cin0, cin1, c, adaptor, shortcut, quant, seed = case
    sd, x, q, ref = _large(case)
    got = _run_block(sd, x, q, F16, shortcut, cin0 if cin1 else None, guard=placement == "guarded")
    TL.compare(got, ref, F16, f"{name} {placement}")


# cin, cout, k, pad, epilogue, in_scale: conv_kernel on 64-pixel tiles (maps of 12 000+ pixels; no small case reaches them) -
# its 1x1 form with a quant vector, and its halo-tile form, which a 3x3 conv with an input scale takes instead of
# conv3x3_t128_kernel
CONV_LARGE = [(256, 256, 1, 0, "quant", False), (64, 64, 3, 1, "bias", True)]


@pytest.mark.parametrize("geom", CONV_LARGE, ids=[str(g) for g in CONV_LARGE])
def test_conv_large_map_fp16_guarded(geom):
    from opendcvc_amd import nn
    cin, cout, k, pad, epi, scale = geom
    H, W = LARGE
    rng = TL._rng(2600 + cin + k)
    sd = make_conv_weights(rng, "m", cout, cin, k)
    x = rng.standard_normal((H, W, cin)).astype(np.float16).astype(np.float32)
    q = rng.uniform(0.5, 1.5, cout).astype(np.float32) if epi == "quant" else None
    s = rng.uniform(0.5, 1.5, cin).astype(np.float32) if scale else None
    # (the scaled input is rounded to fp16 as dcvc_scale_channels stores it: conv_f16 rounds its input)
    ref = O.Net(sd).conv_f16(x * s if scale else x, "m", 1, pad, epilogue=epi, q=q)
    conv = nn.Conv2d(sd, "m", F16, 1, pad, TL.EPI[epi])
    got = _run_conv_guarded(conv, cout, [(x, conv.cin_p)], quant=q, in_scale=s).float().cpu().numpy()
    TL.compare(got[:, :, :cout], ref, F16, f"guarded conv large map {geom}")


# ----------------------------------------------------------------------------- bitwise against the plain run

CHAINS = [(256, (21, 19)), (256, LARGE), (128, (17, 30)), (368, (12, 27)), (512, (14, 20)), (320, LARGE)]
CHAIN_RUNS = [(c, hw, dt) for c, hw in CHAINS for dt in (F16, F32) if dt == F16 or hw != LARGE]   # large maps: the fp16 kernels


@pytest.mark.parametrize("c,hw,dtype", CHAIN_RUNS, ids=[f"{c}-{hw[0]}x{hw[1]}-{str(dt)[6:]}" for c, hw, dt in CHAIN_RUNS])
def test_chains_guarded_equal_plain(c, hw, dtype):
    """dcb_chain of four blocks behind a two-source adaptor block, quant at the end, and a two-block chain ending in a
    fused 1x1 conv with quant: the guarded runs (scratch poisoned once, before the first block) give what the same objects
    give on contiguous tensors, bit for bit - and where every block's output is asked for, each of them."""
    from opendcvc_amd import _lib, nn
    H, W = hw
    rng = TL._rng(1400 + c + H)
    blocks = [nn.DepthConvBlock(TL.make_dcb_weights(rng, "m", 2 * c if i == 0 else c, c, i == 0), "m", dtype) for i in range(5)]
    conv = nn.Conv2d(make_conv_weights(rng, "o", c, c, 1), "o", dtype, epilogue=_lib.EPI_BIAS_QUANT)
    assert conv.fusable_after(blocks[2])
    x = rng.standard_normal((H, W, 2 * c)).astype(np.float32)
    x1 = rng.standard_normal((H, W, c)).astype(np.float32)
    q = rng.uniform(0.5, 1.5, c).astype(np.float32)
    cp, split = blocks[0].c_p, blocks[0].cin_p // 2 // 64 * 64
    every = (c, hw) in ((256, (21, 19)), (320, LARGE))

    want = nn.dcb_chain(blocks, *_sources(x, blocks[0].cin_p, split, dtype, None), quant=_vec(q, None), return_all=True)
    want_conv = nn.dcb_chain(blocks[1:3], *_sources(x1, cp, None, dtype, None), then_conv=conv, conv_quant=_vec(q, None))
    torch.cuda.synchronize()

    g = GuardedRun(dtype)
    srcs = _sources(x, blocks[0].cin_p, split, dtype, g)
    qd, out = g.vec(q), g.out(H, W, cp, c)
    g.scratch(_scratch_bytes(blocks[0], H, W))
    got = nn.dcb_chain(blocks, *srcs, quant=qd, out=out, return_all=every)
    g.check()
    if every:
        assert len(got) == len(want) and got[-1].data_ptr() == out.data_ptr()
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), f"block {i} of the guarded chain differs"
    else:
        assert got.data_ptr() == out.data_ptr() and torch.equal(got, want[-1])

    g = GuardedRun(dtype)
    srcs = _sources(x1, cp, None, dtype, g)
    qd, out = g.vec(q), g.out(H, W, conv.cout_p, c)
    g.scratch(_scratch_bytes(blocks[1], H, W))
    got = nn.dcb_chain(blocks[1:3], *srcs, then_conv=conv, conv_quant=qd, out=out)
    g.check()
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want_conv)


# test_gpu_layers.test_conv3x3_t128_equals_conv_kernel_bitwise's geometries: cin, cout, epi, H, W, k, stride, pad, in_scale
CONV_T128 = [(128, 1024, "shuffle", 68, 120, 3, 1, 1, False), (192, 256, "bias", 21, 37, 3, 1, 1, False),
             (256, 256, "bias", 136, 240, 2, 2, 0, True), (256, 128, "bias", 37, 51, 3, 2, 1, False),
             (128, 128, "bias", 13, 18, 2, 2, 0, False), (368, 256, "bias", 9, 7, 3, 2, 1, True)]


@pytest.mark.parametrize("geom", CONV_T128, ids=[str(g) for g in CONV_T128])
def test_fragment_stream_convs_guarded_equal_plain(geom):
    """conv3x3_t128_kernel and conv_s2_t32_kernel (fp16; pinned to the oracle through conv_kernel, which they equal bit for
    bit): halo loads around a strided map, ragged tiles, in_scale of exactly cin floats"""
    from opendcvc_amd import nn
    cin, cout, epi, H, W, k, stride, pad, scale = geom
    rng = TL._rng(700 + cin + cout + k + stride)
    conv = nn.Conv2d(make_conv_weights(rng, "m", cout, cin, k), "m", F16, stride, pad, TL.EPI[epi])
    x = rng.standard_normal((H, W, cin)).astype(np.float32)
    s = rng.uniform(0.5, 1.5, cin).astype(np.float32) if scale else None
    want = conv(TL.to_dev(x, conv.cin_p, F16), in_scale=_vec(s, None))
    got = _run_conv_guarded(conv, cout // 4 if epi == "shuffle" else cout, [(x, conv.cin_p)], in_scale=s)
    assert torch.equal(got, want)


# kind, width, input map, channel offset of the slice in the 384-wide concat buffer: the temporal prior encoder writes its
# 256 channels behind the hyper decoder's 128 (models.py, _prior_params)
RESIDUAL = [("down", 256, (68, 120), 128), ("down", 128, (34, 60), 0), ("up", 256, (17, 30), 128), ("up", 128, (17, 30), 0)]


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("kind,c,hw,at", RESIDUAL)
def test_residual_blocks_into_concat_slice_guarded_equal_plain(kind, c, hw, at, dtype):
    """ResidualBlockWithStride2 (with the input scale, as `temporal` runs) and ResidualBlockUpsample writing a channel slice
    of a 384-wide buffer: width 256 on a 34 x 60 output behind 128 other channels, width 128 in front of 256 (on 17 x 30 and
    34 x 60 outputs; fp16: the 32-pixel fragment-stream tail with its head inside).  The rest of the buffer stays as it was."""
    from opendcvc_amd import nn
    H, W = hw
    rng = TL._rng(1700 + c + H)
    sd = TL.make_dcb_weights(rng, "m.conv", c, c, False)
    if kind == "down":
        sd.update(make_conv_weights(rng, "m.down", c, c, 2))
        layer, (Ho, Wo) = nn.ResidualBlockWithStride2(sd, "m", dtype), (H // 2, W // 2)
        s = rng.uniform(0.5, 1.5, c).astype(np.float32)
    else:
        sd.update(make_conv_weights(rng, "m.up.conv.0", 4 * c, c, 1))
        layer, (Ho, Wo) = nn.ResidualBlockUpsample(sd, "m", dtype), (2 * H, 2 * W)
        s = None
    x = rng.standard_normal((H, W, c)).astype(np.float32)
    call = lambda xd, sv, out: layer(xd, out=out, in_scale=sv) if kind == "down" else layer(xd, out=out)
    want = call(TL.to_dev(x, c, dtype), _vec(s, None), None)
    torch.cuda.synchronize()

    g = GuardedRun(dtype)
    xd, sv = g.src(x, c), g.vec(s, "in_scale")
    out = g.out(Ho, Wo, c, ld=384 + 32, chan_off=at + 16 // xd.element_size())
    g.scratch(_scratch_bytes(layer.conv, Ho, Wo))
    got = call(xd, sv, out)
    g.check()
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)


# ----------------------------------------------------------------------------- positive control

SMALL = (20, 19)
# One block per head / tail form of plan_dcb (has_tail128, has_head128, has_tail_headin, tail_form):
# name, dtype, cin0, cin1, c, adaptor, map
FORMS = [
    ("tail128<128,G32,HEADIN>", F16, 128, 0, 128, False, SMALL),
    ("tail128<256,G32,HEADIN>", F16, 256, 0, 256, False, SMALL),
    ("head128<384,G32> + tail128<384,G32>", F16, 384, 0, 384, False, SMALL),
    ("head128<512,adapt,G32> + tail128<512,G32>", F16, 256, 256, 512, True, SMALL),
    ("head<2,adapt> (96+160) + tail128<256,G32>", F16, 96, 160, 256, True, SMALL),
    ("tail<2,3,4,HEADIN>", F16, 192, 0, 192, False, SMALL),
    ("head<2> + tail<2,3,8,RAG>", F16, 320, 0, 320, False, SMALL),
    ("head128<256,G128> + tail128<256,G128>", F16, 256, 0, 256, False, LARGE),
    ("head128<320,adapt,G128> + tail128<320,G128>", F16, 256, 0, 320, True, LARGE),
    ("head<4> + tail<4,2,4>", F16, 128, 0, 128, False, LARGE),
    ("head<adapt> (368) + tail<4,3,4>", F16, 368, 0, 192, True, LARGE),
    ("head<adapt> (256+256) + tail<4,4,8>", F16, 256, 256, 512, True, LARGE),
    ("fp32 head<2> + tail<2,4,4>", F32, 256, 0, 256, False, SMALL),
    ("fp32 head<2,adapt> (128+128) + tail<2,2,4>", F32, 128, 128, 128, True, SMALL),
]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_nan_source_pixel_comes_out_in_its_3x3_neighbourhood(form):
    """Each form once as a guarded run (equal to the plain run), then the control: a NaN in one channel of one source pixel
    (on a corner shared by four tiles; then in the map's first and last pixel):
    outside that pixel's 3 x 3 neighbourhood (the depthwise conv's reach), clipped to the map, the output is the clean
    run's bit for bit, and every pixel inside has a non-finite value - no gate, clamp or store of the form squashes a NaN, so
    the guarded runs above see one that reaches it."""
    from opendcvc_amd import nn
    name, dtype, cin0, cin1, c, adaptor, (H, W) = form
    rng = TL._rng(2100 + FORMS.index(form))
    blk = nn.DepthConvBlock(TL.make_dcb_weights(rng, "m", cin0 + cin1, c, adaptor), "m", dtype)
    x = rng.standard_normal((H, W, cin0 + cin1)).astype(np.float32)
    srcs = _sources(x, blk.cin_p, cin0 if cin1 else None, dtype, None)
    clean = blk(*srcs).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(clean).all())
    # the same block as a guarded run: every form, also those no oracle case reaches, equals its plain run bit for bit
    g = GuardedRun(dtype)
    placed = _sources(x, blk.cin_p, cin0 if cin1 else None, dtype, g)
    out = g.out(H, W, blk.c_p, c)
    g.scratch(_scratch_bytes(blk, H, W))
    blk(*placed, out=out)
    g.check()
    assert torch.equal(out, clean), f"{name}: the guarded run differs from the plain one"
    for (py, px) in ((8, 16), (0, 0), (H - 1, W - 1)):
        keep = srcs[-1][py, px, 5].clone()
        srcs[-1][py, px, 5] = float("nan")
        got = blk(*srcs).clone()
        srcs[-1][py, px, 5] = keep
        torch.cuda.synchronize()
        near = torch.zeros((H, W), dtype=torch.bool, device="cuda")
        near[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
        assert torch.equal(got[~near], clean[~near]), f"{name}: NaN at {(py, px)} changed pixels outside its 3 x 3 neighbourhood"
        hit = (~torch.isfinite(got[:, :, :c])).any(dim=2)
        assert bool(hit[near].all()), f"{name}: NaN at {(py, px)} did not reach {int((~hit[near]).sum())} of {int(near.sum())} neighbours"


# ----------------------------------------------------------------------------- contract refusals

@pytest.mark.parametrize("dtype", [F16, F32])
def test_misaligned_views_are_refused_before_any_launch(dtype):
    """Sources and outputs are read and written in 16-byte vectors: a view at an 8-byte channel offset or with a row stride
    that is not a multiple of 16 bytes is refused by every forward entry, and nothing is launched (the output keeps its
    fill)."""
    from opendcvc_amd import _lib, nn
    from opendcvc_amd._lib import DcvcError
    es = torch.empty((), dtype=dtype).element_size()
    H, W, c, half = 6, 7, 256, 8 // es
    rng = TL._rng(77)
    blocks = [nn.DepthConvBlock(TL.make_dcb_weights(rng, "m", c, c, False), "m", dtype) for _ in range(2)]
    conv = nn.Conv2d(make_conv_weights(rng, "o", c, c, 1), "o", dtype, epilogue=_lib.EPI_BIAS)
    assert conv.fusable_after(blocks[0])

    def views(fill):
        wide = torch.full((H * W, c + 32), fill, dtype=dtype, device="cuda")
        odd = torch.full((H * W, c + half), fill, dtype=dtype, device="cuda")
        return {"8-byte channel offset": wide[:, half:half + c].unflatten(0, (H, W)),
                "row stride of 8 bytes modulo 16": odd[:, :c].unflatten(0, (H, W))}, (wide, odd)

    good = torch.zeros((H, W, c), dtype=dtype, device="cuda")
    calls = {"dcb": lambda x, out: blocks[0](x, out=out),
             "dcb chained": lambda x, out: blocks[0](x, out=out, next_block=blocks[1]),
             "dcb then conv": lambda x, out: blocks[0].then_conv(x, None, conv, out=out),
             "conv": lambda x, out: conv(x, out=out)}
    for what, call in calls.items():
        bad, _ = views(0.0)
        for why, v in bad.items():
            assert nn._geom(v) == (H, W, c, v.stride(1))                  # a view the host side lets through
            sink = torch.full((H, W, c), 3.0, dtype=dtype, device="cuda")
            with pytest.raises(DcvcError):
                call(v, sink)
            torch.cuda.synchronize()
            assert bool((sink == 3.0).all()), f"{what}: launched despite a source view with {why}"
        bad, bufs = views(3.0)
        for why, v in bad.items():
            with pytest.raises(DcvcError):
                call(good, v)
        torch.cuda.synchronize()
        assert all(bool((b == 3.0).all()) for b in bufs), f"{what}: launched despite a misaligned output view"
        out = call(good, None)                                            # the same call on aligned operands runs
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
