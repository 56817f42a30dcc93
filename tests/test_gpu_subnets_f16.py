"""The fp16 model's sub-networks on the GPU against the oracle's fp16-storage emulation, tensor by tensor.

The fp16 model runs kernels the fp32 model never does (the 128-pixel tails and heads, the head-inside forms, conv3x3_t128 /
conv_s2_t32, successor heads and 1x1 convs fused into tails), composed by opendcvc_amd/models.py in ways no layer test
reproduces (feature_adaptor_p folded into conv1.0, the padded square y_spatial_prior.conv.2 in a tail, in_scale into a concat
slice, two-source adaptor blocks, twelve-block chains with a quant at the end, the 514-channel fusion head).  Every
sub-network method of DMC / DMCI is called on seeded fp16 inputs (teacher forcing) and compared by subnet_utils.check with the
emulation and with the fp32 oracle: mean, per-slice and maximum error not beyond the emulation's own (margins 1.10 / 1.5 / 2,
from the reference alone).  The figures go to f16_subnets.json in subnet_utils' output directory (committed as profiles/f16_subnets.json)."""
import numpy as np
import pytest
import torch

import subnet_utils as S
from subnet_utils import QP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    from opendcvc_amd.models import DMC, DMCI
    out = {}
    for name, cls in (("dmc", DMC), ("dmci", DMCI)):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in S.state_dict(name).items()})
        m.to("cuda").eval()
        m.update(None)
        m.half()
        m._ensure_layers()
        out[name] = m
    return out


def _dev(x, cp=None):
    """HWC float32 (fp16 values) -> fp16 device tensor, channels zero-padded to a multiple of 32"""
    H, W, C = x.shape
    cp = cp or (C + 31) // 32 * 32
    t = torch.zeros((H, W, cp), dtype=torch.float16, device="cuda")
    t[:, :, :C] = torch.tensor(x, dtype=torch.float16)         # (a copy: the shared inputs are read-only)
    return t


def _frame(x):
    """picture [H, W, 3] -> [1, 3, H, W] fp16 on the device"""
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))[None]).to("cuda", torch.float16)


def _picture(t):
    return t[0].permute(1, 2, 0).contiguous()


def run_hip(case, m, inp, shape):
    """the sub-network `case` through the model's own methods -> {output name: device tensor, HWC}"""
    s = S.SHAPES[shape]
    q = lambda name: m._q[name][QP]
    if case in ("ext_i", "ext_p"):
        variant, ref = ("i", _frame(inp["frame"])) if case == "ext_i" else ("p", _dev(inp["ref"]))
        x1, ctx = m._extractor_both(variant, ref)
        return dict(x1=x1, ctx=ctx)
    if case == "encoder":
        return dict(y=m._encoder(m._unshuffle8(_frame(inp["frame"])), _dev(inp["ctx"]), q("q_encoder")))
    if case in ("hyper_encoder", "i_hyper_encoder"):
        return dict(z=m._hyper_encoder(_dev(inp["y"])))
    if case == "prior_params":
        return dict(params=m._prior_params(_dev(inp["z_hat"]), _dev(inp["x1"]), q("q_feature"), s["yh"], s["yw"]))
    if case == "spatial_prior":
        return dict(sp=m._spatial_prior(_dev(inp["y_hat"]), _dev(inp["params"])))
    if case == "decoder":
        return dict(feature=m._decoder(_dev(inp["y_hat"]), _dev(inp["ctx"]), q("q_decoder")))
    if case == "recon":
        head = m._recon_head(_dev(inp["feature"]), q("q_recon"))
        return dict(head=head, picture=_picture(m._picture_out(head)))
    if case == "i_enc":
        return dict(y=m._enc(_frame(inp["frame"]), q("q_scale_enc")))
    if case == "i_prior_params":
        return dict(params=m._prior_params(_dev(inp["z_hat"]), s["yh"], s["yw"]))
    if case == "i_reduction":
        return dict(common=m._layers["reduction"](_dev(inp["params"])))
    if case.startswith("i_spatial_prior_"):
        return dict(sp=m._spatial_prior(_dev(inp["y_hat"]), _dev(inp["common"]), int(case[-1])))
    if case == "i_dec":
        head = m._dec(_dev(inp["y_hat"]), q("q_scale_dec"))
        return dict(head=head, picture=_picture(m._picture_out(head)))
    raise KeyError(case)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_subnetwork_f16_against_emulation_and_fp32(models, case):
    name, shape = case
    inp, emu, truth = S.reference(name, shape)
    outs = run_hip(name, models[S.model_of(name)], inp, shape)
    torch.cuda.synchronize()
    assert sorted(outs) == sorted(emu)
    failures = []
    for k, t in outs.items():
        got = t.float().cpu().numpy()
        c = emu[k].shape[2]
        assert got.shape[:2] == emu[k].shape[:2] and got.shape[2] >= c, (k, got.shape, emu[k].shape)
        assert not np.any(got[:, :, c:]), f"{name}.{k}: pad channels must be zero"
        try:
            S.check(f"{name}.{k} {shape}", got[:, :, :c], emu[k], truth[k])
        except AssertionError as e:       # (every output of the case is measured and recorded before the test fails)
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("shape", ["small", "large_f"])
@pytest.mark.parametrize("variant", ["i", "p"])
def test_extractor_as_one_chain_equals_its_two_parts(models, variant, shape):
    """_extractor_both (encoder side: one chain, every block started in its predecessor's tail) = _extractor_part1 +
    _extractor_part2 (decoder side), bit for bit"""
    m = models["dmc"]
    case = "ext_" + variant
    inp = S.make_inputs(case, shape)
    ref = _frame(inp["frame"]) if variant == "i" else _dev(inp["ref"])
    x1, ctx = m._extractor_both(variant, ref)
    x1_b = m._extractor_part1(variant, ref)
    ctx_b = m._extractor_part2(x1_b)
    torch.cuda.synchronize()
    assert torch.equal(x1, x1_b) and torch.equal(ctx, ctx_b)


@pytest.mark.parametrize("shape", ["small", "large_f"])
def test_recon_in_two_halves_equals_recon(models, shape):
    """_recon = _recon_first + _recon_second + the picture (the deferred decoder output), bit for bit"""
    m = models["dmc"]
    feature = _dev(S.make_inputs("recon", shape)["feature"])
    q = m._q["q_recon"][QP]
    whole = m._recon(feature, q)
    halves = m._picture_out(m._recon_second(m._recon_first(feature), q))
    torch.cuda.synchronize()
    assert torch.equal(whole, halves)
