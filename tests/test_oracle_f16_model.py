"""The oracle's fp16 mode (OracleDMC / OracleDMCI(sd, f16=True)) and the sub-network checker, on the CPU.

  * composition: every f16 sub-network equals its hand composition from Net.dcb_f16 / Net.conv_f16 on the .half() parameters,
    with the model's own stores (opendcvc_amd/models.py) written out here a second time;
  * the margins of subnet_utils.check are satisfiable: for every (sub-network, small shape) the GPU tests use, a second
    realization of the emulation (subnet_utils.PermutedNet: other summation orders) passes as `got`;
  * the checker is not blind: three seeded faults in the realization that stands in for the kernel are rejected."""
import numpy as np
import pytest

import dcvc_oracle as O
import subnet_utils as S
from subnet_utils import QP, rh


def _hand(case, sd, inp, s):
    """the sub-network written out layer by layer, rounding points included"""
    n = O.Net({k: rh(v) for k, v in sd.items()})          # the model's .half() parameters
    D, C = n.dcb_f16, n.conv_f16
    q = lambda name: n.sd[name][QP, :, 0, 0]
    cat = lambda *a: np.concatenate(a, 2)
    up = lambda x, p, pad=0: O.pixel_shuffle(C(x, p + ".conv.0", 1, pad), 2)
    res_down = lambda x, p: D(C(x, p + ".down", 2, 0), p + ".conv", shortcut=True)
    res_up = lambda x, p: D(up(x, p + ".up"), p + ".conv", shortcut=True)
    pad4 = lambda y: np.pad(y, ((0, -y.shape[0] % 4), (0, -y.shape[1] % 4), (0, 0)), mode="edge")
    pic = lambda head: np.clip(O.pixel_shuffle(head, 8), 0, 1).astype(np.float32)

    def chain(x, fmt, idx, **last):
        for i in idx:
            x = D(x, fmt.format(i), **(last if i == idx[-1] else {}))
        return x

    if case in ("ext_i", "ext_p"):
        f = D(O.pixel_unshuffle(inp["frame"], 8), "feature_adaptor_i") if case == "ext_i" else C(inp["ref"], "feature_adaptor_p")
        x1 = chain(f, "feature_extractor.conv1.{}", (0, 1))
        return dict(x1=x1, ctx=chain(x1, "feature_extractor.conv2.{}", (0, 1, 2, 3)))
    if case == "encoder":
        f = cat(C(O.pixel_unshuffle(inp["frame"], 8), "encoder.conv1"), inp["ctx"])
        f = D(chain(f, "encoder.conv2.{}", (0, 1)), "encoder.conv3", q=q("q_encoder"))       # quant in the block's last store
        return dict(y=C(f, "encoder.down", 2, 1))
    if case == "hyper_encoder":
        return dict(z=res_down(res_down(D(pad4(inp["y"]), "hyper_encoder.conv.0"), "hyper_encoder.conv.1"), "hyper_encoder.conv.2"))
    if case == "prior_params":
        h = D(res_up(res_up(inp["z_hat"], "hyper_decoder.conv.0"), "hyper_decoder.conv.1"), "hyper_decoder.conv.2")
        t = res_down(rh(inp["x1"] * q("q_feature")), "temporal_prior_encoder")               # x1 * q_feature rounded once
        p = chain(cat(h[:s["yh"], :s["yw"]], t), "y_prior_fusion.conv.{}", (0, 1, 2))
        return dict(params=C(p, "y_prior_fusion.conv.3"))
    if case == "spatial_prior":
        return dict(sp=C(chain(cat(inp["y_hat"], inp["params"]), "y_spatial_prior.conv.{}", (0, 1)), "y_spatial_prior.conv.2"))
    if case == "decoder":
        f = chain(cat(up(inp["y_hat"], "decoder.up", 1), inp["ctx"]), "decoder.conv1.{}", (0, 1, 2))
        return dict(feature=C(f, "decoder.conv2", epilogue="quant", q=q("q_decoder")))       # the conv's quant epilogue
    if case == "recon":
        head = C(chain(inp["feature"], "recon_generation_net.conv.{}", (0, 1, 2, 3), q=q("q_recon")), "recon_generation_net.head")
        return dict(head=head, picture=pic(head))                                            # bias in the conv, then data movement
    if case == "i_enc":
        o = D(O.pixel_unshuffle(inp["frame"], 8), "enc.enc_1", q=q("q_scale_enc"))
        return dict(y=C(chain(o, "enc.enc_2.{}", tuple(range(6))), "enc.enc_2.6", 2, 1))
    if case == "i_hyper_encoder":
        return dict(z=res_down(res_down(D(pad4(inp["y"]), "hyper_enc.0"), "hyper_enc.1"), "hyper_enc.2"))
    if case == "i_prior_params":
        p = D(res_up(res_up(inp["z_hat"], "hyper_dec.0"), "hyper_dec.1"), "hyper_dec.2")
        return dict(params=C(chain(p, "y_prior_fusion.{}", (0, 1, 2)), "y_prior_fusion.3")[:s["yh"], :s["yw"]])
    if case == "i_reduction":
        return dict(common=C(inp["params"], "y_spatial_prior_reduction"))
    if case.startswith("i_spatial_prior_"):
        x = D(cat(inp["y_hat"], inp["common"]), "y_spatial_prior_adaptor_" + case[-1])
        return dict(sp=C(chain(x, "y_spatial_prior.{}", (0, 1, 2)), "y_spatial_prior.3"))
    if case == "i_dec":
        o = chain(res_up(inp["y_hat"], "dec.dec_1.0"), "dec.dec_1.{}", tuple(range(1, 13)), q=q("q_scale_dec"))
        head = D(o, "dec.dec_2")
        return dict(head=head, picture=pic(head))
    raise KeyError(case)


@pytest.mark.parametrize("case", S.SMALL_CASES, ids=S.case_id)
def test_f16_subnetwork_equals_hand_composition(case):
    name, shape = case
    inp, emu, _ = S.reference(name, shape)
    want = _hand(name, S.state_dict(S.model_of(name)), inp, S.SHAPES[shape])
    assert sorted(want) == sorted(emu)
    for k in want:
        assert want[k].shape == emu[k].shape and np.array_equal(want[k], emu[k]), f"{name}.{k}"
        assert np.array_equal(emu[k], rh(emu[k])), f"{name}.{k} is not an fp16 tensor"


def test_fp32_mode_is_untouched_by_the_fp16_flag():
    """the default oracle has no rounding: its outputs are not fp16 values, and differ from the emulation's"""
    inp, emu, truth = S.reference("decoder", "small")
    assert not np.array_equal(truth["feature"], rh(truth["feature"]))
    assert not np.array_equal(truth["feature"], emu["feature"])


def _realization(name, shape, net, inp=None):
    orc = S.oracle_for(name, net.sd, True)
    orc.net = net
    return S.run_oracle(name, orc, S.reference(name, shape)[0] if inp is None else inp, shape)


@pytest.mark.parametrize("case", S.SMALL_CASES, ids=S.case_id)
def test_second_realization_meets_the_margins(case):
    """the condition that the margins can be met at all: the emulation in other summation orders passes every check"""
    name, shape = case
    inp, emu, truth = S.reference(name, shape)
    got = _realization(name, shape, S.PermutedNet(S.state_dict(S.model_of(name)), seed=3))
    differs = False
    for k in emu:
        S.check(f"{name}.{k}", got[k], emu[k], truth[k], record=False)
        differs |= not np.array_equal(got[k], emu[k])
    assert differs, "the permuted realization is bit-identical: it does not exercise the margins"


def test_checker_rejects_a_dropped_halo_row():
    """prior network of the P frame, 384-wide fusion chain: the second block's depthwise conv loses the halo row above row 8"""
    inp, emu, truth = S.reference("prior_params", "small")
    net = S.HaloFaultNet(S.state_dict("dmc"), "y_prior_fusion.conv.1", 8)
    got = _realization("prior_params", "small", net)
    assert np.array_equal(got["params"][:5], emu["params"][:5])          # (three blocks below the fault reach three rows up)
    with pytest.raises(AssertionError, match="rows from [789]:"):
        S.check("halo", got["params"], emu["params"], truth["params"], record=False)


def test_checker_rejects_a_dropped_bias_of_the_fused_conv():
    """y_spatial_prior.conv.2 (computed in the preceding block's tail): one output channel without its bias"""
    inp, emu, truth = S.reference("spatial_prior", "small")
    sd = S.state_dict("dmc")
    ch = 77
    assert abs(sd["y_spatial_prior.conv.2.bias"][ch]) > 1e-2
    got = _realization("spatial_prior", "small", O.Net(S.drop_bias(sd, "y_spatial_prior.conv.2", ch), f16=True))
    keep = np.arange(256) != ch
    assert np.array_equal(got["sp"][:, :, keep], emu["sp"][:, :, keep])
    with pytest.raises(AssertionError, match="channels from 77"):
        S.check("bias", got["sp"], emu["sp"], truth["sp"], record=False)


def test_checker_rejects_a_shifted_second_source():
    """decoder.conv1.0 (two sources, 512 -> 256): the context enters one channel off"""
    inp, emu, truth = S.reference("decoder", "small")
    bad = dict(inp, ctx=np.roll(inp["ctx"], 1, axis=2))
    got = _realization("decoder", "small", O.Net(S.state_dict("dmc"), f16=True), inp=bad)
    with pytest.raises(AssertionError, match="mean"):
        S.check("shift", got["feature"], emu["feature"], truth["feature"], record=False)
