"""The fp16 model's sub-networks against the oracle, tensor by tensor: the checker, the cases and the realizations shared by
tests/test_oracle_f16_model.py (CPU) and tests/test_gpu_subnets_f16.py (GPU).

Three values of one sub-network on the same seeded, fp16-rounded inputs (teacher forcing: no quantiser in between):
  truth  the fp32 oracle with the unrounded weights: the plain high-precision value of the operation,
  emu    the oracle's fp16-storage emulation (OracleDMC / OracleDMCI(sd, f16=True)),
  got    what is under test: the HIP fp16 model on the GPU; on the CPU a second realization of the emulation.

check() asserts that `got` is not further from `truth` than `emu` is - over the tensor, over every slice of it (rows, columns,
channel groups of at least MIN_SLICE elements: an error confined to a tile edge or a channel tile) and at the maximum.  The
margins come from the reference alone (two summation orders of dcb_f16 against fp32, six-block chains at widths 128 / 256 /
384: mean ratio 0.990 - 1.015, row / column ratios <= 1.09 at ~3500 elements per slice, channel ratios up to 1.40 at only
72 - 168 elements per slice - hence the floor of 1000 elements -, max ratio <= 1.34)."""
import json
import os

import numpy as np

import dcvc_oracle as O

MEAN_MARGIN, SLICE_MARGIN, MAX_MARGIN, ABS_SLACK = 1.10, 1.5, 2.0, 1e-7
MIN_SLICE = 1000
QP = 21
STATS = {}
# where check() records its figures (f16_subnets.json): DCVC_TEST_OUT, or test_out/ in the repository root (not tracked)
_OUT = os.environ.get("DCVC_TEST_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_out")


# ------------------------------------------------------------------------------------------------ the checker

def _slices(err, axis):
    """mean of err [H, W, C] over slices along `axis`, neighbouring indices merged until a slice holds >= MIN_SLICE
    elements (a short remainder joins the slice before it): (first index of each slice, means)"""
    n = err.shape[axis]
    per = err.size // n
    k = max(1, -(-MIN_SLICE // per))
    starts = list(range(0, n, k))
    if len(starts) > 1 and n - starts[-1] < k:
        starts.pop()
    sums = err.sum(axis=tuple(a for a in range(3) if a != axis))
    tot = np.add.reduceat(sums, starts)
    cnt = np.diff(starts + [n]) * per
    return starts, tot / cnt


def check(name, got, emu, truth, record=True):
    """got / emu / truth: float32 [H, W, C], logical channels only.  Returns the recorded figures; raises AssertionError with the
    figure and the slice that misses its margin."""
    got, emu, truth = (np.asarray(a, np.float64) for a in (got, emu, truth))
    assert got.shape == emu.shape == truth.shape and got.ndim == 3, (name, got.shape, emu.shape, truth.shape)
    rms = float(np.sqrt(np.mean(truth ** 2))) + 1e-9
    e_got, e_emu, d = np.abs(got - truth), np.abs(emu - truth), np.abs(got - emu)
    st = dict(shape=list(got.shape), rms=rms, emu_mean=float(e_emu.mean()) / rms, emu_max=float(e_emu.max()) / rms,
              mean_ratio=float(e_got.mean() / (e_emu.mean() + 1e-30)), max_ratio=float(e_got.max() / (e_emu.max() + 1e-30)),
              got_vs_emu_max=float(d.max()) / rms, got_vs_emu_mean=float(d.mean()) / rms,
              identical_fraction=float(np.mean(got == emu)))
    failures = []
    if not e_got.mean() <= MEAN_MARGIN * e_emu.mean() + ABS_SLACK:
        failures.append(f"mean |got - truth| = {e_got.mean() / rms:.3e} x rms, {st['mean_ratio']:.3f} x the emulation's")
    worst = (0.0, None)
    for axis, what in enumerate(("row", "column", "channel")):
        starts, m_got = _slices(e_got, axis)
        _, m_emu = _slices(e_emu, axis)
        ratio = m_got / (m_emu + 1e-30)
        i = int(np.argmax(np.where(m_got > ABS_SLACK, ratio, 0.0)))
        if m_got[i] > ABS_SLACK and ratio[i] > worst[0]:
            worst = (float(ratio[i]), f"{what}s from {starts[i]}")
        bad = np.nonzero(~(m_got <= SLICE_MARGIN * m_emu + ABS_SLACK))[0]
        if bad.size:
            j = int(bad[np.argmax(ratio[bad])])
            failures.append(f"{what}s from {starts[j]}: mean |got - truth| is {ratio[j]:.2f} x the emulation's "
                            f"({m_got[j] / rms:.3e} x rms; {bad.size} of {len(starts)} {what} slices miss)")
    st["slice_ratio"], st["worst_slice"] = worst
    if not e_got.max() <= MAX_MARGIN * e_emu.max():
        failures.append(f"max |got - truth| = {e_got.max() / rms:.3e} x rms, {st['max_ratio']:.2f} x the emulation's")
    if record:
        STATS[name] = st
        os.makedirs(_OUT, exist_ok=True)
        with open(os.path.join(_OUT, "f16_subnets.json"), "w") as f:
            json.dump(STATS, f, indent=1, sort_keys=True)
    print(name, json.dumps(st))
    assert not failures, f"{name}: " + "; ".join(failures)
    return st


# ------------------------------------------------------------------------------------------------ realizations

def rh(a):
    return O.Net._rh(a)


class PermutedNet(O.Net):
    """A second legitimate realization of the fp16-storage emulation: in every layer, every channel dimension a dot product runs
    over (a conv's input channels; a block's source, residual-stream, depthwise and FFN-hidden channels) is permuted -
    weights, biases, quant steps and input alike - and the layer's output is put back in order.  Putting a tensor back in order
    and permuting it again is exact data movement, so this is the network with its C-wide dimensions permuted consistently and
    un-permuted at the end: the same products, the same stores, another summation order in every fp32 accumulation chain."""

    def __init__(self, sd, seed=1):
        super().__init__(sd, f16=True)
        self._seed = seed

    def _perm(self, prefix, what, n):
        h = sum(ord(c) * (i + 1) for i, c in enumerate(prefix + what))
        return np.random.default_rng([self._seed, h, n]).permutation(n)

    def conv_f16(self, x, prefix, stride=1, pad=0, epilogue="bias", q=None):
        w = self.sd[prefix + ".weight"]
        p = self._perm(prefix, "in", w.shape[1])
        sub = O.Net({"m.weight": w[:, p], "m.bias": self.sd[prefix + ".bias"]})
        return sub.conv_f16(np.ascontiguousarray(x[:, :, p]), "m", stride, pad, epilogue, q)

    def dcb_f16(self, x, prefix, shortcut=False, q=None):
        g = lambda n: self.sd[prefix + n]
        C = g(".dc.0.weight").shape[0]
        ps, pa, pv = self._perm(prefix, "s", C), self._perm(prefix, "a", C), self._perm(prefix, "v", 2 * C)
        pu = np.concatenate([pv, 2 * C + pv])
        m = {"m.dc.0.weight": g(".dc.0.weight")[pa][:, ps], "m.dc.0.bias": g(".dc.0.bias")[pa],
             "m.dc.2.weight": g(".dc.2.weight")[pa], "m.dc.2.bias": g(".dc.2.bias")[pa],
             "m.dc.3.weight": g(".dc.3.weight")[ps][:, pa], "m.dc.3.bias": g(".dc.3.bias")[ps],
             "m.ffn.0.weight": g(".ffn.0.weight")[pu][:, ps], "m.ffn.0.bias": g(".ffn.0.bias")[pu],
             "m.ffn.2.weight": g(".ffn.2.weight")[ps][:, pv], "m.ffn.2.bias": g(".ffn.2.bias")[ps]}
        if (prefix + ".adaptor.weight") in self.sd:
            pi = self._perm(prefix, "in", g(".adaptor.weight").shape[1])
            m["m.adaptor.weight"], m["m.adaptor.bias"] = g(".adaptor.weight")[ps][:, pi], g(".adaptor.bias")[ps]
        else:
            pi = ps
        sub = self._sub(m)
        out_p = sub.dcb_f16(np.ascontiguousarray(x[:, :, pi]), "m", shortcut=shortcut,
                            q=None if q is None else np.asarray(q, np.float32).reshape(-1)[ps])
        out = np.empty_like(out_p)
        out[:, :, ps] = out_p
        return out

    def _sub(self, m):
        return O.Net(m)


class HaloFaultNet(O.Net):
    """the emulation with ONE seeded fault, CPU arithmetic only: in block `prefix` the depthwise 3x3 reads zeros instead of the
    halo row above output row `row` (an 8-row tile boundary) - what a tile that does not load its upper halo computes"""

    def __init__(self, sd, prefix, row):
        super().__init__(sd, f16=True)
        self._fault = (prefix, row)

    def _dw16(self, a, wd, bd, prefix):
        d = super()._dw16(a, wd, bd, prefix)
        if prefix == self._fault[0]:
            r = self._fault[1]
            assert 0 < r < a.shape[0]
            a0 = a.copy()
            a0[r - 1] = 0
            d[r] = super()._dw16(a0, wd, bd, prefix)[r]
        return d


def drop_bias(sd, prefix, channel):
    """state dict with the bias of one output channel of conv `prefix` dropped"""
    sd = dict(sd)
    b = np.array(sd[prefix + ".bias"], np.float32)
    b[channel] = 0
    sd[prefix + ".bias"] = b
    return sd


# ------------------------------------------------------------------------------------------------ shapes and cases

# feature (= picture / 8), y (= feature / 2, stride-2 conv), z (= ceil(y / 4)) map sizes
SHAPES = {
    # ragged against every tile; the 32-pixel forms and the head-inside forms
    "small": dict(fh=22, fw=30, yh=11, yw=15, zh=3, zw=4),
    # 12 444 pixels: the 128-pixel and 64-pixel forms of the feature-resolution networks
    "large_f": dict(fh=102, fw=122, yh=51, yw=61, zh=13, zw=16),
    # 12 423 pixels at y resolution (the class only 4K frames reach): prior networks only
    "large_y": dict(fh=202, fw=246, yh=101, yw=123, zh=26, zw=31),
}

_FEATURE_NETS = ("ext_i", "ext_p", "encoder", "decoder", "recon", "i_enc", "i_dec")
_PRIOR_NETS = ("prior_params", "spatial_prior", "i_prior_params", "i_reduction", "i_spatial_prior_1", "i_spatial_prior_2",
               "i_spatial_prior_3")
_SMALL_ONLY = ("hyper_encoder", "i_hyper_encoder")
CASES = ([(c, "small") for c in _FEATURE_NETS + _SMALL_ONLY + _PRIOR_NETS] + [(c, "large_f") for c in _FEATURE_NETS] +
         [(c, "large_y") for c in _PRIOR_NETS])
SMALL_CASES = [c for c in CASES if c[1] == "small"]


def model_of(case):
    return "dmci" if case.startswith("i_") else "dmc"


def case_id(c):
    return f"{c[0]}-{c[1]}"


def make_inputs(case, shape, seed=7):
    """seeded fp16-rounded inputs of one sub-network: HWC float32 arrays (a picture: [8 fh, 8 fw, 3] in [0, 1])"""
    s = SHAPES[shape]
    rng = np.random.default_rng([seed, sum(map(ord, case)), s["fh"]])
    fh, fw, yh, yw, zh, zw = (s[k] for k in ("fh", "fw", "yh", "yw", "zh", "zw"))
    nrm = lambda h, w, c, g=1.0: rh(rng.standard_normal((h, w, c)) * g)
    pic = lambda: rh(rng.uniform(0, 1, (8 * fh, 8 * fw, 3)))
    z = lambda: np.clip(np.round(rng.standard_normal((zh, zw, 128)) * 3), -128, 127).astype(np.float32)
    if case == "ext_i":
        return dict(frame=pic())
    if case == "ext_p":
        return dict(ref=nrm(fh, fw, 256))
    if case == "encoder":
        return dict(frame=pic(), ctx=nrm(fh, fw, 256))
    if case == "hyper_encoder":
        return dict(y=nrm(yh, yw, 128, 2.0))
    if case == "prior_params":
        return dict(z_hat=z(), x1=nrm(fh, fw, 256))
    if case == "spatial_prior":
        return dict(y_hat=nrm(yh, yw, 128, 2.0), params=nrm(yh, yw, 384))
    if case == "decoder":
        return dict(y_hat=nrm(yh, yw, 128, 2.0), ctx=nrm(fh, fw, 256))
    if case == "recon":
        return dict(feature=nrm(fh, fw, 256))
    if case == "i_enc":
        return dict(frame=pic())
    if case == "i_hyper_encoder":
        return dict(y=nrm(yh, yw, 256, 2.0))
    if case == "i_prior_params":
        return dict(z_hat=z())
    if case == "i_reduction":
        return dict(params=nrm(yh, yw, 514))
    if case.startswith("i_spatial_prior_"):
        return dict(y_hat=nrm(yh, yw, 256, 2.0), common=nrm(yh, yw, 256))
    if case == "i_dec":
        return dict(y_hat=nrm(yh, yw, 256, 2.0))
    raise KeyError(case)


def run_oracle(case, orc, inp, shape):
    """the sub-network `case` of OracleDMC / OracleDMCI `orc` -> {output name: HWC float32}"""
    s = SHAPES[shape]
    q = lambda name: orc.q(name, QP)
    clamp = lambda head: np.clip(O.pixel_shuffle(head, 8), np.float32(0), np.float32(1))
    if case in ("ext_i", "ext_p"):
        orc.ref_feature, orc.ref_frame = (None, inp["frame"]) if case == "ext_i" else (inp["ref"], None)
        x1, _ = orc.extractor_part1(orc.feature_adaptor(), q("q_feature"))
        return dict(x1=x1, ctx=orc.extractor_part2(x1))
    if case == "encoder":
        return dict(y=orc.encoder(inp["frame"], inp["ctx"], q("q_encoder")))
    if case == "hyper_encoder":
        return dict(z=orc.hyper_encoder(orc.pad_for_y(inp["y"])))
    if case == "prior_params":
        return dict(params=orc.prior_params(inp["z_hat"], orc.net.scale(inp["x1"], q("q_feature"))))
    if case == "spatial_prior":
        return dict(sp=orc.spatial_prior(np.concatenate([inp["y_hat"], inp["params"]], 2)))
    if case == "decoder":
        return dict(feature=orc.decoder(inp["y_hat"], inp["ctx"], q("q_decoder")))
    if case == "recon":
        head = orc.recon_head(inp["feature"], q("q_recon"))
        return dict(head=head, picture=clamp(head))
    if case == "i_enc":
        return dict(y=orc.enc(inp["frame"], q("q_scale_enc")))
    if case == "i_hyper_encoder":
        return dict(z=orc.hyper_enc(orc.pad_for_y(inp["y"])))
    if case == "i_prior_params":
        return dict(params=orc.prior_params(inp["z_hat"], s["yh"], s["yw"]))
    if case == "i_reduction":
        return dict(common=orc.reduction(inp["params"]))
    if case.startswith("i_spatial_prior_"):
        return dict(sp=orc.spatial_prior(np.concatenate([inp["y_hat"], inp["common"]], 2), int(case[-1])))
    if case == "i_dec":
        head = orc.dec_head(inp["y_hat"], q("q_scale_dec"))
        return dict(head=head, picture=clamp(head))
    raise KeyError(case)


def oracle_for(case, sd, f16):
    return (O.OracleDMCI if model_of(case) == "dmci" else O.OracleDMC)(sd, f16=f16)


_SD = {}


def state_dict(model):
    from opendcvc_amd import weights
    if model not in _SD:
        _SD[model] = weights.make_state_dict(model, 1234)
    return _SD[model]


_REF = {}


def reference(case, shape):
    """(inputs, emu, truth) of one (sub-network, shape): computed once, shared, never modified"""
    key = (case, shape)
    if key not in _REF:
        sd = state_dict(model_of(case))
        inp = make_inputs(case, shape)
        emu = run_oracle(case, oracle_for(case, sd, True), inp, shape)
        truth = run_oracle(case, oracle_for(case, sd, False), inp, shape)
        for d in (inp, emu, truth):
            for a in d.values():
                a.setflags(write=False)
        _REF[key] = (inp, emu, truth)
    return _REF[key]
