"""tests/prior_ref.py (the CPU restatement the entropy-model glue kernels are checked against, tests/test_gpu_prior.py)
against the oracle codecs themselves: every checkerboard step of OracleDMC.compress (2 groups) and OracleDMCI.compress
(4 groups) on a small seeded frame, from the traced y / params / spatial-prior outputs."""
import numpy as np
import pytest

import dcvc_oracle as O
import prior_ref as R
from opendcvc_amd import weights

THRES = 0.12


@pytest.fixture(scope="module")
def traces():
    sdi, sdp = weights.make_state_dict("dmci", 1234), weights.make_state_dict("dmc", 1234)
    oi, op = O.OracleDMCI(sdi), O.OracleDMC(sdp)
    oi.update(THRES)
    op.update(THRES)
    enc = oi.compress(weights.synthetic_frame_yuv444(64, 64, 0, 0), 32)
    op.clear_dpb()
    op.add_ref_frame(None, enc["x_hat"])
    op.compress(weights.synthetic_frame_yuv444(64, 64, 1, 0), 40)
    return oi.trace, op.trace


def _check_steps(steps, n_groups, packed_want):
    """steps: (q_mode, y, qsrc, scales, means) of each step; the chain must give the oracle's packed streams and y_hat"""
    yhat, packs = None, []
    for step, (q_mode, y, qsrc, scales, means) in enumerate(steps):
        yhat, packed = R.enc_step(n_groups, step, q_mode, y, qsrc, scales, means, THRES, yhat)
        packs.append(packed)
        # the decoder's index step sees the same indexes and sentinels; restoring the encoder's symbols gives its y_hat
        assert np.array_equal(R.dec_index(n_groups, step, scales, THRES), (packed.view(np.uint16) & 0xFF).astype(np.uint8))
        prev = None if step == 0 else restored
        restored = R.dec_restore(n_groups, step, (packed >> 8).astype(np.int8), means, prev)
        assert np.array_equal(restored.view(np.uint32), yhat.view(np.uint32)), step
        if step == 0:
            first = yhat
    for step, want in enumerate(packed_want):
        assert np.array_equal(R.kept(packs[step]), want), step
        # ... and the kept entries are CodecBase.pack_y of the step's collapsed symbols and scales
        pk = R._coder(THRES).pack_y(_sym_hwc(packs[step], yhat.shape, n_groups), _scales_for_pack(steps[step][3], n_groups, step))
        assert np.array_equal(R.kept(packs[step]), pk), step
    return first, yhat


def _sym_hwc(packed, shape, n_groups):
    H, W, C = shape
    return np.ascontiguousarray((packed >> 8).astype(np.float32).reshape(C // n_groups, H, W).transpose(1, 2, 0))


def _scales_for_pack(scales, n_groups, step):
    H, W, C = scales.shape
    return R.collapse(scales * R._masks(n_groups, H, W, C)[step], n_groups)


def test_restatement_reproduces_oracle_dmc(traces):
    t = traces[1]
    y, params = t["y"], t["params"]
    C = y.shape[2]
    sp = t["sp"][0]
    steps = [(0, y, params[:, :, :C], params[:, :, C:2 * C], params[:, :, 2 * C:]),
             (0, y, params[:, :, :C], sp[:, :, :C], sp[:, :, C:])]
    first, yhat = _check_steps(steps, 2, [t["packed0"], t["packed1"]])
    assert np.array_equal(first, t["y_hat_0"])
    assert np.array_equal(R.finish(0, yhat, params[:, :, :C]), t["y_hat"])


def test_restatement_reproduces_oracle_dmci(traces):
    t = traces[0]
    y, params = t["y"], t["params"]
    C = y.shape[2]
    steps = [(1, y, params, params[:, :, 2:2 + C], params[:, :, 2 + C:2 + 2 * C])]
    steps += [(1, y, params, sp[:, :, :C], sp[:, :, C:]) for sp in t["sp"]]
    first, yhat = _check_steps(steps, 4, t["packed"])
    assert np.array_equal(first, t["y_hat_0"])
    assert np.array_equal(R.finish(1, yhat, params), t["y_hat"])


def test_restatement_z_path():
    rng = np.random.default_rng(5)
    z = rng.normal(0, 60, (3, 5, 7)).astype(np.float32)
    z[0, 0, :4] = [2.5, -2.5, 127.5, -128.5]
    z_hat, z8 = R.round_z(z)
    assert list(z_hat[0, 0, :4]) == [2, -2, 127, -128]
    want = np.clip(np.round(z), -128, 127)
    assert np.array_equal(z_hat, want) and np.array_equal(z8, O._chw_flat(want).astype(np.int8))
    assert np.array_equal(R.z_from_int8(z8, 3, 5, 7), want)


def test_seam_f16_contract_vs_reference_half_arithmetic(golden_dir):
    """How far the operator seam's fp16 contract (fp32 arithmetic on the fp16 inputs, one rounding per store - what
    tests/test_gpu_ops.py::test_flat_ops_contract_bit_exact pins the kernels to) is from the reference's own fp16 arithmetic
    (a rounding to fp16 after every operation), on the reference's fallback outputs (tests/golden/make_golden_ops_f16.py).
    Measured on this fixture: 0.45 % of the symbols (0.89 % of the masked-in ones) and 0.76 % of the indexes differ, each
    by exactly 1, so 1.80 % of the entries of the kept stream differ; the masked residual, the masked scales and the skip condition are identical.  The bounds below are those
    measurements rounded up: a change of either arithmetic that moves more symbols fails here."""
    import os
    g = np.load(os.path.join(golden_dir, "ops_f16_ref.npz"))
    f = lambda a: np.asarray(a, np.float32)
    r = O.process_with_mask(f(g["pwm.y"]), f(g["pwm.scales"]), f(g["pwm.means"]), f(g["pwm.mask"]), 0.12)
    got = dict(zip(("y_res", "y_q", "y_hat", "s_hat"), (v.astype(np.float16) for v in r)))
    for name in ("y_res", "s_hat"):
        assert np.array_equal(got[name].view(np.uint16), g["pwm." + name].view(np.uint16)), name
    dq = np.abs(f(got["y_q"]) - f(g["pwm.y_q"]))
    assert dq.max() <= 1 and np.mean(dq > 0) <= 0.006
    s = np.clip(f(g["pwm.scales"]), np.float32(O.SCALE_MIN), np.float32(O.SCALE_MAX))
    idx = O.scale_to_index(s, O.SCALE_MIN, O.SCALE_MAX, O.LOG_SCALE_MIN, O.LOG_STEP_RECIP)
    di = np.abs(idx.astype(np.int64) - g["idx.dec"])
    assert di.max() <= 1 and np.mean(di > 0) <= 0.01
    assert np.array_equal(s > np.float32(0.12), g["idx.cond"])
    # the kept packed stream: same length (same skip condition), entries differ where a symbol or an index does
    packed = ((f(got["y_q"]).astype(np.int32) << 8) + idx).astype(np.int16)[g["idx.cond"]]
    assert packed.size == g["idx.enc"].size and np.mean(packed != g["idx.enc"]) <= 0.02
