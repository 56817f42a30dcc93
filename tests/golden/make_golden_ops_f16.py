"""fp16 fixtures of the operator seam from the REFERENCE ITSELF: runs the CPU fallback branches of the reference's
src/layers/cuda_inference.py (process_with_mask :58-74, build_index_dec :123-143, build_index_enc :146-171) on .half()
tensors and writes tests/golden/ops_f16_ref.npz:

    pwm.{y,scales,means,mask}   fp16 inputs [1, 16, 24, 32] (values spread like a y latent: ties, +-128, tiny scales)
    pwm.{y_res,y_q,y_hat,s_hat} the reference's fp16 outputs, force_zero_thres = THRES
    idx.dec                     build_index_dec indexes of pwm.scales (uint8), idx.cond its skip condition
    idx.enc                     build_index_enc of (pwm.y_q, pwm.scales): the kept packed symbols (int16)

The reference's fp16 arithmetic rounds to fp16 after EVERY operation (torch half tensors here, c10::Half in kernel.cu);
the HIP seam computes each kernel in fp32 on the loaded fp16 inputs and rounds once per store.
tests/test_prior_ref.py measures how many symbols / indexes that changes.  Where this fallback and kernel.cu differ in
rounding: kernel.cu's scale_to_index (:276-286) clamps and scales with Half constants (scale_min, scale_max,
log_scale_min, log_step_recip all of type scalar_t = c10::Half), while the fallback (:138-140, :161-163) uses them as
Python floats (fp32 op-math scalars, not rounded to fp16); kernel.cu compares with Half thresholds (:60 / :78, :292)
and skips the zeroing for a threshold of exactly 0 (:98).  Build container only.

    python tests/golden/make_golden_ops_f16.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_harness  # noqa: E402

THRES = 0.12
SHAPE = (1, 16, 24, 32)
SCALE_MIN, SCALE_MAX, LEVELS = 0.11, 16.0, 128


def inputs(seed=2024):
    rng = np.random.default_rng(seed)
    means = rng.normal(0, 4, SHAPE)
    y = means + np.where(rng.random(SHAPE) < 0.2, rng.choice([0.5, -0.5, 1.5, -2.5, 127.5, -128.5], SHAPE),
                         rng.normal(0, 6, SHAPE))
    scales = np.exp(rng.normal(-1.5, 1.6, SHAPE))
    mask = (rng.random(SHAPE) < 0.5).astype(np.float64)
    return [a.astype(np.float16) for a in (y, scales, means, mask)]


def main():
    _, _, _, ref_ops, _, _ = ref_harness.load()
    torch.set_grad_enabled(False)
    import math
    log_min = math.log(SCALE_MIN)
    log_recip = 1.0 / ((math.log(SCALE_MAX) - log_min) / (LEVELS - 1))
    y, scales, means, mask = inputs()
    t = lambda a: torch.from_numpy(a)
    out = {"pwm.y": y, "pwm.scales": scales, "pwm.means": means, "pwm.mask": mask}
    r = ref_ops.process_with_mask(t(y), t(scales), t(means), t(mask), THRES)
    for name, v in zip(("y_res", "y_q", "y_hat", "s_hat"), r):
        assert v.dtype == torch.float16
        out["pwm." + name] = v.numpy()
    idx, cond = ref_ops.build_index_dec(t(scales).clone(), SCALE_MIN, SCALE_MAX, log_min, log_recip, THRES)
    out["idx.dec"], out["idx.cond"] = idx.numpy(), cond.numpy()
    out["idx.enc"] = ref_ops.build_index_enc(r[1], t(scales).clone(), SCALE_MIN, SCALE_MAX, log_min, log_recip, THRES).numpy()
    path = os.path.join(HERE, "ops_f16_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
