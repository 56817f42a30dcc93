"""prior_ref.py - CPU restatement of the entropy-model glue kernels of dcvc_prior.hip (TEST INFRASTRUCTURE ONLY).

One function per C ABI entry point: dcvc_prior_enc_step, dcvc_prior_dec_index, dcvc_prior_dec_restore, dcvc_prior_finish,
dcvc_round_z and dcvc_z_from_int8.  Tensors are HWC numpy arrays in the storage type (np.float32 or np.float16); an input
may be a channel slice of a wider buffer (params[:, :, 2:2 + C]), which is how a leading dimension larger than C is
written here.  Outputs are new contiguous arrays: [H, W, C] in the storage type, symbol / index arrays flat in the CHW
order of the collapsed [H, W, C / n_groups] tensor.

Built from the oracle's own pieces (masks_2x / masks_4x, process_with_mask, scale_to_index through CodecBase._indexes,
sigmoid, the collapse of compress_prior_2x / _4x and the CHW packing of CodecBase.pack_y), not from the kernels: in fp32 it
is the oracle's arithmetic by construction.  In fp16 it rounds to fp16 exactly where the kernels store and nowhere else
(dcvc_prior.hip, prior_enc_kernel):
  - inputs are loaded from fp16 (exact in fp32);
  - the quantisation step qe, yq = y * qe and v = rint(yq - m) are fp32;
  - y_hat of the step = half(v + m);  after step 0 the running sum is half(prev + y_hat);
  - the channel groups that are not active in the step are copied as stored (step 0: +0);
  - finish: half(y_hat * q) with q in fp32.
Skip rules (force_zero_thres): the symbol is zeroed on the RAW scale (!(s > thres)), the sentinel index 0xFF is chosen on
the CLAMPED scale (clamp(s, 0.11, 16) > thres); thres < 0 disables both.
"""
import numpy as np

import dcvc_oracle as O

SENTINEL = 0xFF


def _f(a):
    """load from the storage type (fp16 -> fp32 is exact)"""
    return np.asarray(a, dtype=np.float32)


def _masks(n_groups, H, W, C):
    assert n_groups in (2, 4) and C % n_groups == 0
    return O.masks_2x(H, W, C) if n_groups == 2 else O.masks_4x(H, W, C)


def collapse(a, n_groups):
    """single_part_for_writing_2x / _4x as the oracle writes it (OracleDMC / OracleDMCI.compress): the sum of the groups"""
    C = a.shape[2]
    if n_groups == 2:
        return a[:, :, :C // 2] + a[:, :, C // 2:]
    return (a[:, :, :C // 4] + a[:, :, C // 4:C // 2]) + (a[:, :, C // 2:3 * C // 4] + a[:, :, 3 * C // 4:])


def _coder(thres):
    """a CodecBase with nothing but the skip threshold: what _indexes / pack_y read"""
    cb = O.CodecBase.__new__(O.CodecBase)
    cb.thres = None if thres < 0 else float(np.float32(thres))
    return cb


def indexes(scales_w, thres):
    """CHW indexes of collapsed scales with the sentinel at the skipped positions (CodecBase._indexes)"""
    idx, keep = _coder(thres)._indexes(O._chw_flat(scales_w))
    return np.where(keep, idx, np.uint8(SENTINEL)).astype(np.uint8) if keep is not None else idx


def _accumulate(step, mask, yh, yhat_in, dt):
    """the step's y_hat (already in the storage type) at its active positions, the stored running sum elsewhere"""
    active = mask > 0
    if step == 0:
        return np.where(active, yh, np.float32(0)).astype(dt)
    prev = _f(yhat_in)
    return np.where(active, prev + yh, prev).astype(dt)


def enc_step(n_groups, step, q_mode, y, qsrc, scales, means, thres, yhat_in=None, dt=np.float32):
    """dcvc_prior_enc_step -> (yhat_out [H, W, C] dt, packed int16 [C / n_groups * H * W], CHW, low byte 0xFF = skipped).
    q_mode 0: qsrc [H, W, C] = q_dec (compress_prior_2x: y * (1 / max(q_dec, 0.5)));
    q_mode 1: qsrc [H, W, >= 1] = raw params, q_enc = sigmoid(qsrc[..., 0]) * 1.5 + 0.5 (separate_prior)."""
    H, W, C = y.shape
    mask = _masks(n_groups, H, W, C)[step]
    if q_mode == 0:
        yq = _f(y) * (np.float32(1.0) / np.maximum(_f(qsrc[:, :, :C]), np.float32(0.5)))
    else:
        yq = _f(y) * (O.sigmoid(_f(qsrc[:, :, 0:1])) * np.float32(1.5) + np.float32(0.5))
    _, y_q, y_hat, s_hat = O.process_with_mask(yq, _f(scales), _f(means), mask, None if thres < 0 else thres)
    yh = y_hat.astype(dt).astype(np.float32)
    sym = O._chw_flat(collapse(y_q, n_groups)).astype(np.int32)
    idx = indexes(collapse(s_hat, n_groups), thres).astype(np.int32)
    packed = (sym * 256 + idx).astype(np.int16)
    return _accumulate(step, mask, yh, yhat_in, dt), packed


def kept(packed):
    """the entries of a packed step that go into the stream (the boolean-mask compaction, CodecBase.pack_y)"""
    return packed[(packed.view(np.uint16) & 0xFF) != SENTINEL]


def dec_index(n_groups, step, scales, thres):
    """dcvc_prior_dec_index -> uint8 [C / n_groups * H * W] (combine_for_reading_* + build_index_dec; 0xFF = skipped)"""
    H, W, C = scales.shape
    mask = _masks(n_groups, H, W, C)[step]
    return indexes(collapse(_f(scales) * mask, n_groups), thres)


def dec_restore(n_groups, step, sym_chw, means, yhat_in=None, dt=np.float32):
    """dcvc_prior_dec_restore: restore_y_2x / _4x of the decoded symbols (CHW int8) + the running sum"""
    H, W, C = means.shape
    mask = _masks(n_groups, H, W, C)[step]
    y_q_r = np.ascontiguousarray(np.asarray(sym_chw, np.int8).astype(np.float32).reshape(C // n_groups, H, W).transpose(1, 2, 0))
    cur = (np.concatenate([y_q_r] * n_groups, 2) + _f(means)) * mask
    return _accumulate(step, mask, cur.astype(dt).astype(np.float32), yhat_in, dt)


def finish(q_mode, yhat, qsrc, dt=np.float32):
    """dcvc_prior_finish: y_hat * q_dec (q_mode 0: max(qsrc, 0.5) per element; 1: sigmoid(qsrc[..., 1]) * 1.5 + 0.5)"""
    C = yhat.shape[2]
    if q_mode == 0:
        q = np.maximum(_f(qsrc[:, :, :C]), np.float32(0.5))
    else:
        q = O.sigmoid(_f(qsrc[:, :, 1:2])) * np.float32(1.5) + np.float32(0.5)
    return (_f(yhat) * q).astype(dt)


def round_z(z, dt=np.float32):
    """dcvc_round_z -> (z_hat [H, W, C] dt, int8 symbols in CHW order)"""
    z_hat = np.clip(np.round(_f(z)), np.float32(-128), np.float32(127))
    return z_hat.astype(dt), O._chw_flat(z_hat).astype(np.int8)


def z_from_int8(z_chw, H, W, C, dt=np.float32):
    """dcvc_z_from_int8: CHW int8 -> [H, W, C] dt"""
    return np.ascontiguousarray(np.asarray(z_chw, np.int8).reshape(C, H, W).transpose(1, 2, 0)).astype(dt)
