"""ctypes binding of libdcvc_amd.so (include/dcvc_amd.h).

The HIP library is the product: there is NO Python/torch fallback for any operator.  If the
shared object is missing or a call fails, an exception is raised (DcvcError) - never a silent
CPU path.
"""
import ctypes
import os
import subprocess
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int, c_int8, c_int16, c_int32, c_int64, c_size_t,
                    c_uint8, c_uint32, c_uint64, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
# DCVC_AMD_DIAG=1 selects the developer build with in-kernel diagnostics (make -C opendcvc_amd/csrc diag)
# DCVC_AMD_LIB=<file name in this directory> selects an experimental build (kernel A/B measurements)
LIB_PATH = os.path.join(_HERE, os.environ.get("DCVC_AMD_LIB") or
                        ("libdcvc_amd_diag.so" if os.environ.get("DCVC_AMD_DIAG") else "libdcvc_amd.so"))

F16, F32 = 0, 1
U8 = 2                    # uint8 planes: the metric entries only (dcvc_sse, dcvc_msssim_stats)
U16 = 3                   # uint16 planes (low-bit-aligned samples above 8 bits): the same entries only
SSE_BLOCKS = 1024         # DCVC_SSE_BLOCKS
DIGEST_PASS_WORDS = 1 << 20          # DCVC_DIGEST_PASS_WORDS: the words one grid-stride pass of dcvc_state_digest covers
EPI_BIAS, EPI_BIAS_QUANT, EPI_SHUFFLE2, EPI_WSILU = 0, 1, 2, 3


class DcvcError(RuntimeError):
    pass


class DigestMismatch(DcvcError):
    """The entry a decoded frame put into the DPB does not have the digest the stream carries for it (docs/state_digest.md):
    the decoder has left the encoder's state at this frame, or the digest unit is damaged.  index: the frame's position in
    decode order; is_i; expected: the stream's digest; got: the decoder's.  Resume at the next I frame."""

    def __init__(self, index, is_i, expected, got):
        super().__init__(f"frame {index} ({'I' if is_i else 'P'}): the decoder's reference state has digest {got:#018x}, "
                         f"the stream carries {expected:#018x}")
        self.index, self.is_i, self.expected, self.got = index, is_i, expected, got


def build(force=False):
    """Compiles opendcvc_amd/csrc into opendcvc_amd/libdcvc_amd.so with hipcc for gfx950."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"])
    subprocess.check_call(["make", "-C", csrc, "-j8"])
    return LIB_PATH


class GrainParamsC(ctypes.Structure):
    """dcvc_grain_params, passed by value (docs/film_grain.md)"""
    _fields_ = [("seed", ctypes.c_uint16), ("corr", c_uint8), ("scale_y", c_uint8 * 8), ("scale_cb", c_uint8),
                ("scale_cr", c_uint8)]


_P = c_void_p
_I = c_int
_L = c_int64
_F = c_float

# name -> (restype, argtypes); mirrors include/dcvc_amd.h one to one
_SIGS = {
    "dcvc_abi_version": (_I, []),
    "dcvc_last_error": (c_char_p, []),
    "dcvc_device_count": (_I, []),
    "dcvc_dcb_create": (_I, [_I, _I, _I, _I] + [_P] * 12 + [POINTER(_P)]),
    "dcvc_dcb_destroy": (None, [_P]),
    "dcvc_dcb_scratch_bytes": (c_size_t, [_P, _I, _I]),
    "dcvc_dcb_forward": (_I, [_P, _P, _L, _I, _P, _L, _I, _I, _I, _P, _P, _L, _P, _P]),
    "dcvc_dcb_forward_chained": (_I, [_P, _P, _L, _I, _P, _L, _I, _I, _I, _P, _P, _L, _P, _P, _I, _I, _P]),
    "dcvc_dcb_forward_then_conv": (_I, [_P, _P, _L, _I, _P, _L, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _L]),
    "dcvc_dcb_profile": (_I, [_P, _P, _L, _I, _I, _I, _P, _L, _P, _P, _I, POINTER(c_float), POINTER(c_float)]),
    "dcvc_dcb_profile_tail": (_I, [_P, _P, _L, _I, _I, _I, _P, _L, _P, _P, _I, POINTER(c_float)]),
    "dcvc_conv_create": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _P, _P, POINTER(_P)]),
    "dcvc_conv_destroy": (None, [_P]),
    "dcvc_conv_forward": (_I, [_P, _P, _L, _I, _P, _L, _I, _I, _I, _P, _P, _L, _P]),
    "dcvc_conv_forward_scaled": (_I, [_P, _P, _L, _I, _P, _L, _I, _I, _I, _P, _P, _P, _L, _P]),
    "dcvc_unshuffle8": (_I, [_I, _P, _I, _I, _I, _P, _L, _P]),
    "dcvc_shuffle8_clamp": (_I, [_I, _P, _L, _P, _I, _I, _I, _I, _P, _P]),
    "dcvc_yuv420_to_frame": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "dcvc_frame_to_yuv420": (_I, [_I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dcvc_rgb_to_frame": (_I, [_I, _P, _I, _I, _I, _I, _P, _P]),
    "dcvc_frame_to_rgb": (_I, [_I, _P, _I, _I, _I, _I, _P, _P]),
    "dcvc_replicate_pad_hwc": (_I, [_I, _P, _L, _I, _I, _I, _I, _I, _P, _L, _P]),
    "dcvc_scale_channels": (_I, [_I, _P, _L, _P, _L, _I, _P, _L, _P]),
    "dcvc_copy_channels": (_I, [_I, _P, _L, _L, _I, _P, _L, _P]),
    "dcvc_crop_hwc": (_I, [_I, _P, _L, _I, _I, _I, _I, _P, _L, _P]),
    "dcvc_round_z": (_I, [_I, _P, _L, _I, _I, _I, _P, _P]),
    "dcvc_z_from_int8": (_I, [_I, _P, _I, _I, _I, _P, _L, _P]),
    "dcvc_prior_enc_step": (_I, [_I, _I, _I, _I, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _F, _P, _L, _P, _L, _P, _P]),
    "dcvc_prior_dec_index": (_I, [_I, _I, _I, _P, _L, _I, _I, _I, _F, _P, _P]),
    "dcvc_prior_dec_restore": (_I, [_I, _I, _I, _P, _P, _L, _I, _I, _I, _P, _L, _P, _L, _P]),
    "dcvc_prior_dec_compact_ws_bytes": (_L, [_I, _I, _I, _I]),
    "dcvc_prior_dec_index_compact": (_I, [_I, _I, _I, _P, _L, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    "dcvc_prior_dec_restore_compact": (_I, [_I, _I, _I, _P, _P, _P, _P, _L, _I, _I, _I, _P, _L, _P, _L, _P]),
    "dcvc_prior_finish": (_I, [_I, _I, _P, _L, _P, _L, _I, _I, _I, _P]),
    "dcvc_op_process_with_mask": (_I, [_I, _P, _P, _P, _P, _F, _P, _P, _P, _P, _L, _P]),
    "dcvc_op_combine_for_reading_2x": (_I, [_I, _P, _P, _P, _L, _P]),
    "dcvc_op_restore_y_2x": (_I, [_I, _P, _P, _P, _P, _L, _P]),
    "dcvc_op_restore_y_4x": (_I, [_I, _P, _P, _P, _P, _L, _P]),
    "dcvc_op_build_index_dec": (_I, [_I, _P, _P, _P, _F, _F, _F, _F, _F, _L, _P]),
    "dcvc_op_build_index_enc": (_I, [_I, _P, _P, _P, _P, _F, _F, _F, _F, _F, _L, _P]),
    "dcvc_op_round_and_to_int8": (_I, [_I, _P, _P, _L, _P]),
    "dcvc_op_clamp_reciprocal_with_quant": (_I, [_I, _P, _P, _F, _P, _L, _P]),
    "dcvc_op_add_and_multiply": (_I, [_I, _P, _P, _P, _L, _P]),
    "dcvc_op_bias_quant": (_I, [_I, _P, _P, _P, _I, _L, _P]),
    "dcvc_op_bias_pixel_shuffle_8": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dcvc_op_replicate_pad": (_I, [_I, _P, _I, _I, _I, _I, _I, _P, _P]),
    "dcvc_op_bias_wsilu_depthwise_conv2d": (_I, [_I, _P, _P, _P, _I, _I, _I, _P, _P]),
    "dcvc_nchw_to_hwc": (_I, [_I, _P, _I, _L, _P, _L, _P]),
    "dcvc_hwc_to_nchw": (_I, [_I, _P, _L, _I, _L, _P, _P]),
    "dcvc_rans_enc_create": (_P, []),
    "dcvc_rans_enc_destroy": (None, [_P]),
    "dcvc_rans_enc_add_cdf": (_I, [_P, _P, _I, _I, _P, _P]),
    "dcvc_rans_enc_empty_cdf": (_I, [_P]),
    "dcvc_rans_enc_set_use_two": (None, [_P, _I]),
    "dcvc_rans_enc_reset": (_I, [_P]),
    "dcvc_rans_enc_encode_y": (_I, [_P, _P, _L, _I]),
    "dcvc_rans_enc_encode_y_borrowed": (_I, [_P, _P, _L, _I]),
    "dcvc_rans_enc_encode_z": (_I, [_P, _P, _L, _I, _I, _I]),
    "dcvc_rans_enc_flush": (_I, [_P]),
    "dcvc_rans_enc_get_stream": (_L, [_P, POINTER(_P)]),
    "dcvc_rans_dec_create": (_P, []),
    "dcvc_rans_dec_destroy": (None, [_P]),
    "dcvc_rans_dec_add_cdf": (_I, [_P, _P, _I, _I, _P, _P]),
    "dcvc_rans_dec_empty_cdf": (_I, [_P]),
    "dcvc_rans_dec_set_use_two": (None, [_P, _I]),
    "dcvc_rans_dec_set_stream": (_I, [_P, _P, _L]),
    "dcvc_rans_dec_decode_y": (_I, [_P, _P, _L, _I]),
    "dcvc_rans_dec_decode_z": (_I, [_P, _L, _I, _I, _I]),
    "dcvc_rans_dec_get": (_L, [_P, _P, _L]),
    "dcvc_rans_dec_decode_and_get_y": (_I, [_P, _P, _L, _I, _P]),
    "dcvc_rans_dec_decode_compact": (_I, [_P, _P, _L, _I, _P]),
    "dcvc_rans_dec_check_end": (_I, [_P]),
    "dcvc_pmf_to_quantized_cdf": (_I, [_P, _I, _I, _P]),
    "dcvc_rans_chunked_encode_y": (_L, [_P, _P, _L, _I, _I, _P, _L]),
    "dcvc_rans_chunked_decode_y": (_I, [_P, _P, _L, _P, _L, _I, _I, _P]),
    "dcvc_rans_dev_create": (_I, [_P, _I, _I, _P, _P, POINTER(_P)]),
    "dcvc_rans_dev_destroy": (None, [_P]),
    "dcvc_rans_dev_enc_ws_bytes": (_L, [_L, _I, _I]),
    "dcvc_rans_dev_encode_y": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _L, _P]),
    "dcvc_rans_dev_dec_ws_bytes": (_L, [_L, _I]),
    "dcvc_rans_dev_decode_y": (_I, [_P, _P, _L, _P, _P, _P, _L, _I, _P, _P, _P, _P]),
    "dcvc_prior_dec_index_compact_dev": (_I, [_I, _I, _I, _P, _L, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    "dcvc_prior_dec_restore_compact_dev": (_I, [_I, _I, _I, _P, _P, _P, _P, _L, _I, _I, _I, _P, _L, _P, _L, _P]),
    "dcvc_compact_symbols_dev": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "dcvc_host_alloc": (_P, [c_size_t]),
    "dcvc_host_free": (None, [_P]),
    "dcvc_host_device_ptr": (_P, [_P]),
    "dcvc_compact_symbols": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "dcvc_frame_to_yuv420_planes": (_I, [_I, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dcvc_sse": (_I, [_I, _P, _I, _P, _L, _P, _P, _P]),
    "dcvc_msssim_ws_bytes": (_L, [_I, _I]),
    "dcvc_msssim_stats": (_I, [_I, _P, _I, _P, _I, _I, c_double, _P, _P, POINTER(_I), _P]),
    "dcvc_planes_to_frame": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _L, _L, _I, _I, _I, _I, _P, _P]),
    "dcvc_frame_to_planes": (_I, [_I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _L, _L, _P]),
    "dcvc_frame_to_metric_planes": (_I, [_I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dcvc_v210_row_bytes": (_L, [_I]),
    "dcvc_yuv422_to_frame": (_I, [_I, _I, _I, _P, _P, _P, _L, _L, _I, _I, _I, _I, _P, _P]),
    "dcvc_frame_to_yuv422": (_I, [_I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _L, _L, _P]),
    "dcvc_resize_frame": (_I, [_I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P]),
    "dcvc_bars_ws_bytes": (_L, [_I, _I]),
    "dcvc_bars_reset": (_I, [_P, _I, _I, _P]),
    "dcvc_bars_scan": (_I, [_I, _P, _I, _I, _I, _I, _P, _P]),
    "dcvc_bars_extent": (_I, [_P, _I, _I, _F, _P, _P]),
    "dcvc_frame_window": (_I, [_I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    "dcvc_frame_paste": (_I, [_I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, POINTER(c_float), _P]),
    "dcvc_frame_maxdiff_ws_bytes": (_L, []),
    "dcvc_frame_maxdiff": (_I, [_I, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "dcvc_deinterlace": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "dcvc_deinterlace_field": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "dcvc_comb_ws_bytes": (_L, []),
    "dcvc_comb_detect": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "dcvc_field_match_ws_bytes": (_L, []),
    "dcvc_field_match": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "dcvc_field_weave": (_I, [_I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "dcvc_grain_apply": (_I, [_I, _P, _I, _I, _I, _I, _P, GrainParamsC, c_uint32, _P]),
    "dcvc_grain_stats": (_I, [_I, _P, _P, _I, _I, _I, _I, _P, _P]),
    "dcvc_tf_pyramid_bytes": (_L, [_I, _I]),
    "dcvc_tf_pyramid": (_I, [_I, _P, _I, _I, _I, _I, _P, _P]),
    "dcvc_tf_motion_ws_bytes": (_L, [_I, _I]),
    "dcvc_tf_motion": (_I, [_P, POINTER(_P), _I, _I, _I, _P, _P, _P, _P]),
    "dcvc_tf_blend": (_I, [_I, _P, POINTER(_P), POINTER(_I), _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P]),
    "dcvc_tf_noise_ws_bytes": (_L, []),
    "dcvc_tf_noise_workgroups": (_I, [_I]),
    "dcvc_tf_noise": (_I, [_P, _P, POINTER(_I), _I, _I, _I, _P, _P, _P, _P]),
    "dcvc_tf_blend_auto": (_I, [_I, _P, POINTER(_P), POINTER(_I), _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "dcvc_tf_refine": (_I, [_P, POINTER(_P), _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "dcvc_tf_blend_subpel": (_I, [_I, _P, POINTER(_P), POINTER(_I), _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P]),
    "dcvc_frame_analysis_ws_bytes": (_L, [_I, _I]),
    "dcvc_frame_analyze": (_I, [_I, _P, _L, _I, _I, _P, _P, _P, _P, _P]),
    "dcvc_lookahead_ws_bytes": (_L, [_I, _I]),
    "dcvc_lookahead_cost": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "dcvc_rate_estimate_ws_bytes": (_L, [_I, _I, _I]),
    "dcvc_rate_estimate": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P, _P, _P]),
    "dcvc_state_digest_ws_bytes": (_L, [_L]),
    "dcvc_state_digest": (_I, [_P, _L, _P, c_uint64, _I, _P, _P]),
    "dcvc_copy_f32": (_I, [_P, _P, _I, _P]),
    "dcvc_memcpy_d2h": (_I, [_P, _P, c_size_t, _P]),
    "dcvc_memcpy_h2d": (_I, [_P, _P, c_size_t, _P]),
    "dcvc_stream_sync": (_I, [_P]),
}

EXPORTS = tuple(_SIGS.keys())
_lib = None


def lib():
    """Returns the loaded library; raises DcvcError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DcvcError(
                f"{LIB_PATH} not found: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C opendcvc_amd/csrc`). "
                "There is no CPU fallback.")
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise DcvcError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise DcvcError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if L.dcvc_abi_version() != 1:
            raise DcvcError("libdcvc_amd.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc, what=""):
    if rc is not None and rc < 0:
        msg = lib().dcvc_last_error()
        raise DcvcError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc


def require_gpu():
    n = lib().dcvc_device_count()
    if n <= 0:
        raise DcvcError("no HIP device visible: the DCVC-RT hot path needs an MI355X (no CPU fallback)")
    return n
