"""The argument checks of the latent-side entries (csrc/dcvc_prior.hip: check_step, check_map, check_yhat, the LDS budget) as far
as a GPU-less host can see them: every entry refuses a bad step, map size, operand, workspace or LDS size before its first
HIP call, names itself (and the operand) in the error and writes nothing.  Only refusals are exercised: no call here would be
valid with its host pointers, so a case that shows a check PASSING (step 0 without yhat_in, ldq = 2 of the intra form) pairs
it with a later refusal and looks at which operand the error names."""
import ctypes

import pytest

from opendcvc_amd import _lib

# a 64-byte-aligned host buffer stands in for every pointer
_BUF = ctypes.create_string_buffer(65536 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63
C0 = 8
BASE = dict(dtype=_lib.F16, n_groups=2, step=0, q_mode=0, H=4, W=6, C=C0, thres=0.12,
            y=_PTR, ldy=C0 + 3, qsrc=_PTR, ldq=C0, scales=_PTR, lds=C0 + 1, means=_PTR, ldm=C0 + 2,
            yhat_in=_PTR, ldhi=C0 + 4, yhat_out=_PTR, ldho=C0 + 5, yhat=_PTR, ldh=C0,
            packed=_PTR, idx=_PTR, sym=_PTR, ws=_PTR, idx_out=_PTR, count_out=_PTR)


def _enc_step(a):
    return _lib.lib().dcvc_prior_enc_step(a["dtype"], a["n_groups"], a["step"], a["q_mode"], a["y"], a["ldy"], a["qsrc"], a["ldq"],
                                          a["scales"], a["lds"], a["means"], a["ldm"], a["H"], a["W"], a["C"], a["thres"],
                                          a["yhat_in"], a["ldhi"], a["yhat_out"], a["ldho"], a["packed"], None)


def _dec_index(a):
    return _lib.lib().dcvc_prior_dec_index(a["dtype"], a["n_groups"], a["step"], a["scales"], a["lds"], a["H"], a["W"], a["C"],
                                           a["thres"], a["idx"], None)


def _dec_restore(a):
    return _lib.lib().dcvc_prior_dec_restore(a["dtype"], a["n_groups"], a["step"], a["sym"], a["means"], a["ldm"], a["H"], a["W"],
                                             a["C"], a["yhat_in"], a["ldhi"], a["yhat_out"], a["ldho"], None)


def _index_compact(fn):
    return lambda a: getattr(_lib.lib(), fn)(a["dtype"], a["n_groups"], a["step"], a["scales"], a["lds"], a["H"], a["W"], a["C"],
                                             a["thres"], a["idx"], a["ws"], a["idx_out"], a["count_out"], None)


def _restore_compact(fn):
    return lambda a: getattr(_lib.lib(), fn)(a["dtype"], a["n_groups"], a["step"], a["sym"], a["idx"], a["ws"], a["means"], a["ldm"],
                                             a["H"], a["W"], a["C"], a["yhat_in"], a["ldhi"], a["yhat_out"], a["ldho"], None)


def _finish(a):
    return _lib.lib().dcvc_prior_finish(a["dtype"], a["q_mode"], a["yhat"], a["ldh"], a["qsrc"], a["ldq"], a["H"], a["W"], a["C"], None)


def _compact_symbols(fn):
    return lambda a: getattr(_lib.lib(), fn)(a["packed"], a["n_per_part"], a["n_parts"], a["out"], a["counts"], a["ws"], None)


# entry -> (call, its HWC operands as (pointer keyword, ld keyword, name in the error), its other pointers, has y_hat, has a workspace)
STEP_ENTRIES = {
    "dcvc_prior_enc_step": (_enc_step, [("y", "ldy", "y"), ("qsrc", "ldq", "qsrc"), ("scales", "lds", "scales"), ("means", "ldm", "means"),
                                        ("yhat_out", "ldho", "yhat_out")], ["packed"], True, False),
    "dcvc_prior_dec_index": (_dec_index, [("scales", "lds", "scales")], ["idx"], False, False),
    "dcvc_prior_dec_restore": (_dec_restore, [("means", "ldm", "means"), ("yhat_out", "ldho", "yhat_out")], ["sym"], True, False),
    "dcvc_prior_dec_index_compact": (_index_compact("dcvc_prior_dec_index_compact"), [("scales", "lds", "scales")],
                                     ["idx", "ws", "idx_out", "count_out"], False, True),
    "dcvc_prior_dec_index_compact_dev": (_index_compact("dcvc_prior_dec_index_compact_dev"), [("scales", "lds", "scales")],
                                         ["idx", "ws", "idx_out", "count_out"], False, True),
    "dcvc_prior_dec_restore_compact": (_restore_compact("dcvc_prior_dec_restore_compact"),
                                       [("means", "ldm", "means"), ("yhat_out", "ldho", "yhat_out")], ["sym", "idx", "ws"], True, True),
    "dcvc_prior_dec_restore_compact_dev": (_restore_compact("dcvc_prior_dec_restore_compact_dev"),
                                           [("means", "ldm", "means"), ("yhat_out", "ldho", "yhat_out")], ["sym", "idx", "ws"], True, True),
}
C_BIG = 2 * 8200          # 8200 channels per group: 8 bytes each (the smallest staging of the entries) are above 64 KiB


def _step_cases():
    """(entry, case id, changed arguments, what the error must name besides the entry)"""
    out = []
    for name, (_, maps, ptrs, has_yhat, has_ws) in STEP_ENTRIES.items():
        out += [(name, "bad_dtype", dict(dtype=_lib.U8), b"dtype"),
                (name, "three_groups", dict(n_groups=3, C=9), b"3 groups"),
                (name, "step_is_n_groups", dict(step=2), b"step 2"),
                (name, "C_not_a_multiple", dict(C=C0 + 1, **{ld: C0 + 8 for _, ld, _ in maps}), b"9 channels"),
                (name, "H_0", dict(H=0), b"0 x 6"),
                (name, "W_0", dict(W=0), b"4 x 0"),
                (name, "lds_over_budget", dict(C=C_BIG, **{ld: C_BIG for _, ld, _ in maps}), b"LDS")]
        for ptr, ld, what in maps:
            out += [(name, "null_" + ptr, {ptr: None}, what.encode()), (name, ld + "_below_C", {ld: C0 - 1}, what.encode())]
        out += [(name, "null_" + ptr, {ptr: None}, b"null") for ptr in ptrs]
        if has_yhat:
            out += [(name, "step_1_without_yhat_in", dict(step=1, yhat_in=None), b"yhat_in required after step 0"),
                    (name, "step_1_ldhi_below_C", dict(step=1, ldhi=C0 - 1), b"yhat_in"),
                    # step 0 looks at neither yhat_in nor its ld: the refusal is the next operand's
                    (name, "step_0_ignores_yhat_in", dict(yhat_in=None, ldhi=0, ldho=C0 - 1), b"yhat_out")]
        if has_ws:
            out.append((name, "workspace_off_by_8", dict(ws=_PTR + 8), b"16-byte aligned"))
    # the intra form reads channels 0 and 1 of params: ldq = 1 is refused, ldq = 2 passes (the refusal is a later operand's)
    out += [("dcvc_prior_enc_step", "intra_ldq_1", dict(q_mode=1, ldq=1), b"qsrc"),
            ("dcvc_prior_enc_step", "intra_ldq_2_passes", dict(q_mode=1, ldq=2, packed=None), b"packed_chw")]
    return [pytest.param(*c, id=f"{c[0]}-{c[1]}") for c in out]


def _refused(name, call, args, names):
    before = bytes(_BUF)
    assert call(args) == -1, name
    err = _lib.lib().dcvc_last_error()
    assert (name + ":").encode() in err, err
    assert names in err, err
    assert bytes(_BUF) == before
    return err


@pytest.mark.parametrize("name, case, change, names", _step_cases())
def test_a_bad_step_argument_is_refused_by_name_before_any_hip_call(name, case, change, names):
    err = _refused(name, STEP_ENTRIES[name][0], dict(BASE, **change), names)
    if case in ("step_0_ignores_yhat_in", "intra_ldq_2_passes"):
        assert b"yhat_in" not in err and b"qsrc" not in err, err


FINISH_CASES = {"bad_dtype": (dict(dtype=_lib.U8), b"dtype"), "H_0": (dict(H=0), b"0 x 6"), "W_0": (dict(W=0), b"4 x 0"),
                "C_0": (dict(C=0), b"x 0"), "null_yhat": (dict(yhat=None), b"yhat"), "null_qsrc": (dict(qsrc=None), b"qsrc"),
                "ldh_below_C": (dict(ldh=C0 - 1), b"yhat"), "ldq_below_C": (dict(ldq=C0 - 1), b"qsrc"),
                "intra_ldq_1": (dict(q_mode=1, ldq=1), b"qsrc"),
                "intra_ldq_2_passes": (dict(q_mode=1, ldq=2, ldh=C0 - 1), b"yhat")}


@pytest.mark.parametrize("case", list(FINISH_CASES))
def test_a_bad_finish_argument_is_refused_by_name(case):
    change, names = FINISH_CASES[case]
    err = _refused("dcvc_prior_finish", _finish, dict(BASE, **change), names)
    if case == "intra_ldq_2_passes":
        assert b"qsrc" not in err, err


SYMBOL_BASE = dict(packed=_PTR, n_per_part=100, n_parts=2, out=_PTR, counts=_PTR, ws=_PTR)
SYMBOL_CASES = {"null_packed": (dict(packed=None), b"null"), "null_out": (dict(out=None), b"null"),
                "null_counts": (dict(counts=None), b"null"), "null_workspace": (dict(ws=None), b"null"),
                "no_parts": (dict(n_parts=0), b"0 x 100"), "nine_parts": (dict(n_parts=9), b"9 x 100"),
                "empty_parts": (dict(n_per_part=0), b"2 x 0")}


@pytest.mark.parametrize("case", list(SYMBOL_CASES))
@pytest.mark.parametrize("name", ["dcvc_compact_symbols", "dcvc_compact_symbols_dev"])
def test_bad_compact_symbols_arguments_are_refused_by_name(name, case):
    change, names = SYMBOL_CASES[case]
    _refused(name, _compact_symbols(name), dict(SYMBOL_BASE, **change), names)
