"""The decoder-state digest (csrc/dcvc_digest.hip, opendcvc_amd/digest.py, docs/state_digest.md) as far as a GPU-less host
can check it: the numpy restatement the GPU tests compare with gives the known answers and has the properties the format
promises, the entry is declared, bound and exported, and its argument errors come back without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from digest_ref import digest_ref
from opendcvc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [(bytes(8), 0xa7a4bb74443478eb),
         (bytes(range(64)), 0x5cf4ad0198dc94f8),
         (np.arange(4096, dtype=np.float16).tobytes(), 0x2ef1d9a44bde0829),
         (np.random.Generator(np.random.PCG64(1)).standard_normal(768).astype(np.float32).tobytes(), 0xba87ef52d843693d)]


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_restatement_gives_the_known_answers(case):
    data, want = KNOWN[case]
    assert digest_ref(data) == want


def test_restatement_equals_the_definition_in_python_integers():
    """the definition once more without numpy: Python integers reduced mod 2^64 by hand"""
    M, G = 2 ** 64 - 1, 0x9E3779B97F4A7C15

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    data = np.random.default_rng(5).integers(0, 256, 8 * 37, dtype=np.uint8).tobytes()
    words = [int.from_bytes(data[8 * j:8 * j + 8], "little") for j in range(37)]
    want = (sum(mix((w + (j + 1) * G) & M) for j, w in enumerate(words)) + mix((len(data) * G) & M)) & M
    assert digest_ref(data) == want


def test_every_single_bit_flip_changes_the_digest():
    data = bytes(range(64))
    base = digest_ref(data)
    seen = set()
    for bit in range(512):
        d = bytearray(data)
        d[bit >> 3] ^= 1 << (bit & 7)
        seen.add(digest_ref(bytes(d)))
        assert digest_ref(bytes(d)) != base, bit
    assert len(seen) == 512


def test_swapping_two_unequal_words_changes_the_digest():
    w = np.random.default_rng(2).integers(0, 2 ** 63, 16, dtype=np.uint64)
    base = digest_ref(w.tobytes())
    for a in range(16):
        for b in range(a + 1, 16):
            s = w.copy()
            s[a], s[b] = w[b], w[a]
            assert digest_ref(s.tobytes()) != base, (a, b)
    assert digest_ref(bytes(8)) != digest_ref(bytes(16))          # (the length counts)


def test_restatement_refuses_what_the_kernel_refuses():
    for bad in (b"", bytes(7), bytes(12)):
        with pytest.raises(ValueError):
            digest_ref(bad)


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "dcvc_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "libdcvc_amd.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dcvc_state_digest", "dcvc_state_digest_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in dcvc_amd.h"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+DCVC_DIGEST_PASS_WORDS\s+%d\b" % _lib.DIGEST_PASS_WORDS, header)
    assert issubclass(_lib.DigestMismatch, _lib.DcvcError)
    e = _lib.DigestMismatch(3, False, 0x12, 0x34)
    assert (e.index, e.is_i, e.expected, e.got) == (3, False, 0x12, 0x34)
    assert "frame 3" in str(e) and "P" in str(e) and "0x0000000000000012" in str(e) and "0x0000000000000034" in str(e)


# a 64-byte-aligned host buffer stands in for every pointer: each call below must be refused before anything is launched
_BUF = ctypes.create_string_buffer(4096 + 64)
_PTR = (ctypes.addressof(_BUF) + 63) & ~63


def _digest(data=_PTR, nbytes=64, ws=_PTR + 1024, out=_PTR + 2048):
    return _lib.lib().dcvc_state_digest(data, nbytes, ws, 0, 0, out, None)


def test_argument_checks_come_before_any_device_call():
    """what the bad-argument cases below rely on, read off the source: inside dcvc_state_digest every DCVC_REQUIRE stands
    in front of the first hip* call and the first launch"""
    src = open(os.path.join(REPO, "opendcvc_amd", "csrc", "dcvc_digest.hip")).read()
    body = src[src.index("int dcvc_state_digest("):]
    first_device = min(body.index("hipHostGetDevicePointer"), body.index("hipLaunchKernelGGL"))
    assert body.count("DCVC_REQUIRE") >= 3 and body.rindex("DCVC_REQUIRE") < first_device


@pytest.mark.parametrize("bad", [dict(nbytes=0), dict(nbytes=-8), dict(nbytes=7), dict(nbytes=12), dict(nbytes=2 ** 33 + 4),
                                 dict(data=_PTR + 4), dict(data=_PTR + 1), dict(data=_PTR + 12),
                                 dict(data=None), dict(ws=None), dict(out=None), dict(ws=_PTR + 1028), dict(out=_PTR + 2052)])
def test_argument_errors_need_no_device(bad):
    assert _digest(**bad) == -1, bad
    assert b"dcvc_state_digest" in _lib.lib().dcvc_last_error()


def test_workspace_size():
    L = _lib.lib()
    for bad in (0, -8, 7, 12):
        assert L.dcvc_state_digest_ws_bytes(bad) == -1, bad
    sizes = [L.dcvc_state_digest_ws_bytes(8 * m) for m in (1, 2, 511, 512, 513, 4096, _lib.DIGEST_PASS_WORDS,
                                                           _lib.DIGEST_PASS_WORDS + 1, 50 * _lib.DIGEST_PASS_WORDS)]
    assert all(s >= 8 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] == sizes[-3] == 8 * _lib.DIGEST_PASS_WORDS // 512        # the full grid: 2 words per thread, 256 threads


def test_the_harness_takes_the_switch_on_both_paths(monkeypatch):
    """--digest reaches run_one_point from the command line of one file and through a manifest job's options"""
    import inspect
    from opendcvc_amd import harness
    from opendcvc_amd.pipeline import SequenceDecoder, SequenceEncoder
    assert inspect.signature(harness.run_one_point).parameters["digest"].default is False
    assert inspect.signature(SequenceEncoder.__init__).parameters["digest"].default is False
    assert "digest" not in inspect.signature(SequenceDecoder.__init__).parameters          # the decoder needs no switch
    ap = harness.build_parser()
    base = "--test-config cfg.json --gpus 1 --gpu-ids 0"
    for argv, want in ((base, False), (base + " --digest", True), (base + " --digest 1", True), (base + " --digest 0", False)):
        opts, _ = harness.manifest_options(ap.parse_args(argv.split()), ap)
        assert opts["digest"] is want, argv
    calls = []
    monkeypatch.setattr(harness, "run_one_point", lambda *a, **kw: calls.append(kw) or {"i_frame_num": 1, "p_frame_num": 1})
    job = dict(src_path="x.yuv", src_width=64, src_height=64, frame_num=2, qp_i=32, qp_p=32, intra_period=-1, reset_interval=32)
    harness.run_job(("i", "p"), job, dict(digest=True))
    harness.run_job(("i", "p"), job, {})
    assert [c["digest"] for c in calls] == [True, False]
