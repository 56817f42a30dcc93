"""Rate control's size estimate on the device: dcvc_rate_estimate against its numpy restatement (tests/rate_ref.py) word
for word, and compress()['est_bytes'] against the length of the stream the frame then gets, for every form of payload."""
import ctypes

import numpy as np
import pytest
import torch

import rate_ref as R
from opendcvc_amd import entropy, weights

pytestmark = pytest.mark.gpu

PER_STEP, PER_CODER = 0.0113, 40          # the bound of tests/test_rate_host.py (DESIGN.md "Rate control")
MAX_GROUPS = 7                            # bypass groups of an escape: raw < 2^10 for int8 values, n_bypass <= 5, 5 / 3 + 1 + 5


# ---------------------------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def tables():
    """the real tables of a DMC with the seeded synthetic weights: restatement rows and the kernel's device rows"""
    from opendcvc_amd.models import DMC
    m = DMC()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict("dmc", 1234).items()})
    m.update(0.12)
    g, z = (m.entropy_coder.tables[k] for k in (m._g_group, m._z_group))
    dev = [torch.from_numpy(entropy.cost_table(*t).view(np.int32)).cuda() for t in (g, z)]
    return dict(g=g, z=z, g_rows=R.cost_rows(*g), z_rows=R.cost_rows(*z), g_dev=dev[0], z_dev=dev[1], zc=m.z_channel)


def _estimate(t, packed, z, zhw, qp, check=True):
    from opendcvc_amd import _lib
    from opendcvc_amd import nn as L
    from opendcvc_amd.entropy import PinnedBuffer
    lib = _lib.lib()
    parts, nsym = packed.shape
    pinned = PinnedBuffer(8 * (3 * parts + 2))
    words = pinned.view(np.uint64, 3 * parts + 2)
    words[:] = 99
    need = lib.dcvc_rate_estimate_ws_bytes(nsym, parts, z.size)
    ws = torch.empty(max(int(need), 4096), dtype=torch.uint8, device="cuda")
    dp, dz = torch.from_numpy(packed).cuda(), torch.from_numpy(z).cuda()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.dcvc_rate_estimate(L._p(dp), nsym, parts, L._p(t["g_dev"]), t["g_dev"].shape[0], t["g_dev"].shape[1], L._p(dz),
                                z.size, zhw, L._p(t["z_dev"]), t["z_dev"].shape[0], t["z_dev"].shape[1], qp * t["zc"], L._p(ws),
                                ctypes.c_void_p(pinned.ptr), st)
    if check:
        _lib.check(rc, "dcvc_rate_estimate")
    _lib.check(lib.dcvc_stream_sync(st), "dcvc_stream_sync")
    return rc, [int(v) for v in words]


def _parts(t, rng, kinds, nsym):
    """one part per kind: 'mixed' (tables over the whole group, 30 % sentinels, 1 % far values), 'sentinel' (nothing kept),
    'escape' (every value outside its table: -128, 127 and the first value past each edge)"""
    _, sizes, offsets = t["g"]
    out = []
    for kind in kinds:
        if kind == "mixed":
            out.append(R.draw_symbols(rng, nsym, sizes, offsets))
        elif kind == "sentinel":
            out.append(((rng.integers(-128, 128, nsym) << 8) | 0xFF).astype(np.uint16).view(np.int16))
        else:
            idx = rng.integers(0, len(sizes), nsym)
            lo, hi = offsets[idx] - 1, offsets[idx] + sizes[idx] - 2
            sym = np.choose(rng.integers(0, 4, nsym), [np.full(nsym, -128), np.full(nsym, 127), lo, hi])
            out.append(((sym.astype(np.int64) << 8) | idx).astype(np.uint16).view(np.int16))
    return np.stack(out)


def _z(rng, n):
    z = np.clip(np.rint(rng.normal(0, 3, n)), -128, 127).astype(np.int8)
    z[rng.integers(0, n, max(2, n // 40))] = rng.choice(np.array([-128, 127, -30, 30], np.int8), max(2, n // 40))
    return z


# nsym: one 16-byte access per 16 lanes; one workgroup; 128 * 9 * 13 = 14976 (30 workgroups per part, a tail) and the
# intra model's 64 * 9 * 13; 1080p's 128 * 68 * 120 per part (the 128-workgroup cap, four accesses per thread)
@pytest.mark.parametrize("nsym", [128, 2048, 128 * 9 * 13, 64 * 9 * 13, 128 * 68 * 120])
@pytest.mark.parametrize("kinds", [("mixed", "mixed"), ("sentinel", "mixed", "escape", "mixed"), ("escape", "sentinel")])
def test_kernel_equals_the_restatement_word_for_word(tables, nsym, kinds):
    rng = np.random.default_rng(nsym + len(kinds))
    packed = _parts(tables, rng, kinds, nsym)
    zhw, qp = ((1, 0), (6, 63), (35, 71))[len(kinds) % 3]
    z = _z(rng, tables["zc"] * zhw)
    want, _ = R.estimate(packed, tables["g_rows"], z, zhw, tables["z_rows"], qp * tables["zc"])
    _, got = _estimate(tables, packed, z, zhw, qp)
    assert got == want
    for p, kind in enumerate(kinds):
        kept, esc = got[3 * p + 1], got[3 * p + 2]
        assert (kind != "sentinel" or (got[3 * p], kept, esc) == (0, 0, 0)) and (kind != "escape" or kept == esc == nsym)
    _, again = _estimate(tables, packed, z, zhw, qp)
    assert again == got


@pytest.mark.parametrize("zhw", [1, 6, 35])
@pytest.mark.parametrize("qp", [0, 63, 71])
def test_z_against_every_qp_row(tables, zhw, qp):
    rng = np.random.default_rng(100 * zhw + qp)
    packed = _parts(tables, rng, ("mixed", "sentinel"), 128)
    z = _z(rng, tables["zc"] * zhw)
    want, _ = R.estimate(packed, tables["g_rows"], z, zhw, tables["z_rows"], qp * tables["zc"])
    assert _estimate(tables, packed, z, zhw, qp)[1] == want and want[-1] > 0
    # a z that is no multiple of 16 bytes long, from a base that is not 16-byte aligned: the byte path
    odd = z[1:tables["zc"] * zhw - 2] if zhw > 1 else z[1:14]
    hw = zhw if zhw > 1 else 1
    want, _ = R.estimate(packed, tables["g_rows"], odd, hw, tables["z_rows"], qp * tables["zc"])
    from opendcvc_amd import _lib
    from opendcvc_amd import nn as L
    from opendcvc_amd.entropy import PinnedBuffer
    lib = _lib.lib()
    pinned = PinnedBuffer(64)
    dz, dp = torch.from_numpy(z).cuda(), torch.from_numpy(packed).cuda()
    ws = torch.empty(int(lib.dcvc_rate_estimate_ws_bytes(128, 2, odd.size)), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.dcvc_rate_estimate(L._p(dp), 128, 2, L._p(tables["g_dev"]), tables["g_dev"].shape[0], tables["g_dev"].shape[1],
                                      ctypes.c_void_p(dz.data_ptr() + 1), odd.size, hw, L._p(tables["z_dev"]),
                                      tables["z_dev"].shape[0], tables["z_dev"].shape[1], qp * tables["zc"], L._p(ws),
                                      ctypes.c_void_p(pinned.ptr), st), "dcvc_rate_estimate")
    _lib.check(lib.dcvc_stream_sync(st), "dcvc_stream_sync")
    assert [int(v) for v in pinned.view(np.uint64, 8)] == want


def test_bad_arguments_launch_nothing(tables):
    from opendcvc_amd import _lib
    lib = _lib.lib()
    assert lib.dcvc_rate_estimate_ws_bytes(100, 2, 128) < 0 and lib.dcvc_rate_estimate_ws_bytes(128, 0, 128) < 0
    assert lib.dcvc_rate_estimate_ws_bytes(128, 2, 0) < 0 and lib.dcvc_rate_estimate_ws_bytes(128, 2, 128) > 0
    rng = np.random.default_rng(5)
    packed, z = _parts(tables, rng, ("mixed", "mixed"), 128), _z(rng, tables["zc"])
    rc, words = _estimate(tables, packed, z, 1, 72, check=False)           # one qp row past the z tables
    assert rc < 0 and words == [99] * 8
    rc, words = _estimate(tables, packed, z, 0, 0, check=False)
    assert rc < 0 and words == [99] * 8


# ---------------------------------------------------------------------------------- compress()['est_bytes']
def _codecs(dtype):
    from opendcvc_amd.models import DMC, DMCI
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(name, 1234, q_ramp=True).items()})
        m.to("cuda").eval()
        m.update(0.12)
        if dtype == torch.float16:
            m.half()
        m.set_use_two_entropy_coders(False)
        nets.append(m)
    return nets


@pytest.fixture(scope="module")
def codecs():
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = _codecs(dtype)
        return cache[dtype]
    return get


def _sequence(i_net, p_net, frames, qp, chunked, monkeypatch, two=False):
    """I + P ... as pipeline.SequenceEncoder codes them (the offsets of INDEX_MAP on top of qp) -> per frame
    (est_bytes, payload, the job of the hand-off)"""
    from opendcvc_amd import handoff
    from opendcvc_amd.pipeline import INDEX_MAP
    jobs = []
    stage = handoff.stage

    def keep(*a, **kw):
        jobs.append(stage(*a, **kw))
        return jobs[-1]
    monkeypatch.setattr(handoff, "stage", keep)
    out = []
    p_net.set_curr_poc(0)
    for m in (i_net, p_net):
        m.rate_estimate = True
        m.set_use_two_entropy_coders(two)
    try:
        for g, x in enumerate(frames):
            if g == 0:
                enc = i_net.compress(x, qp, chunked=chunked)
                p_net.clear_dpb()
                p_net.add_ref_frame(None, enc["x_hat"])
            else:
                enc = p_net.compress(x, p_net.shift_qp(qp, INDEX_MAP[g % 8]), chunked=chunked)
            out.append((enc["est_bytes"], enc["bit_stream"], jobs[-1]))
    finally:
        for m in (i_net, p_net):
            m.rate_estimate = False
            m.set_use_two_entropy_coders(False)
    return out


def _bound_bits(job, payload):
    """the bound of tests/test_rate_host.py on 8 * |len(payload) - est_bytes|: 0.0113 bits per rANS step (an escape is
    at most 1 + MAX_GROUPS steps) and 40 per coder, plus what estimated_bytes adds on top of the bits - one rounding up to
    a byte per rounded part, and the varint of a part's size where that size lies within the bound of a varint step"""
    from opendcvc_amd import handoff
    ybits, (_, zesc) = handoff.estimate_words(job)
    kept = [k for _, k, _ in ybits]
    steps = sum(kept) + job.nz + MAX_GROUPS * (sum(e for _, _, e in ybits) + zesc)
    bound = PER_STEP * steps + PER_CODER * handoff.coders_of(job, kept)
    if job.form == handoff.REFERENCE:
        return bound + 8
    _, z_part, spans = entropy.parse_chunked_payload(payload, job.parts)
    sizes = [len(z_part)] + [s for _, s in spans]
    near = sum(1 for s in sizes for edge in (1 << 7, 1 << 14) if abs(s - edge) <= bound / 8 + 1)
    return bound + 8 * len(sizes) + 16 * near


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("h,w", [(64, 64), (144, 208)])          # (136 x 200 padded to the model's multiple of 16)
@pytest.mark.parametrize("qp", [0, 32, 63])
def test_estimate_against_the_reference_stream(codecs, monkeypatch, dtype, h, w, qp):
    i_net, p_net = codecs(dtype)
    frames = [torch.from_numpy(weights.synthetic_frame_yuv444(h, w, i, 5)).cuda() for i in range(8)]
    for two in ((False, True) if (h, qp) == (144, 32) else (False,)):
        for fi, (est, payload, job) in enumerate(_sequence(i_net, p_net, frames, qp, False, monkeypatch, two)):
            bound = _bound_bits(job, payload)
            print(f"{h}x{w} qp {qp} two {two} frame {fi}: {len(payload)} bytes, estimate {est}, bound {bound / 8:.1f} bytes")
            assert isinstance(est, int) and abs(8 * (len(payload) - est)) <= bound, (fi, two)
            assert job.qp == (qp if fi == 0 else p_net.shift_qp(qp, (0, 1, 0, 2, 0, 2, 0, 2)[fi]))


@pytest.mark.parametrize("entropy_mode", ["host", "device"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_estimate_against_the_chunked_payloads(codecs, monkeypatch, dtype, entropy_mode):
    from opendcvc_amd import handoff
    i_net, p_net = codecs(dtype)
    frames = [torch.from_numpy(weights.synthetic_frame_yuv444(144, 208, i, 5)).cuda() for i in range(8)]
    for m in (i_net, p_net):
        m.entropy = entropy_mode
    try:
        for qp in (0, 32, 63):
            for fi, (est, payload, job) in enumerate(_sequence(i_net, p_net, frames, qp, True, monkeypatch)):
                assert job.form == (handoff.CHUNKED_DEVICE if entropy_mode == "device" else handoff.CHUNKED_HOST)
                bound = _bound_bits(job, payload)
                print(f"{entropy_mode} qp {qp} frame {fi}: {len(payload)} bytes, estimate {est}, bound {bound / 8:.1f} bytes")
                assert abs(8 * (len(payload) - est)) <= bound, (qp, fi)
    finally:
        for m in (i_net, p_net):
            m.entropy = "host"


def test_without_the_attribute_nothing_is_added(codecs):
    i_net, p_net = codecs(torch.float32)
    x = torch.from_numpy(weights.synthetic_frame_yuv444(64, 64, 0, 5)).cuda()
    assert i_net.rate_estimate is False and p_net.rate_estimate is False
    enc = i_net.compress(x, 32)
    assert sorted(enc) == ["bit_stream", "x_hat"]
    p_net.set_curr_poc(0)
    p_net.clear_dpb()
    p_net.add_ref_frame(None, enc["x_hat"])
    assert sorted(p_net.compress(x, 32)) == ["bit_stream"]
