"""The placement helpers of tests/layer_utils.py (guarded operands for the layer kernels' GPU tests), checked on the CPU:
the view they build is what nn._geom and the library's source check accept, and the detector sees a single byte."""
import numpy as np
import pytest
import torch

from layer_utils import GuardedRun, VEC_GUARD, describe_touched, guarded, guarded_vec, touched, untouched

H, W, C, CP = 5, 7, 60, 64


def _values():
    return np.random.default_rng(3).standard_normal((H, W, C)).astype(np.float32)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_view_geometry_and_alignment(dtype):
    from opendcvc_amd import nn
    es = torch.empty((), dtype=dtype).element_size()
    vals = _values()
    view, raw = guarded(vals, CP, dtype, device="cpu")
    ld = CP + 32
    assert raw.dtype == torch.uint8 and raw.dim() == 1
    assert tuple(view.shape) == (H, W, CP) and view.stride() == (W * ld, ld, 1)
    assert nn._geom(view) == (H, W, CP, ld)
    assert view.data_ptr() % 16 == 0 and (ld * es) % 16 == 0
    # the minimum the contract allows, not more: 16 bytes in front of the channels
    band = 8 * W + 16
    assert view.data_ptr() - raw.data_ptr() == (band * ld + 16 // es) * es
    assert raw.numel() == (2 * band + H * W) * ld * es
    # values in the logical channels, exact zeros in the pad channels, NaN everywhere else
    assert torch.equal(view[..., :C], torch.from_numpy(vals).to(dtype)) and not bool(view[..., C:].any())
    everything = raw.view(dtype).view(-1, ld).clone()
    everything[band:band + H * W, 16 // es:16 // es + CP] = float("nan")
    assert bool(torch.isnan(everything).all())
    assert untouched(raw, view)
    # maps one pixel wide or high: the same strides, and the detector still finds its way
    for h, w in ((1, 1), (1, 9), (6, 1)):
        v, r = guarded(np.ones((h, w, C), np.float32), CP, dtype, device="cpu")
        assert v.stride() == (w * ld, ld, 1) and nn._geom(v) == (h, w, CP, ld) and untouched(r, v)
        assert torch.equal(v, r.view(dtype).view(-1, ld)[8 * w + 16:8 * w + 16 + h * w, 16 // es:16 // es + CP].unflatten(0, (h, w)))
        r[(8 * w + 16) * ld * es - 1] = 0
        assert touched(r, v).numel() == 1
    # a view of explicit geometry: a channel slice of a wider map
    view2, raw2 = guarded((H, W), CP, dtype, ld=3 * CP, chan_off=CP + 16 // es, band=3, device="cpu")
    assert view2.stride() == (W * 3 * CP, 3 * CP, 1) and view2.data_ptr() % 16 == 0
    assert bool(torch.isnan(view2).all()) and untouched(raw2, view2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_untouched_sees_a_single_byte(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    ld, band, off = CP + 32, 8 * W + 16, 16 // es
    row = ld * es
    first = (band * ld + off) * es                      # the view's first byte
    last = ((band + H * W - 1) * ld + off + CP) * es - 1  # and its last
    spots = {"in front of the map": first - row, "just in front of the map": first - 1, "behind the map": last + row,
             "just behind the map": last + 1, "the channel in front": first + 2 * row - 1,
             "the channel behind": first + 2 * row + CP * es, "the buffer's first byte": 0, "the buffer's last byte": -1}
    for name, at in spots.items():
        view, raw = guarded(_values(), CP, dtype, device="cpu")
        raw[at] = 0xFE                                   # one bit
        assert not untouched(raw, view), name
        assert touched(raw, view).tolist() == [at % raw.numel()], name
        assert "1 guard bytes" in describe_touched(raw, view)
    # writes inside the view are the kernel's business
    view, raw = guarded(_values(), CP, dtype, device="cpu")
    view.fill_(1.0)
    assert untouched(raw, view)
    # pixel and channel of a touched element as the report names them
    raw.view(dtype).view(-1, ld)[band - 2, off + CP] = 0.0
    assert "(-2, %d)" % CP in describe_touched(raw, view)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_refuses_what_breaks_the_16_byte_rule(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    with pytest.raises(ValueError):
        guarded(_values(), CP, dtype, ld=CP + 32 + 8 // es, device="cpu")      # a row stride of 8 bytes modulo 16
    with pytest.raises(ValueError):
        guarded(_values(), CP, dtype, chan_off=8 // es, device="cpu")         # an 8-byte channel offset
    with pytest.raises(ValueError):
        guarded(_values(), CP, dtype, ld=CP + 32, chan_off=32 + 16 // es, device="cpu")   # channels past the row
    with pytest.raises(ValueError):
        guarded(_values(), C - 28, dtype, device="cpu")                       # fewer physical than logical channels


def test_guarded_vec_holds_exactly_its_floats():
    q = np.random.default_rng(4).uniform(0.5, 1.5, 37).astype(np.float32)
    vec, raw = guarded_vec(q, device="cpu")
    assert vec.dtype == torch.float32 and vec.numel() == 37 and vec.data_ptr() % 16 == 0
    assert np.array_equal(vec.numpy(), q)
    f = raw.view(torch.float32)
    assert f.numel() == 37 + 2 * VEC_GUARD
    assert bool(torch.isnan(f[:VEC_GUARD]).all()) and bool(torch.isnan(f[VEC_GUARD + 37:]).all())


def test_guarded_run_check():
    """check() passes after a well-behaved 'kernel' and names each kind of misbehaviour"""
    def run(misbehave=None):
        g = GuardedRun(torch.float16, device="cpu")
        x0, x1 = g.src(_values(), CP), g.src(_values(), CP, second=True)
        assert x0.stride() != x1.stride() and x0.storage_offset() != x1.storage_offset()
        q = g.vec(np.ones(C, np.float32))
        out = g.out(H, W, CP, C)
        out[..., :C] = (x0 + x1)[..., :C] * q
        out[..., C:] = 0
        if misbehave:
            misbehave(x0, q, out, g)
        g.check()

    run()
    cases = {"non-finite": lambda x0, q, out, g: out[1, 2, 3].fill_(float("inf")),
             "pad channels": lambda x0, q, out, g: out[0, 0, C].fill_(1.0),
             "guard bytes": lambda x0, q, out, g: g.outputs[0][1][:2].zero_(),
             "x0: the call changed": lambda x0, q, out, g: x0[0, 0, 0].fill_(2.0),
             "vector: the call changed": lambda x0, q, out, g: q[5].fill_(2.0)}
    for msg, f in cases.items():
        with pytest.raises(AssertionError, match=msg):
            run(f)
    # an output left unwritten is a NaN
    g = GuardedRun(torch.float32, device="cpu")
    g.out(H, W, CP)
    with pytest.raises(AssertionError, match="non-finite"):
        g.check()
