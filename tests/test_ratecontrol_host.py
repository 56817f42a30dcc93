"""ratecontrol.RateController against a synthetic plant, bits = A_class * exp(b * qp) * (1 + ripple), and the harness's
rate-control options: no GPU.

The sequences are 32 windows long: from 24 qp steps above the answer at b = 0.1 the first frames cost up to eleven times
the target each (the I frame several times that), and a debt is repaid at no more than (1 - T_FLOOR) = 0.75 targets per
frame, so the transient alone may take a hundred frames; the last four windows are what is measured."""
import math

import pytest

from opendcvc_amd.pipeline import INDEX_MAP
from opendcvc_amd.ratecontrol import I_CLASS, RateController

TARGET = 10000.0
A_CLASS = {I_CLASS: 6.0, 0: 1.0, 1: 1.25, 2: 1.12}         # an I frame costs six offset-0 P frames at the same qp
CYCLE_MEAN = sum(A_CLASS[c] for c in INDEX_MAP) / len(INDEX_MAP)
W = RateController(TARGET, 32).window                       # the documented default


def _ripple(f):
    return 0.05 * math.sin(0.9 * f) + 0.03 * math.cos(2.3 * f)


def _run(b, qp_answer, frames, double_at=None, **kw):
    """the plant is scaled so that the P-frame cycle costs TARGET per frame at base qp `qp_answer`"""
    scale = TARGET * math.exp(-b * qp_answer) / CYCLE_MEAN
    rc = RateController(TARGET, **kw)
    qps, bits, debt = [], [], []
    for f in range(frames):
        base = rc.base_qp()
        klass = I_CLASS if f == 0 else INDEX_MAP[f % 8]
        a = scale * A_CLASS[klass] * (2.0 if double_at is not None and f >= double_at else 1.0)
        bits.append(a * math.exp(b * base) * (1.0 + _ripple(f)))
        rc.observe(klass, base, bits[-1])
        qps.append(base)
        debt.append(rc.debt)
    return rc, qps, bits, debt


@pytest.mark.parametrize("b", [0.02, 0.05, 0.1])
@pytest.mark.parametrize("qp_answer,qp_init", [(40, 16), (16, 40)])
def test_converges_from_24_steps_away(b, qp_answer, qp_init):
    rc, qps, bits, _ = _run(b, qp_answer, 32 * W, qp_init=qp_init)
    assert rc.window == W == 6
    tail = bits[-4 * rc.window:]
    err = sum(tail) / len(tail) / TARGET - 1.0
    print(f"b {b} from {qp_init} to {qp_answer}: mean of the last {len(tail)} frames {err:+.4f} of the target "
          f"(bound {math.exp(b) - 1:.4f}), learned b {rc.b:.4f}, qp {qps[:6]} ... {qps[-8:]}")
    assert abs(err) <= math.exp(b) - 1.0
    assert all(0 <= q <= 63 for q in qps)


@pytest.mark.parametrize("b", [0.02, 0.05, 0.1])
def test_qp_stays_inside_its_range(b):
    # the answer (qp 40 / qp 5) lies outside [20, 30]
    for answer in (40, 5):
        _, qps, _, _ = _run(b, answer, 96, qp_init=25, qp_min=20, qp_max=30)
        assert all(20 <= q <= 30 for q in qps) and qps[-1] == (30 if answer == 40 else 20)
    assert RateController(TARGET, qp_init=70, qp_max=63).base_qp() == 63
    with pytest.raises(ValueError):
        RateController(TARGET, 32, qp_min=40, qp_max=30)


@pytest.mark.parametrize("b", [0.02, 0.1])
def test_a_single_allowed_qp_gives_a_constant_trace(b):
    rc, qps, _, _ = _run(b, 40, 64, qp_init=27, qp_min=27, qp_max=27, qp_i_init=20)
    assert qps == [27] * 64 and rc.i_qp(27) == 20


@pytest.mark.parametrize("b", [0.02, 0.05, 0.1])
def test_debt_is_repaid_after_the_content_doubles(b):
    at, w = 20 * W, W
    rc, qps, _, debt = _run(b, 50, at + 4 * W, double_at=at, qp_init=50)
    print(f"b {b}: debt / target before {debt[at - 1] / TARGET:+.2f}, peak {max(debt[at:]) / TARGET:+.2f}, "
          f"after 2 windows {debt[at + 2 * w] / TARGET:+.2f}, qp {qps[at - 2:at + 10]}")
    assert abs(debt[at - 1]) <= TARGET
    assert max(debt[at:at + 4]) > TARGET                   # (the change did cost more than a frame)
    assert all(abs(d) <= TARGET for d in debt[at + 2 * w:])


def test_the_same_inputs_give_the_same_trace():
    a, b = _run(0.05, 40, 128, double_at=60, qp_init=16), _run(0.05, 40, 128, double_at=60, qp_init=16)
    assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3] and a[0].b == b[0].b


def test_exact_sizes_are_recorded_and_never_fed_back():
    a, _, _, _ = _run(0.05, 40, 32, qp_init=16)
    b = RateController(TARGET, qp_init=16)
    for f in range(32):
        base = b.base_qp()
        b.record_exact(f, 10 ** 6)                         # absurd exact sizes, arriving at any time
        klass = I_CLASS if f == 0 else INDEX_MAP[f % 8]
        scale = TARGET * math.exp(-0.05 * 40) / CYCLE_MEAN
        b.observe(klass, base, scale * A_CLASS[klass] * math.exp(0.05 * base) * (1.0 + _ripple(f)))
    assert b.debt == a.debt and b.base == a.base and len(b.exact_bytes) == 32 and not a.exact_bytes


def test_command_line_options():
    from opendcvc_amd import harness
    ap = harness.build_parser()
    base = ["--src", "x.yuv", "--width", "1920", "--height", "1080", "--frames", "2"]
    a = ap.parse_args(base + ["--target-kbps", "6220.8", "--fps", "30", "--qp-i", "20", "40"])
    harness.check_rate_options(a, ap)
    assert (a.qp_i, a.qp_p, a.rate_num) == ([20], [20], 1)
    assert abs(harness.target_bpp(vars(a), 1920, 1080) - 0.1) < 1e-12
    a = ap.parse_args(base + ["--target-bpp", "0.25"])
    harness.check_rate_options(a, ap)
    assert harness.target_bpp(vars(a), 64, 64) == 0.25 and a.qp_i == [32]
    opts, _ = harness.manifest_options(ap.parse_args(["--test-config", "m.json", "--target-bpp", "0.25", "--gpus", "1"]), ap)
    assert opts["target_bpp"] == 0.25 and opts["target_kbps"] is None
    a = ap.parse_args(base)
    harness.check_rate_options(a, ap)
    assert harness.target_bpp(vars(a), 64, 64) is None and a.qp_i is None
    for bad in (["--target-kbps", "100"], ["--target-bpp", "0.1", "--target-kbps", "100", "--fps", "30"], ["--target-bpp", "0"]):
        with pytest.raises(SystemExit):
            harness.check_rate_options(ap.parse_args(base + bad), ap)
