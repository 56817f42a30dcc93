"""Rate control's size estimate on the host: the numpy restatement (tests/rate_ref.py) of dcvc_rate_estimate against the
streams the host rANS coder writes, and the cost tables entropy.cost_table builds.

The bound of test_estimate_against_the_host_coder is derived in DESIGN.md ("Rate control"): byte-wise rANS with a 2^23
lower bound and 16-bit probabilities keeps x / freq >= 128, so one step gains or loses at most log2(1 + 2^-7) < 0.0113
bits against the cost table; a coder's 32-bit flush holds up to 8 bits of slack."""
import numpy as np
import pytest
import torch

import rate_ref as R
from opendcvc_amd import entropy, weights

PER_STEP, PER_CODER = 0.0113, 40


@pytest.fixture(scope="module")
def model():
    """a DMC with the seeded synthetic weights on the CPU: the real Gaussian and factorised tables and their coder"""
    from opendcvc_amd.models import DMC
    m = DMC()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict("dmc", 1234).items()})
    m.update(0.12)
    return m


@pytest.fixture(scope="module")
def rows(model):
    ec = model.entropy_coder
    return R.cost_rows(*ec.tables[model._g_group]), R.cost_rows(*ec.tables[model._z_group])


def _frame(model, seed, parts, nsym, zhw, **kw):
    rng = np.random.default_rng(seed)
    _, g_sizes, g_offsets = model.entropy_coder.tables[model._g_group]
    packed = np.stack([R.draw_symbols(rng, nsym, g_sizes, g_offsets, **kw) for _ in range(parts)])
    z = np.clip(np.rint(rng.normal(0, 3, model.z_channel * zhw)), -128, 127).astype(np.int8)
    z[rng.integers(0, z.size, max(2, z.size // 50))] = rng.choice(np.array([-128, 127, -30, 30], np.int8), max(2, z.size // 50))
    return packed, z


def _stream(model, packed, z, qp, zhw, two):
    ec = model.entropy_coder
    ec.set_use_two_entropy_coders(two)
    ec.reset()
    ec.encode_z(z, model._z_group, qp * model.z_channel, zhw)
    for part in packed:
        ec.encode_y(part, model._g_group)
    ec.flush()
    out = ec.get_encoded_stream()
    ec.set_use_two_entropy_coders(False)
    return out


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("parts,nsym,zhw,qp,kw", [
    (2, 128 * 9 * 13, 6, 0, {}), (4, 64 * 9 * 13, 6, 63, {}), (2, 2048, 1, 71, dict(far=0.2)),
    (2, 128, 1, 32, dict(skip=0.9)), (4, 128 * 35, 35, 40, dict(far=0.0, skip=0.0)), (2, 128 * 68 * 120 // 16, 35, 21, {})])
def test_estimate_against_the_host_coder(model, rows, parts, nsym, zhw, qp, kw, two):
    packed, z = _frame(model, 1000 * parts + nsym % 997 + qp, parts, nsym, zhw, **kw)
    words, steps = R.estimate(packed, rows[0], z, zhw, rows[1], qp * model.z_channel)
    coders = 2 if two else 1
    est_bits = (sum(words[0:3 * parts:3]) + words[3 * parts]) / R.ONE + 32 * coders
    got_bits = 8 * len(_stream(model, packed, z, qp, zhw, two))
    bound = PER_STEP * steps + PER_CODER * coders
    print(f"parts {parts} nsym {nsym} qp {qp} two {two}: stream {got_bits} bits, estimate {est_bits:.1f}, steps {steps}, "
          f"difference {got_bits - est_bits:+.1f} of {bound:.1f} ({(got_bits - est_bits) / steps:+.5f} per step)")
    assert sum(words[2:3 * parts:3]) + words[-1] > 0 or kw.get("far") == 0.0       # (escapes are part of the case)
    assert abs(got_bits - est_bits) <= bound


def test_sentinels_cost_nothing_and_far_values_are_escapes(model, rows):
    _, g_sizes, g_offsets = model.entropy_coder.tables[model._g_group]
    packed = np.full((2, 128), 0x00FF, np.int16)
    packed[1, :4] = np.array([(-128 << 8) | 5, (127 << 8) | 5, (0 << 8) | 5, (3 << 8) | 0xFF], np.int64).astype(np.uint16).view(np.int16)
    z = np.zeros(model.z_channel, np.int8)
    words, _ = R.estimate(packed, rows[0], z, 1, rows[1], 0)
    assert words[0:3] == [0, 0, 0] and words[4:6] == [3, 2]
    cost, max_value, off = rows[0]
    mv, o = int(max_value[5]), int(off[5])
    want = int(cost[5, 0 - o]) + sum(int(cost[5, mv]) + 2 * R.ONE * int(R.bypass_groups(v - o, mv)) for v in (-128, 127))
    assert words[3] == want


# ---------------------------------------------------------------------------------- the cost table
def test_cost_table_of_a_hand_made_table():
    """three symbols 0, 1 and the escape with frequencies 2^15, 2^14, 2^14: exactly 1, 2 and 2 bits"""
    cdf = np.array([[0, 1 << 15, 3 << 14, 1 << 16, 0]], np.int32)
    t = entropy.cost_table(cdf, np.array([4], np.int32), np.array([-1], np.int32))
    assert t.dtype == np.uint32 and t.shape == (1, 4)
    assert int(t[0, 0]) == (2 << 16) | 0xffff                       # max_value 2, offset -1
    assert [int(v) for v in t[0, 1:]] == [1 << 16, 2 << 16, 2 << 16]
    assert np.array_equal(t, R.packed_table(cdf, [4], [-1]))
    # a frequency that is no power of two: rint of the fp64 value
    cdf = np.array([[0, 3, 65535, 65536]], np.int32)
    t = entropy.cost_table(cdf, np.array([4], np.int32), np.array([0], np.int32))
    assert [int(v) for v in t[0, 1:]] == [int(np.rint(65536 * (16 - np.log2(f)))) for f in (3, 65532, 1)]
    assert int(t[0, 3]) == 16 << 16


@pytest.mark.parametrize("n_bypass,value", [(1, 3), (3, 2 + 8), (3, -20), (4, 2 + 64), (4, -100), (7, 2 + 2048), (7, -8000)])
def test_escape_costs_what_the_formula_says(n_bypass, value):
    """max_value 2: raw = 2 * (value - 2) above the table, -2 * value - 1 below it; n_bypass 2-bit groups hold raw"""
    cdf = np.array([[0, 1 << 15, 3 << 14, 1 << 16]], np.int32)
    rows = R.cost_rows(cdf, [4], [0])
    raw = 2 * (value - 2) if value >= 0 else -2 * value - 1
    assert raw >> (2 * (n_bypass - 1)) and not raw >> (2 * n_bypass)
    c, groups = R.symbol_costs([value], [0], rows)
    assert int(groups[0]) == n_bypass // 3 + 1 + n_bypass
    assert int(c[0]) == (2 << 16) + 2 * 65536 * (n_bypass // 3 + 1 + n_bypass)


def test_real_tables_match_the_restatement(model):
    ec = model.entropy_coder
    for group in (model._g_group, model._z_group):
        cdf, sizes, offsets = ec.tables[group]
        sel = slice(None) if group == model._g_group else slice(0, None, 37)
        got, want = entropy.cost_table(cdf, sizes, offsets)[sel], R.packed_table(cdf[sel], sizes[sel], offsets[sel])
        assert np.array_equal(got[:, :want.shape[1]], want) and not got[:, want.shape[1]:].any()
