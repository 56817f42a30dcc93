"""numpy restatement of csrc/dcvc_rate.hip (rate control's size estimate) and of the cost tables it reads, written from
the definition in include/dcvc_amd.h - not from the kernel - so that the two can be compared bit for bit: everything
after the fp64 logarithm of the table is integer arithmetic."""
import numpy as np

ONE = 65536          # one bit in Q16


def cost_rows(cdf, sizes, offsets):
    """-> (cost [n][max size - 1] int64, max_value [n], offset [n]): cost[t][v] = rint(65536 * (16 - log2(freq))) for the
    symbols v = 0 .. sizes[t] - 2 of table t, the last of them the escape symbol"""
    cdf, sizes, offsets = np.asarray(cdf, np.int64), np.asarray(sizes, np.int64), np.asarray(offsets, np.int64)
    cost = np.zeros((cdf.shape[0], int(sizes.max()) - 1), np.int64)
    for t in range(cdf.shape[0]):
        for v in range(int(sizes[t]) - 1):
            cost[t, v] = int(np.rint(65536.0 * (16.0 - np.log2(float(cdf[t, v + 1] - cdf[t, v])))))
    return cost, sizes - 2, offsets


def packed_table(cdf, sizes, offsets):
    """the uint32 rows the kernel is given: [meta, cost ...], meta = (max_value << 16) | (offset & 0xffff)"""
    cost, max_value, off = cost_rows(cdf, sizes, offsets)
    out = np.zeros((cost.shape[0], cost.shape[1] + 1), np.uint32)
    out[:, 0] = ((max_value << 16) | (off & 0xffff)).astype(np.uint32)
    out[:, 1:] = cost.astype(np.uint32)
    return out


def bypass_groups(value, max_value):
    """2-bit groups encode_symbol writes for a value outside [0, max_value): n_bypass / 3 + 1 for the count, n_bypass for
    the value (0 for a value inside)"""
    value, max_value = np.asarray(value, np.int64), np.asarray(max_value, np.int64)
    raw = np.where(value < 0, -2 * value - 1, 2 * (value - max_value))
    n_bypass = np.zeros(value.shape, np.int64)
    for k in range(16):
        n_bypass += (raw >> (2 * k)) != 0
    return np.where((value >= 0) & (value < max_value), 0, n_bypass // 3 + 1 + n_bypass)


def symbol_costs(sym, table, rows):
    """(Q16 cost, bypass groups) of the symbols `sym` (signed values) against the rows `table` of `rows` =
    cost_rows(...)"""
    cost, max_value, off = rows
    sym, table = np.asarray(sym, np.int64), np.asarray(table, np.int64)
    mv = max_value[table]
    value = sym - off[table]
    groups = bypass_groups(value, mv)
    inside = groups == 0
    c = cost[table, np.where(inside, value, mv)] + 2 * ONE * groups
    return c, groups


def estimate(packed, g_rows, z8, zhw, z_rows, z_start):
    """-> (the 3 * parts + 2 words of dcvc_rate_estimate, rANS steps): per part Q16 bits, kept symbols, escapes; z: Q16
    bits, escapes.  steps = coded symbols + bypass groups of the whole frame (what the error bound counts)."""
    packed = np.asarray(packed, np.int16)
    words, steps = [], 0
    for part in packed:
        cs = part.astype(np.int64)
        idx = cs & 0xff
        keep = idx < g_rows[0].shape[0]
        c, groups = symbol_costs(cs[keep] >> 8, idx[keep], g_rows)
        words += [int(c.sum()), int(keep.sum()), int((groups > 0).sum())]
        steps += int(keep.sum() + groups.sum())
    z = np.asarray(z8, np.int8).astype(np.int64)
    c, groups = symbol_costs(z, z_start + np.arange(z.size) // zhw, z_rows)
    words += [int(c.sum()), int((groups > 0).sum())]
    return words, steps + int(z.size + groups.sum())


def draw_symbols(rng, n, g_sizes, g_offsets, skip=0.3, far=0.01, tables=None):
    """n packed y symbols (sym << 8) | idx: table indexes over the whole group, values around the tables' centres with
    `far` of them far outside (-128, 127 and the table edges), `skip` of them the sentinel 0xFF"""
    idx = rng.integers(0, len(g_sizes), n) if tables is None else rng.choice(np.asarray(tables), n)
    centre = -np.asarray(g_offsets)[idx]
    spread = np.maximum(1, (np.asarray(g_sizes)[idx] - 2) // 4)
    sym = np.rint(rng.normal(0, 1, n) * spread).astype(np.int64)
    edge = rng.random(n) < far
    sym[edge] = rng.choice(np.array([-128, 127, -9, 9, -centre.max() - 1, 40, -40]), int(edge.sum()))
    sym = np.clip(sym, -128, 127)
    idx = np.where(rng.random(n) < skip, 0xFF, idx)
    return ((sym << 8) | idx).astype(np.uint16).view(np.int16)
