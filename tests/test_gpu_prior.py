"""The entropy-model glue kernels (dcvc_prior.hip: the checkerboard prior steps, the decoder's index build and restore, the
compacted decoder hand-off, finish; dcvc_elem.hip: the z quantiser) called through the C ABI and compared BIT FOR BIT with the CPU
restatement tests/prior_ref.py, in fp32 and in fp16.  The arithmetic is elementwise and the restatement rounds where the
kernels store, so no tolerance is needed in either storage type.

Every tensor has its own leading dimension (two swapped stride arguments fail), scales / means are channel slices of one
params buffer as the codecs pass them (DMC: [q_dec | scales | means]; DMCI: [2 raw q | scales | means]), y_hat is updated
in place inside guard channels, and every output is pre-filled with a sentinel that must survive outside what the kernel
owns.  Values mix random draws with the edges where a symbol changes: y - mean on .5 ties, past +-128 and at +-1e4,
-0.0, scales at 0 / negative / on 0.11 and 16 and their neighbours / on force_zero_thres / on every scale_to_index bin
edge, q_dec below, on and above 0.5, raw intra q at +-20."""
import ctypes

import numpy as np
import pytest
import torch

import dcvc_oracle as O
import prior_ref as R
from opendcvc_amd import arch

pytestmark = pytest.mark.gpu

GUARD_Y = -77.0          # guard channels of y_hat
GUARD_PACKED = 0x7E7E    # behind the packed symbols
GUARD_IDX = 0xA5         # behind the index array / inside the pinned buffers
DTYPES = {"f32": (torch.float32, np.float32), "f16": (torch.float16, np.float16)}
TIES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 127.5, -127.5, 128.5, -128.5, 1e4, -1e4, 0.0, 3.0, -7.0]
DYADIC_MEANS = [0.0, 0.25, -0.5, 1.75, -3.0]
THRES_LIST = (-1.0, 0.0, 0.05, 0.12, 100.0)

CG_DMC, CG_DMCI = arch.DMC_CH_Y // 2, arch.DMCI_N // 4
# (n_groups, H, W, C / n_groups, thres, q_mode).  Odd C / n_groups where n16 = Cg * ceil(HW / 16) is not a multiple of 4
# (the compacted hand-off's workspace parts), HW = 16 (16-byte paths), the 1080p y map, Cg = 1 (16 work items on 256
# threads), Cg = 512 (LDS 16 KB, several items per thread).
CASES = [
    (2, 1, 1, CG_DMC, 0.12, 0), (4, 1, 1, 1, -1.0, 1),
    (2, 1, 17, 3, 0.05, 0), (4, 1, 17, 5, 0.12, 1),
    (2, 3, 5, 5, 0.0, 1), (4, 3, 5, 3, 100.0, 0),
    (2, 4, 4, CG_DMC, 0.12, 0), (4, 4, 4, 1, 0.05, 1),
    (2, 8, 6, 1, 0.12, 0), (4, 8, 6, 3, -1.0, 1),
    (2, 9, 13, CG_DMC, 100.0, 0), (4, 9, 13, CG_DMCI, 0.12, 1),
    (2, 17, 30, 512, 0.12, 0), (4, 17, 30, 1, 0.0, 1),
    (2, 68, 120, CG_DMC, 0.12, 0), (4, 68, 120, CG_DMCI, 0.05, 1),
]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _lib():
    from opendcvc_amd import _lib as L
    return L


def _check(rc, what):
    _lib().check(rc, what)


# ------------------------------------------------------------------ edge values
def _bin_edges_f32():
    """first fp32 scale of every scale_to_index bin in [0.11, 16] (bisection on the bit patterns) and the one below it"""
    args = (O.SCALE_MIN, O.SCALE_MAX, O.LOG_SCALE_MIN, O.LOG_STEP_RECIP)
    idx = lambda b: O.scale_to_index(b.astype(np.uint32).view(np.float32), *args).astype(np.int64)
    lo0 = int(np.float32(O.SCALE_MIN).view(np.uint32))
    hi0 = int(np.float32(O.SCALE_MAX).view(np.uint32))
    ks = np.arange(int(idx(np.array([lo0]))[0]) + 1, int(idx(np.array([hi0]))[0]) + 1)
    lo, hi = np.full(ks.shape, lo0, np.int64), np.full(ks.shape, hi0, np.int64)
    while np.any(hi - lo > 1):          # invariant: idx(lo) < k <= idx(hi)
        mid = (lo + hi) // 2
        up = idx(mid) >= ks
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    assert np.all(idx(hi) == ks) and np.all(idx(lo) == ks - 1)
    return np.concatenate([hi, lo]).astype(np.uint32).view(np.float32)


def _bin_edges_f16():
    """every fp16 scale in [0.11, 16] whose index differs from that of the next fp16 value, and that next value"""
    b = np.arange(int(np.float16(0.1).view(np.uint16)), int(np.float16(16.5).view(np.uint16)), dtype=np.uint16)
    s = b.view(np.float16)
    i = O.scale_to_index(np.clip(s.astype(np.float32), np.float32(0.11), np.float32(16)), O.SCALE_MIN, O.SCALE_MAX,
                         O.LOG_SCALE_MIN, O.LOG_STEP_RECIP)
    ch = np.nonzero(np.diff(i.astype(np.int64)))[0]
    assert ch.size >= 120
    return np.concatenate([s[ch], s[ch + 1]]).astype(np.float32)


_EDGES = {}


def scale_edges(dt):
    if dt not in _EDGES:
        f32 = np.float32
        base = [0.0, -0.0, -1.0, -0.11, 1e-8, 0.11, 16.0, 1e4]
        for v in [0.11, 16.0] + [t for t in THRES_LIST if t > 0]:
            base += [v, np.nextafter(f32(v), f32(np.inf)), np.nextafter(f32(v), f32(-np.inf))]
            h = np.float16(v)
            base += [h, np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))]
        edges = _bin_edges_f32() if dt == np.float32 else _bin_edges_f16()
        _EDGES[dt] = np.concatenate([np.array(base, np.float32), edges]).astype(dt)
    return _EDGES[dt]


# ------------------------------------------------------------------ inputs
def make_inputs(rng, n_groups, H, W, C, q_mode, dt):
    """y, qsrc and the (scales, means) of every step, in the storage type.  Where the quantisation step is an exact power of
    two (q_dec in {<0.5, 0.5, 1, 64}, raw intra q at +-20), y is placed so that y * qe - mean is one of TIES exactly."""
    shape = (H, W, C)
    if q_mode == 0:
        u = rng.random(shape)
        qd = rng.uniform(0.3, 3.0, shape)
        qd = np.select([u < 0.1, u < 0.2, u < 0.45, u < 0.5], [0.25, 0.5, 1.0, 64.0], qd)
        qe = np.select([u < 0.2, u < 0.45, u < 0.5], [2.0, 1.0, 1.0 / 64], np.nan)
        qsrc = qd
    else:
        qsrc = rng.normal(0, 1.5, (H, W, 2))
        u = rng.random((H, W))
        qsrc[:, :, 0] = np.select([u < 0.3, u < 0.6], [20.0, -20.0], qsrc[:, :, 0])
        qsrc[:, :, 1] = np.where(rng.random((H, W)) < 0.2, 20.0, qsrc[:, :, 1])
        qe = np.broadcast_to(np.select([u < 0.3, u < 0.6], [2.0, 0.5], np.nan)[:, :, None], shape)
    y = rng.normal(0, 8, shape)
    steps = []
    for step in range(n_groups):
        m = rng.normal(0, 3, shape)
        s = np.exp(rng.normal(-1.0, 1.8, shape))
        edge = rng.random(shape) < 0.35
        se = scale_edges(dt)
        s = np.where(edge, se[rng.integers(0, se.size, shape)].astype(np.float64), s)
        s = np.where(rng.random(shape) < 0.05, -s, s)
        # ties: only the step that owns a (pixel, channel) matters for it, so every step places its own
        mask = R._masks(n_groups, H, W, C)[step] > 0
        tie = mask & ~np.isnan(qe) & (rng.random(shape) < 0.5)
        mt = np.array(DYADIC_MEANS)[rng.integers(0, len(DYADIC_MEANS), shape)]
        t = np.array(TIES)[rng.integers(0, len(TIES), shape)]
        yt = (mt + t) / np.where(np.isnan(qe), 1.0, qe)
        tie &= np.abs(yt) < 6e4
        m = np.where(tie, mt, m)
        y = np.where(tie, yt, y)
        steps.append((s, m))
    y = np.where(rng.random(shape) < 0.02, -0.0, y).astype(dt)
    return y, np.asarray(qsrc).astype(dt), [(s.astype(dt), m.astype(dt)) for s, m in steps]


# ------------------------------------------------------------------ device buffers
class Layout:
    """one case's device buffers, laid out like the codecs' (models.py) but with a distinct leading dimension each"""

    def __init__(self, n_groups, H, W, C, q_mode, dt_t, y, qsrc, steps):
        self.n = (C // n_groups) * H * W
        self.C = C
        ld_y = C + 3
        self.ybuf = torch.full((H, W, ld_y), 5.0, dtype=dt_t)
        self.ybuf[:, :, 1:1 + C] = torch.from_numpy(y)
        self.y = self.ybuf.cuda()[:, :, 1:1 + C]
        if q_mode == 0:        # DMC: params = [q_dec | scales | means]
            self.pbuf = torch.zeros((H, W, 3 * C + 5), dtype=dt_t)
            self.pbuf[:, :, :C] = torch.from_numpy(qsrc)
            so, mo = C, 2 * C
        else:                  # DMCI: params = [2 raw q | scales | means]
            self.pbuf = torch.zeros((H, W, 2 + 2 * C + 7), dtype=dt_t)
            self.pbuf[:, :, :2] = torch.from_numpy(qsrc)
            so, mo = 2, 2 + C
        self.pbuf[:, :, so:so + C] = torch.from_numpy(steps[0][0])
        self.pbuf[:, :, mo:mo + C] = torch.from_numpy(steps[0][1])
        self.pbuf = self.pbuf.cuda()
        self.qsrc = self.pbuf[:, :, :C] if q_mode == 0 else self.pbuf
        self.sm = [(self.pbuf[:, :, so:so + C], self.pbuf[:, :, mo:mo + C])]
        for s, m in steps[1:]:  # the spatial prior's output: [scales | means] of a buffer of its own
            sp = torch.zeros((H, W, 2 * C + 1 + len(self.sm)), dtype=dt_t)
            sp[:, :, :C], sp[:, :, C:2 * C] = torch.from_numpy(s), torch.from_numpy(m)
            sp = sp.cuda()
            self.sm.append((sp[:, :, :C], sp[:, :, C:2 * C]))
        # y_hat in place, inside guard channels
        self.hbuf = torch.full((H, W, C + 6), GUARD_Y, dtype=dt_t, device="cuda")
        self.yhat = self.hbuf[:, :, 2:2 + C]


def guards_intact(buf, off, C):
    """the channels of buf outside [off, off + C) still hold GUARD_Y"""
    b = buf.cpu()
    return bool((b[:, :, :off] == GUARD_Y).all() and (b[:, :, off + C:] == GUARD_Y).all())


def _enc_step(dt, n_groups, step, q_mode, lay, thres, packed):
    s, m = lay.sm[step]
    yh = lay.yhat
    _check(_lib().lib().dcvc_prior_enc_step(
        dt, n_groups, step, q_mode, _p(lay.y), lay.y.stride(1), _p(lay.qsrc), lay.qsrc.stride(1), _p(s), s.stride(1),
        _p(m), m.stride(1), yh.shape[0], yh.shape[1], lay.C, thres, _p(yh), yh.stride(1), _p(yh), yh.stride(1), _p(packed),
        _stream()), "prior_enc_step")


def _oracle_chain(n_groups, q_mode, y, qsrc, steps, thres):
    """the oracle's own compress_prior_2x / _4x sequence (OracleDMC / OracleDMCI.compress) in fp32: y_hat, kept streams"""
    H, W, C = y.shape
    if q_mode == 0:
        q_d = np.maximum(qsrc, np.float32(0.5))
        yq = y * (np.float32(1.0) / q_d)
    else:
        qq = O.sigmoid(qsrc[:, :, :2]) * np.float32(1.5) + np.float32(0.5)
        yq, q_d = y * qq[:, :, 0:1], qq[:, :, 1:2]
    cb = R._coder(thres)
    masks = R._masks(n_groups, H, W, C)
    so_far, packed = None, []
    for step, (s, m) in enumerate(steps):
        _, y_q, y_hat_k, s_hat = O.process_with_mask(yq, s, m, masks[step], cb.thres)
        packed.append(cb.pack_y(R.collapse(y_q, n_groups), R.collapse(s_hat, n_groups)))
        so_far = y_hat_k if so_far is None else so_far + y_hat_k
    return so_far * q_d, packed


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("n_groups,H,W,Cg,thres,q_mode", CASES)
def test_prior_chain_matches_restatement(dname, n_groups, H, W, Cg, thres, q_mode):
    """Encoder chain (every step in place, then finish), and at every step the decoder's whole-array index build and
    restore (round trip of the encoder's symbols) and the compacted hand-off, against prior_ref bit for bit."""
    from opendcvc_amd import entropy
    dt_t, dt_n = DTYPES[dname]
    L = _lib()
    lib = L.lib()
    dt = 1 if dt_n == np.float32 else 0
    C = Cg * n_groups
    rng = np.random.default_rng(1000 * H + 10 * W + Cg + n_groups)
    y, qsrc, steps = make_inputs(rng, n_groups, H, W, C, q_mode, dt_n)
    lay = Layout(n_groups, H, W, C, q_mode, dt_t, y, qsrc, steps)
    n, cap = lay.n, (lay.n + 15) // 16 * 16
    st = _stream()
    ws_bytes = int(lib.dcvc_prior_dec_compact_ws_bytes(H, W, C, n_groups))
    assert ws_bytes >= 16 + 4 * ((n + 15) // 16) + cap
    # decoder y_hat: out of place, alternating between two buffers of different leading dimensions
    dbuf = [torch.full((H, W, C + 4), GUARD_Y, dtype=dt_t, device="cuda"), torch.full((H, W, C + 9), GUARD_Y, dtype=dt_t, device="cuda")]
    dview = [dbuf[0][:, :, 1:1 + C], dbuf[1][:, :, 3:3 + C]]
    cbuf = [torch.full((H, W, C + 7), GUARD_Y, dtype=dt_t, device="cuda"), torch.full((H, W, C + 2), GUARD_Y, dtype=dt_t, device="cuda")]
    cview = [cbuf[0][:, :, 5:5 + C], cbuf[1][:, :, :C]]
    ref_yhat = ref_dec = None
    packs = []
    for step, (s_np, m_np) in enumerate(steps):
        what = "%s step %d" % (dname, step)
        # ---- encoder step (in place: yhat_in == yhat_out, as models.py passes it)
        packed = torch.full((n + 8,), GUARD_PACKED, dtype=torch.int16, device="cuda")
        _enc_step(dt, n_groups, step, q_mode, lay, thres, packed)
        ref_yhat, ref_packed = R.enc_step(n_groups, step, q_mode, y, qsrc, s_np, m_np, thres, ref_yhat, dt_n)
        torch.cuda.synchronize()
        got = lay.yhat.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(ref_yhat)), what + ": y_hat"
        assert guards_intact(lay.hbuf, 2, C), what + ": y_hat guard channels written"
        pk = packed.cpu().numpy()
        assert np.array_equal(pk[:n], ref_packed), what + ": packed symbols"
        assert np.all(pk[n:] == GUARD_PACKED), what + ": written past the packed symbols"
        packs.append(pk[:n])
        # ---- decoder: whole-array index build == the packed low bytes (sentinels included) == restatement
        s_dev, m_dev = lay.sm[step]
        idx = torch.full((n + 16,), GUARD_IDX, dtype=torch.uint8, device="cuda")
        _check(lib.dcvc_prior_dec_index(dt, n_groups, step, _p(s_dev), s_dev.stride(1), H, W, C, thres, _p(idx), st), "dec_index")
        torch.cuda.synchronize()
        ix = idx.cpu().numpy()
        ref_idx = R.dec_index(n_groups, step, s_np, thres)
        assert np.array_equal(ix[:n], ref_idx), what + ": indexes"
        assert np.array_equal(ix[:n], (pk[:n].view(np.uint16) & 0xFF).astype(np.uint8)), what + ": indexes vs encoder"
        assert np.all(ix[n:] == GUARD_IDX), what + ": written past the indexes"
        # ---- decoder: restore the encoder's symbols (out of place) == the encoder's y_hat
        sym = torch.from_numpy((pk[:n] >> 8).astype(np.int8)).cuda()
        src, dst = dview[(step + 1) % 2], dview[step % 2]
        _check(lib.dcvc_prior_dec_restore(dt, n_groups, step, _p(sym), _p(m_dev), m_dev.stride(1), H, W, C,
                                          _p(src) if step else None, src.stride(1), _p(dst), dst.stride(1), st), "dec_restore")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(dst.cpu().numpy()), _bits(ref_yhat)), what + ": restore != encoder y_hat"
        assert guards_intact(dbuf[step % 2], (1, 3)[step % 2], C), what + ": restore guard channels"
        # ---- compacted hand-off: kept indexes in CHW order into pinned memory, restore from compacted symbols
        keep = ref_idx != R.SENTINEL
        count_want = int(keep.sum())
        sym_full = np.where(keep, rng.integers(-128, 128, n), 0).astype(np.int8)
        ref_dec = R.dec_restore(n_groups, step, sym_full, m_np, ref_dec, dt_n)
        cidx = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        hidx, hcnt, hsym = entropy.PinnedBuffer(cap), entropy.PinnedBuffer(16), entropy.PinnedBuffer(cap)
        hidx.u8[:] = GUARD_IDX
        hcnt.u8[:] = 0xEE
        _check(lib.dcvc_prior_dec_index_compact(dt, n_groups, step, _p(s_dev), s_dev.stride(1), H, W, C, thres, _p(cidx),
                                                _p(ws), ctypes.c_void_p(hidx.ptr), ctypes.c_void_p(hcnt.ptr), st), "index_compact")
        torch.cuda.synchronize()
        count = int(hcnt.view(np.int32, 1)[0])
        assert count == count_want, what + ": kept count"
        assert np.all(hcnt.u8[4:] == 0xEE), what + ": written past the count"
        assert np.array_equal(hidx.u8[:count], ref_idx[keep]), what + ": compacted indexes"
        assert np.all(hidx.u8[count:] == GUARD_IDX), what + ": written past the compacted indexes"
        hsym.u8[:] = 0x55
        hsym.view(np.int8, cap)[:count] = sym_full[keep]
        csrc, cdst = cview[(step + 1) % 2], cview[step % 2]
        _check(lib.dcvc_prior_dec_restore_compact(dt, n_groups, step, ctypes.c_void_p(hsym.ptr), _p(cidx), _p(ws), _p(m_dev),
                                                  m_dev.stride(1), H, W, C, _p(csrc) if step else None, csrc.stride(1),
                                                  _p(cdst), cdst.stride(1), st), "restore_compact")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(cdst.cpu().numpy()), _bits(ref_dec)), what + ": compacted restore"
        assert guards_intact(cbuf[step % 2], (5, 0)[step % 2], C), what + ": compacted restore guard channels"
    # ---- finish (in place, guard channels intact)
    _check(lib.dcvc_prior_finish(dt, q_mode, _p(lay.yhat), lay.yhat.stride(1), _p(lay.qsrc), lay.qsrc.stride(1), H, W, C, st),
           "prior_finish")
    ref_fin = R.finish(q_mode, ref_yhat, qsrc, dt_n)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(lay.yhat.cpu().numpy()), _bits(ref_fin)), dname + ": finish"
    assert guards_intact(lay.hbuf, 2, C), dname + ": finish wrote the guard channels"
    if dt_n == np.float32:
        # fp32: the oracle's own sequence gives the same y_hat and streams
        o_yhat, o_packed = _oracle_chain(n_groups, q_mode, y, qsrc, [(s, m) for s, m in steps], thres)
        assert np.array_equal(lay.yhat.cpu().numpy(), o_yhat)
        for step, want in enumerate(o_packed):
            assert np.array_equal(R.kept(packs[step]), want), "oracle stream of step %d" % step


@pytest.mark.parametrize("dname", list(DTYPES))
def test_round_z_and_z_from_int8(dname):
    """dcvc_round_z (half-even ties, clamp to [-128, 127], in place with ld > C, int8 copy in CHW order) and dcvc_z_from_int8
    (CHW int8 -> HWC with ldo > C, guard channels untouched)."""
    dt_t, dt_n = DTYPES[dname]
    lib = _lib().lib()
    dt = 1 if dt_n == np.float32 else 0
    st = _stream()
    rng = np.random.default_rng(11)
    for H, W, C in ((1, 1, 1), (3, 5, 7), (17, 30, 128), (4, 4, 3)):
        z = rng.normal(0, 70, (H, W, C))
        edges = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, 127.5, -127.5, -128.5, 128.0, -129.0, 1e4, -1e4, -0.0, 0.49])
        sel = rng.random(z.shape) < 0.4
        z = np.where(sel, edges[rng.integers(0, edges.size, z.shape)], z).astype(dt_n)
        buf = torch.full((H, W, C + 5), GUARD_Y, dtype=dt_t)
        buf[:, :, 2:2 + C] = torch.from_numpy(z)
        buf = buf.cuda()
        zv = buf[:, :, 2:2 + C]
        z8 = torch.full((C * H * W + 8,), 0x33, dtype=torch.int8, device="cuda")
        _check(lib.dcvc_round_z(dt, _p(zv), zv.stride(1), H, W, C, _p(z8), st), "round_z")
        want, want8 = R.round_z(z, dt_n)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(zv.cpu().numpy()), _bits(want))
        assert guards_intact(buf, 2, C)
        got8 = z8.cpu().numpy()
        assert np.array_equal(got8[:C * H * W], want8) and np.all(got8[C * H * W:] == 0x33)
        out = torch.full((H, W, C + 3), GUARD_Y, dtype=dt_t, device="cuda")
        ov = out[:, :, 1:1 + C]
        _check(lib.dcvc_z_from_int8(dt, _p(z8), H, W, C, _p(ov), ov.stride(1), st), "z_from_int8")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(ov.cpu().numpy()), _bits(R.z_from_int8(want8, H, W, C, dt_n)))
        assert guards_intact(out, 1, C)


# ------------------------------------------------------------------ placement: pinned host memory or device memory
# (n_groups, H, W, C / n_groups): HW on and off the 16-byte path, an odd n16, both group counts
PLACEMENT_CASES = [(2, 3, 5, 5), (4, 1, 17, 5), (2, 4, 4, 64), (4, 9, 13, 64)]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("n_groups,H,W,Cg", PLACEMENT_CASES)
def test_compacted_hand_off_in_device_memory_equals_the_pinned_one(dname, n_groups, H, W, Cg):
    """dcvc_prior_dec_index_compact_dev (kept indexes and their count into DEVICE memory) followed by
    dcvc_prior_dec_restore_compact_dev (compacted symbols read from device memory, no gather) against the pinned pair, at every
    step: same indexes, count, index array and y_hat bit for bit, and nothing written behind what each call owns."""
    from opendcvc_amd import entropy
    dt_t, dt_n = DTYPES[dname]
    lib = _lib().lib()
    dt = 1 if dt_n == np.float32 else 0
    C, thres, st = Cg * n_groups, 0.12, _stream()
    n = Cg * H * W
    cap = (n + 15) // 16 * 16
    rng = np.random.default_rng(100 * H + W + Cg + n_groups)
    draw = lambda f: torch.from_numpy(f((H, W, C)).astype(np.float32)).to(dt_t).cuda()
    ws_bytes = int(lib.dcvc_prior_dec_compact_ws_bytes(H, W, C, n_groups))
    for step in range(n_groups):
        what = "%s step %d" % (dname, step)
        scales = draw(lambda s: np.exp(rng.normal(-2.4, 1.0, s)))
        means, prev = draw(lambda s: rng.normal(0, 2, s)), draw(lambda s: rng.normal(0, 2, s))
        # ---- index: pinned, then device
        idx_p, idx_d = (torch.full((n,), 9, dtype=torch.uint8, device="cuda") for _ in range(2))
        ws_p, ws_d = (torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda") for _ in range(2))
        hidx, hcnt, hsym = entropy.PinnedBuffer(cap), entropy.PinnedBuffer(16), entropy.PinnedBuffer(cap)
        hidx.u8[:] = GUARD_IDX
        _check(lib.dcvc_prior_dec_index_compact(dt, n_groups, step, _p(scales), scales.stride(1), H, W, C, thres, _p(idx_p),
                                                _p(ws_p), ctypes.c_void_p(hidx.ptr), ctypes.c_void_p(hcnt.ptr), st), "index_compact")
        cidx = torch.full((cap + 16,), GUARD_IDX, dtype=torch.uint8, device="cuda")
        cnt = torch.full((4,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
        _check(lib.dcvc_prior_dec_index_compact_dev(dt, n_groups, step, _p(scales), scales.stride(1), H, W, C, thres, _p(idx_d),
                                                    _p(ws_d), _p(cidx), _p(cnt), st), "index_compact_dev")
        torch.cuda.synchronize()
        count = int(hcnt.view(np.int32, 1)[0])
        got_cnt, got_cidx = cnt.cpu().numpy(), cidx.cpu().numpy()
        assert 0 < count < n, what + ": the case keeps some positions, not all"
        assert got_cnt[0] == count and np.all(got_cnt[1:] == 0x6E6E6E6E), what + ": count in device memory"
        assert np.array_equal(got_cidx[:count], hidx.u8[:count]), what + ": compacted indexes in device memory"
        assert np.all(got_cidx[count:] == GUARD_IDX), what + ": written past the compacted indexes"
        assert np.array_equal(idx_d.cpu().numpy(), idx_p.cpu().numpy()), what + ": index array"
        # ---- restore: the same compacted symbols from pinned memory (gathered) and from device memory
        csym = rng.integers(-128, 128, count).astype(np.int8)
        hsym.u8[:] = 0x55
        hsym.view(np.int8, cap)[:count] = csym
        dsym = torch.full((cap,), 0x55, dtype=torch.int8)
        dsym[:count] = torch.from_numpy(csym)
        dsym = dsym.cuda()
        bufs = [torch.full((H, W, C + 5), GUARD_Y, dtype=dt_t, device="cuda") for _ in range(2)]
        out_p, out_d = bufs[0][:, :, 2:2 + C], bufs[1][:, :, 2:2 + C]
        _check(lib.dcvc_prior_dec_restore_compact(dt, n_groups, step, ctypes.c_void_p(hsym.ptr), _p(idx_p), _p(ws_p), _p(means),
                                                  means.stride(1), H, W, C, _p(prev) if step else None, prev.stride(1),
                                                  _p(out_p), out_p.stride(1), st), "restore_compact")
        _check(lib.dcvc_prior_dec_restore_compact_dev(dt, n_groups, step, _p(dsym), _p(idx_d), _p(ws_d), _p(means),
                                                      means.stride(1), H, W, C, _p(prev) if step else None, prev.stride(1),
                                                      _p(out_d), out_d.stride(1), st), "restore_compact_dev")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out_d.cpu().numpy()), _bits(out_p.cpu().numpy())), what + ": restore from device symbols"
        assert guards_intact(bufs[0], 2, C) and guards_intact(bufs[1], 2, C), what + ": restore guard channels"


@pytest.mark.parametrize("parts,n", [(1, 1), (4, 777), (2, 5000)])
def test_compact_symbols_in_device_memory_equals_the_pinned_one(parts, n):
    """dcvc_compact_symbols_dev against dcvc_compact_symbols: the kept symbols of every part in order and the counts, in device
    memory as in pinned memory, nothing else touched."""
    from opendcvc_amd import entropy
    lib = _lib().lib()
    st = _stream()
    rng = np.random.default_rng(parts * 1000 + n)
    a = rng.integers(-32768, 32767, (parts, n), dtype=np.int16)
    skip = rng.random((parts, n)) < 0.7
    skip[:, 0] = False
    a = np.where(skip, (a & ~0xFF) | 0xFF, np.where((a & 0xFF) == 0xFF, a & ~1, a)).astype(np.int16)
    dev = torch.from_numpy(a).cuda()
    out, cnt = entropy.PinnedBuffer(parts * n * 2), entropy.PinnedBuffer(4 * parts)
    out.u8[:] = 0x7E
    ws = torch.zeros(256 * parts, dtype=torch.int32, device="cuda")
    _check(lib.dcvc_compact_symbols(_p(dev), n, parts, ctypes.c_void_p(out.ptr), ctypes.c_void_p(cnt.ptr), _p(ws), st), "compact")
    dout = torch.full((parts * n + 8,), GUARD_PACKED, dtype=torch.int16, device="cuda")
    dcnt = torch.full((parts + 2,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
    ws_d = torch.zeros(256 * parts, dtype=torch.int32, device="cuda")
    _check(lib.dcvc_compact_symbols_dev(_p(dev), n, parts, _p(dout), _p(dcnt), _p(ws_d), st), "compact_dev")
    torch.cuda.synchronize()
    want, kept = out.view(np.int16, parts * n), cnt.view(np.int32, parts)
    got, got_cnt = dout.cpu().numpy(), dcnt.cpu().numpy()
    assert np.array_equal(kept, (~skip).sum(axis=1))
    assert np.array_equal(got_cnt[:parts], kept) and np.all(got_cnt[parts:] == 0x6E6E6E6E)
    assert np.array_equal(got[:parts * n], want)     # (kept symbols, then the sentinel of either buffer: 0x7E7E)
    assert np.all(got[parts * n:] == GUARD_PACKED)
