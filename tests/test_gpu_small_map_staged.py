"""The staged small-map DepthConvBlock tail (fp16, widths 256 / 384 / 512 below 12 000 pixels: depthwise + W2 -> o, W3 + gate -> v,
W4 + epilogue -> out, three launches) stores o and v where the fused 32-pixel tail rounds them and slices output channels
only: its outputs equal the fused tail's (DCVC_T32S=0) bit for bit.  The switch is read once per process, so each setting
runs in a subprocess of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO, os.path.join(REPO, "oracle")]

pytestmark = pytest.mark.gpu


def _blocks_outputs():
    """Single blocks and short chains on small maps: plain, shortcut, quant step, two-source adaptor head, fused next head,
    then_conv with and without its quant vector; widths 256 / 368 (-> 384) / 384 / 512; regular and ragged maps."""
    from opendcvc_amd import _lib, nn
    from test_gpu_layers import _rng, make_dcb_weights, to_dev
    outs = []
    for c in (256, 368, 384, 512):
        for (H, W) in ((68, 120), (34, 60), (67, 119)):
            rng = _rng(7000 + c + H)
            f16 = torch.float16
            plain = nn.DepthConvBlock(make_dcb_weights(rng, "m", c, c, False), "m", f16)
            x = to_dev(rng.standard_normal((H, W, c)).astype(np.float32), plain.cin_p, f16)
            q = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32)).cuda()
            outs.append(plain(x))
            outs.append(plain(x, quant=q))
            sc = nn.DepthConvBlock(make_dcb_weights(rng, "m", c, c, False), "m", f16, shortcut=True)
            outs.append(sc(x))
            outs.append(sc(x, quant=q))
            ad = nn.DepthConvBlock(make_dcb_weights(rng, "m", 2 * c, c, True), "m", f16)
            x2 = to_dev(rng.standard_normal((H, W, 2 * c)).astype(np.float32), ad.cin_p, f16)
            outs.append(ad(x2))
            s0 = ad.cin_p // 2 // 64 * 64
            outs.append(ad(x2[..., :s0].contiguous(), x2[..., s0:].contiguous()))
            outs.append(nn.dcb_chain([ad, plain, plain], x2, quant=q))
            csd = {"o.weight": (rng.standard_normal((c, c, 1, 1)) / np.sqrt(c)).astype(np.float32),
                   "o.bias": (rng.standard_normal(c) * 0.1).astype(np.float32)}
            convq = nn.Conv2d(csd, "o", f16, epilogue=_lib.EPI_BIAS_QUANT)
            conv = nn.Conv2d(csd, "o", f16, epilogue=_lib.EPI_BIAS)
            outs.append(nn.dcb_chain([plain, plain], x, then_conv=convq, conv_quant=q))
            outs.append(nn.dcb_chain([plain], x, then_conv=conv))
    torch.cuda.synchronize()
    return np.concatenate([o.float().cpu().numpy().ravel() for o in outs])


def _codec_outputs():
    """An I frame and two P frames at 1920x1088 through DMCI / DMC: bit streams and reconstructions."""
    from opendcvc_amd import weights
    from opendcvc_amd.models import DMC, DMCI
    from seq_utils import INDEX_MAP, run_sequence
    torch.set_grad_enabled(False)
    sdi, sdp = weights.make_state_dict("dmci", 1234), weights.make_state_dict("dmc", 1234)
    i_net, p_net = DMCI(), DMC()
    qps = [32] + [p_net.shift_qp(32, INDEX_MAP[fi % 8]) for fi in (1, 2)]
    rec = dict(h=1088, w=1920, qp=32, two=0, reset_interval=0, seed=1234, thres=0.12,
               frames=[dict(qp=q, use_ada_i=0) for q in qps])
    i_net.load_state_dict({k: torch.from_numpy(v) for k, v in sdi.items()})
    p_net.load_state_dict({k: torch.from_numpy(v) for k, v in sdp.items()})
    for m in (i_net, p_net):
        m.to("cuda:0").eval()
        m.update(0.12)
        m.half()
    got = run_sequence(i_net, p_net, rec, to_x=lambda a: torch.from_numpy(a).cuda(), to_np=lambda t: t.float().cpu().numpy())
    parts = []
    for g in got:
        parts.append(np.frombuffer(bytes(g["bits"]), dtype=np.uint8).astype(np.float32))
        parts.append(np.asarray(g["x_hat"], dtype=np.float32).ravel())
    return np.concatenate(parts)


def _run_both(tmp_path, fn):
    outs = {}
    for v in ("1", "0"):
        path = tmp_path / f"{fn}_{v}.npy"
        code = ("import sys, numpy as np; sys.path[:0] = [%r, %r, %r]; import test_gpu_small_map_staged as t; np.save(%r, t.%s())"
                % (HERE, REPO, os.path.join(REPO, "oracle"), str(path), fn))
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, DCVC_T32S=v), timeout=900)
        outs[v] = np.load(path)
    return outs


def test_staged_small_map_layers_equal_fused(tmp_path):
    """test_gpu_layers._small_map_outputs (chains behind an adaptor block, shortcut + quant, fused 1x1 conv) staged = fused."""
    outs = {}
    for v in ("1", "0"):
        path = tmp_path / f"o{v}.npy"
        code = ("import sys, numpy as np; sys.path[:0] = [%r, %r, %r]; import test_gpu_layers as t; np.save(%r, t._small_map_outputs())"
                % (HERE, REPO, os.path.join(REPO, "oracle"), str(path)))
        subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, DCVC_T32S=v), timeout=900)
        outs[v] = np.load(path)
    assert np.isfinite(outs["1"]).all() and np.array_equal(outs["1"], outs["0"])


def test_staged_small_map_blocks_equal_fused(tmp_path):
    outs = _run_both(tmp_path, "_blocks_outputs")
    assert np.isfinite(outs["1"]).all() and np.array_equal(outs["1"], outs["0"])


def test_staged_small_map_codec_equal_fused(tmp_path):
    outs = _run_both(tmp_path, "_codec_outputs")
    assert outs["1"].shape == outs["0"].shape and np.array_equal(outs["1"], outs["0"])


def test_scratch_bytes_cover_the_staged_tail():
    """dcvc_dcb_scratch_bytes: + o (P x C) and v (P x 2C) on small fp16 maps of the staged widths, unchanged elsewhere."""
    from opendcvc_amd import _lib, nn
    from test_gpu_layers import _rng, make_dcb_weights
    L = _lib.lib()
    for c, cp in ((256, 256), (368, 384), (512, 512)):
        blk = nn.DepthConvBlock(make_dcb_weights(_rng(c), "m", c, c, False), "m", torch.float16)
        for (H, W) in ((68, 120), (34, 60), (67, 119)):
            P = H * W
            assert L.dcvc_dcb_scratch_bytes(blk.h, H, W) >= 3 * P * cp * 2 + 3 * P * cp * 2
        for (H, W) in ((136, 240), (100, 120)):
            assert L.dcvc_dcb_scratch_bytes(blk.h, H, W) == 3 * H * W * cp * 2
    blk = nn.DepthConvBlock(make_dcb_weights(_rng(1), "m", 128, 128, False), "m", torch.float16)
    assert L.dcvc_dcb_scratch_bytes(blk.h, 68, 120) == 3 * 68 * 120 * 128 * 2
    blk = nn.DepthConvBlock(make_dcb_weights(_rng(2), "m", 256, 256, False), "m", torch.float32)
    assert L.dcvc_dcb_scratch_bytes(blk.h, 68, 120) == 3 * 68 * 120 * 256 * 4
