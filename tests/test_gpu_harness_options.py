"""run_one_point with every per-point extension switched on at once (no other test does): the order of the log's extension
keys, the digest count, the reconstruction file against pipeline.StreamDecoder on the written container, and the container's
independence of where the metrics are computed."""
import numpy as np
import pytest
import torch

from opendcvc_amd import harness, weights
from opendcvc_amd.grain import GrainParams

pytestmark = pytest.mark.gpu

H, W, N = 96, 128, 8
CODED = (64, 80)
PARAMS = GrainParams(4242, 1, (8, 40, 72, 104, 136, 168, 200, 255), 90, 160)
EXTENSION_KEYS = ["scene_cuts", "target_bpp", "rc_qp", "rc_est_bpp", "frame_rc_qp", "frame_rc_est_bpp", "digests_checked",
                  "coded_height", "coded_width", "scale_filter", "grain_units", "grain_scale_y", "grain_corr"]


def test_every_extension_at_once(tmp_path):
    from opendcvc_amd.models import DMC, DMCI
    from opendcvc_amd.pipeline import StreamDecoder, store_yuv420_frame
    nets = []
    for cls, name in ((DMCI, "dmci"), (DMC, "dmc")):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(name, 1234).items()})
        m.to("cuda").eval()
        m.update(0.12)
        nets.append(m)
    src = tmp_path / "clip.yuv"
    with open(src, "wb") as f:
        for i in range(N):
            for plane in weights.synthetic_frame_yuv420(H, W, i, 3):
                f.write(plane.tobytes())

    def run(name, metrics):
        path, rec = str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}.yuv")
        log = harness.run_one_point(nets[0], nets[1], str(src), W, H, N, 32, 32, intra_period=4, scenecut=150, target_bpp=0.5,
                                    digest=True, coded_size=CODED, film_grain=PARAMS, metrics=metrics, entropy="device",
                                    verbose_json=True, bin_path=path, rec_path=rec)
        return log, path, open(rec, "rb").read()

    log, path, rec = run("device", "device")
    assert list(log.keys())[-len(EXTENSION_KEYS):] == EXTENSION_KEYS
    assert "ave_all_frame_msssim_v" == list(log.keys())[-len(EXTENSION_KEYS) - 1]          # (the last key of summarize)
    assert log["digests_checked"] == N and len(log["frame_rc_qp"]) == N
    assert (log["coded_height"], log["coded_width"], log["scale_filter"]) == (*CODED, "lanczos3")
    assert log["grain_units"] == log["i_frame_num"] >= 2 and log["grain_scale_y"] == list(PARAMS.scale_y) and log["grain_corr"] == 1
    data = open(path, "rb").read()
    assert round(sum(log["frame_bpp"]) * H * W) == 8 * len(data)

    # the container through the decode-side entry point: what it shows is what the harness stored
    with open(path, "rb") as f:
        decoder = StreamDecoder(f, nets[0], nets[1], "cuda:0")
        shown = b""
        for _ in range(N):
            frame = decoder.next()
            assert (frame.sps["height"], frame.sps["width"]) == CODED and frame.display == (H, W, "lanczos3")
            assert frame.grain == PARAMS and frame.shown is not frame.x_hat and frame.x_hat.shape == (1, 3, H, W)
            for plane in store_yuv420_frame(frame.shown, H, W):
                shown += plane.cpu().numpy().tobytes()
        decoder.flush()
        assert decoder.digests_checked == N
    assert shown == rec and len(rec) == N * H * W * 3 // 2

    # where the metrics are computed changes neither the container nor the stored pictures
    host_log, host_path, host_rec = run("host", "host")
    assert open(host_path, "rb").read() == data and host_rec == rec
    assert list(host_log.keys()) == list(log.keys())
