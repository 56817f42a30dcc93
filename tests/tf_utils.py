"""What the GPU tests of the temporal pre-filter share (test_gpu_tf.py, test_gpu_tf_auto.py, test_gpu_tf_subpel.py): frames on
the device, bit views, the texture and the synthetic clip with its codecs.  The fixtures are imported by name."""
import numpy as np
import pytest
import torch

import tf_ref as R
from opendcvc_amd import weights


def _pad(n, to=16):
    return n + (-n) % to


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _padded_shape(size):
    return (48, 48) if size == (33, 40) else (_pad(size[0]), _pad(size[1]))


def _to_device(host, misaligned=False):
    """host [3, Hp, Wp] -> [1, 3, Hp, Wp] on the device; misaligned: one element into a larger allocation"""
    if not misaligned:
        return torch.from_numpy(np.array(host))[None].cuda()
    flat = torch.empty(host.size + 8, dtype=torch.from_numpy(np.zeros(1, host.dtype)).dtype, device="cuda")
    dev = flat[1:1 + host.size].view(1, *host.shape)
    dev.copy_(torch.from_numpy(np.array(host))[None])
    assert dev.data_ptr() % 16 == host.itemsize and dev.is_contiguous()
    return dev


@pytest.fixture(scope="module")
def tex():
    return R.texture()


def clip_fixture(h, w, n, name):
    """a module's `clip`: fp32 codecs with the synthetic weights and an h x w, n-frame synthetic 4:2:0 clip in a folder `name`
    -> ((DMCI, DMC), folder)"""
    @pytest.fixture(scope="module")
    def clip(tmp_path_factory):
        from opendcvc_amd.models import DMC, DMCI
        nets = []
        for cls, key in ((DMCI, "dmci"), (DMC, "dmc")):
            m = cls()
            m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.make_state_dict(key, 1234).items()})
            m.to("cuda").eval()
            m.update(0.12)
            nets.append(m)
        folder = tmp_path_factory.mktemp(name)
        with open(folder / "clip.yuv", "wb") as f:
            for i in range(n):
                for plane in weights.synthetic_frame_yuv420(h, w, i, 3):
                    f.write(plane.tobytes())
        return nets, folder
    return clip
