"""numpy restatement of field-rate deinterlacing (docs/deinterlace.md, "Field-rate output"; csrc/dcvc_deint_field.hip): the
second picture of a frame is the document's filter - tests/deint_ref.py's, unchanged - on the field-shifted frames, with the
other parity kept.  The kernel is held against field_picture bit for bit (tests/test_gpu_deint_field.py)."""
import numpy as np

import deint_ref as R


def shifted(a, b, H, parity, chroma_lines):
    """S: per plane the rows with (y / L) % 2 != parity from a (its second field), the others from b (its first field);
    a, b [3, Hp, Wp]; rows from H on are a's"""
    out = np.array(a)
    for p in range(3):
        L = 1 if p == 0 else chroma_lines
        rows = [y for y in range(H) if (y // L) % 2 == parity]
        out[p, rows] = b[p, rows]
    return out


def field_picture(before, cur, after, H, W, parity, chroma_lines):
    """B_n [3, Hp, Wp] of F_{n-1}, F_n, F_{n+1} (before / after None: none - the spatial predictor alone, from cur's second
    field); parity: the SOURCE's kept parity"""
    if before is None or after is None:
        return R.deinterlace(cur, None, H, W, 1 - parity, chroma_lines)
    return R.deinterlace(shifted(cur, after, H, parity, chroma_lines), shifted(before, cur, H, parity, chroma_lines), H, W,
                         1 - parity, chroma_lines)


def truth_at(k, frames, H, W, speed, seed=0, blur=2):
    """the noise-free full-resolution picture [3, H, W] of deint_ref.make_clip(kind, frames, H, W, speed=speed, seed=seed) at
    FIELD time k < 2 * frames, in 8-bit codes: make_clip's truth of frame t is this at k = 2 t"""
    tex = [R.texture(H, 2 * W + speed * 2 * frames, seed * 3 + p, blur) for p in range(3)]
    return np.stack([np.clip(np.rint(t[:, speed * k:speed * k + 2 * W:2] * 255.0), 0, 255) for t in tex])


class FieldRate:
    """opendcvc_amd.deinterlace.Deinterlacer(mode "on", rate "field") on numpy frames [3, Hp, Wp]"""

    def __init__(self, order="tff", chroma_lines=1):
        assert order in ("tff", "bff")
        self.parity, self.chroma_lines = 0 if order == "tff" else 1, chroma_lines
        self.frames = self.pictures = 0
        self.reset()

    def reset(self):
        self.before = self.cur = None                      # (frame, size) of the last two inputs; cur's B is pending

    @staticmethod
    def _like(a, b):
        return a is not None and b is not None and a[1] == b[1] and a[0].shape == b[0].shape and a[0].dtype == b[0].dtype

    def _second(self, after):
        (x, (H, W)), ok = self.cur, self._like(self.before, self.cur) and self._like(self.cur, after)
        return field_picture(self.before[0] if ok else None, x, after[0] if ok else None, H, W, self.parity, self.chroma_lines)

    def fields(self, x, size):
        H, W = size
        R.check_size(H, self.chroma_lines)
        new = (x, (H, W))
        out = [self._second(new)] if self.cur is not None else []
        prev = self.cur[0] if self._like(self.cur, new) else None
        out.append(R.deinterlace(x, prev, H, W, self.parity, self.chroma_lines))
        self.before, self.cur = self.cur, new
        self.frames += 1
        self.pictures += len(out)
        return out

    def drain(self):
        out = [self._second(None)] if self.cur is not None else []
        self.pictures += len(out)
        self.reset()
        return out


def field_rate_mse(speed, lines=1, H=64, W=96, n=5, ndt=np.float32, seed=0):
    """[luma, chroma] x (first pictures, second pictures, first pictures held over the half instant, the first second picture,
    the last one): MSE in squared 8-bit codes against the true picture at each picture's own instant; the first three are means
    over the interior pictures, the last two the clip's spatial-only ends (tools/deint_field_tables.py prints these).  The
    chroma of 4:2:0 is judged as the loader leaves it: the truth goes the clip's way"""
    clip = R.make_clip("interlaced", n, H, W, speed=speed, seed=seed, chroma_lines=lines)[0]
    fr = FieldRate("tff", lines)
    out = [p for c in clip for p in fr.fields(R.to_frame(c, ndt), (H, W))] + fr.drain()
    first, second = out[0:1] + out[2::2], out[1::2]

    def truth(k):
        t = truth_at(k, n, H, W, speed, seed)
        if lines == 2:
            t[1:] = np.repeat(np.repeat(t[1:, ::2, ::2], 2, 1), 2, 2)
        return t

    def mse(pic, k):
        e = (pic.astype(np.float64) * 255.0 - truth(k)) ** 2
        return np.array([e[0].mean(), e[1:].mean()])

    a = np.mean([mse(first[t], 2 * t) for t in range(1, n)], axis=0)
    b = np.mean([mse(second[t], 2 * t + 1) for t in range(1, n - 1)], axis=0)
    hold = np.mean([mse(first[t], 2 * t + 1) for t in range(1, n - 1)], axis=0)
    return np.stack([a, b, hold, mse(second[0], 1), mse(second[n - 1], 2 * n - 1)], axis=1)
