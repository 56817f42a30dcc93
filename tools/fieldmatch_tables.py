"""Developer tool: the tables of docs/deinterlace.md's "Film mode", made on the CPU with the numpy restatement
(tests/fieldmatch_ref.py) on deint_ref.make_clip's synthetic clips, 96 x 128: max_m, the largest number of combed samples in one
16 x 16 block, per class of candidate field, at the threshold T of the document and at the ones either side of it.
    python tools/fieldmatch_tables.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import deint_ref as R
import fieldmatch_ref as M

H, W = 96, 128


def maxima(frames, t, parity=0):
    """(max_c, max_p) of frame t of a clip of model frames"""
    q = R.quant(frames[t][0])
    return M.comb_max(q, q, H, W, parity), M.comb_max(q, R.quant(frames[t - 1][0]), H, W, parity)


class Range:
    def __init__(self):
        self.lo, self.hi = None, None

    def add(self, v):
        self.lo, self.hi = (v, v) if self.lo is None else (min(self.lo, v), max(self.hi, v))

    def __str__(self):
        return f"{self.lo} .. {self.hi}"


def small_object(speed, blur, sigma):
    """a 16 x 16 interlaced object over columns 24 .. 39 - half in one block, half in the next - on a static ground"""
    ground = R.make_clip("static", 3, H, W, speed=speed, sigma=sigma, seed=speed, blur=blur)[0]
    moving = R.make_clip("interlaced", 3, H, W, speed=speed, sigma=sigma, seed=speed + 50, blur=blur)[0]
    out = []
    for g, m in zip(ground, moving):
        g = np.array(g)
        g[:, 32:48, 24:40] = m[:, 32:48, 24:40]
        out.append(g)
    return out


for T in (24, 36, 48):
    M.T = T
    rows = {name: Range() for name in ("clean", "clean, blur 1 under sigma 4", "wrong candidate of a telecined frame",
                                       "interlaced video, speed 1, blur 2", "interlaced video otherwise",
                                       "small interlaced object, speed 1, blur 2", "small interlaced object otherwise")}
    for blur in (1, 2):
        for sigma in (0.0, 4.0):
            clean = rows["clean, blur 1 under sigma 4" if (blur, sigma) == (1, 4.0) else "clean"]
            for speed in (1, 2, 4, 8):
                film = R.make_clip("progressive", 6, H, W, speed=speed, sigma=sigma, seed=5, blur=blur)[0]
                fr = [R.to_frame(f) for f in M.telecine(film, M.PULLDOWN)]
                for t in range(1, 7):
                    (i, j), (_, pj) = M.PULLDOWN[t], M.PULLDOWN[t - 1]
                    mc, mp = maxima(fr, t)
                    (clean if i == j else rows["wrong candidate of a telecined frame"]).add(mc)
                    (clean if i == pj else rows["wrong candidate of a telecined frame"]).add(mp)
                slow = speed == 1 and blur == 2
                fr = [R.to_frame(f) for f in R.make_clip("interlaced", 3, H, W, speed=speed, sigma=sigma, seed=5, blur=blur)[0]]
                for t in (1, 2):
                    for m in maxima(fr, t):
                        rows["interlaced video, speed 1, blur 2" if slow else "interlaced video otherwise"].add(m)
                fr = [R.to_frame(f) for f in small_object(speed, blur, sigma)]
                for t in (1, 2):
                    for m in maxima(fr, t):
                        rows["small interlaced object, speed 1, blur 2" if slow else "small interlaced object otherwise"].add(m)
            fr = [R.to_frame(f) for f in R.make_clip("static", 3, H, W, sigma=sigma, seed=5, blur=blur)[0]]
            for t in (1, 2):
                for m in maxima(fr, t):
                    clean.add(m)
    print(f"\nT = {T}\n| candidate | max_m |\n|---|---|")
    for name, r in rows.items():
        print(f"| {name} | {r} |")

# the clip of tests/test_fieldmatch_host.py
M.T = 36
film = R.make_clip("progressive", 6, H, W, speed=4, seed=5, blur=2)[0]
fr = [R.to_frame(f) for f in M.telecine(film, M.PULLDOWN)]
print("\nthe telecined test clip (blur 2, speed 4, sigma 0, seed 5): (max_c, max_p), filter, weave per frame")
for t in range(7):
    print(t, M.PULLDOWN[t], M.field_match(fr[t], fr[t - 1] if t else None, H, W, 0))
