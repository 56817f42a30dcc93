"""Developer tool: the two tables of docs/deinterlace.md, made on the CPU with the numpy restatement (tests/deint_ref.py) on
synthetic clips whose truth is known - a smooth random texture moving S pixels per frame (S / 2 per field).
1. MSE, in squared 8-bit codes, of the woven frames, of the spatial predictor alone and of the filter against the true
   progressive frames, luma and chroma apart, in fp32 and fp16, 4:4:4 and 4:2:0.
2. dc / dp of the rule with a previous frame and dc / ds of the rule without one, over progressive, interlaced and static
   clips, two textures, noise of sigma 0 .. 4 codes, with and without a vertical motion of one line per field.
    python tools/deint_tables.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import deint_ref as R

H, W, N = 64, 96, 4
print("| storage | chroma | plane | S | weave | spatial only | filter |\n|---|---|---|---|---|---|---|")
for ndt in (np.float32, np.float16):
    for lines in (1, 2):
        for speed in (1, 2, 4, 8):
            clip, truth = R.make_clip("interlaced", N, H, W, speed=speed, seed=speed, chroma_lines=lines)
            full, alone = R.Deinterlacer("on", "tff", lines), R.Deinterlacer("on", "tff", lines)
            err = np.zeros((2, 3))
            for planes, true in zip(clip, truth):
                x, t = R.to_frame(planes, ndt), R.to_frame(true, ndt).astype(np.float64)
                alone.reset()
                for k, y in enumerate((x, alone.filter(x, (H, W)), full.filter(x, (H, W)))):
                    e = (y.astype(np.float64) - t) ** 2 * 255.0 ** 2 / N
                    err[0, k] += np.mean(e[0])
                    err[1, k] += np.mean(e[1:])
            for name, e in zip(("luma", "chroma"), err):
                print(f"| {'fp32' if ndt is np.float32 else 'fp16'} | {'4:4:4' if lines == 1 else '4:2:0'} | {name} | {speed} | "
                      f"{e[0]:.1f} | {e[1]:.1f} | {e[2]:.1f} |")

H, W = 96, 128
print("\n| class | vertical | dc / dp, frames 1 .. 3 | dc / ds, frame 0 |\n|---|---|---|---|")
for kind in ("progressive", "interlaced", "static"):
    for vy in (0, 1):
        lo, hi, flo, fhi = 9.0, 0.0, 9.0, 0.0
        for blur in (1, 2):
            for sigma in (0.0, 2.0, 4.0):
                for speed in ((1,) if kind == "static" else (1, 2, 4, 8)):
                    clip, _ = R.make_clip(kind, 4, H, W, speed=speed, vy=vy, sigma=sigma, seed=speed + 7 * vy, blur=blur)
                    fr = [R.to_frame(f) for f in clip]
                    for t in (1, 2, 3):
                        dc, dp = R.comb_sums(fr[t], fr[t - 1], H, W, 0)
                        lo, hi = min(lo, dc / dp), max(hi, dc / dp)
                    dc, ds = R.comb_sums(fr[0], None, H, W, 0)
                    flo, fhi = min(flo, dc / ds), max(fhi, dc / ds)
        print(f"| {kind}, 1 .. 8 pixels per frame, sigma 0 .. 4 | {'one line per field' if vy else 'none'} | {lo:.2f} .. {hi:.2f} | "
              f"{flo:.2f} .. {fhi:.2f} |")
clip, _ = R.make_clip("interlaced", 1, H, W, speed=0, vy=1, seed=2, blur=1)
dc, ds = R.comb_sums(R.to_frame(clip[0]), None, H, W, 0)
print(f"| interlaced, one line per field straight up | - | - | {dc / ds:.2f} |")
