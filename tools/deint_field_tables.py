"""Developer tool: the table of docs/deinterlace.md's "Field-rate output", made on the CPU with the numpy restatement
(tests/deint_field_ref.py) on deint_ref.make_clip's synthetic clips - a smooth random texture moving S pixels per frame (S / 2
per field), 64 x 96, five frames, seed 0, fp32 storage.  MSE in squared 8-bit codes against the true picture at each picture's
OWN instant: the first pictures (the frame-rate output), the second pictures, the first pictures held over the half instant
(what a display does with frame-rate output), and the clip's two spatial-only second pictures; luma and chroma apart, 4:4:4
and 4:2:0.
    python tools/deint_field_tables.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import deint_field_ref as FR

print("| chroma | plane | S | first pictures | second pictures | second / first | first held over the half instant | held / second "
      "| B_0 | B_last |\n|---|---|---|---|---|---|---|---|---|---|")
for lines in (1, 2):
    rows = [(speed, FR.field_rate_mse(speed, lines)) for speed in (1, 2, 4, 8)]
    for plane, name in ((0, "luma"), (1, "chroma")):
        for speed, err in rows:
            a, b, hold, b0, bl = err[plane]
            print(f"| {'4:4:4' if lines == 1 else '4:2:0'} | {name} | {speed} | {a:.1f} | {b:.1f} | {b / a:.2f} | {hold:.1f} | "
                  f"{hold / b:.1f} | {b0:.1f} | {bl:.1f} |")
