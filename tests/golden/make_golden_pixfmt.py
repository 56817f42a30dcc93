"""Golden vectors for the high-bit-depth / 4:4:4 frame I/O kernels (csrc/dcvc_pixfmt.hip), generated in the BUILD
container by calling the reference family's own reader, writer and transforms (the older harnesses' raw-video I/O):
  source side   DCVC-family/DCVC-FM/src/utils/video_reader.py:130-181 YUVReader.read_one_frame (astype(float32) / max_val),
                src/transforms/functional.py:98-109 ycbcr420_to_444 (scipy zoom, order 0)
  decoder side  src/transforms/functional.py:112-131 ycbcr444_to_420 (numpy mean over the 2x2 block, clip),
                src/utils/video_writer.py:85-128 YUVWriter.write_one_frame (clip(rint(. * max_val), 0, max_val))
For the three sizes of frame_io.npz (36 x 50, 16 x 32, 70 x 98), chroma 4:2:0 and 4:4:4, bit depths 10, 12 and 16:
  src_<tag>_<chroma>                 seeded 16-bit source planes y, u, v in file order (one flat array); the b-bit source of a
                                     case is these >> (16 - b)
  frame_<tag>_<chroma>_<bits>        the reference's normalised 4:4:4 frame [3, h, w], fp32 (fp16 expectation: .astype(float16);
                                     the replicate pad is this project's and is asserted as a property)
  rec_<tag>                          a seeded reconstruction [3, h, w], fp32, leaving [0, 1] on both sides at a few percent of the
                                     samples (fp16 reconstruction: .astype(float16); both are fed to the writer as fp32 values)
  out_<tag>_<chroma>_<bits>_{f32,f16}   the file the reference's writer wrote for that reconstruction: y, u, v, flat
The source planes are shared between the bit depths and one reconstruction serves every case of a size; at the two larger
sizes the planes and the reconstruction are constant over horizontal runs of 1 .. 16 pixels (independent values
and run boundaries in every row and plane, so every alignment of an edge against the kernels' 8-pixel pieces and every
2x2 mix of values occurs), the smallest size is independent in every sample: this keeps the file below the size of
frame_io.npz.  (Fully random planes at 1080p are the GPU tests' business, against tests/pixfmt_ref.py, which
tests/test_pixfmt_host.py pins to this file.)  Output: tests/golden/frame_io_hbd.npz (arrays only).

    python tests/golden/make_golden_pixfmt.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SIZES = (("a", (36, 50)), ("b", (16, 32)), ("c", (70, 98)))
BITS = (10, 12, 16)


def runs(rng, shape, draw, longest):
    """an array of `shape` whose rows are runs of 1 .. longest equal values, each value one draw(n) sample"""
    h, w = shape
    rows = []
    for _ in range(h):
        lengths = rng.integers(1, longest + 1, w)
        lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), w)) + 1]
        rows.append(np.repeat(draw(len(lengths)), lengths)[:w])
    return np.stack(rows)


def main():
    import ref_harness
    sys.path.insert(0, os.path.join(ref_harness.REF_ROOT, "DCVC-family", "DCVC-FM"))
    sys.dont_write_bytecode = True
    from src.transforms.functional import ycbcr420_to_444, ycbcr444_to_420
    from src.utils.video_reader import YUVReader
    from src.utils.video_writer import YUVWriter
    rng = np.random.default_rng(2025)
    out = {}
    tmp = tempfile.mkdtemp()
    for tag, (h, w) in SIZES:
        rec = None
        for chroma in (444, 420):
            ch, cw = (h, w) if chroma == 444 else (h // 2, w // 2)
            longest = 1 if tag == "b" else 16
            base = [runs(rng, s, lambda n: rng.integers(0, 65536, n, dtype=np.uint16), longest) for s in ((h, w), (ch, cw), (ch, cw))]
            base[0][0, :4] = (0, 65535, 1 << 15, (1 << 15) - 1)
            out[f"src_{tag}_{chroma}"] = np.concatenate([p.ravel() for p in base])
            for bits in BITS:
                path = os.path.join(tmp, f"{tag}_{chroma}_{bits}.yuv")
                with open(path, "wb") as f:
                    for p in base:
                        f.write((p >> (16 - bits)).astype("<u2").tobytes())
                reader = YUVReader(path, w, h, src_format=str(chroma), bit_depth=bits)
                y, uv = reader.read_one_frame(str(chroma))
                reader.close()
                frame = ycbcr420_to_444(y, uv) if chroma == 420 else np.concatenate((y, uv), axis=0)
                assert frame.dtype == np.float32 and frame.shape == (3, h, w)
                out[f"frame_{tag}_{chroma}_{bits}"] = frame
                if rec is None:
                    rec = np.stack([runs(rng, (h, w), lambda n: rng.uniform(-0.02, 1.02, n), longest) for _ in range(3)]).astype(np.float32)
                    rec[0, 1, :4] = (0.5, 0.25, 0.75, 1.0)
                    out[f"rec_{tag}"] = rec
                for name, x in (("f32", rec), ("f16", rec.astype(np.float16).astype(np.float32))):
                    path = os.path.join(tmp, f"out_{tag}_{chroma}_{bits}_{name}.yuv")
                    writer = YUVWriter(path, w, h, dst_format=str(chroma), bit_depth=bits)
                    if chroma == 420:
                        yy, cc = ycbcr444_to_420(x)
                        writer.write_one_frame(y=yy, uv=cc, src_format="420")
                    else:
                        writer.write_one_frame(y=x[:1], uv=x[1:], src_format="444")
                    writer.close()
                    a = np.fromfile(path, "<u2")
                    assert a.size == h * w + 2 * ch * cw
                    out[f"out_{tag}_{chroma}_{bits}_{name}"] = a.astype(np.uint16)
        frac = float(np.mean((rec < 0) | (rec > 1)))
        print(f"size {tag}: {100 * frac:.1f} % of the reconstruction outside [0, 1] ({100 * float(np.mean(rec < 0)):.1f} % below)")
    dst = os.path.join(HERE, "frame_io_hbd.npz")
    np.savez_compressed(dst, **out)
    print("wrote frame_io_hbd.npz:", len(out), "arrays,", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
