"""Generates rans_random.npz: random inputs through the REFERENCE's own rANS coder (compiled into oracle/_ref), with
the reference's gaussian tables (gauss_cdf.npz) - the record tests/test_oracle_rans.py::test_against_reference_build_random
checks the oracle's coder against.

    python tests/golden/make_golden_rans_random.py

Only data is written: for each case (one / two coders, 1000 / 50001 symbols) the packed symbols (int16: symbol << 8 |
table index) and the stream the reference wrote for them.  The GPU box never runs this script.
"""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CASES = [(two, n) for two in (False, True) for n in (1000, 50001)]


def main():
    ref_dir = os.path.join(REPO, "oracle", "_ref")
    if not glob.glob(os.path.join(ref_dir, "MLCodec_extensions_cpp*.so")):
        sys.exit("oracle/_ref not built (make -C oracle ref, with the reference present)")
    sys.path.insert(0, ref_dir)
    import MLCodec_extensions_cpp as R
    t = np.load(os.path.join(HERE, "gauss_cdf.npz"))
    g = (t["cdf"], t["length"], t["offset"])
    rng = np.random.default_rng(3)
    out = {}
    for two, n in CASES:
        idx = rng.integers(0, 128, n).astype(np.uint8)
        sigma = 0.11 * (16 / 0.11) ** (idx / 127.0)
        sym = np.clip(np.round(rng.standard_normal(n) * sigma), -128, 127).astype(np.int16)
        p = ((sym.astype(np.int32) << 8) + idx).astype(np.int16)
        enc = R.RansEncoder()
        enc.add_cdf(*g)
        enc.set_use_two_encoders(two)
        enc.reset()
        enc.encode_y(p, 0)
        enc.flush()
        key = "two%d_n%d" % (int(two), n)
        out[key + "_packed"] = p
        out[key + "_stream"] = np.array(enc.get_encoded_stream(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "rans_random.npz"), **out)
    print("wrote", os.path.join(HERE, "rans_random.npz"))


if __name__ == "__main__":
    main()
