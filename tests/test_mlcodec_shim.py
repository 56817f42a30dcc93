"""Drop-in seam 3: opendcvc_amd.mlcodec_shim presents the API of the reference's pybind module
MLCodec_extensions_cpp (src/cpp/py_rans/py_rans.cpp:366-393) over the C ABI of libdcvc_amd.so.
  * known-answer tests against the streams the reference's own module produced (tests/golden/rans_kat.npz) - always run;
  * the boundary proven against the reference's real caller: every call the REFERENCE's DMCI / DMC (torch CPU fallback
    ops) made into the reference's own coder while coding three golden sequences (tests/golden/shim_trace.npz, written by
    tests/golden/make_golden_shim_trace.py), replayed through the shim, must return what the reference's coder returned."""
import hashlib
import json
import os

import numpy as np
import pytest

from opendcvc_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libdcvc_amd.so not built")


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "rans_kat.npz"))


def _packed(k):
    return ((k["sym"].astype(np.int32) << 8) + k["idx"]).astype(np.int16)


@pytest.mark.parametrize("two", [False, True])
def test_encoder_reproduces_reference_streams(kat, two):
    from opendcvc_amd import mlcodec_shim as M
    enc = M.RansEncoder()
    assert enc.add_cdf(kat["cdf"], kat["sizes"], kat["offsets"]) == 0
    enc.set_use_two_encoders(two)
    assert enc.get_use_two_encoders() is two
    p = _packed(kat)
    enc.reset()
    enc.encode_z(kat["z"], 0, 0, 6)
    enc.encode_y(p, 0)
    enc.encode_y(p[:777], 0)
    enc.encode_y(p[:0], 0)                                   # zero-length task
    enc.flush()
    out = enc.get_encoded_stream()
    assert out.dtype == np.uint8 and np.array_equal(out, kat[f"stream_two{int(two)}"])
    small = ((np.clip(kat["sym"], -2, 2).astype(np.int32) << 8) + kat["idx"]).astype(np.int16)
    for m in (64, 201):
        enc.reset()
        enc.encode_y(small[:m], 0)
        enc.flush()
        assert np.array_equal(enc.get_encoded_stream(), kat[f"stream_two{int(two)}_y{m}"])


@pytest.mark.parametrize("two", [False, True])
def test_decoder_reads_reference_streams(kat, two):
    from opendcvc_amd import mlcodec_shim as M
    dec = M.RansDecoder()
    assert dec.add_cdf(kat["cdf"], kat["sizes"], kat["offsets"]) == 0
    dec.set_use_two_decoders(two)
    assert dec.get_use_two_decoders() is two
    dec.set_stream(kat[f"stream_two{int(two)}"])
    dec.decode_z(kat["z"].size, 0, 0, 6)
    z = dec.get_decoded_tensor()
    assert z.dtype == np.int8 and np.array_equal(z, kat["z"])
    dec.decode_y(kat["idx"], 0)
    assert np.array_equal(dec.get_decoded_tensor(), kat["sym"].astype(np.int8))
    assert np.array_equal(dec.decode_and_get_y(kat["idx"][:777], 0), kat["sym"][:777].astype(np.int8))


def test_pmf_and_cdf_buffer(kat):
    from opendcvc_amd import mlcodec_shim as M
    for i in range(len(kat["pmf_len"])):
        n = int(kat["pmf_len"][i])
        got = M.pmf_to_quantized_cdf([float(v) for v in kat["pmf_in"][i][:n]], 16)
        assert isinstance(got, list) and got == [int(v) for v in kat["pmf_out"][i][:n + 1]]
    enc, dec = M.RansEncoder(), M.RansDecoder()
    for c in (enc, dec):
        assert c.add_cdf(kat["cdf"], kat["sizes"], kat["offsets"]) == 0
        assert c.add_cdf(kat["cdf"][:8], kat["sizes"][:8], kat["offsets"][:8]) == 1
        c.empty_cdf_buffer()
        assert c.add_cdf(kat["cdf"][:8], kat["sizes"][:8], kat["offsets"][:8]) == 0
    with pytest.raises(_lib.DcvcError):
        enc.add_cdf(kat["cdf"], kat["sizes"][:5], kat["offsets"])


def _digest(a):
    """tests/golden/make_golden_shim_trace.py: digest()"""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def reference_setup():
    """What the reference's DMCI / DMC hand their coder while they are set up (update()), rebuilt by the oracle's
    restatement of the same code with the same weights: the pmfs given to pmf_to_quantized_cdf, in order, and the CDF
    tables given to add_cdf that the trace holds by digest only (the factorised z tables).  Like
    test_oracle_nn.py::test_factorized_tables_match_reference, this relies on torch's CPU operators rounding as they did
    where the records were made (the reference computes these in fp32 with the same operators)."""
    import dcvc_oracle as O
    from opendcvc_amd import weights
    pmfs, tables = [], {}
    real = O.pmf_to_quantized_cdf

    def spy(pmf, precision=16):
        pmfs.append(np.asarray(pmf, np.float32))
        return real(pmf, precision)

    O.pmf_to_quantized_cdf = spy
    try:
        for cls, name in ((O.OracleDMCI, "dmci"), (O.OracleDMC, "dmc")):
            m = cls(weights.make_state_dict(name, 1234))
            m.update(0.12)
            for t in tuple(m.g_tables) + tuple(m.z_tables):
                t = np.ascontiguousarray(t, np.int32)
                tables[_digest(t)] = t
    finally:
        O.pmf_to_quantized_cdf = real
    return pmfs, tables


@pytest.mark.parametrize("name,args", [("seq_64", (64, 64, 7, 32, False, 4)), ("seq_64_two", (64, 64, 3, 21, True, 0)),
                                       ("seq_80x48", (48, 80, 3, 40, False, 0))])
def test_reference_models_run_on_the_shim(golden_dir, reference_setup, name, args):
    """The reference's own DMCI / DMC and entropy_models.py, entropy coding through mlcodec_shim: every call they made
    into the reference's coder while coding the sequence (tests/golden/make_golden_shim_trace.py), replayed in order
    through the shim, returns what the reference's coder returned - streams, decoded symbols, CDF group indices and
    every quantised CDF of the model set-up."""
    import torch
    from opendcvc_amd import mlcodec_shim as M
    trace = np.load(os.path.join(golden_dir, "shim_trace.npz"))
    meta = json.loads(str(trace[name + "__meta"]))
    h, w, n, qp, two, reset = args
    assert (meta["h"], meta["w"], meta["frames"], meta["qp"], meta["two"], meta["reset_interval"]) == (h, w, n, qp, int(two), reset)
    # the trace is that of the run the golden records were made from
    if name == "seq_64":
        want = json.loads(str(np.load(os.path.join(golden_dir, "seq_64.npz"))["meta"]))
    else:
        want = json.load(open(os.path.join(golden_dir, "sequences.json")))[name]
    assert meta["frame_sha256"] == [f["sha256"] for f in want["frames"]]

    pmfs, tables = reference_setup
    pmf_iter = iter(pmfs)

    def arg(v):
        if v["k"] in ("none", "bool", "int", "float"):
            return v.get("v")
        if "sha" in v:
            assert v["sha"] in tables, "the oracle's CDF tables are not the reference's"
            a = tables[v["sha"]]
        else:
            a = trace["%s__%s" % (name, v["a"])]
        return {"np": lambda: a, "torch": lambda: torch.from_numpy(a.copy()), "list": a.tolist,
                "bytes": a.tobytes}[v["k"]]()

    objs = {}
    kinds = set()
    for c in meta["calls"]:
        if c["m"] == "pmf_to_quantized_cdf":
            h_in, h_out = hashlib.sha256(), hashlib.sha256()
            for _ in range(c["count"]):
                p = next(pmf_iter).astype(np.float64)
                h_in.update(np.int64(p.size).tobytes() + p.tobytes())
                r = np.asarray(M.pmf_to_quantized_cdf(p.tolist(), c["precision"]), np.int64)
                h_out.update(np.int64(r.size).tobytes() + r.tobytes())
            assert h_in.hexdigest() == c["in_sha256"], "the oracle's pmfs are not the reference's"
            assert h_out.hexdigest() == c["out_sha256"], "pmf_to_quantized_cdf differs from the reference's"
            continue
        if c["o"] not in objs:
            objs[c["o"]] = (M.RansEncoder if c["o"][0] == "E" else M.RansDecoder)()
        got = getattr(objs[c["o"]], c["m"])(*[arg(v) for v in c["args"]])
        kinds.add(c["m"])
        want_ret = c["ret"]
        if want_ret["k"] == "none":
            assert got is None, c["m"]
        elif want_ret["k"] in ("bool", "int"):
            assert got == want_ret["v"] and type(got) is type(want_ret["v"]), c["m"]
        else:
            ref = arg(want_ret)
            got = np.asarray(got)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), c["m"]
    assert next(pmf_iter, None) is None                 # every pmf of the set-up was replayed
    assert {"add_cdf", "encode_y", "encode_z", "get_encoded_stream", "decode_y", "decode_z", "get_decoded_tensor"} <= kinds
