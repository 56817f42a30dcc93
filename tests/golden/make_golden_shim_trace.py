"""Generates shim_trace.npz: every call the REFERENCE's models make into their host-coder module MLCodec_extensions_cpp
(the reference's own rANS coder, compiled into oracle/_ref) while they code the golden sequences seq_64, seq_64_two and
seq_80x48 - method, arguments and what the reference coder returned.  tests/test_mlcodec_shim.py replays the calls
through opendcvc_amd.mlcodec_shim and requires the same results: what the reference's DMCI / DMC would see if the shim
were registered in the reference coder's place.

    python tests/golden/make_golden_shim_trace.py

Only data is written (call names, numbers, arrays); the run is checked against the golden records first.  The model
set-up is kept small: a run of consecutive pmf_to_quantized_cdf calls becomes one entry with the SHA-256 of its inputs and
of the reference's outputs, and an array above INLINE_BYTES (the factorised CDF tables) is kept as its SHA-256 only -
the test rebuilds both with the oracle's restatement of the reference's table code and checks them against the digests.
The GPU box never runs this script.
"""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
import ref_harness  # noqa: E402

# name -> (h, w, frames, qp, two coders, reset interval): the cases of test_reference_models_run_on_the_shim
CASES = {"seq_64": (64, 64, 7, 32, False, 4), "seq_64_two": (64, 64, 3, 21, True, 0), "seq_80x48": (48, 80, 3, 40, False, 0)}
INLINE_BYTES = 64 * 1024


def digest(a):
    """SHA-256 of an array's dtype, shape and bytes (tests/test_mlcodec_shim.py computes the same)"""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def compact(calls, arrays):
    """(calls, arrays) -> (calls, arrays kept inline): pmf runs folded into digests, large arrays by digest only"""
    out, keep = [], {}

    def ref(v):
        if "a" not in v:
            return v
        a = arrays[v["a"]]
        if a.nbytes > INLINE_BYTES:
            return {"k": v["k"], "sha": digest(a)}
        keep[v["a"]] = a
        return v

    for c in calls:
        if c["m"] == "pmf_to_quantized_cdf":
            pmf, precision, ret = arrays[c["args"][0]["a"]], c["args"][1]["v"], arrays[c["ret"]["a"]]
            if not (out and out[-1]["m"] == "pmf_to_quantized_cdf" and out[-1]["precision"] == precision):
                out.append({"o": "M", "m": "pmf_to_quantized_cdf", "precision": precision, "count": 0,
                            "h_in": hashlib.sha256(), "h_out": hashlib.sha256()})
            run = out[-1]
            run["count"] += 1
            for h, a in ((run["h_in"], np.asarray(pmf, np.float64)), (run["h_out"], np.asarray(ret, np.int64))):
                h.update(np.int64(a.size).tobytes() + a.tobytes())
            continue
        out.append(dict(c, args=[ref(v) for v in c["args"]], ret=ref(c["ret"])))
    for c in out:
        if c["m"] == "pmf_to_quantized_cdf":
            c["in_sha256"], c["out_sha256"] = c.pop("h_in").hexdigest(), c.pop("h_out").hexdigest()
    return out, keep


class Recorder:
    """Call log; arrays are stored once per distinct content."""

    def __init__(self):
        self.calls, self.arrays, self._seen = [], {}, {}
        self.count = {"E": 0, "D": 0}

    def _array(self, a):
        a = np.ascontiguousarray(a)
        h = digest(a)
        if h not in self._seen:
            self._seen[h] = "a%d" % len(self._seen)
            self.arrays[self._seen[h]] = a.copy()
        return self._seen[h]

    def value(self, v):
        if v is None:
            return {"k": "none"}
        if isinstance(v, torch.Tensor):
            return {"k": "torch", "a": self._array(v.detach().cpu().numpy())}
        if isinstance(v, np.ndarray):
            return {"k": "np", "a": self._array(v)}
        if isinstance(v, (bool, np.bool_)):
            return {"k": "bool", "v": bool(v)}
        if isinstance(v, (int, np.integer)):
            return {"k": "int", "v": int(v)}
        if isinstance(v, (float, np.floating)):
            return {"k": "float", "v": float(v)}
        if isinstance(v, (bytes, bytearray)):
            return {"k": "bytes", "a": self._array(np.frombuffer(bytes(v), np.uint8))}
        if isinstance(v, (list, tuple)):
            a = np.asarray(v)
            assert a.dtype.kind in "if", type(v[0]) if len(v) else "empty list"
            return {"k": "list", "a": self._array(a)}
        raise TypeError("unrecorded type %s" % type(v))

    def module(self, R):
        rec = self

        def proxy(cls, tag):
            class Proxy:
                def __init__(self):
                    self._obj = cls()
                    self._id = "%s%d" % (tag, rec.count[tag])
                    rec.count[tag] += 1

                def __getattr__(self, name):
                    fn = getattr(self._obj, name)

                    def call(*args):
                        entry = {"o": self._id, "m": name, "args": [rec.value(a) for a in args]}
                        r = fn(*args)
                        entry["ret"] = rec.value(r)
                        rec.calls.append(entry)
                        return r
                    return call
            return Proxy

        def pmf_to_quantized_cdf(pmf, precision):
            entry = {"o": "M", "m": "pmf_to_quantized_cdf", "args": [rec.value(pmf), rec.value(precision)]}
            r = R.pmf_to_quantized_cdf(pmf, precision)
            entry["ret"] = rec.value(r)
            rec.calls.append(entry)
            return r

        mod = types.ModuleType("MLCodec_extensions_cpp")
        mod.RansEncoder, mod.RansDecoder = proxy(R.RansEncoder, "E"), proxy(R.RansDecoder, "D")
        mod.pmf_to_quantized_cdf = pmf_to_quantized_cdf
        return mod


def main():
    if not ref_harness.available():
        sys.exit("the reference is not present")
    DMC, DMCI, _, _, R, _ = ref_harness.load(coder="reference")
    assert R.__name__ == "MLCodec_extensions_cpp" and "shim" not in getattr(R, "__file__", "")
    torch.set_grad_enabled(False)
    seqs = json.load(open(os.path.join(HERE, "sequences.json")))
    out = {}
    for name, (h, w, n, qp, two, reset) in CASES.items():
        rec = Recorder()
        sys.modules["MLCodec_extensions_cpp"] = rec.module(R)
        try:
            i_net, p_net = make_golden.load_models(DMC, DMCI)
            got, _ = make_golden.run_sequence(i_net, p_net, h, w, n, qp, two, reset, False)
        finally:
            sys.modules["MLCodec_extensions_cpp"] = R
        want = (json.loads(str(np.load(os.path.join(HERE, "seq_64.npz"))["meta"])) if name == "seq_64" else seqs[name])
        for fi, (g, f) in enumerate(zip(got["frames"], want["frames"])):
            assert (g["bytes"], g["sha256"]) == (f["bytes"], f["sha256"]), (name, fi)
        calls, keep = compact(rec.calls, rec.arrays)
        meta = dict(h=h, w=w, frames=n, qp=qp, two=int(two), reset_interval=reset, calls=calls,
                    frame_sha256=[g["sha256"] for g in got["frames"]])
        out[name + "__meta"] = np.array(json.dumps(meta))
        for k, a in keep.items():
            out["%s__%s" % (name, k)] = a
        print(name, len(rec.calls), "calls ->", len(calls), "entries,", len(keep), "arrays inline,",
              sum(a.nbytes for a in keep.values()), "bytes")
    np.savez_compressed(os.path.join(HERE, "shim_trace.npz"), **out)
    print("wrote", os.path.join(HERE, "shim_trace.npz"))


if __name__ == "__main__":
    main()
