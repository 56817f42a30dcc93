"""Deinterlacing in front of the encoder (docs/deinterlace.md; csrc/dcvc_deint.hip): an interlaced source frame - two fields
woven into one picture - becomes a progressive picture at the same frame rate before anything else looks at it.  The first
field's rows are kept bit for bit, the second field's are rebuilt from the current and the previous frame - or, in film mode
(csrc/dcvc_fieldmatch.hip), taken from wherever the matching field lies.  No reference counterpart: the reference codes the
comb.  tests/deint_ref.py and tests/fieldmatch_ref.py restate the kernels in numpy.  At field rate (rate="field";
csrc/dcvc_deint_field.hip, tests/deint_field_ref.py) every source frame gives TWO pictures, one per field, a frame behind."""
import ctypes

MODES = ("on", "auto", "film")
ORDERS = ("tff", "bff")
RATES = ("frame", "field")


def check_deinterlace(mode, order="tff"):
    """run_one_point's deinterlace / field_order -> (mode or None, keep_parity); ValueError under the option's name, also for a
    field_order that is set while deinterlace is not"""
    if order not in ORDERS:
        raise ValueError(f"field_order {order!r}: one of {', '.join(ORDERS)}")
    if mode is None:
        if order != "tff":
            raise ValueError(f"field_order {order!r} is the field order of deinterlace: it has no effect without it")
        return None, 0
    if mode not in MODES:
        raise ValueError(f"deinterlace {mode!r}: None or one of {', '.join(MODES)}")
    return mode, ORDERS.index(order)


def check_rate(rate, mode):
    """run_one_point's deint_rate beside its (checked) deinterlace -> "frame" or "field"; None is "frame", today's one picture
    per frame; "field" needs deinterlace "on".  ValueError under the option's name"""
    if rate is None:
        return "frame"
    if rate not in RATES:
        raise ValueError(f"deint_rate {rate!r}: None or one of {', '.join(RATES)}")
    if rate == "field" and mode != "on":
        raise ValueError(f"deint_rate 'field' is the field-rate output of deinterlace 'on': it cannot go with deinterlace {mode!r}")
    return rate


def check_height(height, chroma_lines, name="deinterlace"):
    """two fields of whole lines: the height is a multiple of 2 * chroma_lines"""
    if chroma_lines not in (1, 2):
        raise ValueError(f"{name}: chroma_lines {chroma_lines!r} is not 1 or 2")
    if height <= 0 or height % (2 * chroma_lines):
        raise ValueError(f"{name}: height {height} is not a multiple of {2 * chroma_lines} (two fields of "
                         f"{chroma_lines}-row lines)")


class Deinterlacer:
    """Deinterlacer(device, mode="on" | "auto" | "film", order="tff" | "bff", chroma_lines=1, rate="frame" | "field").  order: the
    field whose rows are kept (tff: the even lines); chroma_lines: rows per chroma line of the model frame - 2 where the loader
    doubled the rows of a 4:2:0 source, else 1.  rate "frame": filter(), a picture per frame; "field" (mode "on" only):
    fields() and drain(), two pictures per frame.

    filter(x, size) -> a NEW tensor of x's shape: the size = (H, W) picture of the model frame x [1, 3, Hp, Wp] deinterlaced,
    with its replicate pad.  "on" filters every frame; "auto" asks dcvc_comb_detect first and a frame found progressive
    passes bit for bit - the decision stays on the device, the filter's launch reads it there, and the call waits for nothing.
    The first frame, the first one after reset(), and a frame whose size, shape or dtype differs from the one before it have
    no previous frame (the spatial predictor alone; auto's weaker rule).  "film" asks dcvc_field_match which field completes
    the kept one: the frame's own - it passes bit for bit -, the previous frame's - dcvc_field_weave puts its rows in - or
    neither - the filter, as with "on".  Its two decision words stay on the device in the same way.

    The object HOLDS the previous INPUT tensor, it does not copy it: the caller must not overwrite a tensor it has passed to
    filter() before the next call (the harness's loader allocates a tensor per frame).

    fields(x, size) -> a list of NEW tensors, at field rate (docs/deinterlace.md, "Field-rate output"): [A_0] on the first call,
    [B_(m-1), A_m] on later ones - A_m is filter()'s picture of frame m, B_(m-1) the picture of frame m - 1's second field, which
    needs frame m.  drain() -> [B_last], or [] with nothing pending; afterwards the object is as after reset(), which drops a
    pending picture.  A frame whose size, shape or dtype differs from the one before it still gives two pictures, both from
    the spatial predictor alone.  At field rate the object holds the last TWO input tensors in the same way: the caller must
    not overwrite a tensor it has passed to fields() before the second call after it, or drain().  pictures: the pictures
    handed out so far.  filter() at field rate and fields() / drain() at frame rate are ValueErrors.

    counts() -> (frames judged, frames found interlaced) of mode "auto", (frames judged, frames filtered) of mode "film", ONE
    read-back, for the log after the pass; matches() -> (passed, woven, filtered) of mode "film", likewise; frames: the calls
    of filter() so far."""

    def __init__(self, device="cuda:0", mode="on", order="tff", chroma_lines=1, rate="frame"):
        import torch
        from . import _lib
        self.mode, self.parity = check_deinterlace(mode, order)
        if self.mode is None:
            raise ValueError("deinterlace None: a Deinterlacer is not made where the option is off")
        self.rate = check_rate(rate, self.mode)
        if chroma_lines not in (1, 2):
            raise ValueError(f"chroma_lines {chroma_lines!r} is not 1 or 2")
        self.order, self.chroma_lines = order, int(chroma_lines)
        self.device = torch.device(device)
        self._lib = _lib.lib()
        self._ws = None
        if self.mode == "auto":          # the workspace and, behind it, the decision word (zero once: every call leaves its sums zero)
            need = _lib.check(self._lib.dcvc_comb_ws_bytes(), "dcvc_comb_ws_bytes")
            self._ws = torch.zeros(need + 8, dtype=torch.uint8, device=self.device)
            self._decision = ctypes.c_void_p(self._ws.data_ptr() + need)
        if self.mode == "film":          # the same, with two words behind it: filter, weave
            need = _lib.check(self._lib.dcvc_field_match_ws_bytes(), "dcvc_field_match_ws_bytes")
            self._ws = torch.zeros(need + 8, dtype=torch.uint8, device=self.device)
            self._decision = ctypes.c_void_p(self._ws.data_ptr() + need)
            self._weave = ctypes.c_void_p(self._ws.data_ptr() + need + 4)
        self._prev = None                # (tensor, size) of the last input
        self._before = None              # field rate: the same of the input before it, while _prev's second picture is pending
        self.frames = self.pictures = 0

    def reset(self):
        self._prev = self._before = None

    def filter(self, x, size):
        if self.rate != "frame":
            raise ValueError("filter() is the frame-rate call: a field-rate Deinterlacer has fields() and drain()")
        return self._first(x, size)

    @staticmethod
    def _like(a, b):
        """two (tensor, size) records, either may be None: may the one be the other's neighbour in a launch"""
        return a is not None and b is not None and a[1] == b[1] and a[0].shape == b[0].shape and a[0].dtype == b[0].dtype

    def _second(self, after):
        """B of the pending frame _prev between _before and after (a record or None): ONE launch of dcvc_deinterlace_field"""
        import torch
        from . import _lib
        from . import nn as L
        x, size = self._prev
        both = self._like(self._before, self._prev) and self._like(self._prev, after)
        out = torch.empty_like(x)
        args = L.frame_args(x, size)
        _lib.check(self._lib.dcvc_deinterlace_field(args[0], L._p(self._before[0]) if both else None, args[1],
                                                    L._p(after[0]) if both else None, *args[2:], self.parity, self.chroma_lines,
                                                    L._p(out), L._stream(self.device)), "dcvc_deinterlace_field")
        self.pictures += 1
        return out

    def _field_rate(self, name):
        if self.rate != "field":
            raise ValueError(f"{name}() is a field-rate call: make the Deinterlacer with rate='field'")

    def fields(self, x, size):
        from . import nn as L
        self._field_rate("fields")
        size = (int(size[0]), int(size[1]))
        check_height(size[0], self.chroma_lines)
        x = L.frame(x)
        pending = self._prev
        out = [self._second((x, size))] if pending is not None else []
        out.append(self._first(x, size))             # (makes x the pending frame)
        self._before = pending
        return out

    def drain(self):
        self._field_rate("drain")
        out = [self._second(None)] if self._prev is not None else []
        self.reset()
        return out

    def _first(self, x, size):
        import torch
        from . import _lib
        from . import nn as L
        size = (int(size[0]), int(size[1]))
        check_height(size[0], self.chroma_lines)
        x = L.frame(x)
        prev = self._prev
        if prev is not None and (prev[1] != size or prev[0].shape != x.shape or prev[0].dtype != x.dtype):
            prev = None
        p = L._p(prev[0]) if prev is not None else None
        out = torch.empty_like(x)
        st = L._stream(self.device)
        args = L.frame_args(x, size)
        decision = None
        if self.mode == "auto":
            decision = self._decision
            _lib.check(self._lib.dcvc_comb_detect(args[0], args[1], p, *args[2:], self.parity, L._p(self._ws), decision, st),
                       "dcvc_comb_detect")
        if self.mode == "film":
            decision = self._decision
            _lib.check(self._lib.dcvc_field_match(args[0], args[1], p, *args[2:], self.parity, L._p(self._ws), decision, st),
                       "dcvc_field_match")
        _lib.check(self._lib.dcvc_deinterlace(args[0], args[1], p, *args[2:], self.parity, self.chroma_lines, decision,
                                              L._p(out), st), "dcvc_deinterlace")
        if self.mode == "film" and p is not None:
            _lib.check(self._lib.dcvc_field_weave(args[0], p, *args[2:], self.parity, self.chroma_lines, self._weave, L._p(out),
                                                  st), "dcvc_field_weave")
        self._prev = (x, size)
        self.frames += 1
        self.pictures += 1
        return out

    def counts(self):
        import numpy as np
        if self._ws is None:
            return (0, 0)
        if self.mode == "film":
            judged, _, _, filtered = self._film_words()
            return judged, filtered
        words = self._ws.cpu().numpy()[:64].view(np.uint64)
        return int(words[3]), int(words[4])

    def _film_words(self):
        """dcvc_field_match's running counters: judged, passed, woven, filtered"""
        import numpy as np
        return [int(w) for w in self._ws.cpu().numpy()[:64].view(np.uint32)[4:8]]

    def matches(self):
        """(frames passed, frames woven, frames filtered) of mode 'film'; (0, 0, 0) in the other modes"""
        return tuple(self._film_words()[1:]) if self.mode == "film" else (0, 0, 0)

    def filtered(self):
        """the frames that went through the filter: every frame with 'on', those found interlaced with 'auto', those
        that matched neither field with 'film'; at field rate the pictures"""
        if self.rate == "field":
            return self.pictures
        return self.frames if self.mode == "on" else self.counts()[1]
