"""Motion-compensated temporal pre-filter of the encoder's input (docs/temporal_filter.md, csrc/dcvc_tf.hip; no reference
counterpart): every frame is blended with up to four of its unfiltered neighbours, each gathered block by block at the vector
an integer-pyramid motion search finds for it, with weights that fall to zero where the neighbour does not match.  Encoder
side only - the stream and the decoder know nothing of it.  The arithmetic is integer up to one fp32 blend per sample; the
kernels and the numpy restatement tests/tf_ref.py agree bit for bit.  Level "auto": the level is chosen per frame on the device
from a noise estimate of the picture and never read back (tests/tf_auto_ref.py restates it).  subpel 1 / 2: the vectors are refined
to half / quarter pels and the blend interpolates its reference samples (csrc/dcvc_tf_subpel.hip, tests/tf_subpel_ref.py)."""
import ctypes

LEVELS = (1, 2, 3, 4, 5)                               # strength: T = 4 << level 10-bit codes
RADII = (1, 2)
MAX_REFS = 4
AUTO = "auto"                                          # the level chosen per frame from the picture's noise
SUBPELS = (0, 1, 2)                                    # the vectors' precision: whole, half, quarter pels


def check_options(level, radius):
    """(level, radius) as integers; level 0 (off) .. 5 or "auto", radius 1 or 2"""
    auto = isinstance(level, str) and level == AUTO
    if not auto and (isinstance(level, bool) or not isinstance(level, int) or not 0 <= level <= LEVELS[-1]):
        raise ValueError(f"temporal filter level {level!r}: 0 (off) .. {LEVELS[-1]}")
    if isinstance(radius, bool) or radius not in RADII:
        raise ValueError(f"temporal filter radius {radius!r}: 1 or 2")
    return (AUTO if auto else level), int(radius)


def check_subpel(subpel):
    """subpel as an integer: 0 (whole-pel vectors), 1 (refined to half pels) or 2 (to quarter pels)"""
    if isinstance(subpel, bool) or subpel not in SUBPELS:
        raise ValueError(f"temporal filter subpel {subpel!r}: 0, 1 or 2")
    return int(subpel)


def window(n_frames, radius):
    """for every frame t of an n_frames sequence the (index, distance) list of its references in accumulation order
    (distance -1, +1, -2, +2, those inside the sequence).  Pure."""
    n_frames, radius = int(n_frames), int(radius)
    if n_frames < 0 or radius not in RADII:
        raise ValueError(f"window({n_frames}, {radius}): a frame count >= 0 and radius 1 or 2")
    return [_refs_of(t, n_frames, radius) for t in range(n_frames)]


def _refs_of(t, n_frames, radius):
    return [(t + d, d) for k in range(1, radius + 1) for d in (-k, k) if 0 <= t + d < n_frames]


class TemporalFilter:
    """The filter on `device` at strength `level` (1 .. 5, or "auto": chosen per frame from a noise estimate that stays on the
    device) with references up to `radius` (1, 2) frames away, at vectors of whole pels (`subpel` 0) or refined to half (1) or
    quarter pels (2).
    filter() and motion() are stateless; push() / flush() run a sequence through a ring of 2 * radius + 1 source frames whose
    pyramids are made once per frame.  Everything is sized at the first frame (and again if the frames change shape) and
    nothing is allocated per frame; all work is enqueued on the current stream and nothing is waited for, except by
    weight_sum(), levels() and noise().  A frame push() / flush() returns lives in one of radius + 1 buffers of the object: it holds until radius + 1
    further frames have come out."""

    def __init__(self, device="cuda:0", level=3, radius=2, subpel=0):
        import torch
        level, radius = check_options(level, radius)
        self.subpel = check_subpel(subpel)
        if level == 0:
            raise ValueError("temporal filter level 0 is 'off': make no TemporalFilter")
        self.device, self.level, self.radius = torch.device(device), level, radius
        self._total = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._levels = torch.zeros(8, dtype=torch.int64, device=self.device)        # six level counts, the sum of N, the frames
        self._result = torch.zeros(4, dtype=torch.int32, device=self.device)        # level, N, temporal, spatial of the last estimate
        self._noise_ws = None
        self._key = None
        self.reset()

    # ------------------------------------------------------------------------------ sizing
    @staticmethod
    def _frame(x):
        from . import nn as L
        return L.frame(x)

    def _size(self, x, size):
        """buffers for frames like x with the picture size = (H, W)"""
        import torch
        from . import _lib
        H, W = (int(v) for v in size)
        key = (tuple(x.shape), x.dtype, H, W)
        if key == self._key:
            return
        if H < 1 or W < 1 or H > x.shape[2] or W > x.shape[3]:
            raise ValueError(f"a {H} x {W} picture does not lie in a frame of {x.shape[2]} x {x.shape[3]}")
        L = _lib.lib()
        n = 2 * self.radius + 1
        dev = self.device
        gh, gw = (H + 7) // 8, (W + 7) // 8
        self._ring = torch.empty((n,) + tuple(x.shape), dtype=x.dtype, device=dev)
        self._out = torch.empty((self.radius + 1,) + tuple(x.shape), dtype=x.dtype, device=dev)
        self._pyr_elems = L.dcvc_tf_pyramid_bytes(H, W) // 2
        self._pyr = torch.empty((n + 1 + MAX_REFS, self._pyr_elems), dtype=torch.int16, device=dev)      # the ring's, then filter()'s own
        self._ws = torch.empty(max(L.dcvc_tf_motion_ws_bytes(H, W), 1), dtype=torch.uint8, device=dev)
        self._mv = torch.empty((MAX_REFS, gh, gw, 2), dtype=torch.int16, device=dev)
        self._err = torch.empty((MAX_REFS, gh, gw), dtype=torch.int32, device=dev)
        # what _noise() and _blend() read: the search's own outputs, or (subpel, filter()'s motions) these two
        self._mvq = torch.empty_like(self._mv) if self.subpel else None
        self._errq = torch.empty_like(self._err) if self.subpel else None
        if self._noise_ws is None:
            self._noise_ws = torch.empty(L.dcvc_tf_noise_ws_bytes(), dtype=torch.uint8, device=dev)
        self._key = key
        self.reset()

    def reset(self):
        """forgets the frames pushed so far and zeroes the weight sum and the levels' totals; the buffers stay"""
        self._pushed = self._emitted = 0
        self._size_of_sequence = None
        self._total.zero_()
        self._levels.zero_()

    # ------------------------------------------------------------------------------ the kernels
    def _pyramid(self, x, size, slot):
        from . import _lib
        from . import nn as L
        _lib.check(_lib.lib().dcvc_tf_pyramid(*L.frame_args(x, size), L._p(self._pyr[slot]), L._stream()), "dcvc_tf_pyramid")

    def _motion(self, cur_slot, ref_slots, size):
        from . import _lib
        from . import nn as L
        n = len(ref_slots)
        pyrs = (ctypes.c_void_p * n)(*[self._pyr[s].data_ptr() for s in ref_slots])
        _lib.check(_lib.lib().dcvc_tf_motion(L._p(self._pyr[cur_slot]), pyrs, n, size[0], size[1], L._p(self._mv), L._p(self._err),
                                             L._p(self._ws), L._stream()), "dcvc_tf_motion")
        if self.subpel:
            _lib.check(_lib.lib().dcvc_tf_refine(L._p(self._pyr[cur_slot]), pyrs, n, size[0], size[1], self.subpel, L._p(self._mv),
                                                 L._p(self._err), L._p(self._mvq), L._p(self._errq), L._stream()), "dcvc_tf_refine")

    def _search(self, cur, refs, size):
        """filter()'s own slots: the pyramid of cur into slot n = 2 * radius + 1, those of refs into n + 1 .., and _motion()
        of cur on them (none without a reference) -> n"""
        n = 2 * self.radius + 1
        self._pyramid(cur, size, n)
        for i, r in enumerate(refs):
            self._pyramid(r, size, n + 1 + i)
        if refs:
            self._motion(n, [n + 1 + i for i in range(len(refs))], size)
        return n

    def _noise(self, cur_slot, dists, size, totals):
        """the estimate of the frame whose pyramid is in cur_slot, after _motion() on its references -> self._result"""
        from . import _lib
        from . import nn as L
        n = len(dists)
        _lib.check(_lib.lib().dcvc_tf_noise(L._p(self._pyr[cur_slot]), L._p(self._errq if self.subpel else self._err), (ctypes.c_int * max(n, 1))(*dists), n, size[0],
                                            size[1], L._p(self._noise_ws), L._p(self._result), L._p(self._levels) if totals else None,
                                            L._stream()), "dcvc_tf_noise")

    def _blend(self, cur, refs, dists, size, out):
        """at the object's level; "auto": at the level _noise() left in self._result (a frame without references is a copy)"""
        from . import _lib
        from . import nn as L
        n = len(refs)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[r.data_ptr() for r in refs])
        code, cur_p, Hp, Wp, H, W = L.frame_args(cur, size)
        tail = (L._p(out), L._p(self._total), L._stream())
        if self.subpel:
            auto = self.level == AUTO and n
            _lib.check(_lib.lib().dcvc_tf_blend_subpel(code, cur_p, ptrs, (ctypes.c_int * max(n, 1))(*dists), n, Hp, Wp, H, W,
                                                       L._p(self._mvq), L._p(self._errq), LEVELS[0] if self.level == AUTO else self.level,
                                                       L._p(self._result) if auto else None, *tail), "dcvc_tf_blend_subpel")
            return
        head = (code, cur_p, ptrs, (ctypes.c_int * max(n, 1))(*dists), n, Hp, Wp, H, W, L._p(self._mv), L._p(self._err))
        if self.level == AUTO and n:
            _lib.check(_lib.lib().dcvc_tf_blend_auto(*head, L._p(self._result), *tail), "dcvc_tf_blend_auto")
        else:
            _lib.check(_lib.lib().dcvc_tf_blend(*head, LEVELS[0] if self.level == AUTO else self.level, *tail), "dcvc_tf_blend")

    def _check(self, cur, refs, dists, size):
        cur = self._frame(cur)
        refs = [self._frame(r) for r in refs]
        dists = [int(d) for d in dists]
        if len(refs) != len(dists) or len(refs) > MAX_REFS:
            raise ValueError(f"{len(refs)} references with {len(dists)} distances: at most {MAX_REFS}, one distance each")
        if any(d not in (-2, -1, 1, 2) for d in dists):
            raise ValueError(f"distances {dists}: each -2, -1, 1 or 2")
        if any(r.shape != cur.shape or r.dtype != cur.dtype for r in refs):
            raise ValueError("the references must have the current frame's shape and type")
        return cur, refs, dists, tuple(int(v) for v in size)

    # ------------------------------------------------------------------------------ stateless
    def filter(self, cur, refs, dists, size, out=None, motions=None):
        """cur filtered against refs (accumulated in the order given; dists: their distances, +-1 / +-2) on its
        size = (H, W) picture, replicate-padded to cur's shape.  out: None (a new tensor) or a contiguous tensor like cur that
        overlaps no input.  Adds to the weight sum (level "auto": and to the levels' totals).  Frames of another shape, type or
        picture size than the object's current ones make it size its buffers anew, which is a reset().  motions: None, or per
        reference the (vectors, errors) to use instead of searching - tensors like motion()'s of a subpel 0 object,
        like motion_subpel()'s (quarter pels) otherwise."""
        import torch
        cur, refs, dists, size = self._check(cur, refs, dists, size)
        if motions is not None and len(motions) != len(refs):
            raise ValueError(f"{len(motions)} motions for {len(refs)} references")
        if out is None:
            out = torch.empty_like(cur)
        elif out.shape != cur.shape or out.dtype != cur.dtype or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor of cur's shape and type")
        self._size(cur, size)
        n = 2 * self.radius + 1
        if refs:
            if motions is None:
                self._search(cur, refs, size)
            else:
                if self.level == AUTO:
                    self._pyramid(cur, size, n)
                mv, err = (self._mvq, self._errq) if self.subpel else (self._mv, self._err)
                for i, (v, e) in enumerate(motions):
                    mv[i].copy_(v)
                    err[i].copy_(e)
            if self.level == AUTO:
                self._noise(n, dists, size, True)
        self._blend(cur, refs, dists, size, out)
        return out

    def noise(self, cur, refs, dists, size):
        """the estimate of cur against refs (dists: their distances; none: the spatial table alone) as Python ints
        (level, N, the smallest temporal figure or -1, the spatial figure); adds to no total; one read-back.  Like filter(),
        motion() and pyramid() it keeps no frame, but frames of another shape, type or picture size than the object's current
        ones make it size its buffers anew, which is a reset(): a push() sequence under way and the totals are dropped"""
        cur, refs, dists, size = self._check(cur, refs, dists, size)
        self._size(cur, size)
        self._noise(self._search(cur, refs, size), dists, size, False)
        return tuple(int(v) for v in self._result.tolist())

    def motion(self, cur, ref, size):
        """the level-0 vectors and errors of one reference: (mv int16 [gh, gw, 2] as (y, x), err int32 [gh, gw]), new tensors"""
        cur, (ref,), _, size = self._check(cur, [ref], [1], size)
        self._size(cur, size)
        self._search(cur, [ref], size)
        return self._mv[0].clone(), self._err[0].clone()

    def motion_subpel(self, cur, ref, size):
        """the refined vectors and errors of one reference (a subpel 1 or 2 object): (mvq int16 [gh, gw, 2] as (y, x) in
        quarter pels, errq int32 [gh, gw]), new tensors"""
        if not self.subpel:
            raise ValueError("motion_subpel() needs an object made with subpel 1 or 2")
        self.motion(cur, ref, size)
        return self._mvq[0].clone(), self._errq[0].clone()

    def pyramid(self, x, size):
        """Q0 | Q1 | Q2 of x's luma as one int16 tensor holding the uint16 codes (a new tensor)"""
        x = self._frame(x)
        size = tuple(int(v) for v in size)
        self._size(x, size)
        self._pyramid(x, size, 2 * self.radius + 1)
        return self._pyr[2 * self.radius + 1].clone()

    # ------------------------------------------------------------------------------ a sequence
    def _emit(self, n_known):
        """frame self._emitted of a sequence of which n_known frames are in the ring"""
        t, n = self._emitted, 2 * self.radius + 1
        refs = _refs_of(t, n_known, self.radius)
        slots = [i % n for i, _ in refs]
        if refs:
            self._motion(t % n, slots, self._size_of_sequence)
            if self.level == AUTO:
                self._noise(t % n, [d for _, d in refs], self._size_of_sequence, True)
        out = self._out[t % (self.radius + 1)]
        self._blend(self._ring[t % n], [self._ring[s] for s in slots], [d for _, d in refs], self._size_of_sequence, out)
        self._emitted += 1
        return out

    def push(self, x, size):
        """the next source frame (copied into the ring) -> the list of filtered frames it completes: none for the first
        `radius` frames, then one per call, `radius` frames behind the input"""
        x = self._frame(x)
        size = tuple(int(v) for v in size)
        if self._pushed and (self._key != (tuple(x.shape), x.dtype) + size or size != self._size_of_sequence):
            raise ValueError("the frames of a sequence must have one shape, type and picture size: reset() first")
        self._size(x, size)
        self._size_of_sequence = size
        slot = self._pushed % (2 * self.radius + 1)
        self._ring[slot].copy_(x)
        self._pyramid(self._ring[slot], size, slot)
        self._pushed += 1
        # frame t is complete once frame t + radius is in; the window of an early frame is cut at the sequence's start only
        return [self._emit(self._pushed)] if self._pushed > self.radius else []

    def flush(self):
        """the filtered frames still owed (at most `radius`), in order; the sequence is over - the next push starts another,
        the weight sum stays"""
        out = [self._emit(self._pushed) for _ in range(self._pushed - self._emitted)]
        self._pushed = self._emitted = 0
        return out

    def weight_sum(self):
        """the sum over the luma samples filtered since reset() of (Wsum - 256); one read-back"""
        return int(self._total.item())

    def levels(self):
        """of the frames estimated since reset() (level "auto"; a frame without references is not one): the number that got
        level 0 .. 5, the sum of their N, their number - eight ints; one read-back"""
        return [int(v) for v in self._levels.tolist()]
