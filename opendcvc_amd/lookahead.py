"""Frame lookahead for the encoder's scene-cut decision (docs/lookahead.md is the normative text; csrc/dcvc_lookahead.hip;
no reference counterpart).  The decision for frame t waits for `depth` more frames: a change that is undone a few frames
later is a flash, a change that one gain and one offset explain is a fade, and neither costs an I frame.  The measure is
motion compensated (8 x 8 tiles of the 1/8-resolution plane, +-3 samples), so a pan is no cut either.  Encoder side only.

CutPolicy is pure host code over any object that gives costs(i, j) -> (mc, wp) and intra(i); Lookahead puts it on the
device: a ring of low-resolution planes made by dcvc_frame_analyze, pair costs by dcvc_lookahead_cost, computed lazily for
the pairs the policy asks about.  tests/lookahead_ref.py restates both in numpy, bit for bit."""
import ctypes

MAX_DEPTH = 16


def check_depth(depth):
    """the lookahead depth as an integer 0 (off) .. MAX_DEPTH"""
    if isinstance(depth, bool) or not isinstance(depth, int) or not 0 <= depth <= MAX_DEPTH:
        raise ValueError(f"lookahead depth {depth!r}: 0 (off) .. {MAX_DEPTH}")
    return depth


def cutlike(cost, intra, scenecut):
    """the cost is at least scenecut percent of the frame's own spatial activity (Python integers: nothing overflows)"""
    return 100 * int(cost) >= int(scenecut) * max(int(intra), 1)


class CutPolicy:
    """The decisions of one sequence, frame by frame in order.  costs: an object with costs(i, j) -> (mc, wp) of frame i
    against frame j and intra(i), asked only about frames the caller has said are known.  decide(t, n_known) -> is frame t
    a cut, given frames 0 .. n_known - 1; flashes / fades list the frames so labelled.  The anchor is the last frame before t
    that was not labelled a flash frame:
      1. mc(t, a) not cut-like: no cut.
      2. otherwise the first k = 1 .. depth with t + k known and mc(t + k, a) not cut-like marks a flash: frames t .. t + k - 1
         are flash frames, none of them a cut, the anchor stays.
      3. otherwise wp(t, a) not cut-like: a fade, no cut.
      4. otherwise a cut."""

    def __init__(self, costs, depth, scenecut):
        self.costs, self.depth, self.scenecut = costs, check_depth(depth), int(scenecut)
        if self.scenecut <= 0:
            raise ValueError("the lookahead decides scene cuts: scenecut must be a percentage above 0")
        self.reset()

    def reset(self):
        self.flashes, self.fades = [], []
        self._anchor = self._flash_end = self._next = 0

    def decide(self, t, n_known):
        if t != self._next or not t < n_known:
            raise ValueError(f"frame {t} is decided in order and once it is known (next: {self._next}, known: {n_known})")
        self._next += 1
        if t == 0 or t < self._flash_end:            # the first frame; a frame labelled a flash frame: the anchor stays
            return False
        c, a = self.costs, self._anchor
        mc, wp = c.costs(t, a)
        if cutlike(mc, c.intra(t), self.scenecut):
            for k in range(1, min(self.depth, n_known - 1 - t) + 1):
                if not cutlike(c.costs(t + k, a)[0], c.intra(t + k), self.scenecut):
                    self.flashes.append(t)
                    self._flash_end = t + k
                    return False
            if not cutlike(wp, c.intra(t), self.scenecut):
                self.fades.append(t)
            else:
                self._anchor = t
                return True
        self._anchor = t
        return False


class Lookahead:
    """The lookahead on `device`: push(x, ready) takes the next frame the encoder is to see (the [1, 3, Hp, Wp] model input; ready
    as FrameAnalyzer.analyze takes it) and returns the list of (x, cut) it completes - none for the first `depth` frames,
    then one per call, `depth` frames behind the input; flush() returns the rest, decided from what lies ahead of each, and
    ends the sequence.  Hand cut to SequenceEncoder.encode(x, cut=cut).

    Owns a ring of depth + 2 low-resolution planes (the anchor of the frame being decided and the depth frames ahead of it),
    the depth + 1 frames it holds back - references, not copies: the caller leaves them alone until they come out - the two
    workspaces, pinned result words and a HIP stream of its own, which alone is waited for.  Every frame costs one
    dcvc_frame_analyze (into the ring) and one pair cost against its anchor; further pairs are computed only where a frame
    looks like a cut."""

    def __init__(self, device="cuda:0", depth=4, scenecut=150):
        import numpy as np
        import torch
        from . import _lib
        from .entropy import PinnedBuffer
        if check_depth(depth) == 0:
            raise ValueError("lookahead depth 0 is 'off': make no Lookahead")
        self.device = torch.device(device)
        self.depth = depth
        self.policy = CutPolicy(self, depth, scenecut)
        self._lib = _lib.lib()
        self.stream = torch.cuda.Stream(self.device)
        self._ready = torch.cuda.Event()
        self._pinned = PinnedBuffer(12 * 8)
        self._stats = self._pinned.view(np.uint64, 12)[:4]        # dcvc_frame_analyze's words
        self._cost = self._pinned.view(np.uint64, 12)[4:]         # dcvc_lookahead_cost's
        self._size = None
        self.pair_costs = 0                                       # dcvc_lookahead_cost calls so far
        self.reset()

    @property
    def flashes(self):
        return self.policy.flashes

    @property
    def fades(self):
        return self.policy.fades

    def reset(self):
        """forgets the sequence: the frames held back are dropped, the next push is frame 0"""
        self.policy.reset()
        self._held, self._intra, self._cache = [], {}, {}
        self._pushed = self._emitted = 0
        self._over = False

    def _buffers(self, h, w):
        import torch
        from . import _lib
        if self._size != (h, w):
            if self._pushed:
                raise ValueError("the frames of a sequence must have one size: reset() first")
            need = _lib.check(self._lib.dcvc_frame_analysis_ws_bytes(h, w), "dcvc_frame_analysis_ws_bytes")
            need_c = _lib.check(self._lib.dcvc_lookahead_ws_bytes(h // 8, w // 8), "dcvc_lookahead_ws_bytes")
            self._planes = torch.empty((self.depth + 2, h // 8, w // 8), dtype=torch.uint16, device=self.device)
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws_cost = torch.empty(need_c, dtype=torch.uint8, device=self.device)
            self._size = (h, w)

    def _plane(self, i):
        if not max(self._pushed - (self.depth + 2), 0) <= i < self._pushed:
            raise ValueError(f"the plane of frame {i} is not in the ring (frames pushed: {self._pushed})")
        return self._planes[i % (self.depth + 2)]

    def _sync(self, what):
        from . import _lib
        _lib.check(self._lib.dcvc_stream_sync(ctypes.c_void_p(self.stream.cuda_stream)), what)

    # ------------------------------------------------------------------------------ what the policy asks
    def intra(self, i):
        return self._intra[i]

    def words(self, i, j):
        """the eight words of dcvc_lookahead_cost for frame i against frame j, both in the ring: mc, wp, w, o, mean and ac of
        i, mean and ac of j (one launch group, one wait on the object's stream)"""
        from . import _lib
        from . import nn as L
        cur, ref = self._plane(i), self._plane(j)
        _lib.check(self._lib.dcvc_lookahead_cost(L._p(cur), L._p(ref), cur.shape[0], cur.shape[1], L._p(self._ws_cost),
                                                 ctypes.c_void_p(self._pinned.ptr + 4 * 8),
                                                 ctypes.c_void_p(self.stream.cuda_stream)), "dcvc_lookahead_cost")
        self._sync("dcvc_lookahead_cost")
        self.pair_costs += 1
        v = [int(x) for x in self._cost]
        v[3] -= (v[3] >> 63) << 64                  # o: two's complement
        return tuple(v)

    def costs(self, i, j):
        if (i, j) not in self._cache:
            self._cache[(i, j)] = self.words(i, j)[:2]
        return self._cache[(i, j)]

    # ------------------------------------------------------------------------------ a sequence
    def _emit(self):
        t = self._emitted
        cut = self.policy.decide(t, self._pushed)
        self._emitted += 1
        for key in [k for k in self._cache if k[0] < t]:          # (a pair found while looking ahead is asked for again: kept)
            del self._cache[key]
        self._intra.pop(t - 1, None)
        return self._held.pop(0), cut

    def push(self, x, ready=None):
        import torch
        from . import _lib
        from . import nn as L
        if x.dim() != 4 or x.shape[0] != 1 or x.stride(3) != 1:
            raise ValueError("push() takes the [1, C, H, W] model input with unit column stride")
        if self._over:
            self.reset()
        h, w = int(x.shape[2]), int(x.shape[3])
        self._buffers(h, w)
        if ready is None:
            ready = self._ready
            ready.record(torch.cuda.current_stream(self.device))
        self.stream.wait_event(ready)
        t = self._pushed
        self._pushed += 1
        prev = self._plane(t - 1) if t else None
        _lib.check(self._lib.dcvc_frame_analyze(L.dtype_code(x.dtype), L._p(x), int(x.stride(2)), h, w,
                                                L._p(prev) if t else None, L._p(self._plane(t)), L._p(self._ws),
                                                ctypes.c_void_p(self._pinned.ptr), ctypes.c_void_p(self.stream.cuda_stream)),
                   "dcvc_frame_analyze")
        self._sync("dcvc_frame_analyze")
        self._intra[t] = int(self._stats[1])
        self._held.append(x)
        return [self._emit()] if self._pushed > self.depth else []

    def flush(self):
        """the frames still owed (at most `depth`) with their decisions, in order; the sequence is over: the next push starts
        another (flashes and fades stay readable until then)"""
        out = [self._emit() for _ in range(self._pushed - self._emitted)]
        self._over = True
        return out
