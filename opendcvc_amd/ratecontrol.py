"""Target-bitrate control for pipeline.SequenceEncoder: pure host arithmetic (no torch, no GPU, no clock), so that it can be
tested against a synthetic plant and takes the same decisions wherever it runs.

The controller moves the BASE qp of the P frames.  The reference's hierarchical offsets stay on top of it
(shift_qp(base, INDEX_MAP[g % 8])), and the I-frame qp keeps the distance to the base it had at the start.  What it is fed
is one number per frame: the size the device predicted for the frame (handoff.estimated_bytes, known before the host coder
starts) plus the container's bytes - never the exact stream length, which arrives one frame late on the deferred paths.
"""
import math

B_MIN, B_MAX, B_INIT = 0.01, 0.2, 0.05     # clamp and starting value of the slope b of ln bits over qp
B_PRIOR_WEIGHT = 8.0                       # the starting value counts like slope observations with sum dqp^2 = 8
MAX_STEP = 16                              # the base qp moves by at most this much from one frame to the next
T_FLOOR = 0.25                             # a frame is never asked to be smaller than this fraction of the target
LEVEL_GAIN, CLASS_GAIN = 0.5, 0.25         # smoothing of the common level / of a class's distance to it
CYCLE_WEIGHTS = {0: 4 / 8, 1: 1 / 8, 2: 3 / 8}      # how often INDEX_MAP = (0, 1, 0, 2, 0, 2, 0, 2) uses each offset
I_CLASS = "I"


class RateController:
    """RateController(target_bits_per_frame, qp_init, qp_min=0, qp_max=63, window=6, qp_i_init=None)

    State:
      debt      sum(observed - target) over every frame observed, I frames included (an I frame - the first one, one
                the period or a scene cut asks for - is just an expensive frame the debt absorbs)
      model     ln bits = level + class[c] + b * (base qp - anchor) for the P classes c = the frame's INDEX_MAP offset
                (0, 1, 2); I frames are a class of their own, kept for predict() only.  `level` is re-anchored at the
                frame's qp and smoothed from every P observation (gain 0.5), class[c] from every observation of c (gain
                0.25), so a change of content moves all classes at once.
      b         learned from consecutive observations of one class at different qp by least squares through the origin over
                (dqp, d ln bits), started as B_INIT with the weight of sum dqp^2 = 8, clamped to [B_MIN, B_MAX] =
                [0.01, 0.2] per qp step (the synthetic q_ramp weights have about 0.022, trained models are several times
                steeper).  A pair whose own slope lies outside [0, B_MAX] - a scene change between the two - is not used.
    Decision (base_qp(), once per frame, before the frame is coded): the frame's budget is
      max(target - debt / window, T_FLOOR * target)
    i.e. the debt is repaid over `window` frames (default 6: an I frame's excess is down to a tenth after 13 frames), a
    frame is never asked to go below a quarter of the target, and the base qp is the one at which the model's mean over
    the 8-frame offset cycle equals that budget.  The real-valued answer is turned into integers by error feedback (the
    rounding error is carried to the next frame), so that the mean of the integer qp is the real-valued one and the debt
    settles at zero rather than at the offset a plain rounding would hold.  The base moves by at most MAX_STEP = 16 per
    frame and stays in [qp_min, qp_max]; qp_min == qp_max gives a constant trace.  Until the first P frame has been
    observed the base is qp_init.
    Deterministic: the trace is a function of the observations alone."""

    def __init__(self, target_bits_per_frame, qp_init, qp_min=0, qp_max=63, window=6, qp_i_init=None):
        if not target_bits_per_frame > 0 or window < 1 or not 0 <= qp_min <= qp_max <= 63:
            raise ValueError("a positive target, a window of at least one frame and 0 <= qp_min <= qp_max <= 63 are needed")
        self.target = float(target_bits_per_frame)
        self.qp_min, self.qp_max, self.window = int(qp_min), int(qp_max), int(window)
        self.base = min(max(int(qp_init), self.qp_min), self.qp_max)
        self.i_delta = (int(qp_init) if qp_i_init is None else int(qp_i_init)) - int(qp_init)
        self.debt = 0.0
        self.b = B_INIT
        self._sxx, self._sxy = B_PRIOR_WEIGHT, B_PRIOR_WEIGHT * B_INIT
        self._level = None            # ln bits of an offset-0-like P frame at base qp self._anchor
        self._anchor = self.base
        self._class = {}              # P class -> its distance to the level
        self._i_level = None          # (ln bits, base qp) of the I class
        self._last = {}               # class -> (base qp, ln bits) of its latest observation
        self._carry = 0.0
        self.frames = 0
        self.exact_bytes = []         # (frame index, len(bit_stream)) as they arrive: for the log, never fed back

    # ---- decision
    def i_qp(self, base):
        return min(max(base + self.i_delta, 0), 63)

    def _cycle_level(self):
        """ln of the model's mean size over the offset cycle at the anchor qp (classes not seen yet: like the level)"""
        return self._level + math.log(sum(w * math.exp(self._class.get(c, 0.0)) for c, w in CYCLE_WEIGHTS.items()))

    def base_qp(self):
        """the base qp of the frame about to be coded"""
        if self._level is not None and self.qp_min < self.qp_max:
            budget = max(self.target - self.debt / self.window, T_FLOOR * self.target)
            want = self._anchor + (math.log(budget) - self._cycle_level()) / self.b
            lo, hi = max(self.qp_min, self.base - MAX_STEP), min(self.qp_max, self.base + MAX_STEP)
            q = int(math.floor(want + self._carry + 0.5))
            if lo <= q <= hi:
                self._carry = min(max(want + self._carry - q, -1.0), 1.0)
            else:                     # (against a limit there is nothing to carry)
                q, self._carry = min(max(q, lo), hi), 0.0
            self.base = q
        return self.base

    def predict(self, klass, base):
        """the model's size in bits of a frame of class `klass` (I_CLASS or an INDEX_MAP offset) at base qp `base`"""
        if klass == I_CLASS:
            return None if self._i_level is None else math.exp(self._i_level[0] + self.b * (base - self._i_level[1]))
        if self._level is None:
            return None
        return math.exp(self._level + self._class.get(klass, 0.0) + self.b * (base - self._anchor))

    # ---- feedback
    def observe(self, klass, base, bits):
        """one coded frame: its class, the base qp it was coded at and its (predicted) size in bits"""
        self.frames += 1
        self.debt += bits - self.target
        ln = math.log(max(float(bits), 1.0))
        last = self._last.get(klass)
        if last is not None and last[0] != base:
            dq, dl = base - last[0], ln - last[1]
            if 0.0 <= dl / dq <= B_MAX:
                self._sxx += dq * dq
                self._sxy += dq * dl
                self.b = min(max(self._sxy / self._sxx, B_MIN), B_MAX)
        self._last[klass] = (base, ln)
        if klass == I_CLASS:
            self._i_level = (ln, base)
            return
        if self._level is None:
            self._level, self._anchor = ln, base
            self._class[klass] = 0.0
            return
        at = self._level + self.b * (base - self._anchor)
        resid = ln - at - self._class.get(klass, 0.0)
        self._level, self._anchor = at + LEVEL_GAIN * resid, base
        self._class[klass] = self._class.get(klass, 0.0) + CLASS_GAIN * resid

    def skip(self, bits):
        """one frame that was not coded (a repeat unit of `bits` bits, docs/frame_repeat.md): it counts and pays into the
        debt like any frame - the budget it leaves goes to its neighbours - and teaches the model nothing"""
        self.frames += 1
        self.debt += bits - self.target

    def record_exact(self, frame_idx, nbytes):
        self.exact_bytes.append((int(frame_idx), int(nbytes)))
