"""The encoder's front end (opendcvc_amd/frontend.py) on stub stages, without a device: the order of the written units, what
every stage sees, and the clock rule.  Every stub step advances a fake clock by a power of two of its own, so a reported time
decodes, exactly, to the set of steps that were charged to it."""
import itertools

import pytest

from opendcvc_amd.frontend import Delay, EncodePass, Frame, FrontEnd

SIZE, CODED = (128, 160), (48, 96, False)
I_FRAMES = (0, 4, 5)                                      # the source frames the stub encoder codes as I frames (if it gets them)


def cut_of(k):
    return k % 3 == 1                                     # the stub lookahead's fixed decisions


class Clock:
    """event e advances the clock by 1 << e; events: (kind, the source frame the step is about or None)"""
    def __init__(self):
        self.t, self.events = 0, []

    def now(self):
        return self.t

    def tick(self, kind, k=None):
        self.t += 1 << len(self.events)
        self.events.append((kind, k))


class Pic:
    def __init__(self, clock, k, tags=()):
        self.clock, self.k, self.tags = clock, k, tags

    def tagged(self, tag):
        return Pic(self.clock, self.k, self.tags + (tag,))

    def clone(self):
        self.clock.tick("clone", self.k)
        return self.tagged("clone")


class Holder:
    """a stage that holds `delay` frames back: the filter (tags what it returns) or the lookahead ((x, cut) pairs)"""
    def __init__(self, clock, name, delay, args, out):
        self.clock, self.name, self.delay, self.args, self.out, self.held, self.seen = clock, name, delay, args, out, [], []

    def push(self, x, *args):
        assert args == self.args
        self.clock.tick(self.name + ".push", x.k)
        self.seen.append(x.k)
        self.held.append(x)
        return [self.out(self.held.pop(0))] if len(self.held) > self.delay else []

    def flush(self):
        self.clock.tick(self.name + ".flush", self.held[0].k if self.held else None)     # (about the first frame it returns)
        out, self.held = [self.out(x) for x in self.held], []
        return out


class Detector:
    def __init__(self, clock, pattern):
        self.clock, self.pattern, self.seen = clock, pattern, []

    def is_repeat(self, x, size):
        assert size == SIZE and not x.tags
        self.clock.tick("compare", x.k)
        self.seen.append(x.k)
        return bool(self.pattern[x.k])


class Packet:
    def __init__(self, k, is_i=False):
        self.k, self.is_i = k, is_i                       # k None: a repeat unit


class Encoder:
    """front: set once the FrontEnd is made; calls: (x, keywords, the record's source, the units written) at every encode"""
    def __init__(self, clock, writer):
        self.clock, self.writer, self.front, self.calls = clock, writer, None, []

    def encode(self, x, **kw):
        self.clock.tick("encode", x.k)
        self.calls.append((x, kw, self.front.coding.source, len(self.front.units)))
        return Packet(x.k, x.k in I_FRAMES)

    def repeat(self):
        self.clock.tick("repeat", len(self.writer.units))     # (the units are the source frames in order: the next one's index)
        return Packet(None)


class Writer:
    def __init__(self, clock):
        self.clock, self.units = clock, []

    def write_frame(self, h, w, two, pkt):
        assert (h, w, two) == CODED
        self.clock.tick("write", len(self.units))
        self.units.append(pkt)
        return 1 if pkt.k is None else 100 + pkt.k


class Run:
    """n frames with the repeat pattern (None: no detector) through a filter of delay R and a lookahead of delay N (0: none)"""
    def __init__(self, n, pattern, R, N, scaled):
        self.clock = clock = Clock()
        self.pics = [Pic(clock, k) for k in range(n)]
        self.det = Detector(clock, pattern) if pattern is not None else None
        self.tf = Holder(clock, "tf", R, (SIZE,), lambda x: x.tagged("tf")) if R else None
        self.la = Holder(clock, "la", N, (), lambda x: (x, cut_of(x.k))) if N else None
        self.writer = Writer(clock)
        self.enc = Encoder(clock, self.writer)

        def resample(x):
            clock.tick("resample", x.k)
            return x.tagged("resampled")
        self.front = FrontEnd(self.enc, self.writer, CODED, lambda: clock.tick("sync"), clock.now, SIZE, self.det, self.tf,
                              resample if scaled else None, self.la)
        self.enc.front = self.front
        for pic in self.pics:
            clock.tick("read")                            # the file read and the copy to the device: on nobody's clock
            t0 = clock.now()
            clock.tick("load", pic.k)
            self.front.feed(pic, t0)
        self.front.flush()
        self.types, self.bits, self.times, self.repeated = ([u[i] for u in self.front.units] for i in range(4))

    def charged(self, k):
        """the steps that source frame k's reported time is the sum of"""
        t = self.times[k]
        return [ev for e, ev in enumerate(self.clock.events) if t >> e & 1]

    def owners(self):
        """the clock rule, step by step: the source frame each step is to be charged to, or None.  A step about frame k is
        frame k's, also the flush call, which is about the first frame it returns (about nobody if it returns none); a
        synchronisation goes with the step in front of it; the read is nobody's"""
        out = []
        for kind, k in self.clock.events:
            out.append(out[-1] if kind == "sync" else k)
        return out


PATTERNS = {"none": [0] * 6, "behind-0": [0, 1, 0, 0, 0, 0, 0], "runs": [0, 0, 1, 1, 0, 1, 1, 1, 0], "last": [0, 0, 0, 0, 0, 1, 1, 1],
            "all-but-first": [0, 1, 1, 1, 1, 1], "short": [0, 1, 0], "two": [0, 0], "no-detector": None}
CASES = list(itertools.product(PATTERNS, (0, 1, 2), (0, 2, 4), (False, True)))


@pytest.fixture(scope="module")
def runs():
    return {case: Run(len(PATTERNS[case[0]] or [0] * 7), PATTERNS[case[0]], *case[1:]) for case in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-R{c[1]}-N{c[2]}" + ("-scaled" if c[3] else ""))
def test_order_and_what_every_stage_sees(runs, case):
    run, (name, R, N, scaled) = runs[case], case
    pattern = PATTERNS[name] or [0] * 7
    n, coded = len(pattern), [k for k, rep in enumerate(pattern) if not rep]
    # the written units are the source frames in source order, each repeat directly behind the frame it repeats
    assert [pkt.k for pkt in run.writer.units] == [None if rep else k for k, rep in enumerate(pattern)]
    # every stage, and the encoder, sees exactly the sequence without the repeats, in order; the detector sees every frame
    assert run.det is None or run.det.seen == list(range(n))
    assert run.tf is None or run.tf.seen == coded
    assert run.la is None or run.la.seen == coded
    assert [x.k for x, _, _, _ in run.enc.calls] == coded
    clone = bool(R and N and not scaled)                  # filter, lookahead, no down-resample: the one case
    tags = ("tf",) * bool(R) + ("resampled",) * scaled + ("clone",) * clone
    for x, kw, source, written in run.enc.calls:
        assert source is run.pics[x.k]                    # its own unfiltered source
        assert kw == ({"cut": cut_of(x.k)} if N else {})  # its own cut; without a lookahead the encoder decides
        assert x.tags == tags                             # filtered, then resampled (or cloned), in that nesting
        assert written == x.k                             # grain "auto"'s index: the frames written so far, repeats included
    assert sum(kind == "clone" for kind, _ in run.clock.events) == (len(coded) if clone else 0)
    assert run.types == [1 if rep else 0 if k in I_FRAMES else 1 for k, rep in enumerate(pattern)]
    assert run.bits == [8 if rep else 8 * (100 + k) for k, rep in enumerate(pattern)]
    assert run.repeated == pattern and len(run.times) == n
    assert all(not d.queue for d in run.front.stages if isinstance(d, Delay))
    assert run.front.last.written and not run.front.last.repeats


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-R{c[1]}-N{c[2]}" + ("-scaled" if c[3] else ""))
def test_the_clock_rule_frame_by_frame(runs, case):
    run = runs[case]
    owners = run.owners()
    for k in range(len(run.times)):
        assert run.times[k] == sum(1 << e for e, owner in enumerate(owners) if owner == k), (k, run.charged(k))
    # the sum of all times is what the clock advanced inside timed regions: everything but the reads and a flush of nothing
    untimed = sum(1 << e for e, (kind, k) in enumerate(run.clock.events) if kind == "read" or (kind.endswith(".flush") and k is None))
    assert sum(run.times) == run.clock.now() - untimed
    # a queued frame is charged nothing that is about another frame (its synchronisations aside)
    for k in range(len(run.times)):
        assert {ev[1] for ev in run.charged(k) if ev[0] != "sync"} == {k}


def test_the_clock_rule_on_a_clip_worked_by_hand():
    """filter of delay 1, three frames, the last a repeat of frame 1, which only comes out in the flush"""
    run = Run(3, [0, 0, 1], 1, 0, False)
    S = ("sync", None)
    assert run.charged(0) == [("load", 0), ("compare", 0), ("tf.push", 0), S,           # queued: nothing of frame 1's is charged
                              ("encode", 0), ("write", 0), S]
    assert run.charged(1) == [("load", 1), ("compare", 1), ("tf.push", 1), S,           # frame 0 is coded in between
                              ("tf.flush", 1), ("encode", 1), ("write", 1), S]          # the flush call: on its first frame
    assert run.charged(2) == [("load", 2), ("compare", 2), ("repeat", 2), ("write", 2)]      # loader + compare + its own write
    assert [kind for kind, _ in run.clock.events[-6:]] == ["tf.flush", "encode", "write", "sync", "repeat", "write"]


def test_a_flush_charges_each_later_frame_from_where_the_one_before_finished():
    """a clip no longer than R: everything comes out in the flushes"""
    run = Run(2, None, 2, 4, True)
    kinds = [[kind for kind, _ in run.charged(k)] for k in range(2)]
    assert [kind for kind, _ in run.clock.events if kind.endswith(".flush")] == ["tf.flush", "la.flush"]
    head, code = ["load", "tf.push", "sync"], ["encode", "write", "sync"]
    assert kinds[0] == head + ["tf.flush", "resample", "la.push", "sync", "la.flush"] + code
    assert kinds[1] == head + ["resample", "la.push", "sync"] + code


def test_the_record_and_the_result():
    f = Frame("x", 10)
    assert (f.source, f.x, f.cut, f.spent, f.written, f.repeats) == ("x", "x", None, 0, False, [])
    f.pause(13)
    f.since = 20                                          # (queued from 13 to 20: not charged)
    f.pause(24)
    assert f.spent == 7
    with pytest.raises(AttributeError):
        f.other = 1
    assert EncodePass._fields == ("enc", "stream", "frame_types", "bits", "times", "scaler", "grainer", "tf", "lookahead", "repeated")
