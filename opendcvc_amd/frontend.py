"""The encoder's front end ("The encode front end"): one record per source frame, one queue for every stage that
holds frames back, one clock rule.  No reference counterpart.  Nothing here touches the device: the stages, the encoder, the
writer, the synchronisation and the clock are handed in (tests/test_frontend_host.py runs it on stubs).  THE CLOCK RULE: a
frame's clock runs from the reading it is fed with until it is queued in a delaying stage (the stage's push and the
synchronisation behind it count), stands still while it is queued, and runs again from when it comes out until its packet is
written and the device synchronised.  The call of a flush() goes onto the first frame it returns; each later frame of one
push() or flush() starts when the one before it is finished.  A repeat: loader + window + compare + its unit's write."""
from collections import namedtuple

EncodePass = namedtuple("EncodePass", "enc stream frame_types bits times scaler grainer tf lookahead repeated")       # of harness._encode_pass


class Frame:
    """what belongs to one source frame that is no repeat, and follows it through every queue.  source: the unfiltered input,
    windowed, at source size (grain "auto" estimates from it); x: the picture as it stands - every stage replaces it; cut:
    the lookahead's decision (None: the encoder decides); since: the reading its clock runs from; spent: the seconds on its
    clock so far; written: its packet is out; repeats: the seconds of each repeat found behind it that is not yet written"""
    __slots__ = ("source", "x", "cut", "since", "spent", "written", "repeats")

    def __init__(self, x, since):
        self.source, self.x, self.cut, self.since, self.spent, self.written, self.repeats = x, x, None, since, 0, False, []

    def pause(self, now):
        self.spent += now - self.since


class Delay:
    """a stage that holds frames back, and the FIFO of their records: stage.push(x, *args) and stage.flush() return what comes
    out, in order - the new x, or with cuts (x, cut) pairs - and the oldest record leaves with each"""
    def __init__(self, stage, sync, clock, args=(), cuts=False):
        self.stage, self.sync, self.clock, self.args, self.cuts, self.queue = stage, sync, clock, args, cuts, []

    def push(self, rec):
        outs = self.stage.push(rec.x, *self.args)
        self.sync()
        rec.pause(self.clock())
        self.queue.append(rec)
        return self._leave(self.clock(), outs)

    def flush(self):
        return self._leave(self.clock(), self.stage.flush())         # (the reading FIRST: the call goes onto the first frame's clock)

    def _leave(self, now, outs):
        for out in outs:
            rec = self.queue.pop(0)
            rec.x, rec.cut = out if self.cuts else (out, rec.cut)
            rec.since = now
            yield rec                                    # (back here once the frame is finished)
            now = self.clock()


class FrontEnd:
    """feed(x, t0) every source frame (as the loader and the window leave it; t0: the reading its clock started at), then flush().
    What is None is off.  In order: detector - is_repeat(x, size) diverts the repeats, nothing behind it sees one; tf - push(x,
    size) / flush() -> frames; resample - x -> x; lookahead - push(x) / flush() -> (x, cut) pairs; encoder - encode(x[, cut=]),
    repeat(); writer - write_frame(*coded, packet), coded: (height, width, two coders).  units: (frame type, bits, seconds,
    repeat 0 / 1) per source frame, in written order; coding: the record of the frame the encoder is at."""
    def __init__(self, encoder, writer, coded, sync, clock, size=None, detector=None, tf=None, resample=None, lookahead=None):
        self.encoder, self.writer, self.coded, self.sync, self.clock, self.size, self.detector = encoder, writer, coded, sync, clock, size, detector
        self.units, self.last, self.coding = [], None, None                          # last: the last frame that was no repeat
        self.stages = ([Delay(tf, sync, clock, (size,))] if tf is not None else []) + ([resample] if resample is not None else [])
        if lookahead is not None:        # (after a filter its output buffers come round again before the frame is coded: a clone, unless resampled)
            clone = [lambda x: x.clone()] if tf is not None and resample is None else []
            self.stages += clone + [Delay(lookahead, sync, clock, cuts=True)]

    def feed(self, x, t0):
        if self.detector is not None and self.detector.is_repeat(x, self.size):      # (has waited for its compare)
            self.last.repeats.append(self.clock() - t0)
            if self.last.written:
                self._trailer(self.last)
            return
        self.last = Frame(x, t0)
        self._run((self.last,), 0)

    def flush(self):
        for i, stage in enumerate(self.stages):
            if isinstance(stage, Delay):
                self._run(stage.flush(), i + 1)

    def _run(self, recs, i):
        """recs into stage i and on down the chain, each to the end before the next; behind the last stage they are written"""
        for rec in recs:
            if i == len(self.stages):
                self._write(rec)
            elif isinstance(self.stages[i], Delay):
                self._run(self.stages[i].push(rec), i + 1)
            else:
                rec.x = self.stages[i](rec.x)
                self._run((rec,), i + 1)

    def _write(self, rec):
        self.coding = rec
        pkt = self.encoder.encode(rec.x) if rec.cut is None else self.encoder.encode(rec.x, cut=rec.cut)
        bits = 8 * self.writer.write_frame(*self.coded, pkt)
        self.sync()
        rec.pause(self.clock())
        self.units.append((0 if pkt.is_i else 1, bits, rec.spent, 0))
        rec.written = True
        self._trailer(rec)

    def _trailer(self, rec):
        """the repeats found behind rec and not yet written: a unit each, right behind the packet written last"""
        while rec.repeats:
            t1 = self.clock()
            bits = 8 * self.writer.write_frame(*self.coded, self.encoder.repeat())
            self.units.append((1, bits, rec.repeats.pop(0) + (self.clock() - t1), 1))        # (a repeat counts as a P frame)
