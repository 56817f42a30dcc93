"""Per-sequence encode / decode drivers: the frame-type, qp-offset and feature-refresh policy of the
reference harness (test_video.py:164-214 encoder side, :258-285 decoder side) packaged as two
small state machines, so bench.py / smoke() / the tests all drive the codecs the same way the
reference's run_one_point_with_stream does.
"""
from dataclasses import dataclass
from typing import Optional

INDEX_MAP = (0, 1, 0, 2, 0, 2, 0, 2)          # test_video.py:164
REPEAT = object()                             # in EncodeDecodePipeline.run's frames: "the picture of the frame before, again"


@dataclass
class FramePacket:
    is_i: bool
    qp: int
    use_ada_i: int
    bit_stream: bytes
    chunked: bool = False        # chunked payload (the models' entropy="device" mode): written as NAL_I_CHUNKED / NAL_P_CHUNKED
    grain: Optional[object] = None   # grain.GrainParams in force from this frame on (docs/film_grain.md): a NAL_GRAIN unit,
                                     # written in front of the digest unit as it stands in front of it here
    repeat: bool = False             # the picture of the frame before, again (docs/frame_repeat.md): a NAL_REPEAT unit, no payload
    digest: Optional[int] = None     # digest of the entry the frame puts into the DPB (docs/state_digest.md): a NAL_DIGEST unit


def _dpb_entry(p_net):
    """what a frame has just put into the DPB, the object both sides hold: an I frame's picture, a P frame's feature buffer"""
    ref = p_net.dpb[0]
    return ref.frame if ref.feature is None else ref.feature


class SequenceEncoder:
    """defer_stream=False: encode(x) returns the frame's packet (the reference's loop).
    defer_stream=True: P-frame packets come out one call late - encode(x) returns a LIST of the packets completed by
    the call, in order, flush() the rest; the host entropy coding of a P frame then runs underneath the next frame's
    kernels (DMC.compress(defer_stream=True)), which makes a sequential encoder GPU-bound.

    scenecut (percent, None / 0 = off: exactly the reference's placement, no analyzer, nothing launched): adaptive I
    frames.  Every frame is analysed on the device (analysis.FrameAnalyzer) and the policy counts GOP-relative: with g
    the number of frames since the most recent I frame (g = 0 at an I frame), a frame is an I frame if it is frame 0, if
    intra_period > 0 and g == intra_period, or if analysis.is_cut(stats, scenecut) and g >= min_keyint (a cut closer to
    the last I frame is coded as a P frame); P frames take use_ada_i from g % reset_interval == 1 and the qp offset
    INDEX_MAP[g % 8].  Without a cut the stream equals the scenecut-off stream whenever g == fi for every frame:
    intra_period = -1, or an intra_period that is a multiple of 8 and of reset_interval.  scene_cuts lists the frames
    whose cut was honoured with an I frame (also where the period asked for one at the same frame).  encode(x, ready):
    `ready` is a torch.cuda.Event recorded where x became ready, so the analysis need not wait for the kernels of the
    previous frame that defer_stream keeps in flight.  analyzer: any object with analyze(x, ready) -> FrameStats.
    encode(x, cut=True / False) takes the caller's word in place of is_cut(stats, scenecut) and runs no analyzer for that
    frame (lookahead.Lookahead decides with later frames in view); g, min_keyint, intra_period, reset_interval and scene_cuts
    stay the encoder's.  cut=None is the analysis above; without scenecut a cut= is refused (ValueError).

    rate (a ratecontrol.RateController, None = off: the fixed qp_i / qp_p above, nothing launched): target-bitrate control.
    Both models then estimate every frame's payload size on the device (their rate_estimate attribute is set); before a
    frame's qp is chosen the controller is fed the previous frame's estimate plus the container's bytes - the same number
    with and without defer_stream, since it never waits for the exact stream - and gives the base qp: a P frame is coded at
    shift_qp(base, INDEX_MAP[g % 8]), an I frame at rate.i_qp(base).  Per frame: rc_qp (the qp in the packet), rc_est_bytes
    (what the controller was fed) and rc_bytes (payload + container bytes, filled in when the packet comes out).

    digest (False = off: nothing launched, the packets of today): every packet carries the digest of the entry its frame put
    into the DPB (digest.StateDigest on the encode stream, right behind the call that made the entry; the P frame's feature
    buffer is overwritten by the next frame, which stream order puts behind the read).  Without defer_stream encode() waits
    for the digest's event - the tail of the frame's kernels it otherwise leaves in flight - before it returns the packet;
    with it the value is read when the packet comes out, one call later.  With rate control the unit's 9 bytes count in what
    the controller is fed and in rc_bytes.

    grain (None = off: nothing changes): film grain for the decoder to synthesise (docs/film_grain.md).  A grain.GrainParams:
    every I frame's packet carries it.  A callable (x, x_hat) -> GrainParams | None: called at every I frame with the
    encoder's input and the I frame's reconstruction, and the packet carries what it returns (None: no unit); refused
    together with defer_stream, where the picture is not at hand when the packet is made.  grain_units lists what was
    attached.  With rate control a unit's 14 bytes count in what the controller is fed and in rc_bytes of its I frame."""

    def __init__(self, i_net, p_net, qp_i, qp_p=None, intra_period=-1, reset_interval=32, defer_stream=False,
                 scenecut=None, min_keyint=4, analyzer=None, rate=None, digest=False, grain=None):
        self.i_net, self.p_net = i_net, p_net
        self.defer = defer_stream
        self._held = None            # (qp, use_ada_i, chunked, digest handle) of the P frame whose stream is still pending
        self.digest = bool(digest)
        self._digester = None        # (made at the first frame, on the frame's device)
        if callable(grain) and defer_stream:
            raise ValueError("a grain estimator cannot be combined with defer_stream: give the GrainParams themselves")
        self.grain = grain
        self.grain_units = []
        self.qp_i = qp_i
        self.qp_p = qp_i if qp_p is None else qp_p
        self.intra_period = intra_period
        self.reset_interval = reset_interval
        self.frame_idx = 0
        self.last_qp = 0
        self.scenecut = int(scenecut) if scenecut else 0
        if self.scenecut < 0 or min_keyint < 1:
            raise ValueError("scenecut is a percentage >= 0 and min_keyint is at least 1")
        self.min_keyint = int(min_keyint)
        self._analyzer = analyzer if self.scenecut else None      # (made at the first frame, on the frame's device)
        self._gop_pos = 0            # g of the previous frame
        self.scene_cuts = []
        self.rate = rate
        self.rc_qp, self.rc_est_bytes, self.rc_bytes = [], [], []
        self._rc_pending = None      # (class, base qp, estimated bytes) of the frame coded last, not yet fed back
        self._rc_out = 0             # packets handed out so far (their order is the frame order)
        if rate is not None:
            i_net.rate_estimate = p_net.rate_estimate = True
        p_net.set_curr_poc(0)

    def encode(self, x_padded, ready=None, cut=None):
        from .models import CAPTURE_GUARD
        if cut is not None and not self.scenecut:
            raise ValueError("encode(cut=...) places adaptive I frames: it needs an encoder made with scenecut")
        with CAPTURE_GUARD.frame():          # (a HIP graph capture on another thread waits for / holds back this frame)
            if self.scenecut:
                return self._sized(self._encode_adaptive(x_padded, ready, cut))
            return self._sized(self._encode(x_padded))

    def _sized(self, pkts):
        """rate control's log: the exact size of every packet handed out (never fed back to the controller)"""
        if self.rate is not None:
            from .bitstream import frame_overhead_bytes
            from .bitstream import REPEAT_UNIT_BYTES
            for pkt in (pkts if isinstance(pkts, list) else [pkts]):
                n = len(pkt.bit_stream)
                if getattr(pkt, "repeat", False):        # (the unit is its header: no qp, no length, no digest)
                    self.rc_bytes.append(REPEAT_UNIT_BYTES)
                else:
                    self.rc_bytes.append(n + frame_overhead_bytes(n) + self._unit_bytes(getattr(pkt, "grain", None)))
                self.rate.record_exact(self._rc_out, n)
                self._rc_out += 1
        return pkts

    def _rc_feed(self):
        """feeds the estimate of the frame coded last to the controller, once"""
        if self._rc_pending is not None:
            klass, base, est = self._rc_pending
            self.rate.observe(klass, base, 8 * est)
            self._rc_pending = None

    def _rc_base(self):
        """feeds the previous frame's estimate to the controller and returns the base qp of this frame"""
        self._rc_feed()
        return self.rate.base_qp()

    def _rc_note(self, klass, base, qp, enc, grain=None):
        from .bitstream import frame_overhead_bytes
        est = int(enc["est_bytes"])          # (compress() has waited for the hand-off's event, not for the host coder)
        est += frame_overhead_bytes(est) + self._unit_bytes(grain)
        self._rc_pending = (klass, base, est)
        self.rc_qp.append(qp)
        self.rc_est_bytes.append(est)

    def _unit_bytes(self, grain=None):
        from .bitstream import DIGEST_UNIT_BYTES, GRAIN_UNIT_BYTES
        return (DIGEST_UNIT_BYTES if self.digest else 0) + (GRAIN_UNIT_BYTES if grain is not None else 0)

    def _grain_of(self, x_padded, x_hat):
        """the I frame's grain unit (None: none)"""
        grain = self.grain(x_padded, x_hat) if callable(self.grain) else self.grain
        if grain is not None:
            self.grain_units.append(grain)
        return grain

    def _enqueue_digest(self):
        """digest on: the handle of the newest DPB entry's digest, enqueued on the current stream"""
        if not self.digest:
            return None
        entry = _dpb_entry(self.p_net)
        if self._digester is None:
            from .digest import StateDigest
            self._digester = StateDigest(entry.device)
        return self._digester.enqueue(entry)

    def _take_held(self, stream):
        out = []
        if self._held is not None and stream is not None:
            qp, use_ada_i, chunked, handle = self._held
            out.append(FramePacket(False, qp, use_ada_i, stream, chunked=chunked,
                                   digest=None if handle is None else handle.value()))
            self._held = None
        return out

    def _encode(self, x_padded):
        fi = self.frame_idx
        self.frame_idx += 1
        return self._code(x_padded, fi == 0 or (self.intra_period > 0 and fi % self.intra_period == 0), fi)

    def _encode_adaptive(self, x_padded, ready, cut=None):
        fi = self.frame_idx
        self.frame_idx += 1
        if cut is None:
            from .analysis import is_cut
            if self._analyzer is None:
                from .analysis import FrameAnalyzer
                self._analyzer = FrameAnalyzer(x_padded.device)
            stats = self._analyzer.analyze(x_padded, ready)      # every frame: the next one needs this one's plane
            looks_cut = is_cut(stats, self.scenecut)
        else:
            looks_cut = bool(cut)                                # the caller's word (lookahead.Lookahead): no analyzer runs
        g = self._gop_pos + 1
        cut = fi > 0 and g >= self.min_keyint and looks_cut
        is_i = fi == 0 or cut or (self.intra_period > 0 and g == self.intra_period)
        if cut:
            self.scene_cuts.append(fi)
        self._gop_pos = 0 if is_i else g
        return self._code(x_padded, is_i, self._gop_pos)

    def _code(self, x_padded, is_i, pos):
        """pos: what the P-frame rules count - the frame index (the reference), or the distance to the last I frame"""
        if is_i:
            done = self._take_held(self.p_net.finish_stream()) if self.defer else []
            base = self._rc_base() if self.rate is not None else None
            qp_i = self.qp_i if base is None else self.rate.i_qp(base)
            enc = self.i_net.compress(x_padded, qp_i)
            grain = self._grain_of(x_padded, enc["x_hat"]) if self.grain is not None else None
            if base is not None:
                from .ratecontrol import I_CLASS
                self._rc_note(I_CLASS, base, qp_i, enc, grain)
            self.p_net.clear_dpb()
            self.p_net.add_ref_frame(None, enc["x_hat"])
            handle = self._enqueue_digest()
            pkt = FramePacket(True, qp_i, 0, enc["bit_stream"], chunked=bool(enc.get("chunked", False)),
                              digest=None if handle is None else handle.value(), grain=grain)
            return done + [pkt] if self.defer else pkt
        use_ada_i = 0
        if self.reset_interval > 0 and pos % self.reset_interval == 1:
            use_ada_i = 1
            self.p_net.prepare_feature_adaptor_i(self.last_qp)
        base = self._rc_base() if self.rate is not None else self.qp_p
        qp = self.p_net.shift_qp(base, INDEX_MAP[pos % 8])
        enc = self.p_net.compress(x_padded, qp, defer_stream=self.defer)
        if self.rate is not None:
            self._rc_note(INDEX_MAP[pos % 8], base, qp, enc)
        self.last_qp = qp
        handle = self._enqueue_digest()
        chunked = bool(enc.get("chunked", False))         # (the models' entropy="device" mode: NAL_*_CHUNKED)
        if not self.defer:
            return FramePacket(False, qp, use_ada_i, enc["bit_stream"], chunked=chunked,
                               digest=None if handle is None else handle.value())
        done = self._take_held(enc.get("bit_stream_prev"))
        self._held = (qp, use_ada_i, chunked, handle)
        return done

    def repeat(self):
        """the frame is the picture of the frame before (docs/frame_repeat.md) -> its repeat packet; with defer_stream a
        list: the held P packet, finished first so that the order is kept, then the repeat packet.  ValueError before the
        first frame.  Nothing is launched and no counter moves: frame_idx, the GOP position, reset_interval and the
        INDEX_MAP cycle are untouched, so the coded frames are exactly the sequence they would be with the repeated frames
        deleted from the source - intra_period and min_keyint thereby count CODED frames.  With rate control the pending
        observation is fed first, then the controller is told of a frame of 8 bits that was not coded
        (RateController.skip: the budget a repeat frees goes to its neighbours, the model learns nothing); rc_qp repeats
        the last qp, rc_est_bytes and rc_bytes get the unit's one byte."""
        from .bitstream import REPEAT_UNIT_BYTES
        from .models import CAPTURE_GUARD
        if self.frame_idx == 0:
            raise ValueError("repeat() before the first frame: there is no picture to repeat")
        with CAPTURE_GUARD.frame():
            done = self._take_held(self.p_net.finish_stream()) if self.defer else []
            if self.rate is not None:
                self._rc_feed()
                self.rate.skip(8 * REPEAT_UNIT_BYTES)
                self.rc_qp.append(self.rc_qp[-1])
                self.rc_est_bytes.append(REPEAT_UNIT_BYTES)
            pkt = FramePacket(False, 0, 0, b"", repeat=True)
            return self._sized(done + [pkt] if self.defer else pkt)

    def flush(self):
        """defer_stream: the packet still pending (empty list otherwise)"""
        from .models import CAPTURE_GUARD
        with CAPTURE_GUARD.frame():
            return self._sized(self._take_held(self.p_net.finish_stream()) if self.defer else [])


class SequenceDecoder:
    """defer_output=False: decode(pkt) returns the packet's picture (the reference's loop).
    defer_output=True: P pictures come out one call late - decode(pkt) returns a LIST of the pictures completed
    by the call, in order (usually one: the previous frame), flush() the rest; the reconstruction network of a
    P frame then runs inside the host entropy-decoding gaps of the next frame (DMC.decompress).

    A packet that carries a digest (docs/state_digest.md) is checked, one without is not: behind the frame's entry into the
    DPB the device forms the entry's digest and compares it with the packet's.  The result is read lazily - at the start of
    the next decode(), in flush() (so call it at the end of a stream, deferring or not) and in check_digests() for callers
    that have synchronised anyway - and a difference raises _lib.DigestMismatch naming the frame's index in decode order;
    digests_checked counts the frames that passed.  After a mismatch resume at the next I frame, as after DcvcError.

    A repeat packet (docs/frame_repeat.md) gives the previous picture, the same tensor: nothing is launched, the DPB and the
    digests are not touched, frame_idx counts it; with defer_output the pending picture is finished first and both come out
    in order.  Before any picture it raises DcvcError."""

    def __init__(self, i_net, p_net, height, width, use_two, defer_output=False):
        self.i_net, self.p_net = i_net, p_net
        self.h, self.w, self.two = height, width, use_two
        self.defer = defer_output
        self.frame_idx = 0           # packets handed to decode() so far
        self.digests_checked = 0
        self._digester = None        # (made at the first packet with a digest, on the entry's device)
        self._unchecked = []         # (index, is_i, expected, handle) of the digests enqueued and not yet read
        self._last_pic = None        # the picture handed out last: what a repeat packet shows again
        p_net.set_curr_poc(0)

    def decode(self, pkt):
        from .models import CAPTURE_GUARD
        with CAPTURE_GUARD.frame():
            self._check_digests()
            index, self.frame_idx = self.frame_idx, self.frame_idx + 1
            if getattr(pkt, "repeat", False):
                return self._repeat()
            out = self._decode(pkt)
            last = out[-1:] if self.defer else [out]
            if last:
                self._last_pic = last[0]
            expected = getattr(pkt, "digest", None)
            if expected is not None:
                entry = _dpb_entry(self.p_net)
                if self._digester is None:
                    from .digest import StateDigest
                    self._digester = StateDigest(entry.device)
                self._unchecked.append((index, pkt.is_i, expected, self._digester.enqueue(entry, expected)))
            return out

    def _check_digests(self):
        from ._lib import DigestMismatch
        from .digest import EQUAL
        while self._unchecked:
            index, is_i, expected, handle = self._unchecked.pop(0)
            if handle.status() != EQUAL:
                raise DigestMismatch(index, is_i, expected, handle.value())
            self.digests_checked += 1

    def _repeat(self):
        """a repeat packet: the previous picture, the same tensor; nothing is launched, the DPB and the digests stay as they
        are.  defer_output: the pending picture is finished first, as an I frame finishes it, and both are returned"""
        from ._lib import DcvcError
        done = []
        if self.defer:
            last = self.p_net.finish_output()
            if last is not None:
                done.append(last)
                self._last_pic = last
        if self._last_pic is None:
            raise DcvcError("a repeat packet before any picture: there is nothing to repeat")
        done.append(self._last_pic)
        return done if self.defer else done[-1]

    def check_digests(self):
        """reads the digests enqueued so far (waits for the newest one's event: free behind a synchronisation)"""
        from .models import CAPTURE_GUARD
        with CAPTURE_GUARD.frame():
            self._check_digests()

    def _decode(self, pkt):
        sps = dict(height=self.h, width=self.w, ec_part=1 if self.two else 0, use_ada_i=pkt.use_ada_i)
        done = []
        # the payload's mode comes with the packet (its NAL type); codecs without the mode never see the keyword
        mode = {"chunked": bool(getattr(pkt, "chunked", False))} if hasattr(self.p_net, "entropy") else {}
        if pkt.is_i:
            if self.defer:
                last = self.p_net.finish_output()
                if last is not None:
                    done.append(last)
            dec = self.i_net.decompress(pkt.bit_stream, sps, pkt.qp, **mode)
            self.p_net.clear_dpb()
            self.p_net.add_ref_frame(None, dec["x_hat"])
            done.append(dec["x_hat"])
        else:
            if pkt.use_ada_i:
                self.p_net.reset_ref_feature()
            dec = self.p_net.decompress(pkt.bit_stream, sps, pkt.qp, defer_output=self.defer, **mode)
            for k in ("x_hat_prev", "x_hat"):
                if dec.get(k) is not None:
                    done.append(dec[k])
        return done if self.defer else done[-1]

    def flush(self):
        from .models import CAPTURE_GUARD
        with CAPTURE_GUARD.frame():
            last = self.p_net.finish_output() if self.defer else None
            self._check_digests()
        if last is not None:
            self._last_pic = last
        return [] if last is None else [last]


@dataclass
class DecodedFrame:
    x_hat: object                    # the decoded picture at the size it is displayed at: what metrics read
    shown: object                    # x_hat with the film grain in force on it: what gets stored (x_hat itself without grain)
    sps: dict
    is_i: bool
    display: Optional[tuple]         # StreamReader.display / grain / grain_t behind this frame
    grain: Optional[object]
    grain_t: int
    active: Optional[object] = None  # StreamReader.active behind this frame: x_hat and shown are then the full picture
    repeat: bool = False             # a repeat unit (docs/frame_repeat.md): the picture of the frame before, its own grain_t


class StreamDecoder:
    """Container in, pictures out: the decode-side entry point.  Owns the StreamReader of the binary file-like `f`, the
    SequenceDecoder (sequential: defer_output=False; made at the first frame, from then on it follows every frame's SPS) and
    what the stream's extension units ask for behind it - the display unit's resample (docs/reduced_resolution.md) and the
    grain unit's synthesis (docs/film_grain.md), then the active-area unit's paste into the full picture
    (docs/active_area.md; one paste without grain, shown is x_hat then as ever).  scaler / grainer: a resize.Resampler / grain.FilmGrain to use; otherwise
    each is made when the stream first needs one, so a stream without these units launches the decoder's own kernels only.
    A repeat unit (docs/frame_repeat.md) decodes and resamples nothing: the frame keeps the last resampled picture, gets the
    grain of its own grain_t - the grain moves on a still picture - and is pasted as any frame; DecodedFrame.repeat says so."""

    def __init__(self, f, i_net, p_net, device, scaler=None, grainer=None):
        from .bitstream import StreamReader
        self.reader = StreamReader(f)
        self.i_net, self.p_net, self.device = i_net, p_net, device
        self.scaler, self.grainer = scaler, grainer
        self.dec = None
        self._resampled = None       # (picture at its display size, that size) of the frame before: what a repeat unit shows

    def next(self):
        """the next frame of the stream -> DecodedFrame; everything is enqueued on the current stream, nothing is waited for"""
        rd = self.reader
        sps, pkt = rd.read_packet()
        size = (sps["height"], sps["width"])
        if self.dec is None:
            self.dec = SequenceDecoder(self.i_net, self.p_net, *size, bool(sps["ec_part"]))
        self.dec.h, self.dec.w, self.dec.two = *size, bool(sps["ec_part"])
        x_hat = self.dec.decode(pkt)
        if pkt.repeat:                               # the picture as it was resampled for the frame it repeats
            x_hat, size = self._resampled
        elif rd.display is not None:
            if self.scaler is None:
                from .resize import Resampler
                self.scaler = Resampler(self.device)
            x_hat, size = self.scaler.resample(x_hat, size, rd.display[:2], rd.display[2]), rd.display[:2]
        self._resampled = (x_hat, size)
        shown = x_hat
        if rd.grain is not None:
            if self.grainer is None:
                from .grain import FilmGrain
                self.grainer = FilmGrain(self.device)
            shown = self.grainer.apply(x_hat, size, rd.grain, rd.grain_t)
        if rd.active is not None:                    # the grain went onto the window's picture: the bars stay clean
            from .bars import paste
            full = paste(x_hat, rd.active)
            x_hat, shown = full, (full if shown is x_hat else paste(shown, rd.active))
            return DecodedFrame(x_hat, shown, sps, pkt.is_i, rd.display, rd.grain, rd.grain_t, rd.active, repeat=pkt.repeat)
        return DecodedFrame(x_hat, shown, sps, pkt.is_i, rd.display, rd.grain, rd.grain_t, repeat=pkt.repeat)

    def check_digests(self):
        if self.dec is not None:
            self.dec.check_digests()

    @property
    def digests_checked(self):
        return self.dec.digests_checked if self.dec is not None else 0

    def flush(self):
        """at the end of a stream: reads the digests still unchecked"""
        if self.dec is not None:
            self.dec.flush()


class EncodeDecodePipeline:
    """Encoder and decoder of one stream as a two-stage pipeline on one GPU: each stage has its own host
    thread and HIP stream, so frame n is decoded while frame n+1 is encoded and one stage's host entropy
    coding overlaps the other stage's kernels.  (The reference runs the two loops one after the other,
    test_video.py:164-214 then :258-285; the frames, packets and reconstructions are the same.)"""

    def __init__(self, encoder, decoder, device, depth=None):
        import os
        import torch
        if depth is None:
            depth = int(os.environ.get("DCVC_PIPE_DEPTH", "4"))
        self.encoder, self.decoder, self.device, self.depth = encoder, decoder, device, depth
        # (a high-priority decoder stream was measured: no difference - the pair is GPU-bound either way)
        self.enc_stream, self.dec_stream = torch.cuda.Stream(device), torch.cuda.Stream(device)

    @staticmethod
    def _emit(frames, on_frame):
        if on_frame is not None:
            for x in (frames if isinstance(frames, list) else [frames]):
                on_frame(x)

    def run(self, frames, on_packet=None, on_frame=None):
        """frames: iterable of padded model inputs (device tensors, ready on the calling stream); REPEAT in place of a frame
        that is the picture of the one before (docs/frame_repeat.md): its repeat packet travels in order like any other.
        on_packet(pkt) is called on the encoder thread, on_frame(x_hat) on the decoder thread with the
        decoder stream current.  Returns when every frame has been encoded and decoded."""
        import queue
        import threading
        import torch
        from .models import CAPTURE_GUARD
        torch.cuda.current_stream().synchronize()
        frames = iter(frames)
        # HIP graph captures (first frames, new resolutions, new variants) are serialised against the other
        # stage's host calls by models.CAPTURE_GUARD inside encode() / decode(): no warm-up phase is needed.
        q = queue.Queue(maxsize=self.depth)
        errors = []

        def enc_stage():
            try:
                torch.cuda.set_device(self.device)
                with torch.cuda.stream(self.enc_stream):
                    def emit(pkts):
                        # a deferring encoder (SequenceEncoder(defer_stream=True)) returns a LIST of packets - the previous
                        # frame's, possibly none - and keeps the last one until flush()
                        for pkt in (pkts if isinstance(pkts, (list, tuple)) else [pkts]):
                            if on_packet is not None:
                                with CAPTURE_GUARD.frame():     # the callback may touch the device too
                                    on_packet(pkt)
                            q.put(pkt)                          # (never block on the queue inside the scope)

                    for x in frames:
                        with CAPTURE_GUARD.frame():
                            pkts = self.encoder.repeat() if x is REPEAT else self.encoder.encode(x)
                        emit(pkts)
                    if getattr(self.encoder, "defer", False):
                        with CAPTURE_GUARD.frame():
                            pkts = self.encoder.flush()
                        emit(pkts)
                    with CAPTURE_GUARD.frame():
                        self.enc_stream.synchronize()
            except BaseException as e:                      # re-raised by run()
                errors.append(e)
            finally:
                q.put(None)

        def dec_stage():
            try:
                torch.cuda.set_device(self.device)
                with torch.cuda.stream(self.dec_stream):
                    while True:
                        pkt = q.get()
                        if pkt is None:
                            break
                        with CAPTURE_GUARD.frame():
                            self._emit(self.decoder.decode(pkt), on_frame)
                    with CAPTURE_GUARD.frame():
                        self._emit(self.decoder.flush(), on_frame)
                        self.dec_stream.synchronize()
            except BaseException as e:
                errors.append(e)
                while q.get() is not None:                  # keep the encoder from blocking on a full queue
                    pass

        # The two stage threads share the interpreter lock: with the default 5 ms switch interval a stage that becomes
        # runnable (its GPU event fired, its packet arrived) may wait that long for the other stage's Python code; 0.2 ms
        # for the duration of the run (steadier frame times: profiles/r04_host_threads_ab.txt)
        import sys
        old_interval = sys.getswitchinterval()
        sys.setswitchinterval(min(old_interval, 2e-4))
        threads = [threading.Thread(target=enc_stage), threading.Thread(target=dec_stage)]
        try:
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            sys.setswitchinterval(old_interval)
        if errors:
            raise errors[0]


def load_yuv420_frame(y, u, v, dtype, pad_to=16):
    """uint8 CUDA planes y [H,W], u/v [H/2,W/2] -> padded model input [1,3,H',W'] (one fused kernel;
    reference: get_src_frame + replicate_pad, test_video.py:74-91,150,179)."""
    import torch
    from . import _lib
    from . import nn as L
    H, W = y.shape
    pr, pb = (-W) % pad_to, (-H) % pad_to
    out = torch.empty((1, 3, H + pb, W + pr), dtype=dtype, device=y.device)
    _lib.check(_lib.lib().dcvc_yuv420_to_frame(L.dtype_code(dtype), L._p(y.contiguous()), L._p(u.contiguous()),
                                               L._p(v.contiguous()), H, W, pb, pr, L._p(out), L._stream()),
               "dcvc_yuv420_to_frame")
    return out


def store_yuv420_frame(x_hat, height, width, round_uv=False):
    """decoded [1,3,H',W'] -> uint8 CUDA planes (y, u, v) of the height x width picture
    (reference: yuv_444_to_420 + clamp*255 + uint8, test_video.py:307-311)."""
    import torch
    from . import _lib
    from . import nn as L
    x = x_hat.contiguous()
    y = torch.empty((height, width), dtype=torch.uint8, device=x.device)
    u = torch.empty((height // 2, width // 2), dtype=torch.uint8, device=x.device)
    v = torch.empty_like(u)
    _lib.check(_lib.lib().dcvc_frame_to_yuv420(*L.frame_args(x, (height, width)), int(round_uv), L._p(y), L._p(u), L._p(v),
                                               L._stream()), "dcvc_frame_to_yuv420")
    return y, u, v


# ---------------------------------------------------------------------------------- the other raw formats
@dataclass(frozen=True)
class PixelFormat:
    """A raw video format the frame I/O kernels of csrc/dcvc_pixfmt.hip read and write: chroma 420 / 444, bit depth
    8 .. 16 (little-endian 16-bit words above 8 bits), planar or semi-planar (Y plane + one plane of interleaved (U, V)
    pairs), value in the low or in the top bits of its word.  PixelFormat.parse(name) knows the ffmpeg spellings below."""
    name: str
    chroma: int
    bit_depth: int
    semi_planar: bool = False
    msb_aligned: bool = False

    def __post_init__(self):
        if self.chroma not in (420, 444) or not 8 <= self.bit_depth <= 16:
            raise ValueError(f"pixel format {self.name!r}: chroma 420 / 444 and 8 .. 16 bits")
        if (self.semi_planar and self.chroma != 420) or (self.msb_aligned and self.bit_depth == 8):
            raise ValueError(f"pixel format {self.name!r}: semi-planar is 4:2:0, msb_aligned needs more than 8 bits")

    @staticmethod
    def parse(name):
        """'yuv420p10le', 'yuv444p', 'nv12', 'p010le', ... -> PixelFormat; ValueError for any other name ('yuv420', the
        8-bit planar 4:2:0 of the reference harness, keeps its own kernels and is not one of these)"""
        if isinstance(name, PixelFormat):
            return name
        try:
            return PIXEL_FORMATS[name]
        except (KeyError, TypeError):
            raise ValueError(f"unknown pixel format {name!r}: one of {', '.join(PIXEL_FORMATS)}") from None

    @property
    def max_val(self):
        return (1 << self.bit_depth) - 1

    @property
    def sample_bytes(self):
        return 2 if self.bit_depth > 8 else 1

    @property
    def numpy_dtype(self):
        import numpy as np
        return np.dtype("<u2") if self.bit_depth > 8 else np.dtype(np.uint8)

    @property
    def torch_dtype(self):
        import torch
        return torch.uint16 if self.bit_depth > 8 else torch.uint8

    def plane_shapes(self, height, width):
        """shapes of a frame's planes in file order: (y, u, v), or (y, uv) with uv [H/2, W] interleaved for semi-planar"""
        if self.chroma == 420 and (height % 2 or width % 2):
            raise ValueError(f"{self.name}: 4:2:0 needs an even height and width (got {width}x{height})")
        if self.chroma == 444:
            return ((height, width),) * 3
        if self.semi_planar:
            return ((height, width), (height // 2, width))
        return ((height, width), (height // 2, width // 2), (height // 2, width // 2))

    def frame_bytes(self, height, width):
        return sum(h * w for h, w in self.plane_shapes(height, width)) * self.sample_bytes


PIXEL_FORMATS = {f.name: f for f in (
    [PixelFormat(f"yuv420p{b}le", 420, b) for b in (10, 12, 16)] + [PixelFormat("yuv444p", 444, 8)] +
    [PixelFormat(f"yuv444p{b}le", 444, b) for b in (10, 12, 16)] +
    [PixelFormat("nv12", 420, 8, semi_planar=True), PixelFormat("p010le", 420, 10, semi_planar=True, msb_aligned=True)])}


def _plane_args(planes, fmt, height, width, strides):
    """(y, u_or_uv, v_or_None pointers, y_stride, c_stride) for the library; strides in samples (default: tight)"""
    import ctypes
    shapes = fmt.plane_shapes(height, width)
    if len(planes) != len(shapes):
        raise ValueError(f"{fmt.name}: {len(shapes)} planes expected, got {len(planes)}")
    for p in planes:
        if p.element_size() != fmt.sample_bytes:
            raise ValueError(f"{fmt.name}: planes of {fmt.sample_bytes}-byte samples expected, got {p.dtype}")
    ys, cs = strides if strides is not None else (shapes[0][1], shapes[1][1])
    ptrs = [ctypes.c_void_p(p.data_ptr()) for p in planes] + [None] * (3 - len(planes))
    return ptrs, int(ys), int(cs)


def load_frame(planes, fmt, dtype, pad_to=16, height=None, width=None, strides=None):
    """device planes of a PixelFormat -> padded model input [1,3,H',W'] (one kernel: sample / max_val as an fp32
    division, one rounding to `dtype`, nearest chroma up-sampling for 4:2:0, replicate pad - the reference family's
    YUVReader + ycbcr420_to_444 + this project's cast and replicate_pad).  planes: (y, u, v), or (y, uv) for semi-planar;
    uint8, or torch.uint16 / an int16 view above 8 bits.  strides=(y_stride, c_stride) in samples with height / width
    given reads pitched surfaces (flat or wider tensors) in place; by default the planes are tight [H, W] tensors."""
    import torch
    from . import _lib
    from . import nn as L
    fmt = PixelFormat.parse(fmt)
    if strides is None:
        planes = [p.contiguous() for p in planes]
        height, width = planes[0].shape
    if pad_to % 8:
        raise ValueError("pad_to must be a multiple of 8 (the kernels store 8 pixels at a time)")
    ptrs, ys, cs = _plane_args(planes, fmt, height, width, strides)
    pr, pb = (-width) % pad_to, (-height) % pad_to
    out = torch.empty((1, 3, height + pb, width + pr), dtype=dtype, device=planes[0].device)
    _lib.check(_lib.lib().dcvc_planes_to_frame(L.dtype_code(dtype), fmt.chroma, fmt.bit_depth, int(fmt.semi_planar),
                                               int(fmt.msb_aligned), *ptrs, ys, cs, height, width, pb, pr, L._p(out),
                                               L._stream()), "dcvc_planes_to_frame")
    return out


def store_frame(x_hat, height, width, fmt):
    """decoded [1,3,H',W'] -> the device planes of the height x width picture in `fmt` ((y, u, v), or (y, uv) for
    semi-planar; uint8 / torch.uint16): crop, fp32, 4:2:0 chroma = 2x2 mean, clip(., 0, 1) * max_val, round to nearest
    even, clip (the reference family's ycbcr444_to_420 + YUVWriter), shifted up for msb-aligned formats."""
    import torch
    from . import _lib
    from . import nn as L
    fmt = PixelFormat.parse(fmt)
    x = x_hat.contiguous()
    planes = [torch.empty(s, dtype=fmt.torch_dtype, device=x.device) for s in fmt.plane_shapes(height, width)]
    ptrs, ys, cs = _plane_args(planes, fmt, height, width, None)
    code, *frame = L.frame_args(x, (height, width))
    _lib.check(_lib.lib().dcvc_frame_to_planes(code, fmt.chroma, fmt.bit_depth, int(fmt.semi_planar), int(fmt.msb_aligned),
                                               *frame, *ptrs, ys, cs, L._stream()), "dcvc_frame_to_planes")
    return tuple(planes)


def use_two_entropy_coders(height, width):
    """test_video.py:152"""
    return height * width > 1280 * 720
