"""Bitstream container of DCVC-RT: SPS / I / P NAL units with variable-length integers, byte-compatible
with the reference's ``src/utils/stream_helper.py`` (write_uint_adaptive :68-89, read_uint_adaptive
:92-105, NalType :108, SPSHelper :114-145, write_sps :148-162, read_header :165-184,
read_sps_remaining :187-195, write_ip :198-209, read_ip_remaining :212-217), so ``.bin`` files are
interchangeable with the reference's encoder / decoder.  Same function names for drop-in use; `f` is any
binary file-like object (io.BytesIO, open(..., 'wb')).

Layout:  NAL header byte = type(4 bits) | sps_id(4 bits)
  SPS :  header, height (varint), width (varint), flags = ec_part << 2 | use_ada_i
  I/P :  header, qp (1 byte), payload length (varint), payload (the rANS stream of the frame)
         (types 3 / 4 = I / P with a chunked payload: this project's extension, docs/chunked_stream.md)
  DIGEST: header (type 5), 8 bytes: the digest, little endian, of the entry the NEXT unit's frame puts into the DPB - that
         unit must be an I or P unit.  This project's extension (docs/state_digest.md): the reference's reader rejects
         type 5, streams written without digests are unchanged.
  DISPLAY: header (type 6), display height (varint), display width (varint), filter id (1 byte: 0 bilinear, 1 bicubic,
         2 lanczos3): the pictures of this SPS are to be resampled to that size after decoding.  Written directly behind
         an SPS.  This project's extension (docs/reduced_resolution.md): the reference's reader rejects type 6, streams
         written without it are unchanged.
  GRAIN: header (type 7), 13 bytes: seed (2 bytes, little endian), corr (0, 1, 2), the eight luma strengths, the Cb and the Cr
         strength (grain.GrainParams): film grain to be put on the displayed pictures from the NEXT unit's frame on, until
         the next grain unit; all strengths 0 switches it off.  Written in front of an I frame, in front of its digest unit
         if it has one.  This project's extension (docs/film_grain.md): the reference's reader rejects type 7, streams
         written without it are unchanged.
  ACTIVE: header (type 8), full height, full width, top, left (varints), the bars' colour (3 x 4 bytes: Y, U, V as
         little-endian fp32): the pictures of this SPS - at their display size if the SPS has a display unit, else at the
         SPS's size - are the window at (top, left) of a full height x full width picture that is `colour` everywhere else.
         Written behind an SPS, after its display unit.  This project's extension (docs/active_area.md): the reference's
         reader rejects type 8, streams written without it are unchanged.
  REPEAT: header (type 9) and nothing else: show the picture of the frame before once more.  sps_id is that frame's.  It
         counts as a frame (a grain unit's counter goes on), changes no decoder state, and no SPS, digest or grain unit
         is written for it.  This project's extension (docs/frame_repeat.md): the reference's reader rejects type 9,
         streams written without it are unchanged.
varint:  0xxxxxxx                      value < 2**7
         10xxxxxx xxxxxxxx             value < 2**14   (big endian)
         11xxxxxx + 3 bytes            value < 2**30   (big endian)
"""
import enum


class NalType(enum.IntEnum):
    NAL_SPS = 0
    NAL_I = 1
    NAL_P = 2
    # this project's extension (docs/chunked_stream.md), not readable by the reference: same NAL layout, the payload carries
    # the y symbols in independent chunks that the GPU entropy-codes
    NAL_I_CHUNKED = 3
    NAL_P_CHUNKED = 4
    # this project's extension (docs/state_digest.md), not readable by the reference: the digest of the decoder state behind
    # the frame unit that follows
    NAL_DIGEST = 5
    # this project's extension (docs/reduced_resolution.md), not readable by the reference: the size the pictures of an SPS
    # are shown at, and the filter that takes them there
    NAL_DISPLAY = 6
    # this project's extension (docs/film_grain.md), not readable by the reference: the film grain to synthesise on the
    # displayed pictures from the next frame on
    NAL_GRAIN = 7
    # this project's extension (docs/active_area.md), not readable by the reference: the full picture the pictures of an SPS
    # are a window of, and the colour of the rest
    NAL_ACTIVE = 8
    # this project's extension (docs/frame_repeat.md), not readable by the reference: the picture of the frame before, again
    NAL_REPEAT = 9


DISPLAY_FILTERS = ("bilinear", "bicubic", "lanczos3")       # filter id = position (resize.FILTERS)


def write_uint_adaptive(f, value):
    if value < 0 or value >= (1 << 30):
        raise ValueError(f"varint out of range: {value}")
    if value < (1 << 7):
        data = bytes((value,))
    elif value < (1 << 14):
        data = bytes((0x80 | (value >> 8), value & 0xff))
    else:
        data = bytes((0xc0 | (value >> 24), (value >> 16) & 0xff, (value >> 8) & 0xff, value & 0xff))
    f.write(data)
    return len(data)


def _byte(f):
    b = f.read(1)
    if len(b) != 1:
        raise EOFError("truncated DCVC-RT stream")
    return b[0]


def read_uint_adaptive(f):
    first = _byte(f)
    if first < 0x80:
        return first
    if (first >> 6) == 0x02:
        return ((first & 0x3f) << 8) | _byte(f)
    rest = f.read(3)
    if len(rest) != 3:
        raise EOFError("truncated DCVC-RT stream")
    return ((first & 0x3f) << 24) | (rest[0] << 16) | (rest[1] << 8) | rest[2]


class SPSHelper:
    """Deduplicates sequence parameter sets (at most 16 ids), reference stream_helper.py:114-145."""
    _KEYS = ("height", "width", "use_ada_i", "ec_part")

    def __init__(self):
        self.spss = []

    def get_sps_id(self, target_sps):
        for sps in self.spss:
            if all(sps[k] == target_sps[k] for k in self._KEYS):
                return sps["sps_id"], False
        new_id = max((s["sps_id"] for s in self.spss), default=-1) + 1
        if new_id > 15:
            raise ValueError("more than 16 distinct SPS in one stream")
        sps = dict(target_sps, sps_id=new_id)
        self.spss.append(sps)
        return new_id, True

    def add_sps_by_id(self, sps):
        for i, s in enumerate(self.spss):
            if s["sps_id"] == sps["sps_id"]:
                self.spss[i] = dict(sps)
                return
        self.spss.append(dict(sps))

    def get_sps_by_id(self, sps_id):
        for s in self.spss:
            if s["sps_id"] == sps_id:
                return s
        return None


def write_sps(f, sps):
    if not (0 <= sps["sps_id"] < 16 and sps["use_ada_i"] in (0, 1) and sps["ec_part"] in (0, 1)):
        raise ValueError(f"bad SPS {sps}")
    f.write(bytes(((int(NalType.NAL_SPS) << 4) | sps["sps_id"],)))
    n = 1 + write_uint_adaptive(f, sps["height"]) + write_uint_adaptive(f, sps["width"])
    f.write(bytes(((sps["ec_part"] << 2) | sps["use_ada_i"],)))
    return n + 1


def read_header(f):
    flag = _byte(f)
    nal_type = flag >> 4
    header = {"nal_type": NalType(nal_type)}
    header["sps_id"] = flag & 0x0f
    return header


def read_sps_remaining(f, sps_id):
    height = read_uint_adaptive(f)
    width = read_uint_adaptive(f)
    flag = _byte(f)
    return {"sps_id": sps_id, "height": height, "width": width, "ec_part": (flag >> 2) & 1, "use_ada_i": flag & 1}


def write_ip(f, is_i_frame, sps_id, qp, bit_stream, chunked=False):
    if not 0 <= qp < 256:
        raise ValueError(f"qp {qp} out of range")
    if chunked:
        nal = NalType.NAL_I_CHUNKED if is_i_frame else NalType.NAL_P_CHUNKED
    else:
        nal = NalType.NAL_I if is_i_frame else NalType.NAL_P
    f.write(bytes(((int(nal) << 4) | sps_id, qp)))
    n = 2 + write_uint_adaptive(f, len(bit_stream))
    f.write(bit_stream)
    return n + len(bit_stream)


DIGEST_UNIT_BYTES = 9        # header + 8


def write_digest(f, sps_id, digest):
    if not 0 <= digest < (1 << 64):
        raise ValueError(f"digest {digest} is not a 64-bit word")
    f.write(bytes(((int(NalType.NAL_DIGEST) << 4) | sps_id,)) + int(digest).to_bytes(8, "little"))
    return DIGEST_UNIT_BYTES


def read_digest_remaining(f):
    data = f.read(8)
    if len(data) != 8:
        raise EOFError("truncated DCVC-RT digest unit")
    return int.from_bytes(data, "little")


GRAIN_UNIT_BYTES = 14        # header + grain.UNIT_BODY_BYTES


def write_grain(f, sps_id, params):
    """params: a grain.GrainParams"""
    if not 0 <= sps_id < 16:
        raise ValueError(f"bad sps_id {sps_id}")
    f.write(bytes(((int(NalType.NAL_GRAIN) << 4) | sps_id,)) + params.to_bytes())
    return GRAIN_UNIT_BYTES


def read_grain_remaining(f):
    """-> grain.GrainParams; ValueError for a corr above 2, EOFError for a unit cut short"""
    from .grain import GrainParams
    data = f.read(GRAIN_UNIT_BYTES - 1)
    if len(data) != GRAIN_UNIT_BYTES - 1:
        raise EOFError("truncated DCVC-RT grain unit")
    return GrainParams.from_bytes(data)


def write_display(f, sps_id, height, width, filter_name):
    if filter_name not in DISPLAY_FILTERS:
        raise ValueError(f"display filter {filter_name!r}: one of {', '.join(DISPLAY_FILTERS)}")
    if not 0 <= sps_id < 16:
        raise ValueError(f"bad sps_id {sps_id}")
    f.write(bytes(((int(NalType.NAL_DISPLAY) << 4) | sps_id,)))
    n = 1 + write_uint_adaptive(f, height) + write_uint_adaptive(f, width)
    f.write(bytes((DISPLAY_FILTERS.index(filter_name),)))
    return n + 1


def read_display_remaining(f):
    """-> (height, width, filter_name)"""
    height = read_uint_adaptive(f)
    width = read_uint_adaptive(f)
    fid = _byte(f)
    if fid >= len(DISPLAY_FILTERS):
        raise ValueError(f"display unit with unknown filter id {fid}")
    return height, width, DISPLAY_FILTERS[fid]


def write_active(f, sps_id, area):
    """area: a bars.ActiveArea (only the full size, the offsets and the colour are written: the window's size is the
    display unit's, else the SPS's)"""
    import struct
    if not 0 <= sps_id < 16:
        raise ValueError(f"bad sps_id {sps_id}")
    f.write(bytes(((int(NalType.NAL_ACTIVE) << 4) | sps_id,)))
    n = 1 + sum(write_uint_adaptive(f, v) for v in (area.full_height, area.full_width, area.top, area.left))
    f.write(struct.pack("<3f", *area.colour))
    return n + 12


def read_active_remaining(f):
    """-> (full_height, full_width, top, left, colour); ValueError for a unit cut short"""
    import struct
    try:
        full_h, full_w, top, left = (read_uint_adaptive(f) for _ in range(4))
    except EOFError:
        raise ValueError("truncated DCVC-RT active-area unit") from None
    data = f.read(12)
    if len(data) != 12:
        raise ValueError("truncated DCVC-RT active-area unit")
    return full_h, full_w, top, left, struct.unpack("<3f", data)


def _active_area(unit, size):
    """the bars.ActiveArea of a unit's fields around a window of size = (height, width); ValueError where the window leaves
    the full picture or starts at an odd offset"""
    from .bars import ActiveArea
    full_h, full_w, top, left, colour = unit
    return ActiveArea(full_h, full_w, top, left, size[0], size[1], tuple(colour))


REPEAT_UNIT_BYTES = 1        # the header


def write_repeat(f, sps_id):
    """sps_id: that of the frame whose picture is repeated"""
    if not 0 <= sps_id < 16:
        raise ValueError(f"bad sps_id {sps_id}")
    f.write(bytes(((int(NalType.NAL_REPEAT) << 4) | sps_id,)))
    return REPEAT_UNIT_BYTES


def frame_overhead_bytes(payload_len):
    """bytes write_ip puts in front of a payload of that length: NAL header, qp, the varint of the length (an SPS, written
    when a frame's parameters are new to the stream - twice in a typical one - is not counted)"""
    return 2 + (1 if payload_len < (1 << 7) else 2 if payload_len < (1 << 14) else 4)


def read_ip_remaining(f):
    qp = _byte(f)
    length = read_uint_adaptive(f)
    bit_stream = f.read(length)
    if len(bit_stream) != length:
        raise EOFError("truncated DCVC-RT frame payload")
    return qp, bit_stream


class StreamWriter:
    """What test_video.py:166,216-224 does per frame: SPS dedup + NAL writing; returns bytes written.  display =
    (height, width, filter_name): the size the decoded pictures are to be resampled to; where it differs from a frame's
    size a display unit follows every SPS the writer emits (None, or equal sizes: the stream of the reference).  A packet
    whose `grain` is a grain.GrainParams gets a grain unit in front of its digest unit / its frame.  active = a
    bars.ActiveArea: the frames are the window of a larger picture (docs/active_area.md); an active-area unit follows every
    SPS the writer emits, after the display unit; its window must be the display size where there is one, else the frame's
    size (None: no unit, the stream of before).  A packet with repeat=True is written as the one-byte repeat unit
    (docs/frame_repeat.md) under the SPS of the frame before it, which must be of the same size; nothing else is written
    for it, and a repeat in front of any frame is a ValueError."""

    def __init__(self, f, display=None, active=None):
        self.f = f
        self.sps_helper = SPSHelper()
        if display is not None:
            display = (int(display[0]), int(display[1]), display[2])
            if display[2] not in DISPLAY_FILTERS:
                raise ValueError(f"display filter {display[2]!r}: one of {', '.join(DISPLAY_FILTERS)}")
        self.display = display
        self.active = active
        self._last_sps = None        # the SPS of the frame written last

    def write_frame(self, height, width, use_two_entropy_coders, pkt):
        if getattr(pkt, "repeat", False):
            last = self._last_sps
            if last is None:
                raise ValueError("a repeat unit in front of any frame: there is no picture to repeat")
            if (last["height"], last["width"]) != (height, width):
                raise ValueError(f"a repeat of a {width}x{height} picture behind a frame of {last['width']}x{last['height']}")
            return write_repeat(self.f, last["sps_id"])
        sps = {"sps_id": -1, "height": height, "width": width, "ec_part": 1 if use_two_entropy_coders else 0,
               "use_ada_i": pkt.use_ada_i}
        scaled = self.display is not None and self.display[:2] != (height, width)
        if scaled and (self.display[0] < height or self.display[1] < width):
            raise ValueError(f"display {self.display[1]}x{self.display[0]} below the coded size {width}x{height}")
        sps_id, is_new = self.sps_helper.get_sps_id(sps)
        sps["sps_id"] = sps_id
        self._last_sps = sps
        n = write_sps(self.f, sps) if is_new else 0
        if is_new and scaled:
            n += write_display(self.f, sps_id, *self.display)
        if self.active is not None:
            shown = self.display[:2] if scaled else (height, width)
            if self.active.size != shown:
                raise ValueError(f"the active area's window {self.active.width}x{self.active.height} is not the pictures' "
                                 f"{shown[1]}x{shown[0]}")
            if is_new:
                n += write_active(self.f, sps_id, self.active)
        if getattr(pkt, "grain", None) is not None:
            n += write_grain(self.f, sps_id, pkt.grain)
        if getattr(pkt, "digest", None) is not None:
            n += write_digest(self.f, sps_id, pkt.digest)
        return n + write_ip(self.f, pkt.is_i, sps_id, pkt.qp, pkt.bit_stream, chunked=getattr(pkt, "chunked", False))


class StreamReader:
    """test_video.py:265-276: yields (sps, is_i_frame, qp, payload) per frame; `chunked` tells whether the frame returned
    last carries a chunked payload (NAL_I_CHUNKED / NAL_P_CHUNKED), `digest` the digest unit in front of it (an int; None:
    the frame came without one), `display` the (height, width, filter_name) of the display unit that belongs to that
    frame's SPS (None until a display unit was read), `grain` the grain.GrainParams in force for that frame (None: no grain
    unit so far, or the last one switched grain off) and `grain_t` the frame's counter since that unit (0 for the frame the
    unit stands in front of), `active` the bars.ActiveArea of the active-area unit that belongs to that frame's SPS (None until
    such a unit was read; it follows the SPS exactly as `display` does), `repeat` whether the frame is a repeat unit
    (docs/frame_repeat.md): read_frame() then returns (sps, False, 0, b"") with the SPS, `display` and `active` of the picture
    it repeats, `digest` None and `grain_t` one further as for any frame.  read_packet() is read_frame() with the frame as a pipeline.FramePacket."""

    def __init__(self, f):
        self.f = f
        self.sps_helper = SPSHelper()
        self.chunked = False
        self.digest = None
        self.display = None
        self._displays = {}          # sps_id -> the display unit behind that SPS
        self._display_seen = False
        self.grain = None
        self.grain_t = 0
        self.active = None
        self._actives = {}           # sps_id -> the active area behind that SPS
        self._active_seen = False
        self.repeat = False
        self._last_sps_id = None     # of the frame returned last

    def read_frame(self):
        header = read_header(self.f)
        digest = None
        grain = None
        while header["nal_type"] in (NalType.NAL_SPS, NalType.NAL_DIGEST, NalType.NAL_DISPLAY, NalType.NAL_GRAIN,
                                     NalType.NAL_ACTIVE):
            if digest is not None:
                raise ValueError(f"a digest unit is followed by {header['nal_type'].name}, not by the frame it describes")
            if header["nal_type"] == NalType.NAL_SPS:
                self.sps_helper.add_sps_by_id(read_sps_remaining(self.f, header["sps_id"]))
                self._displays.pop(header["sps_id"], None)          # (a new SPS under this id: its display unit follows, if any)
                self._actives.pop(header["sps_id"], None)
            elif header["nal_type"] == NalType.NAL_DISPLAY:
                display = read_display_remaining(self.f)
                sps = self.sps_helper.get_sps_by_id(header["sps_id"])
                if sps is None:
                    raise ValueError(f"display unit refers to unknown SPS {header['sps_id']}")
                if header["sps_id"] in self._actives:                # (the active-area unit took its window's size from what stood before it)
                    raise ValueError(f"a display unit follows the active-area unit of SPS {header['sps_id']}: it belongs in front of it")
                if display[0] < sps["height"] or display[1] < sps["width"]:
                    raise ValueError(f"display {display[1]}x{display[0]} below the coded size {sps['width']}x{sps['height']}")
                self._displays[header["sps_id"]] = display
                self._display_seen = True
            elif header["nal_type"] == NalType.NAL_GRAIN:
                grain = read_grain_remaining(self.f)
            elif header["nal_type"] == NalType.NAL_ACTIVE:
                unit = read_active_remaining(self.f)
                sps = self.sps_helper.get_sps_by_id(header["sps_id"])
                if sps is None:
                    raise ValueError(f"active-area unit refers to unknown SPS {header['sps_id']}")
                shown = self._displays.get(header["sps_id"], (sps["height"], sps["width"]))[:2]
                self._actives[header["sps_id"]] = _active_area(unit, shown)
                self._active_seen = True
            else:
                digest = read_digest_remaining(self.f)
            header = read_header(self.f)
        sps = self.sps_helper.get_sps_by_id(header["sps_id"])
        repeat = header["nal_type"] == NalType.NAL_REPEAT
        if repeat:
            for unit, name in ((digest, "digest"), (grain, "grain")):
                if unit is not None:
                    raise ValueError(f"a {name} unit is followed by NAL_REPEAT, not by the frame it describes")
            if sps is None:
                raise ValueError(f"repeat unit refers to unknown SPS {header['sps_id']}")
            if self._last_sps_id is None:
                raise ValueError("a repeat unit stands before the first frame: there is no picture to repeat")
            if header["sps_id"] != self._last_sps_id:
                raise ValueError(f"repeat unit names SPS {header['sps_id']}, the frame before it has SPS {self._last_sps_id}")
            qp, payload = 0, b""
        else:
            if sps is None:
                raise ValueError(f"frame refers to unknown SPS {header['sps_id']}")
            qp, payload = read_ip_remaining(self.f)
        self.repeat = repeat
        self._last_sps_id = header["sps_id"]
        self.digest = digest
        if grain is not None:
            self.grain, self.grain_t = (grain if grain.active else None), 0
        else:
            self.grain_t += 1
        if self._display_seen:
            self.display = self._displays.get(header["sps_id"])
        if self._active_seen:
            self.active = self._actives.get(header["sps_id"])
        self.chunked = header["nal_type"] in (NalType.NAL_I_CHUNKED, NalType.NAL_P_CHUNKED)
        return sps, header["nal_type"] in (NalType.NAL_I, NalType.NAL_I_CHUNKED), qp, payload

    def read_packet(self):
        """read_frame() as what a decoder takes: -> (sps, pipeline.FramePacket), the packet with the frame's `chunked` and
        `digest` and `repeat`; `display`, `grain` and `grain_t` are left as read_frame() leaves them"""
        from .pipeline import FramePacket
        sps, is_i, qp, payload = self.read_frame()
        return sps, FramePacket(is_i, qp, sps["use_ada_i"], payload, chunked=self.chunked, digest=self.digest,
                                repeat=self.repeat)
