"""Decoder-state digests (csrc/dcvc_digest.hip, docs/state_digest.md; no reference counterpart): a 64-bit digest of the
entry a frame puts into the DPB - the picture of an I frame, the feature buffer of a P frame - formed on the device where the
entry lies.  The encoder writes it into the stream in front of the frame (bitstream.NalType.NAL_DIGEST), the decoder forms
it again from its own entry and the kernel compares: a decoder that has left the encoder's state is told so at the frame
where it happened (_lib.DigestMismatch), not by wrong pictures.  The sum is commutative integer arithmetic: the kernel and
the numpy restatement tests/digest_ref.py agree bit for bit.  A drift and damage check, not a cryptographic hash."""
import ctypes

NOT_COMPARED, EQUAL, DIFFERS = 0, 1, 2          # the status word of dcvc_state_digest
RING = 8                                        # result slots: a handle still unread when its slot comes round again is read first


class DigestHandle:
    """One enqueued digest: value() and status() wait for this call's event only (once; the result is kept)."""
    __slots__ = ("_words", "_event", "_result")

    def __init__(self, words, event):
        self._words, self._event, self._result = words, event, None

    def _resolve(self):
        if self._result is None:
            self._event.synchronize()
            self._result = (int(self._words[0]), int(self._words[1]))
            self._words = self._event = None
        return self._result

    def value(self):
        return self._resolve()[0]

    def status(self):
        return self._resolve()[1]


class StateDigest:
    """Owns the workspace, a ring of pinned {digest, status} slots and their events: no allocation per frame.  One instance
    serves one host thread; calls belong inside the models' frame scope (they create events and wait for them)."""

    def __init__(self, device="cuda:0"):
        import numpy as np
        import torch
        from . import _lib
        from .entropy import PinnedBuffer
        self.device = torch.device(device)
        self._lib = _lib.lib()
        need = _lib.check(self._lib.dcvc_state_digest_ws_bytes(8 * _lib.DIGEST_PASS_WORDS), "dcvc_state_digest_ws_bytes")
        self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)      # (the full grid's: enough for any size)
        self._pinned = PinnedBuffer(RING * 16)
        self._words = self._pinned.view(np.uint64, 2 * RING)
        self._events = [torch.cuda.Event() for _ in range(RING)]
        self._handles = [None] * RING
        self._next = 0

    def enqueue(self, tensor, expected=None):
        """the digest of `tensor`'s bytes (contiguous, a multiple of 8 bytes, 8-byte aligned) on the current stream, compared
        on the device with `expected` if one is given -> DigestHandle"""
        import torch
        from . import _lib
        assert tensor.is_contiguous(), "the digest is of a contiguous byte string"
        k = self._next
        self._next = (k + 1) % RING
        if self._handles[k] is not None:
            self._handles[k]._resolve()           # (its kernel ran RING calls ago)
        st = torch.cuda.current_stream(self.device)
        _lib.check(self._lib.dcvc_state_digest(ctypes.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size(),
                                               ctypes.c_void_p(self._ws.data_ptr()), int(expected or 0) & (2 ** 64 - 1),
                                               int(expected is not None), ctypes.c_void_p(self._pinned.ptr + 16 * k),
                                               ctypes.c_void_p(st.cuda_stream)), "dcvc_state_digest")
        self._events[k].record(st)
        h = self._handles[k] = DigestHandle(self._words[2 * k:2 * k + 2], self._events[k])
        return h
