"""``.gsc`` bytes back to PCM: the reference decoder (decoder/decoder.lpr:37-220)
on the MI355X.

``Decoder().decode(gsc)`` returns ``(int16 array [n, channels], sample_rate)``.
The host walks the stream once (``Decoder.index``: frame offsets, checkpoints,
validation); symbols are unpacked and samples synthesised on the GPU.  There is
no CPU fallback for the decode itself; the index needs no GPU.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _lib


def _u8(buf: bytes):
    a = np.frombuffer(buf, dtype=np.uint8)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _take(lib, pcm, n: int) -> np.ndarray:
    try:
        return np.ctypeslib.as_array(pcm, shape=(n,)).copy() if n > 0 else np.zeros(0, np.int16)
    finally:
        lib.gsc_free(pcm)


class Index:
    """The host index of one ``.gsc`` stream (``gsc_index``): per frame the
    byte offset, FrameLength, ChunkSize, ChunkCount and first sample."""

    def __init__(self, gsc: bytes):
        lib = _lib.load()
        self.gsc = gsc
        self._arr, self._ptr = _u8(gsc)
        h = lib.gsc_index_create(self._ptr, len(self._arr))
        if not h:
            raise _lib.GscError(lib.gsc_last_error().decode(errors="replace"))
        self._h = h
        n = self.frame_count = lib.gsc_index_frame_count(h)
        ch, sr, ns = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_longlong(0)
        _lib.check(lib.gsc_index_info(h, ctypes.byref(ch), ctypes.byref(sr), ctypes.byref(ns)))
        self.channels, self.sample_rate, self.samples_per_channel = ch.value, sr.value, ns.value
        off = (ctypes.c_size_t * (n + 1))()
        first = (ctypes.c_longlong * (n + 1))()
        fl, cs, cc = (ctypes.c_int * max(n, 1))(), (ctypes.c_int * max(n, 1))(), (ctypes.c_int * max(n, 1))()
        _lib.check(lib.gsc_index_frames(h, off, fl, cs, cc, first))
        self.byte_offset = np.array(off[:], dtype=np.int64)
        self.first_sample = np.array(first[:], dtype=np.int64)
        self.frame_length = np.array(fl[:n], dtype=np.int64)
        self.chunk_size = np.array(cs[:n], dtype=np.int64)
        self.chunk_count = np.array(cc[:n], dtype=np.int64)

    def decode(self, frame_begin: int = 0, frame_end: int = -1) -> np.ndarray:
        """Frames [frame_begin, frame_end) -> int16 array [n, channels]."""
        lib = _lib.load()
        pcm = ctypes.POINTER(ctypes.c_int16)()
        n = ctypes.c_size_t(0)
        _lib.check(lib.gsc_decode_indexed(self._ptr, len(self._arr), self._h, frame_begin, frame_end,
                                          ctypes.byref(pcm), ctypes.byref(n)))
        return _take(lib, pcm, n.value).reshape(-1, self.channels)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().gsc_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def wav_header(channels: int, rate: int, size: int) -> bytes:
    """CreateWAVHeader(channels, 16, rate, size) (decoder.lpr:16-35): 44 bytes."""
    return struct.pack("<IiIIiHHiiHHIi", 0x46464952, 36 + size, 0x45564157, 0x20746D66, 16, 1, channels, rate,
                       channels * rate * 2, channels * 2, 16, 0x61746164, size)


class Decoder:
    """GSCUnpack: .gsc bytes -> 16-bit PCM, bit-identical to the reference decoder."""

    @staticmethod
    def index(gsc: bytes) -> Index:
        return Index(gsc)

    @staticmethod
    def checkpoint_symbols() -> int:
        return _lib.load().gsc_decode_checkpoint_symbols()

    def decode(self, gsc: bytes, frame_begin: int = 0, frame_end: int = -1):
        """(int16 array [n, channels], sample_rate) of frames [frame_begin, frame_end)."""
        lib = _lib.load()
        if frame_begin != 0 or frame_end != -1:
            ix = Index(gsc)
            try:
                return ix.decode(frame_begin, frame_end), ix.sample_rate
            finally:
                ix.close()
        arr, ptr = _u8(gsc)
        pcm = ctypes.POINTER(ctypes.c_int16)()
        n = ctypes.c_size_t(0)
        ch, sr = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.gsc_decode(ptr, len(arr), ctypes.byref(pcm), ctypes.byref(n), ctypes.byref(ch),
                                  ctypes.byref(sr)))
        return _take(lib, pcm, n.value).reshape(-1, ch.value), sr.value

    def decode_wav(self, gsc: bytes) -> bytes:
        """The WAV file the reference decoder writes (decoder.lpr:214-216)."""
        pcm, rate = self.decode(gsc)
        data = pcm.astype("<i2", copy=False).tobytes()
        return wav_header(pcm.shape[1], rate, len(data)) + data

    def decode_many(self, gscs):
        """A batch as one job: ([int16 array [n_i, channels] per file], sample_rate)."""
        lib = _lib.load()
        gscs = list(gscs)
        arrs = [_u8(g) for g in gscs]
        ptrs = (ctypes.POINTER(ctypes.c_uint8) * len(arrs))(*[p for _, p in arrs])
        lens = (ctypes.c_size_t * len(arrs))(*[len(a) for a, _ in arrs])
        sizes = (ctypes.c_size_t * max(1, len(arrs)))()
        pcm = ctypes.POINTER(ctypes.c_int16)()
        ch, sr = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.gsc_decode_many(ptrs, lens, len(arrs), ctypes.byref(pcm), sizes, ctypes.byref(ch),
                                       ctypes.byref(sr)))
        flat = _take(lib, pcm, sum(int(s) for s in sizes[: len(arrs)]))
        outs, o = [], 0
        for i in range(len(arrs)):
            outs.append(flat[o:o + int(sizes[i])].reshape(-1, ch.value))
            o += int(sizes[i])
        return outs, sr.value

    @staticmethod
    def last_timing() -> dict:
        t = _lib.GscDecodeTiming()
        _lib.load().gsc_last_decode_timing(ctypes.byref(t))
        return {k: getattr(t, k) for k, _ in t._fields_}
