"""``.gsc`` bytes back to PCM: the reference decoder (decoder/decoder.lpr:37-220)
on the MI355X.

``Decoder().decode(gsc)`` returns ``(int16 array [n, channels], sample_rate)``.
The host walks the stream once (``Decoder.index``: frame offsets, checkpoints,
validation); symbols are unpacked and samples synthesised on the GPU.  There is
no CPU fallback for the decode itself; the index needs no GPU.

``Decoder.open(gsc)`` keeps a stream on the device (``ResidentStream``);
``Decoder.decode_crops`` then decodes batches of sample ranges of such streams
straight into a torch tensor on the device, and ``decode_samples`` one range to
numpy.  ``Decoder.open_many(gscs, tables)`` opens a whole corpus as one
``StreamSet`` at a fixed number of runtime calls.  ``Decoder.bind(streams)``
describes streams once on the device (``CropBinding``), whose ``decode_crops``
takes the crops from a device tensor, whose ``mix`` sums several crops per row
with integer gains in the same launch, and whose ``envelope`` gives the block
energy and peak of every bound stream (``Envelope``), from which
``Envelope.sample_crops`` draws crops where there is sound, and whose
``fidelity`` gives the block error energy of every bound stream against its
source PCM (``Fidelity``).  torch is imported by the crop, envelope and fidelity
calls alone.
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


def _byte_arrays(seq):
    """(uint8_t *[n], size_t[n], what keeps them alive) of a list of bytes-like objects; None entries
    become NULL with length 0.  bytes objects are passed as they are, without a numpy view each."""
    n = len(seq)
    U8P = ctypes.POINTER(ctypes.c_uint8)
    lens = (ctypes.c_size_t * max(1, n))(*[0 if b is None else len(b) for b in seq])
    if all(b is None or isinstance(b, bytes) for b in seq):
        arr = (ctypes.c_char_p * max(1, n))(*seq)
        return ctypes.cast(arr, ctypes.POINTER(U8P)), lens, (arr, seq)
    views = [None if b is None else _u8(b) for b in seq]
    arr = (U8P * max(1, n))(*[U8P() if v is None else v[1] for v in views])
    return arr, lens, views


class Index:
    """The host index of one ``.gsc`` stream (``gsc_index``): per frame the
    byte offset, FrameLength, ChunkSize, ChunkCount and first sample."""

    def __init__(self, gsc: bytes, _handle=None, table: bytes | None = None):
        lib = _lib.load()
        self.gsc = gsc
        self._arr, self._ptr = _u8(gsc)
        self._owned = _handle is None  # a resident stream's index belongs to the stream
        if _handle is not None:
            h = _handle
        elif table is None:
            h = lib.gsc_index_create(self._ptr, len(self._arr))
        else:  # no host walk: the table is checked against the stream on the device
            tarr, tptr = _u8(table)
            h = lib.gsc_index_create_with_table(self._ptr, len(self._arr), tptr, len(tarr))
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

    def table(self) -> bytes:
        """The stream's seek table (layout: include/soundchunks.h): frame
        offsets, bit counts and checkpoints, so that a later ``Decoder.index``,
        ``open`` or ``decode`` of the same bytes needs no host walk.  Host only."""
        lib = _lib.load()
        out = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_size_t(0)
        _lib.check(lib.gsc_index_table(self._h, ctypes.byref(out), ctypes.byref(n)))
        try:
            return ctypes.string_at(out, n.value)
        finally:
            lib.gsc_free(out)

    def locate(self, sample: int):
        """(frame, symbol row, position inside the chunk, checkpoint) of a
        per-channel sample position in [0, samples_per_channel)."""
        fr, within = ctypes.c_int(0), ctypes.c_int(0)
        row, cp = ctypes.c_longlong(0), ctypes.c_longlong(0)
        _lib.check(_lib.load().gsc_index_locate(self._h, int(sample), ctypes.byref(fr), ctypes.byref(row),
                                                ctypes.byref(within), ctypes.byref(cp)))
        return fr.value, row.value, within.value, cp.value

    def plan_crop(self, begin: int, count: int, length: int, rate=None, stream: int = 0, nstreams: int = 1) -> dict:
        """What the kernels of a ``CropBinding`` make of crop (stream, begin,
        count) of this stream (``gsc_crop_plan_model``; host only): ``status``
        0 good, 1 / 2 / 3 a bad stream index / begin / count; ``written``, the
        source range ``src_begin`` .. ``src_end`` and the frames ``f0`` .. ``f1``."""
        w, sb, se = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
        f0, f1 = ctypes.c_int(0), ctypes.c_int(0)
        rc = _lib.load().gsc_crop_plan_model(self._h, int(nstreams), int(stream), int(begin), int(count), int(length),
                                             0 if rate is None else int(rate), ctypes.byref(w), ctypes.byref(f0),
                                             ctypes.byref(f1), ctypes.byref(sb), ctypes.byref(se))
        if rc < 0:
            _lib.check(rc)
        return {"status": rc, "written": w.value, "f0": f0.value, "f1": f1.value, "src_begin": sb.value,
                "src_end": se.value}

    def close(self) -> None:
        if getattr(self, "_h", None):
            if self._owned:
                _lib.load().gsc_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResidentStream:
    """One ``.gsc`` stream kept on the device (``gsc_stream``): walked and
    uploaded once by ``Decoder.open``; sample ranges then decode without
    touching the bytes again (``decode_samples``, ``Decoder.decode_crops``)."""

    def __init__(self, gsc: bytes, table: bytes | None = None, _member=None):
        lib = _lib.load()
        self._set = None
        if _member is not None:  # a StreamSet's view of one member: the handle is the set's
            self._set, h = _member
        else:
            arr, ptr = _u8(gsc)
            if table is None:
                h = lib.gsc_stream_open(ptr, len(arr))
            else:
                tarr, tptr = _u8(table)
                h = lib.gsc_stream_open_with_table(ptr, len(arr), tptr, len(tarr))
        if not h:
            raise _lib.GscError(lib.gsc_last_error().decode(errors="replace"))
        self._h = h
        ch, sr, ns, nf = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_longlong(0), ctypes.c_int(0)
        _lib.check(lib.gsc_stream_info(h, ctypes.byref(ch), ctypes.byref(sr), ctypes.byref(ns), ctypes.byref(nf)))
        self.channels, self.sample_rate, self.samples_per_channel, self.frame_count = (ch.value, sr.value, ns.value,
                                                                                       nf.value)
        self.device = lib.gsc_stream_device(h)
        self.index = Index(gsc, _handle=lib.gsc_stream_index(h))

    def decode_samples(self, begin: int, end: int) -> np.ndarray:
        """Samples [begin, end) -> int16 array [end - begin, channels] on the host."""
        n = int(end) - int(begin)
        if n < 0:
            raise _lib.GscError(f"decode_samples: end {end} < begin {begin}")
        out = np.zeros((n, self.channels), np.int16)
        _lib.check(_lib.load().gsc_stream_decode_samples(self._handle(), int(begin), n,
                                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))))
        return out

    def envelope(self, hop: int = 1024) -> "Envelope":
        """``Decoder.envelope([self], hop)``."""
        return Decoder.envelope([self], hop)

    def fidelity(self, ref, hop: int = 1024) -> "Fidelity":
        """``Decoder.fidelity([self], [ref], hop)``."""
        return Decoder.fidelity([self], [ref], hop)

    def _handle(self):
        if not getattr(self, "_h", None):
            raise _lib.GscError("the resident stream is closed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_set", None) is not None:
            self._set.close()  # a member lives and ends with its set
        elif getattr(self, "_h", None):
            self.index.close()
            _lib.load().gsc_stream_free(self._h)
            self._h = None

    def __del__(self):
        try:
            if getattr(self, "_set", None) is None:
                self.close()
        except Exception:
            pass


class StreamSet:
    """Many ``.gsc`` streams opened as one resident set (``gsc_stream_set``):
    one set of device slabs, tables expanded and seek tables checked on the
    device, a fixed number of runtime calls whatever ``len(gscs)``.  ``ss[i]``
    is a ``ResidentStream`` view of member i; ``ss.streams`` goes wherever a
    list of resident streams goes, alone or mixed with others."""

    def __init__(self, gscs, tables=None):
        gscs = list(gscs)
        tables = None if tables is None else list(tables)
        if tables is not None and len(tables) != len(gscs):
            raise _lib.GscError(f"open_many: {len(gscs)} streams, {len(tables)} tables")
        for what, seq in (("stream", gscs), ("table", tables or [])):
            for i, b in enumerate(seq):
                if not isinstance(b, (bytes, bytearray, memoryview)) and not (what == "table" and b is None):
                    raise _lib.GscError(f"open_many: {what} {i} is {type(b).__name__}, not bytes")
        # the set keeps the streams for Index.decode, which builds the host tables from them on first
        # use: they must stay the bytes the device holds, so anything mutable is copied now
        gscs = [g if isinstance(g, bytes) else bytes(g) for g in gscs]
        lib = _lib.load()
        n = len(gscs)
        ptrs, lens, _alive = _byte_arrays(gscs)  # the library copies what it keeps during the call
        tptrs = tlens = None
        if tables is not None:
            tptrs, tlens, _alive_t = _byte_arrays(tables)
        h = lib.gsc_stream_set_open(ptrs, lens, tptrs, tlens, n)
        if not h:
            raise _lib.GscError(lib.gsc_last_error().decode(errors="replace"))
        self._h = h
        self._gscs = gscs
        self._streams = [None] * n  # views are made when asked for: an open costs no Python per stream

    def __len__(self) -> int:
        return len(self._streams)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        i = range(len(self))[i]
        if self._streams[i] is None:
            if not getattr(self, "_h", None):
                raise _lib.GscError("the resident stream is closed")
            self._streams[i] = ResidentStream(self._gscs[i],
                                              _member=(self, _lib.load().gsc_stream_set_stream(self._h, i)))
        return self._streams[i]

    @property
    def streams(self):
        return [self[i] for i in range(len(self))]

    def decode_crops(self, crops, length: int, dtype=None, layout: str = "TC", out=None, rate=None, channels=None):
        """``Decoder.decode_crops(self.streams, ...)``: crop stream indices count the set's members."""
        return Decoder.decode_crops(self.streams, crops, length, dtype=dtype, layout=layout, out=out, rate=rate,
                                    channels=channels)

    def bind(self, rate=None, channels=None):
        """``Decoder.bind(self.streams, ...)``: crop stream indices count the set's members."""
        return CropBinding(self.streams, rate=rate, channels=channels)

    def envelope(self, hop: int = 1024) -> "Envelope":
        """``Decoder.envelope(self.streams, hop)``: stream indices count the set's members."""
        return Decoder.envelope(self.streams, hop)

    def fidelity(self, refs, hop: int = 1024) -> "Fidelity":
        """``Decoder.fidelity(self.streams, refs, hop)``: stream indices count the set's members."""
        return Decoder.fidelity(self.streams, refs, hop)

    def close(self) -> None:
        if getattr(self, "_h", None):
            for s in self._streams:
                if s is not None:
                    s.index.close()
                    s._h = None
            _lib.load().gsc_stream_set_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CropBinding:
    """The streams of a loader described once on the device
    (``gsc_crop_binding``): ``decode_crops`` then takes ``(stream, begin,
    count)`` from a device tensor and does nothing on the host but launch one
    kernel, which plans every crop itself.  ``begin`` is in source samples of
    the crop's stream; ``count`` and ``length`` are output samples at ``rate``.
    The binding keeps its streams alive; once one of them, or its set, is
    closed, ``decode_crops`` raises."""

    def __init__(self, streams, rate=None, channels=None):
        import torch

        streams = list(streams)
        if not streams:
            raise _lib.GscError("bind: no streams")
        if rate is not None and int(rate) <= 0:
            raise _lib.GscError(f"bind: rate {rate} Hz: a rate must be positive")
        if channels is not None and int(channels) <= 0:
            raise _lib.GscError(f"bind: channels {channels}")
        lib = _lib.load()
        self._streams = streams
        # what closes a stream: itself, or the set it belongs to
        owners = {}
        for s in streams:
            o = s._set if getattr(s, "_set", None) is not None else s
            owners[id(o)] = o
        self._owners = list(owners.values())
        self.channels = streams[0].channels if channels is None else int(channels)
        self.rate = None if rate is None else int(rate)
        self._converts = rate is not None or channels is not None  # the resampling kernels, not the fused ones
        self.device = torch.device("cuda", streams[0].device)
        hs = (ctypes.c_void_p * len(streams))(*[s._handle() for s in streams])
        with torch.cuda.device(self.device):
            h = lib.gsc_crop_binding_create(hs, len(streams), 0 if rate is None else int(rate),
                                            0 if channels is None else int(channels))
        if not h:
            raise _lib.GscError(lib.gsc_last_error().decode(errors="replace"))
        self._h = h

    def decode_crops(self, crops, length: int, dtype=None, layout: str = "TC", out=None, written=None):
        """``crops``: a contiguous ``torch.int64`` tensor [B, 3] of (stream
        index, begin, count) on the streams' device.  Returns ``(x, n)``: ``x``
        as ``Decoder.decode_crops`` returns it, ``n`` a ``torch.int64`` tensor
        [B] on the device with each crop's clipped length (``written`` if
        given).  A bad crop (stream index, ``begin`` or ``count`` out of range)
        gets an all-zero row and ``n[i] == -1``; the other rows do not notice.
        The work is enqueued on torch's current stream; nothing is synchronised,
        allocated or copied by the library, and no crop is read on the host."""
        import torch

        if not getattr(self, "_h", None):
            raise _lib.GscError("the crop binding is closed")
        for o in self._owners:
            if not getattr(o, "_h", None):
                raise _lib.GscError("a stream of the crop binding is closed")
        device = self.device
        if not isinstance(crops, torch.Tensor) or crops.device != device:
            where = crops.device if isinstance(crops, torch.Tensor) else type(crops).__name__
            raise _lib.GscError(f"bound decode_crops: crops must be a torch.int64 tensor [B, 3] on {device}, got "
                                f"{where}; Decoder.decode_crops takes crops as a host list")
        if crops.dtype != torch.int64 or crops.dim() != 2 or crops.shape[1] != 3 or not crops.is_contiguous():
            raise _lib.GscError(f"bound decode_crops: crops must be a contiguous torch.int64 tensor [B, 3], got "
                                f"{crops.dtype} {tuple(crops.shape)}; Decoder.decode_crops takes crops as a host list")
        length, out, written, pcm, lay = self._row_outputs("bound decode_crops", crops.shape[0], length, dtype, layout,
                                                           out, written)
        B = crops.shape[0]
        with torch.cuda.device(device):
            hip_stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            _lib.check(_lib.load().gsc_crop_binding_decode(self._h, crops.data_ptr(), B, pcm, lay, length,
                                                           out.data_ptr(), written.data_ptr(), hip_stream))
        return out, written

    def _row_outputs(self, who, B, length, dtype, layout, out, written):
        """What a call that writes B rows checks and makes: (length, out, written, pcm, lay)."""
        import torch

        device = self.device
        dtype = torch.int16 if dtype is None else dtype
        if dtype not in (torch.int16, torch.float32):
            raise _lib.GscError(f"{who}: dtype {dtype} is neither torch.int16 nor torch.float32")
        if layout not in ("TC", "CT"):
            raise _lib.GscError(f"{who}: layout {layout!r} is neither 'TC' nor 'CT'")
        length = int(length)
        if length < 0:
            raise _lib.GscError(f"{who}: length {length}")
        ch = self.channels
        shape = (B, length, ch) if layout == "TC" else (B, ch, length)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=device)
        else:
            if out.device != device:
                raise _lib.GscError(f"{who}: out is on {out.device}, the streams live on {device}")
            if out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
                raise _lib.GscError(f"{who}: out must be a contiguous {dtype} tensor of shape {shape}, "
                                    f"got {out.dtype} {tuple(out.shape)}")
        if written is None:
            # without a row to write the library launches nothing and reports nothing
            written = (torch.empty if length else torch.zeros)((B,), dtype=torch.int64, device=device)
        elif (written.device != device or written.dtype != torch.int64 or tuple(written.shape) != (B,) or
              not written.is_contiguous()):
            raise _lib.GscError(f"{who}: written must be a contiguous torch.int64 tensor [{B}] on "
                                f"{device}")
        pcm = _lib.PCM_FLOAT32 if dtype == torch.float32 else _lib.PCM_INT16
        lay = _lib.LAYOUT_CT if layout == "CT" else _lib.LAYOUT_TC
        return length, out, written, pcm, lay

    def mix(self, sources, length: int, dtype=None, layout: str = "TC", out=None, written=None):
        """Gain-weighted sums of crops (include/soundchunks.h "mixing crops").
        ``sources``: a contiguous ``torch.int64`` tensor [R, K, 4] of (stream
        index, begin, count, gain) on the streams' device, 1 <= K <= 256;
        (stream, begin, count) is a crop of ``decode_crops``, ``gain`` is Q15
        (32768 is unity, ``round(g * 32768)`` for a linear gain g) within
        +-2**20.  Row r is ``clamp((sum_k gain_k * x_k + 16384) >> 15)`` of its K
        crops ``x_k`` in exact integer arithmetic; a slot with ``count == 0``
        adds nothing.  Returns ``(x, n)`` shaped as ``decode_crops`` returns
        them: ``n[r]`` is the largest clipped count of the row's sources.  A row
        with one bad source (a bad crop, or a gain out of range) is all zero and
        has ``n[r] == -1``; the other rows do not notice.  The work is one
        kernel on torch's current stream; nothing is synchronised, allocated or
        copied by the library, and no source is read on the host.

        A list or numpy array is accepted for ``sources`` as a convenience: the
        wrapper uploads it, which is a copy outside that contract."""
        import torch

        self._check_open()
        device = self.device
        if not isinstance(sources, torch.Tensor):
            try:
                host = np.asarray(sources)
            except Exception as e:
                raise _lib.GscError(f"mix: sources: {e}") from None
            if host.dtype.kind not in "iu":
                raise _lib.GscError(f"mix: sources must be integers, got {host.dtype}")
            sources = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int64)).to(device)
        if sources.device != device:
            raise _lib.GscError(f"mix: sources must be a torch.int64 tensor [R, K, 4] on {device}, got "
                                f"{sources.device}")
        if sources.dtype != torch.int64 or sources.dim() != 3 or sources.shape[2] != 4 or not sources.is_contiguous():
            raise _lib.GscError(f"mix: sources must be a contiguous torch.int64 tensor [R, K, 4], got {sources.dtype} "
                                f"{tuple(sources.shape)}")
        R, K = sources.shape[0], sources.shape[1]
        if K < 1 or K > 256:
            raise _lib.GscError(f"mix: {K} sources per row, 1 to 256 are possible")
        length, out, written, pcm, lay = self._row_outputs("mix", R, length, dtype, layout, out, written)
        with torch.cuda.device(device):
            hip_stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            _lib.check(_lib.load().gsc_crop_binding_mix(self._h, sources.data_ptr(), R, K, pcm, lay, length,
                                                        out.data_ptr(), written.data_ptr(), hip_stream))
        return out, written

    def mix_tile(self) -> int:
        """Output samples of one workgroup of ``mix`` for this binding: what 4096 accumulators
        (kMixAccElems, csrc/gsc_mix.h) hold of its channels, at most ``Decoder.resample_tile()``
        when the binding converts."""
        fit = max(1, 4096 // self.channels)
        return min(fit, Decoder.resample_tile()) if self._converts else fit

    def envelope(self, hop: int = 1024, energy=None, peak=None) -> "Envelope":
        """Block energy and peak of every bound stream (include/soundchunks.h
        has the definition): per block of ``hop`` source samples (64 ..
        65536) of a stream, all channels, the sum of squares as ``torch.int64``
        and the largest magnitude as ``torch.int32``, the streams' blocks back
        to back in the binding's order.  One kernel launch on torch's current
        stream, straight from the compressed slabs; the binding's ``rate`` and
        ``channels`` play no part.  A once-per-corpus call: it allocates,
        copies its layout and waits for the stream.  ``energy`` / ``peak``:
        contiguous tensors of the layout's total on the streams' device to
        write into."""
        import torch

        self._check_open()
        device = self.device
        hop = int(hop)
        samples = [int(s.samples_per_channel) for s in self._streams]
        channels = [int(s.channels) for s in self._streams]
        offsets = Decoder.envelope_layout(samples, hop)
        total = offsets[-1]
        energy, peak = self._block_outputs("envelope", total, (("energy", energy, torch.int64),
                                                               ("peak", peak, torch.int32)))
        with torch.cuda.device(device):
            hip_stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            _lib.check(_lib.load().gsc_crop_binding_envelope(self._h, hop, energy.data_ptr(), peak.data_ptr(), total,
                                                             hip_stream))
        return Envelope(hop, samples, channels, offsets, energy, peak)

    def fidelity(self, refs, hop: int = 1024, err_energy=None, ref_energy=None, err_peak=None) -> "Fidelity":
        """Block error energy of every bound stream against its source PCM
        (include/soundchunks.h has the definition): per block of ``hop`` source
        samples (the envelope's blocks) of a stream, all channels, the sum of
        ``(decoded - reference)**2`` and of ``reference**2`` as ``torch.int64``
        and the largest ``|decoded - reference|`` as ``torch.int32``.  ``refs``
        has one entry per stream: a contiguous ``torch.int16`` tensor ``[R, C]``
        on the streams' device, read in place, or a numpy int16 ``[R, C]``
        array, which the call uploads; ``C`` is the stream's channel count,
        sample t of the reference is sample t of the stream, ``R`` may be
        anything: the reference is zero past its end and ignored past the
        stream's.  One kernel launch on torch's current stream, straight from
        the compressed slabs; the binding's ``rate`` and ``channels`` play no
        part.  A once-per-corpus call, as ``envelope``: it allocates, copies and
        waits for the stream.  ``err_energy`` / ``ref_energy`` / ``err_peak``:
        contiguous tensors of the layout's total on the streams' device to
        write into."""
        import torch

        self._check_open()
        device = self.device
        hop = int(hop)
        refs = list(refs)
        n = len(self._streams)
        if len(refs) != n:
            raise _lib.GscError(f"fidelity: {len(refs)} references for {n} streams")
        held = []  # the references as device tensors, alive until the call has waited for its stream
        for i, (r, st) in enumerate(zip(refs, self._streams)):
            ch = int(st.channels)
            if isinstance(r, np.ndarray):
                dtype_ok, contiguous = r.dtype == np.int16, r.flags.c_contiguous
            elif isinstance(r, torch.Tensor):
                dtype_ok, contiguous = r.dtype == torch.int16, r.is_contiguous()
            else:
                raise _lib.GscError(f"fidelity: reference {i} is {type(r).__name__}, neither a torch tensor nor a "
                                    f"numpy array")
            if not dtype_ok:
                raise _lib.GscError(f"fidelity: reference {i} must be int16, got {r.dtype}")
            if r.ndim != 2 or r.shape[1] != ch:
                raise _lib.GscError(f"fidelity: reference {i} must be [R, {ch}], stream {i} has {ch} channels, got "
                                    f"{tuple(r.shape)}")
            if not contiguous:
                raise _lib.GscError(f"fidelity: reference {i} is not contiguous")
            if isinstance(r, np.ndarray):
                r = torch.from_numpy(r if r.flags.writeable else r.copy()).to(device)
            elif r.device != device:
                raise _lib.GscError(f"fidelity: reference {i} is on {r.device}, the streams live on {device}")
            held.append(r)
        samples = [int(s.samples_per_channel) for s in self._streams]
        channels = [int(s.channels) for s in self._streams]
        offsets = Decoder.envelope_layout(samples, hop)
        total = offsets[-1]
        err_energy, ref_energy, err_peak = self._block_outputs(
            "fidelity", total, (("err_energy", err_energy, torch.int64), ("ref_energy", ref_energy, torch.int64),
                                ("err_peak", err_peak, torch.int32)))
        ptrs = (ctypes.c_void_p * n)(*[r.data_ptr() if r.numel() else None for r in held])
        lens = (ctypes.c_longlong * n)(*[int(r.shape[0]) for r in held])
        with torch.cuda.device(device):
            hip_stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            _lib.check(_lib.load().gsc_crop_binding_fidelity(self._h, hop, ptrs, lens, err_energy.data_ptr(),
                                                             ref_energy.data_ptr(), err_peak.data_ptr(), total,
                                                             hip_stream))
        del held
        return Fidelity(hop, samples, channels, offsets, err_energy, ref_energy, err_peak)

    def _check_open(self):
        if not getattr(self, "_h", None):
            raise _lib.GscError("the crop binding is closed")
        for o in self._owners:
            if not getattr(o, "_h", None):
                raise _lib.GscError("a stream of the crop binding is closed")

    def _block_outputs(self, who, total, wanted):
        """The per-block outputs of ``who``: (name, given tensor or None, dtype) each, made where not given."""
        import torch

        device = self.device
        made = []
        for name, t, dt in wanted:
            if t is None:
                t = torch.empty((total,), dtype=dt, device=device)
            elif not isinstance(t, torch.Tensor) or t.device != device:
                where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
                raise _lib.GscError(f"{who}: {name} must be a tensor on {device}, got {where}")
            elif t.dtype != dt or tuple(t.shape) != (total,) or not t.is_contiguous():
                raise _lib.GscError(f"{who}: {name} must be a contiguous {dt} tensor [{total}], got {t.dtype} "
                                    f"{tuple(t.shape)}")
            made.append(t)
        return made

    @staticmethod
    def last_call() -> dict:
        """The runtime calls of this thread's last ``decode_crops`` or ``mix`` of a binding, and its host time."""
        s = _lib.GscCropCallStats()
        _lib.load().gsc_crop_binding_last_call(ctypes.byref(s))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().gsc_crop_binding_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Blocks:
    """The blocks of ``hop`` samples of several streams back to back
    (``Decoder.envelope_layout``): ``hop``; ``samples`` and ``channels`` per
    stream (host lists); ``offsets``: ``torch.int64`` [n + 1] on ``device``,
    stream i's first block, and ``offsets_host``, the same as a list."""

    def __init__(self, hop, samples, channels, offsets_host, device):
        import torch

        self.hop = int(hop)
        self.samples, self.channels = list(samples), list(channels)
        self.offsets_host = list(offsets_host)
        i64 = dict(dtype=torch.int64, device=device)
        self.offsets = torch.tensor(self.offsets_host, **i64)
        self._samples = torch.tensor(self.samples, **i64).reshape(-1)
        total = self.offsets_host[-1]
        # per block: its stream, its first sample and its samples (the last block of a stream is partial)
        b = torch.arange(total, **i64)
        self._stream = torch.searchsorted(self.offsets[1:].contiguous(), b, right=True)
        self._first = (b - self.offsets[self._stream]) * self.hop
        self._len = torch.clamp(self._samples[self._stream] - self._first, max=self.hop)
        self._elems = self._len * torch.tensor(self.channels, **i64).reshape(-1)[self._stream]

    def __len__(self) -> int:
        return self.offsets_host[-1]

    def _range(self, i: int):
        i = range(len(self.samples))[i]
        return self.offsets_host[i], self.offsets_host[i + 1]


class Envelope(_Blocks):
    """Block energy and peak of the streams of a binding
    (``CropBinding.envelope``).  ``hop``; ``samples`` and ``channels`` per stream
    (host lists); ``offsets``: ``torch.int64`` [n + 1] on the device, stream i's
    first block, and ``offsets_host``, the same as a list; ``energy``
    ``torch.int64`` [total] and ``peak`` ``torch.int32`` [total] on the device.
    It owns plain tensors, so it outlives the binding and the streams."""

    def __init__(self, hop, samples, channels, offsets_host, energy, peak):
        super().__init__(hop, samples, channels, offsets_host, energy.device)
        self.energy, self.peak = energy, peak

    def blocks(self, i: int):
        """(energy, peak) of stream i: views of its blocks."""
        a, b = self._range(i)
        return self.energy[a:b], self.peak[a:b]

    def active(self, min_rms=None, min_peak=None):
        """``torch.bool`` [total]: the blocks that hold sound.  ``min_rms`` (an
        int, int16 units) is the exact integer test ``energy[b] >= min_rms**2 *
        (samples in block b * channels of its stream)``; ``min_peak`` is
        ``peak[b] >= min_peak``; both given: both must hold; neither: ``energy >
        0``."""
        if min_rms is None and min_peak is None:
            return self.energy > 0
        act = None
        if min_rms is not None:
            if int(min_rms) != min_rms or not 0 <= int(min_rms) <= 32768:
                raise _lib.GscError(f"active: min_rms {min_rms!r} is not an int in [0, 32768]")
            act = self.energy >= int(min_rms) ** 2 * self._elems  # at most 2^30 * 2^24
        if min_peak is not None:
            if int(min_peak) != min_peak:
                raise _lib.GscError(f"active: min_peak {min_peak!r} is not an int")
            p = self.peak >= int(min_peak)
            act = p if act is None else act & p
        return act

    def sample_crops(self, n: int, span: int, count=None, min_rms=None, min_peak=None, generator=None):
        """``torch.int64`` [n, 3] on the device for ``CropBinding.decode_crops``
        of the same streams: n crops of ``span`` source samples, each around a
        sample drawn uniformly from a uniformly drawn active block
        (``active(min_rms, min_peak)``): ``begin = clamp(p - span // 2, 0,
        max(samples - span, 0))``, so the crop holds p or is the whole stream.
        Column 2 is ``count`` (default ``span``), the crop's length at the
        binding's rate.  With no active block every row's stream is -1, which
        the bound call reports as ``n[i] == -1`` and a zero row.  Device-side
        ops on torch's current stream only: nothing is synchronised.
        ``generator``: a ``torch.Generator`` of the envelope's device."""
        import torch

        n, span = int(n), int(span)
        count = span if count is None else int(count)
        if n < 0 or span < 1 or count < 0:
            raise _lib.GscError(f"sample_crops: n {n}, span {span}, count {count}")
        device = self.energy.device
        i64 = dict(dtype=torch.int64, device=device)
        total = len(self)
        if total == 0 or n == 0:
            out = torch.zeros((n, 3), **i64)
            out[:, 0] = -1
            out[:, 2] = count
            return out
        cum = torch.cumsum(self.active(min_rms, min_peak).to(torch.int64), 0)
        active = cum[-1]  # stays on the device
        u = torch.rand((2, n), dtype=torch.float64, device=device, generator=generator)
        # the (r + 1)-th active block, r uniform in [0, active)
        r = torch.minimum((u[0] * active).to(torch.int64), active - 1)
        blk = torch.clamp(torch.searchsorted(cum, r, right=True), max=total - 1)
        ln = self._len[blk]
        p = self._first[blk] + torch.minimum((u[1] * ln).to(torch.int64), ln - 1)
        stream = self._stream[blk]
        last = torch.clamp(self._samples[stream] - span, min=0)
        begin = torch.minimum(torch.clamp(p - span // 2, min=0), last)
        some = active > 0
        out = torch.empty((n, 3), **i64)
        out[:, 0] = torch.where(some, stream, -1)
        out[:, 1] = torch.where(some, begin, 0)
        out[:, 2] = count
        return out


class Fidelity(_Blocks):
    """Block error energy of the streams of a binding against their source PCM
    (``CropBinding.fidelity``).  ``hop``, ``samples``, ``channels``, ``offsets``
    and ``offsets_host`` as ``Envelope`` has them; ``err_energy`` and
    ``ref_energy`` ``torch.int64`` [total], ``err_peak`` ``torch.int32``
    [total].  It owns plain tensors, so it outlives the binding and the
    streams.  Its methods are torch ops on the tensors' device and synchronise
    nothing; they work on CPU tensors too."""

    def __init__(self, hop, samples, channels, offsets_host, err_energy, ref_energy, err_peak):
        super().__init__(hop, samples, channels, offsets_host, err_energy.device)
        self.err_energy, self.ref_energy, self.err_peak = err_energy, ref_energy, err_peak

    def blocks(self, i: int):
        """(err_energy, ref_energy, err_peak) of stream i: views of its blocks."""
        a, b = self._range(i)
        return self.err_energy[a:b], self.ref_energy[a:b], self.err_peak[a:b]

    @staticmethod
    def _snr_db(ref, err):
        import torch

        # 0 / x is 0 and log10(0) is -inf; x / 0 and 0 / 0 are replaced: no error is +inf whatever the reference
        ratio = ref.to(torch.float64) / err.to(torch.float64)
        return torch.where(err == 0, torch.full_like(ratio, float("inf")), 10.0 * torch.log10(ratio))

    def snr_db(self):
        """``torch.float64`` [total]: ``10 * log10(ref_energy / err_energy)`` per
        block; ``+inf`` where the error is 0, ``-inf`` where only the reference is."""
        return self._snr_db(self.ref_energy, self.err_energy)

    def stream_sums(self):
        """(err_energy, ref_energy) summed over each stream's blocks: exact ``torch.int64`` [n]."""
        import torch

        def per_stream(x):
            c = torch.cat([x.new_zeros(1), torch.cumsum(x, 0)])
            return c[self.offsets[1:]] - c[self.offsets[:-1]]

        return per_stream(self.err_energy), per_stream(self.ref_energy)

    def stream_snr_db(self):
        """``torch.float64`` [n]: the SNR of each whole stream, from the exact
        int64 sums over its blocks; the infinities as in ``snr_db`` (a stream
        without samples has no error: ``+inf``)."""
        err, ref = self.stream_sums()
        return self._snr_db(ref, err)

    def worst(self, k: int):
        """The ``min(k, total)`` blocks with the lowest SNR, lowest first, equal
        ones in block order: ``(stream, first_sample, snr_db)``, ``torch.int64``,
        ``torch.int64`` and ``torch.float64`` [k].  ``first_sample`` is the
        block's first sample in its stream."""
        import torch

        k = int(k)
        if k < 0:
            raise _lib.GscError(f"worst: k {k}")
        snr, order = torch.sort(self.snr_db(), stable=True)
        order = order[:k]
        return self._stream[order], self._first[order], snr[:k]


def wav_header(channels: int, rate: int, size: int) -> bytes:
    """CreateWAVHeader(channels, 16, rate, size) (decoder.lpr:16-35): 44 bytes."""
    return struct.pack("<IiIIiHHiiHHIi", 0x46464952, 36 + size, 0x45564157, 0x20746D66, 16, 1, channels, rate,
                       channels * rate * 2, channels * 2, 16, 0x61746164, size)


class Decoder:
    """GSCUnpack: .gsc bytes -> 16-bit PCM, bit-identical to the reference decoder."""

    @staticmethod
    def index(gsc: bytes, table: bytes | None = None) -> Index:
        """The stream's index: by the host walk, or from a seek table
        (``Index.table()``, ``Encoder.encode(..., with_table=True)``), which is
        checked on the device; a table that is not the stream's own raises."""
        return Index(gsc, table=table)

    @staticmethod
    def checkpoint_symbols() -> int:
        return _lib.load().gsc_decode_checkpoint_symbols()

    @staticmethod
    def open(gsc: bytes, table: bytes | None = None) -> ResidentStream:
        return ResidentStream(gsc, table)

    @staticmethod
    def open_many(gscs, tables=None) -> StreamSet:
        """Every stream of ``gscs`` as one resident set.  ``tables``: None (every
        stream is walked on the host) or one entry per stream, a seek table or
        None.  A stream that ``open`` would refuse fails the whole call; the
        message names the lowest such stream."""
        return StreamSet(gscs, tables)

    @staticmethod
    def last_set_open_timing() -> dict:
        """Where the last ``open_many`` of this thread spent its time, and how many runtime calls it made."""
        t = _lib.GscSetOpenTiming()
        _lib.load().gsc_last_set_open_timing(ctypes.byref(t))
        return {k: getattr(t, k) for k, _ in t._fields_}

    @staticmethod
    def last_open_timing() -> dict:
        """Where the last ``open`` / ``index(gsc, table)`` of this thread spent its time."""
        t = _lib.GscOpenTiming()
        _lib.load().gsc_last_open_timing(ctypes.byref(t))
        return {k: getattr(t, k) for k, _ in t._fields_}

    @staticmethod
    def resample_tile() -> int:
        """Output samples of one workgroup of the resampling crop kernel."""
        return _lib.load().gsc_resample_tile()

    @staticmethod
    def resample_table(in_rate: int, out_rate: int) -> np.ndarray:
        """The resampler of a pair of rates (include/soundchunks.h has the
        definition): int32 array [phases, taps], every row summing to 2**24.
        Host only; a pair the library refuses raises with both rates named."""
        lib = _lib.load()
        phases, taps = ctypes.c_int(0), ctypes.c_int(0)
        coeff = ctypes.POINTER(ctypes.c_int32)()
        _lib.check(lib.gsc_resample_table(int(in_rate), int(out_rate), ctypes.byref(phases), ctypes.byref(taps),
                                          ctypes.byref(coeff)))
        return np.ctypeslib.as_array(coeff, shape=(phases.value, taps.value)).copy()

    @staticmethod
    def prepare_resample(in_rate: int, out_rate: int, device=None) -> None:
        """Builds and uploads the table of a pair of rates now (a blocking copy),
        so that no later ``decode_crops(..., rate=out_rate)`` has to."""
        import torch

        with torch.cuda.device(torch.cuda.current_device() if device is None else device):
            _lib.check(_lib.load().gsc_resample_prepare(int(in_rate), int(out_rate)))

    @staticmethod
    def decode_crops(streams, crops, length: int, dtype=None, layout: str = "TC", out=None, rate=None,
                     channels=None):
        """``crops``: (stream index, begin, count) in per-channel samples.
        Returns (tensor on the streams' device, [B, length, C] for layout "TC"
        or [B, C, length] for "CT", int16 or float32 = int16 / 32768; written
        lengths).  Crop i fills row i, clipped at its stream's end, zero after.
        The work is enqueued on torch's current stream; nothing is synchronised.

        ``rate`` (Hz) and ``channels`` bring every row to one sample rate and
        channel count on the device, whatever its stream's own; ``begin`` then
        stays in source samples of the crop's stream, ``count`` and ``length``
        are output samples at ``rate``.  ``rate=None``: no resampling;
        ``channels=None``: the streams' count, which must agree.  The first call
        that meets a new pair of rates on a device uploads its table with a
        blocking copy (``prepare_resample`` does it ahead of time)."""
        import torch

        lib = _lib.load()
        streams, crops = list(streams), [tuple(int(v) for v in c) for c in crops]
        if not streams:
            raise _lib.GscError("decode_crops: no streams")
        fmt = rate is not None or channels is not None
        if rate is not None and int(rate) <= 0:
            raise _lib.GscError(f"decode_crops: rate {rate} Hz: a rate must be positive")
        if channels is not None and int(channels) <= 0:
            raise _lib.GscError(f"decode_crops: channels {channels}")
        dtype = torch.int16 if dtype is None else dtype
        if dtype not in (torch.int16, torch.float32):
            raise _lib.GscError(f"decode_crops: dtype {dtype} is neither torch.int16 nor torch.float32")
        if layout not in ("TC", "CT"):
            raise _lib.GscError(f"decode_crops: layout {layout!r} is neither 'TC' nor 'CT'")
        length = int(length)
        if length < 0:
            raise _lib.GscError(f"decode_crops: length {length}")
        ch = streams[0].channels if channels is None else int(channels)
        device = torch.device("cuda", streams[0].device)
        shape = (len(crops), length, ch) if layout == "TC" else (len(crops), ch, length)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=device)
        else:
            if out.device != device:
                raise _lib.GscError(f"decode_crops: out is on {out.device}, the streams live on {device}")
            if out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
                raise _lib.GscError(f"decode_crops: out must be a contiguous {dtype} tensor of shape {shape}, got "
                                    f"{out.dtype} {tuple(out.shape)}")
        # an empty tensor has no memory: the library still checks the crops, and writes nothing
        dst = out if out.numel() else torch.empty(1, dtype=dtype, device=device)
        hs = (ctypes.c_void_p * len(streams))(*[s._handle() for s in streams])
        cr = (_lib.GscCrop * max(1, len(crops)))(*[_lib.GscCrop(*c) for c in crops])
        written = (ctypes.c_longlong * max(1, len(crops)))()
        pcm = _lib.PCM_FLOAT32 if dtype == torch.float32 else _lib.PCM_INT16
        lay = _lib.LAYOUT_CT if layout == "CT" else _lib.LAYOUT_TC
        with torch.cuda.device(device):
            hip_stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            if fmt:
                f = _lib.GscCropFormat(pcm, lay, length, 0 if rate is None else int(rate),
                                       0 if channels is None else int(channels))
                _lib.check(lib.gsc_decode_crops_fmt(hs, len(streams), cr, len(crops), ctypes.byref(f),
                                                    dst.data_ptr(), hip_stream, written))
            else:
                _lib.check(lib.gsc_decode_crops(hs, len(streams), cr, len(crops), pcm, lay, length, dst.data_ptr(),
                                                hip_stream, written))
        return out, [int(written[i]) for i in range(len(crops))]

    @staticmethod
    def bind(streams, rate=None, channels=None) -> CropBinding:
        """The streams described once on the device, for crop lists that live
        there: ``bind(...).decode_crops(crops_tensor, length)`` is
        ``decode_crops(streams, crops_list, length, rate=, channels=)`` without
        the host plan, the allocation and the copy of each call.  ``rate`` and
        ``channels`` as in ``decode_crops``; every resampler table is uploaded
        here.  Refuses what ``decode_crops`` refuses of a stream, naming it."""
        return CropBinding(streams, rate=rate, channels=channels)

    @staticmethod
    def envelope_layout(samples, hop: int):
        """``offsets`` [n + 1] of an envelope of streams of ``samples[i]`` samples
        per channel at ``hop``: stream i's first block, then the total
        (``gsc_envelope_layout``).  Host only; raises for a hop outside 64 ..
        65536, a negative length and 2**31 or more blocks."""
        samples = [int(v) for v in samples]
        n = len(samples)
        arr = (ctypes.c_longlong * max(1, n))(*samples)
        off = (ctypes.c_longlong * (n + 1))()
        _lib.check(_lib.load().gsc_envelope_layout(arr, n, int(hop), off))
        return [int(v) for v in off]

    @staticmethod
    def envelope(streams, hop: int = 1024) -> Envelope:
        """The envelope of resident streams: binds them for the call
        (``rate=None, channels=None``, so their channel counts must agree),
        runs ``CropBinding.envelope`` and closes the binding again."""
        b = CropBinding(streams)
        try:
            return b.envelope(hop)
        finally:
            b.close()

    @staticmethod
    def fidelity(streams, refs, hop: int = 1024) -> Fidelity:
        """The fidelity of resident streams against ``refs``, one per stream:
        binds them for the call (``rate=None, channels=None``, so their channel
        counts must agree), runs ``CropBinding.fidelity`` and closes the binding
        again."""
        b = CropBinding(streams)
        try:
            return b.fidelity(refs, hop)
        finally:
            b.close()

    def decode(self, gsc: bytes, frame_begin: int = 0, frame_end: int = -1, table: bytes | None = None):
        """(int16 array [n, channels], sample_rate) of frames [frame_begin, frame_end).
        With a seek table the index comes from it instead of the host walk."""
        lib = _lib.load()
        if frame_begin != 0 or frame_end != -1 or table is not None:
            ix = Index(gsc, table=table)
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
