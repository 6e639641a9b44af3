"""A small pure-Python ``.gsc`` writer for the decoder tests, written from the
reference decoder's reading order (decoder/decoder.lpr:76-211), so crafted
streams can hold what the encoder never emits: redundant or missing headers,
codes at the wrap-around edge, odd shapes, malformed fields.

A symbol is ``(neg, rev, header, idx)``: ``header`` None writes hasHeader = 0
(the decoder keeps its current width), 0..3 writes hasHeader = 1 plus the two
header bits; the index then takes 3 * (width + 1) bits, most significant block
first, where width is the decoder's state after this symbol's header (-1 at
the frame start: zero index bits, index 0).
"""
from __future__ import annotations

import struct

import numpy as np


def width_of(idx: int) -> int:
    return 0 if idx < 8 else 1 if idx < 64 else 2 if idx < 512 else 3


def pack_symbols(symbols, ver: int):
    """LSB-first bitstream in 16-bit little-endian words: (bytes, bit count)."""
    acc, n, width = 0, 0, -1

    def put(v, bits):
        nonlocal acc, n
        assert 0 <= v < (1 << bits) or bits == 0
        acc |= v << n
        n += bits

    for neg, rev, header, idx in symbols:
        put(int(neg), 1)
        if ver > 0:
            put(int(rev), 1)
        else:
            assert not rev
        if header is None:
            put(0, 1)
        else:
            put(1, 1)
            put(header, 2)
            width = header
        assert idx < (1 << (3 * (width + 1))), (idx, width)
        for j in range(width, -1, -1):
            put((idx >> (3 * j)) & 7, 3)
    words = (n + 15) // 16
    return acc.to_bytes(words * 2, "little"), n


def frame(symbols, *, ver=1, ch=1, count, bd=8, cs, rate=44100, adiv=6, att, codes, flen=None, blend=0):
    """One frame.  ``att``: count attenuations 0..15; ``codes``: count x cs raw
    codebook codes (0..255 at 8 bits, 0..4095 at 12); ``symbols``: flen * ch."""
    if flen is None:
        assert len(symbols) % ch == 0
        flen = len(symbols) // ch
    att = list(att)
    codes = np.asarray(codes, dtype=np.int64).reshape(count, cs) if count else np.zeros((0, cs), np.int64)
    out = bytearray()
    out += struct.pack("<BBHBB", ver, ch, count, bd, cs)
    out += struct.pack("<I", (rate & 0xFFFFFF) | (blend << 24))
    out += struct.pack("<H", adiv)
    for i in range(count // 2):
        out.append((att[2 * i] << 4) | att[2 * i + 1])
    if count & 1:
        out.append(att[count - 1] << 4)
    if bd == 8:
        out += bytes(int(v) for v in codes.reshape(-1))
    else:
        for row in codes:
            for j in range(cs // 2):
                s1, s2 = int(row[2 * j]), int(row[2 * j + 1])
                out += bytes([((s1 >> 8) & 0xF) << 4 | ((s2 >> 8) & 0xF), s1 & 0xFF, s2 & 0xFF])
            if cs & 1:
                s1 = int(row[cs - 1])
                out += bytes([((s1 >> 8) & 0xF) << 4, s1 & 0xFF])
    out += struct.pack("<I", flen)
    bits, _ = pack_symbols(symbols, ver)
    out += bits
    return bytes(out)


def random_symbols(rng, n, count, policy="minimal", ver=1):
    """n symbols with indices < min(count, 4096) (an index has at most 12 bits).  policy: 'minimal' (a header only when
    the needed width changes, as the encoder writes), 'always' (a header on
    every symbol, a random width that fits), 'once' (one header of width 3)."""
    syms, width = [], -1
    for i in range(n):
        idx = int(rng.integers(0, min(count, 4096)))
        neg = int(rng.integers(0, 2))
        rev = int(rng.integers(0, 2)) if ver > 0 else 0
        if policy == "always":
            header = int(rng.integers(width_of(idx), 4))
        elif policy == "once":
            header = 3 if i == 0 else None
        else:
            header = width_of(idx) if width_of(idx) != width else None
        if header is not None:
            width = header
        syms.append((neg, rev, header, idx))
    return syms


def random_frame(rng, nsym, *, ch=1, count=100, bd=8, cs=4, policy="minimal", ver=1, **kw):
    assert nsym % ch == 0
    hi = 256 if bd == 8 else 4096
    return frame(random_symbols(rng, nsym, count, policy, ver), ver=ver, ch=ch, count=count, bd=bd, cs=cs,
                 att=rng.integers(0, 16, count), codes=rng.integers(0, hi, (count, cs)), **kw)
