"""Stream sets (``Decoder.open_many``): many streams in one set of device slabs,
their codebooks and attenuations expanded by expand_tables_kernel, every seek
table checked in one launch.  A member must be indistinguishable from the same
stream opened on its own, and a refusal must name the lowest refused stream.
The crafted streams (``gsc_writer``) are the smallest that reach each edge of
the expansion; the goldens the smallest that cover mono, a 12-bit odd
ChunkSize, an empty frame 0 and a -py file.
"""
from __future__ import annotations

import ctypes
import functools
import struct

import numpy as np
import pytest

import gsc_writer as gw
from golden.cases import HERE
from test_seek_table import parse_table

pytestmark = pytest.mark.gpu

GOLDENS = ["syn2s_cs7_mono_cbd12", "square_empty_frame0_cs4", "tone_lsb45_cs4_cpf256_py", "tiny_passthrough_cs8"]
S_BUILD = 128  # the checkpoint distance the crafted refusal streams are sized for (checked against the library's)


@pytest.fixture(scope="module")
def sc():
    # torch before the library loads, as when the whole suite is collected: torch brings a HIP runtime of
    # its own and the library then shares it; loaded the other way round the process would hold two
    import torch  # noqa: F401

    import soundchunks_amd

    assert soundchunks_amd.Decoder.checkpoint_symbols() == S_BUILD
    return soundchunks_amd


# ---- decoder.lpr:115-158, restated -------------------------------------------------

def frame_fields(gsc: bytes, off: int):
    """(ChunkCount, ChunkBitDepth, ChunkSize, attenuation bytes, codebook bytes, ChannelCount, FrameLength,
    offset of the bitstream) of the frame at byte `off`."""
    _, ch, count, bd, cs = struct.unpack_from("<BBHBB", gsc, off)
    count &= 0x1FFF
    na = (count + 1) // 2
    nc = count * cs if bd == 8 else count * ((cs // 2) * 3 + (cs & 1) * 2)
    a0 = off + 12
    (flen,) = struct.unpack_from("<I", gsc, a0 + na + nc)
    return count, bd, cs, gsc[a0:a0 + na], gsc[a0 + na:a0 + na + nc], ch, flen, a0 + na + nc + 4


def expand_tables(count, bd, cs, att_bytes, cb_bytes):
    """Attenuations [count] and Chunks [count * cs] as the reference decoder reads them."""
    a = np.frombuffer(att_bytes, np.uint8).astype(np.int64)
    att = np.stack([a >> 4, a & 15], axis=1).reshape(-1)[:count]  # high nibble first; an odd count ends half a byte
    b = np.frombuffer(cb_bytes, np.uint8).astype(np.int64)
    if bd == 8:
        v = (b - 128) * 2047
        cb = np.sign(v) * (np.abs(v) // 127)  # Pascal div: toward zero
    else:
        cb = np.zeros((count, cs), np.int64)
        per = (cs // 2) * 3 + (cs & 1) * 2
        rows = b.reshape(count, per) if count else b.reshape(0, per)
        for j in range(cs // 2):
            b0, b1, b2 = rows[:, 3 * j], rows[:, 3 * j + 1], rows[:, 3 * j + 2]
            cb[:, 2 * j] = (b1 | (b0 & 0xF0) << 4) - 2048
            cb[:, 2 * j + 1] = (b2 | (b0 & 0x0F) << 8) - 2048
        if cs & 1:
            b0, b1 = rows[:, per - 2], rows[:, per - 1]
            cb[:, cs - 1] = (b1 | (b0 & 0xF0) << 4) - 2048
        cb = cb.reshape(-1)
    return att.astype(np.uint8), cb.astype(np.int16)


def device_tables(sc, st, frame, count, cs):
    slots = (count * cs + 7) // 8 * 8
    cb = np.full(max(slots, 1), 0x5A5A, np.int16)
    att = np.full(max(count, 1), 0xA5, np.uint8)
    rc = sc.load().gsc_stream_tables(st._handle(), frame, cb.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                     att.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    assert rc == 0, sc.load().gsc_last_error()
    return att[:count], cb[:slots]


@functools.lru_cache(maxsize=None)
def crafted():
    """Mono streams of 1-3 frames of at most 300 symbols: both bit depths at every ChunkSize of
    (1, 2, 3, 7, 8, 15, 16); ChunkCount 1, odd counts and 40; the 8-bit codes around the sign change;
    a frame of FrameLength 0; lengths that leave the following streams at every byte offset modulo 4."""
    rng = np.random.default_rng(4242)
    counts = [1, 5, 40, 37, 3, 9, 2]
    frames = []
    for bd in (8, 12):
        for k, cs in enumerate((1, 2, 3, 7, 8, 15, 16)):
            count = counts[(k + (bd == 12)) % len(counts)]
            frames.append(gw.random_frame(rng, int(rng.integers(1, 301)), count=count, bd=bd, cs=cs))
    edge = np.array([[0, 127, 128, 129, 255, 1, 126, 130], [254, 64, 192, 127, 129, 128, 0, 255],
                     [2, 3, 125, 131, 253, 200, 100, 50]])
    frames.append(gw.frame(gw.random_symbols(rng, 200, 3), count=3, cs=8, att=[15, 0, 7], codes=edge))
    frames.append(gw.random_frame(rng, 0, count=7, cs=2))  # FrameLength 0
    frames.append(gw.random_frame(rng, 300, count=40, bd=12, cs=3))
    sizes = [1, 2, 3, 1, 3, 2, 1, 1, 2, 1]
    assert sum(sizes) == len(frames)
    out, at = [], 0
    for n in sizes:
        out.append(b"".join(frames[at:at + n]))
        at += n
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _walk(gsc):
    import soundchunks_amd as sc

    return sc.Decoder.index(gsc)


def _assert_coverage():
    """The coverage the expansion test relies on, read back from the bytes."""
    seen, offsets, at = set(), set(), 0
    for g in crafted():
        offsets.add(at % 4)
        at += len(g)
        for off in _walk(g).byte_offset[:-1]:
            count, bd, cs, _, cb, ch, flen, _ = frame_fields(g, int(off))
            seen.update([(bd, cs), ("count", count), ("pad", (count * cs) % 8 != 0), ("flen0", flen == 0)])
            if bd == 8:
                seen.update(("code", c) for c in cb)
            assert ch == 1 and flen <= 300
    for bd in (8, 12):
        for cs in (1, 2, 3, 7, 8, 15, 16):
            assert (bd, cs) in seen
    for c in (1, 5, 37, 40):
        assert ("count", c) in seen
    for c in (0, 127, 128, 129, 255):
        assert ("code", c) in seen
    assert ("pad", True) in seen and ("pad", False) in seen and ("flen0", True) in seen
    assert offsets == {0, 1, 2, 3}


def _assert_restatement():
    """The restatement against the codes the writer was given: 12 bit is code - 2048, 8 bit truncates toward zero."""
    rng = np.random.default_rng(5)
    for bd, cs, count in ((8, 3, 5), (12, 7, 3), (12, 1, 1), (12, 16, 2), (8, 1, 1)):
        hi = 256 if bd == 8 else 4096
        att, codes = rng.integers(0, 16, count), rng.integers(0, hi, (count, cs))
        g = gw.frame([], count=count, bd=bd, cs=cs, att=att, codes=codes)
        c, b, s, ab, cbb, _, flen, _ = frame_fields(g, 0)
        assert (c, b, s, flen) == (count, bd, cs, 0)
        got_att, got_cb = expand_tables(c, b, s, ab, cbb)
        want = codes.reshape(-1) - 2048 if bd == 12 else np.trunc((codes.reshape(-1) - 128) * 2047 / 127)
        assert np.array_equal(got_att, att) and np.array_equal(got_cb, want.astype(np.int16))
    assert list(expand_tables(1, 8, 5, b"\0", bytes([0, 127, 128, 129, 255]))[1]) == [-2063, -16, 0, 16, 2047]


def test_expansion_every_entry(sc):
    _assert_coverage()
    _assert_restatement()
    streams = list(crafted())
    tables = [_walk(g).table() for g in streams]
    n = len(streams)
    # every stream twice: once with its table, once walked
    ss = sc.Decoder.open_many(streams + streams, tables + [None] * n)
    try:
        assert len(ss) == 2 * n
        for i in range(2 * n):
            g, ix = streams[i % n], _walk(streams[i % n])
            assert ss[i].frame_count == ix.frame_count
            for k in range(ix.frame_count):
                count, bd, cs, ab, cbb, _, _, _ = frame_fields(g, int(ix.byte_offset[k]))
                want_att, want_cb = expand_tables(count, bd, cs, ab, cbb)
                att, cb = device_tables(sc, ss[i], k, count, cs)
                assert np.array_equal(att, want_att), (i, k, "attenuations")
                assert np.array_equal(cb[:count * cs], want_cb), (i, k, "codebook")
                assert not cb[count * cs:].any(), (i, k, "padding")
    finally:
        ss.close()


def test_a_thousand_members(sc):
    """1024 members (the crafted streams over and over, tables and walks alternating): every member's
    first frame's device tables and its first samples, so a lane that finds the wrong frame among
    thousands, or a rebase that drifts, shows."""
    base = list(crafted())
    streams = [base[i % len(base)] for i in range(1024)]
    tables = [_walk(g).table() if i % 2 else None for i, g in enumerate(streams)]
    pcm = [sc.Decoder().decode(g)[0] for g in base]
    want = []
    for g in base:
        count, bd, cs, ab, cbb, _, _, _ = frame_fields(g, 0)
        want.append((count, cs) + expand_tables(count, bd, cs, ab, cbb))
    ss = sc.Decoder.open_many(streams, tables)
    try:
        assert sc.Decoder.last_set_open_timing()["streams"] == 1024
        for i in range(1024):
            count, cs, want_att, want_cb = want[i % len(base)]
            att, cb = device_tables(sc, ss[i], 0, count, cs)
            assert np.array_equal(att, want_att) and np.array_equal(cb[:count * cs], want_cb), i
            assert not cb[count * cs:].any(), i
            n = min(len(pcm[i % len(base)]), 300)
            assert np.array_equal(ss[i].decode_samples(0, n), pcm[i % len(base)][:n]), i
    finally:
        ss.close()


# ---- a member equals the stream opened on its own -----------------------------------

FIELDS = ("byte_offset", "first_sample", "frame_length", "chunk_size", "chunk_count")


def _same_index(a, b):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.channels, a.sample_rate, a.samples_per_channel, a.frame_count) == \
        (b.channels, b.sample_rate, b.samples_per_channel, b.frame_count)


def _ranges(ix):
    """Sample ranges that cross a frame edge and the stream's end."""
    n = ix.samples_per_channel
    if n == 0:
        return [(0, 0)]
    out = [(0, min(n, 97)), (max(0, n - 53), n)]
    for b in [int(v) for v in ix.first_sample[1:-1] if 0 < v < n][:2]:
        out.append((max(0, b - 37), min(n, b + 41)))
    return out


def test_members_equal_single_opens(sc):
    streams = [(HERE / f"{name}.gsc").read_bytes() for name in GOLDENS] + list(crafted())
    tables = [_walk(g).table() if i % 2 == 0 else None for i, g in enumerate(streams)]
    dec = sc.Decoder()
    ss = sc.Decoder.open_many(streams, tables)
    try:
        tim = sc.Decoder.last_set_open_timing()
        assert tim["streams"] == len(streams) == len(ss)
        assert tim["frames"] == sum(_walk(g).frame_count for g in streams)
        for i, g in enumerate(streams):
            walked = _walk(g)
            m = ss[i]
            _same_index(m.index, walked)
            assert (m.channels, m.sample_rate, m.samples_per_channel, m.frame_count) == \
                (walked.channels, walked.sample_rate, walked.samples_per_channel, walked.frame_count)
            assert m.index.table() == walked.table(), i
            want, _ = dec.decode(g)
            single = sc.Decoder.open(g)
            try:
                assert m.device == single.device
                for a, b in _ranges(walked):
                    got = m.decode_samples(a, b)
                    assert np.array_equal(got, single.decode_samples(a, b)), (i, a, b)
                    assert np.array_equal(got, want[a:b]), (i, a, b)
            finally:
                single.close()
            assert np.array_equal(m.index.decode(), want), i  # the host tables, built on first use
            assert np.array_equal(m.index.decode(0, 1), dec.decode(g, 0, 1)[0]), i
    finally:
        ss.close()


# ---- crops across owners -------------------------------------------------------------

def _mono(rng, nsym, **kw):
    return gw.random_frame(rng, nsym, ch=1, **kw)


@pytest.fixture(scope="module")
def owners(sc):
    """Two members of one set, a member of a second set, a stream opened on its own; all mono."""
    rng = np.random.default_rng(99)
    gscs = [_mono(rng, 300, count=40, cs=4) + _mono(rng, 200, count=9, bd=12, cs=7),
            _mono(rng, 290, count=600, cs=3),
            _mono(rng, 150, count=5, cs=8) + _mono(rng, 0, count=7, cs=2) + _mono(rng, 260, count=37, bd=12, cs=15),
            _mono(rng, 280, count=100, cs=5)]
    pcm = [sc.Decoder().decode(g)[0] for g in gscs]
    one = sc.Decoder.open_many(gscs[:2], [_walk(gscs[0]).table(), None])
    two = sc.Decoder.open_many([gscs[3], gscs[2]], [None, _walk(gscs[2]).table()])
    alone = sc.Decoder.open(gscs[3])
    yield [one[0], one[1], two[1], alone], pcm
    one.close()
    two.close()
    alone.close()


def _check_crops(sc, streams, pcm, crops, length, dtype, layout):
    import torch

    x, written = sc.Decoder.decode_crops(streams, crops, length, dtype=getattr(torch, dtype), layout=layout)
    x = x.cpu().numpy()
    for i, (s, b, n) in enumerate(crops):
        want = pcm[s][b:b + n]
        assert written[i] == len(want), (i, written[i])
        row = x[i] if layout == "TC" else x[i].T
        if dtype == "float32":
            want = want.astype(np.float32) / 32768
        assert np.array_equal(row[:len(want)], want), i
        assert not row[len(want):].any(), i


def test_crops_across_owners(sc, owners):
    streams, pcm = owners
    n = [len(p) for p in pcm]
    crops = [(0, 3, 500), (1, 0, 450), (2, 1190, 512), (3, n[3] - 20, 64), (0, 1150, 512), (2, 0, 1), (1, n[1], 5)]
    assert n[0] > 1200 + 150 and n[2] > 1200 + 600  # crops 2 and 4 cross a frame edge (and an empty frame)
    _check_crops(sc, streams, pcm, crops, 512, "int16", "TC")
    _check_crops(sc, streams, pcm, crops, 512, "float32", "CT")


def test_crops_on_members(sc, owners):
    streams, pcm = owners
    _check_crops(sc, streams, pcm, [(0, 1190, 100), (2, 5, 90), (3, len(pcm[3]) - 7, 30), (1, 40, 100)], 100,
                 "int16", "TC")


# ---- refusals, each from the lowest refused stream -------------------------------------

@pytest.fixture(scope="module")
def four(sc):
    """Four two-frame streams of 4 + 3 checkpoints, and their tables."""
    rng = np.random.default_rng(77)
    S = S_BUILD
    gscs = [gw.random_frame(rng, 3 * S + 5, count=600, cs=3) + gw.random_frame(rng, 2 * S + 1, count=90, cs=4)
            for _ in range(4)]
    tables = [_walk(g).table() for g in gscs]
    assert all(parse_table(t)[1:4:2] == (2, 7) for t in tables)
    return gscs, tables


CP0 = 32 + 16 * 2  # the first checkpoint of a `four` table


def _moved(t, cp, delta):
    b = bytearray(t)
    (v,) = struct.unpack_from("<Q", b, CP0 + 8 * cp)
    struct.pack_into("<Q", b, CP0 + 8 * cp, v + delta)
    return bytes(b)


def _still_opens(sc, gscs, tables):
    ss = sc.Decoder.open_many(gscs, tables)
    try:
        assert ss[len(gscs) - 1].decode_samples(0, 64).shape == (64, 1)
    finally:
        ss.close()


def test_a_moved_checkpoint_names_its_stream(sc, four):
    gscs, tables = four
    bad = list(tables)
    bad[2] = _moved(tables[2], 6, -8)  # frame 1's third checkpoint: its second segment no longer lands on it
    with pytest.raises(sc.GscError, match=r"stream 2: .*frame 1.*checkpoint 1.*another bit offset"):
        sc.Decoder.open_many(gscs, bad)
    bad = list(tables)
    bad[1] = _moved(tables[1], 2, 8)
    bad[3] = _moved(tables[3], 1, 8)
    with pytest.raises(sc.GscError, match=r"stream 1: .*frame 0.*checkpoint 1.*another bit offset"):
        sc.Decoder.open_many(gscs, bad)
    _still_opens(sc, gscs, tables)


def test_other_refusals(sc, four):
    gscs, tables = four
    other = (HERE / "tiny_passthrough_cs8.gsc").read_bytes()
    with pytest.raises(sc.GscError, match=r"stream 1: gsc seek table: made for a stream of"):
        sc.Decoder.open_many(gscs, [tables[0], _walk(other).table(), tables[2], tables[3]])
    with pytest.raises(sc.GscError, match=r"stream 2: gsc decode: frame 1"):
        sc.Decoder.open_many([gscs[0], gscs[1], gscs[2][:-2], gscs[3][:-2]], [tables[0], tables[1], None, None])
    with pytest.raises(sc.GscError, match="no streams"):
        sc.Decoder.open_many([])
    # a well-formed table at twice the checkpoint distance: every second checkpoint of each frame
    S, F, length, P, off, nbits, cps = parse_table(tables[1])
    keep = np.concatenate([cps[0:4:2], cps[4:7:2]])
    wide = struct.pack("<4sIIIQQ", b"GSCT", 1, 2 * S, F, length, len(keep)) + \
        np.stack([off, nbits], axis=1).astype("<u8").tobytes() + keep.astype("<u8").tobytes()
    assert parse_table(wide)[0] == 2 * S
    with pytest.raises(sc.GscError, match=rf"stream 1: gsc seek table: written with {2 * S} symbols per checkpoint"):
        sc.Decoder.open_many(gscs, [None, wide, tables[2], wide])
    _still_opens(sc, gscs, tables)


def test_member_after_close_and_stream_free_on_a_member(sc, four):
    gscs, tables = four
    want = sc.Decoder().decode(gscs[0])[0]
    ss = sc.Decoder.open_many(gscs, tables)
    m = ss[0]
    lib = sc.load()
    lib.gsc_stream_free(m._handle())  # borrowed: frees nothing
    assert b"belongs to a stream set" in lib.gsc_last_error()
    assert np.array_equal(m.decode_samples(0, 200), want[:200])
    assert np.array_equal(ss[3].decode_samples(5, 60), sc.Decoder().decode(gscs[3])[0][5:60])
    streams = ss.streams
    ss.close()
    with pytest.raises(sc.GscError, match="the resident stream is closed"):
        m.decode_samples(0, 10)
    with pytest.raises(sc.GscError, match="the resident stream is closed"):
        sc.Decoder.decode_crops(streams, [(1, 0, 10)], 10)
    with pytest.raises(sc.GscError, match="the resident stream is closed"):
        ss[2].decode_samples(0, 1)
    ss.close()
    m.close()


# ---- the runtime calls do not follow the stream count -----------------------------------

def test_fixed_call_counts(sc):
    small = list(crafted())[:4]
    counts = []
    for gscs in (small[:2], small * 10):
        tables = [_walk(g).table() if i % 3 else None for i, g in enumerate(gscs)]
        ss = sc.Decoder.open_many(gscs, tables)
        try:
            tim = sc.Decoder.last_set_open_timing()
            assert tim["streams"] == len(gscs)
            counts.append({k: tim[k] for k in ("device_allocations", "h2d_copies", "launches", "synchronisations")})
            assert ss[len(gscs) - 1].decode_samples(0, 1).shape == (1, 1)
        finally:
            ss.close()
    assert counts[0] == counts[1], counts
    # counted in Dev::alloc, in the launchers and at the wait: the five slabs and one block, two kernels, one wait
    assert counts[0] == {"device_allocations": 6, "h2d_copies": 4, "launches": 2, "synchronisations": 1}, counts
