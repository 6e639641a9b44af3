"""Opening a stream with a seek table: the contract is that it succeeds if and
only if the walk accepts the stream and the walk's own table equals the given
one byte for byte, and that the index is then the walk's.  The streams are the
smallest that reach each edge (``gsc_writer``) plus the committed goldens.
"""
from __future__ import annotations

import functools
import struct

import numpy as np
import pytest

import gsc_writer as gw
from golden.cases import CASES, HERE
from test_seek_table import parse_table

pytestmark = pytest.mark.gpu

GOLDENS = sorted(p.stem for p in HERE.glob("*.gsc"))
RES_FRAME_BYTES = 192  # sizeof(gsc::ResFrame): what an open uploads per frame besides the slabs


@pytest.fixture(scope="module")
def sc():
    import soundchunks_amd

    return soundchunks_amd


@pytest.fixture(scope="module")
def S(sc):
    return sc.Decoder.checkpoint_symbols()


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


def _check_equal(sc, gsc, table=None, what=""):
    dec = sc.Decoder()
    walked = sc.Decoder.index(gsc)
    t = walked.table() if table is None else table
    assert t == walked.table(), what
    ix = sc.Decoder.index(gsc, table=t)
    _same_index(ix, walked)
    assert ix.table() == t, what
    want, rate = dec.decode(gsc)
    got, grate = dec.decode(gsc, table=t)
    assert grate == rate and got.dtype == want.dtype and np.array_equal(got, want), what
    sw, st = sc.Decoder.open(gsc), sc.Decoder.open(gsc, table=t)
    try:
        _same_index(st.index, walked)
        for a, b in _ranges(walked):
            assert np.array_equal(st.decode_samples(a, b), sw.decode_samples(a, b)), (what, a, b)
            assert np.array_equal(st.decode_samples(a, b), want[a:b]), (what, a, b)
    finally:
        sw.close()
        st.close()
    return t


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_opens_with_its_table(sc, name):
    _check_equal(sc, (HERE / f"{name}.gsc").read_bytes(), what=name)


# ---- segment edges -------------------------------------------------------------

def _frame_with_bits(rng, rem, **kw):
    for _ in range(2000):
        syms = gw.random_symbols(rng, 2 * 128 + 77, kw["count"])
        if gw.pack_symbols(syms, 1)[1] % 16 == rem:
            return gw.frame(syms, att=rng.integers(0, 16, kw["count"]),
                            codes=rng.integers(0, 256, (kw["count"], kw["cs"])), **kw)
    raise AssertionError("no stream with that bit count")


@functools.lru_cache(maxsize=None)
def _edge_streams(S):
    rng = np.random.default_rng(2024)
    out = {}
    for n in (0, 1, S - 1, S, S + 1, 2 * S):
        out[f"{n} symbols"] = gw.random_frame(rng, n, count=600, cs=3)
    att, codes = rng.integers(0, 16, 70), rng.integers(0, 256, (70, 3))
    # width -1 throughout: 3-bit symbols at StreamVersion 1, 2-bit symbols at version 0
    out["no header, 3-bit symbols"] = gw.frame([(i & 1, (i >> 1) & 1, None, 0) for i in range(2 * S + 44)], count=70,
                                               cs=3, att=att, codes=codes)
    out["no header, 2-bit symbols"] = gw.frame([(i & 1, 0, None, 0) for i in range(2 * S + 44)], ver=0, count=70,
                                               cs=3, att=att, codes=codes)
    out["StreamVersion 0"] = gw.random_frame(rng, 3 * S + 5, count=600, cs=3, ver=0)
    for policy in ("always", "once"):
        out[f"headers {policy}"] = gw.random_frame(rng, 3 * S + 5, ch=1, count=4096, cs=2, policy=policy)
    for rem in (0, 1, 15):
        out[f"{rem} bits into the last word"] = _frame_with_bits(rng, rem, count=300, cs=4)
    odd = gw.random_frame(rng, S + 9, count=5, cs=4)  # 12 + 3 + 20 + 4: the bitstream starts at byte 39
    assert (12 + (5 + 1) // 2 + 5 * 4 + 4) % 2 == 1
    out["bitstream at an odd byte"] = odd
    out["two stereo frames, other ChunkSize and depth"] = (
        gw.random_frame(rng, 2 * S + 2, ch=2, count=300, cs=4, bd=8) +
        gw.random_frame(rng, S + 6, ch=2, count=900, cs=6, bd=12))
    out["an empty frame between two"] = (gw.random_frame(rng, S + 3, count=100, cs=4) +
                                          gw.random_frame(rng, 0, count=7, cs=2) +
                                          gw.random_frame(rng, 2 * S + 1, count=50, cs=5))
    return out


EDGE_NAMES = list(_edge_streams(128))


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_segment_edges(sc, S, name):
    gsc = _edge_streams(S)[name]
    t = _check_equal(sc, gsc, what=name)
    _, F, _, P, _, _, _ = parse_table(t)
    if name.endswith("symbols") and name[0].isdigit():
        assert (F, P) == (1, -(-int(name.split()[0]) // S))


# ---- the encoder's own table ----------------------------------------------------

@pytest.mark.parametrize("name", ["syn1s_cs1_cpf256", "syn2s_cs7_mono_cbd12", "square_empty_frame0_cs4",
                                  "tiny_passthrough_cs8"])
def test_encoder_emits_the_walks_table(sc, name):
    make, argv = CASES[name][:2]
    wav = make()
    enc = sc.Encoder(argv)
    gsc, t = enc.encode(wav, with_table=True)
    assert gsc == enc.encode(wav) == (HERE / f"{name}.gsc").read_bytes()
    assert t == sc.Decoder.index(gsc).table()
    _check_equal(sc, gsc, table=t, what=name)


@pytest.mark.parametrize("name", ["syn13s_48k_cs4_cpf256_fl13000", "c1_test_cs8_cpf256"])
def test_encoder_table_of_a_frame_range(sc, name):
    """Prepared.encode(1, 3, with_table=True): offsets are relative to the
    returned bytes.  The first case has one frame, so its range is empty: no
    bytes, and no table either (an empty stream has no index)."""
    make, argv = CASES[name][:2]
    p = sc.Encoder(argv).prepare(make())
    try:
        gsc, t = p.encode(1, 3, with_table=True)
        assert gsc == p.encode(1, 3)
        if p.frame_count <= 1:
            assert gsc == b"" and t == b""
            return
        assert t == sc.Decoder.index(gsc).table()
        assert parse_table(t)[1] == min(3, p.frame_count) - 1
        _check_equal(sc, gsc, table=t, what=name)
    finally:
        p.close()


# ---- refusals -------------------------------------------------------------------

def _refused(sc, gsc, bad, good, match=None):
    """Both entry points refuse `bad`; the next valid open still works."""
    for opener in (sc.Decoder.index, sc.Decoder.open):
        with pytest.raises(sc.GscError, match=match):
            opener(gsc, table=bytes(bad))
    st = sc.Decoder.open(gsc, table=good)
    try:
        n = st.samples_per_channel
        assert st.decode_samples(0, min(n, 64)).shape == (min(n, 64), st.channels)
    finally:
        st.close()


@pytest.fixture(scope="module")
def two_frames(sc, S):
    rng = np.random.default_rng(77)
    gsc = gw.random_frame(rng, 3 * S + 5, count=600, cs=3) + gw.random_frame(rng, 2 * S + 1, count=90, cs=4)
    t = sc.Decoder.index(gsc).table()
    assert parse_table(t)[1:4:2] == (2, 7)
    return gsc, t


def _edit(t, at, fmt, fn):
    b = bytearray(t)
    (v,) = struct.unpack_from(fmt, b, at)
    struct.pack_into(fmt, b, at, fn(v) & ((1 << (8 * struct.calcsize(fmt))) - 1))
    return b


CP0 = 32 + 16 * 2  # the first checkpoint of the two_frames table


@pytest.mark.parametrize("cp,delta,where", [(2, 8, "frame 0.*checkpoint 1"), (2, -8, "frame 0.*checkpoint 1"),
                                            (3, 8, "frame 0.*checkpoint 2"), (6, -8, "frame 1.*checkpoint 1"),
                                            (5, 8, "frame 1.*checkpoint 0")])
def test_checkpoint_bit_offset_off_by_one(sc, two_frames, cp, delta, where):
    gsc, t = two_frames
    _refused(sc, gsc, _edit(t, CP0 + 8 * cp, "<Q", lambda v: v + delta), t, match=where)


@pytest.mark.parametrize("cp", [1, 3, 6])
def test_checkpoint_header_state_changed(sc, two_frames, cp):
    gsc, t = two_frames
    for state in range(5):
        bad = _edit(t, CP0 + 8 * cp, "<Q", lambda v: (v & ~7) | state)
        if bytes(bad) != t:
            _refused(sc, gsc, bad, t, match="checkpoint")


@pytest.mark.parametrize("low", [5, 6, 7])
def test_checkpoint_low_bits_out_of_range(sc, two_frames, low):
    gsc, t = two_frames
    _refused(sc, gsc, _edit(t, CP0 + 8 * 2, "<Q", lambda v: (v & ~7) | low), t, match="header state out of range")


def test_checkpoints_swapped(sc, two_frames):
    gsc, t = two_frames
    for a, b in ((1, 2), (2, 5), (0, 4)):
        bad = bytearray(t)
        bad[CP0 + 8 * a:CP0 + 8 * a + 8], bad[CP0 + 8 * b:CP0 + 8 * b + 8] = \
            t[CP0 + 8 * b:CP0 + 8 * b + 8], t[CP0 + 8 * a:CP0 + 8 * a + 8]
        if bytes(bad) != t:
            _refused(sc, gsc, bad, t, match="checkpoint")


@pytest.mark.parametrize("delta", [-2, -1, 1, 2])
def test_frame_offset_shifted(sc, two_frames, delta):
    gsc, t = two_frames
    _refused(sc, gsc, _edit(t, 32 + 16, "<Q", lambda v: v + delta), t, match="frame")
    _refused(sc, gsc, _edit(t, 32, "<Q", lambda v: v + 1), t, match="frame 0 is not at offset 0")


@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("delta", [-16, -1, 1, 16])
def test_nbits_changed(sc, two_frames, frame, delta):
    gsc, t = two_frames
    _refused(sc, gsc, _edit(t, 32 + 16 * frame + 8, "<Q", lambda v: v + delta), t, match=f"frame {frame}")


def test_counts_sizes_and_header_fields(sc, S, two_frames):
    gsc, t = two_frames
    for at, fmt, fn in ((24, "<Q", lambda v: v + 1), (24, "<Q", lambda v: v - 1), (12, "<I", lambda v: v + 1),
                        (12, "<I", lambda v: v - 1), (4, "<I", lambda v: v + 1), (0, "<I", lambda v: v ^ 1)):
        _refused(sc, gsc, _edit(t, at, fmt, fn), t, match="seek table")
    # P and F off by one with the size to match
    _refused(sc, gsc, _edit(t, 24, "<Q", lambda v: v + 1) + bytes(8), t, match="seek table")
    _refused(sc, gsc, _edit(t, 24, "<Q", lambda v: v - 1)[:-8], t, match="seek table")
    _refused(sc, gsc, _edit(t, 12, "<I", lambda v: v - 1)[:32 + 16] + t[CP0:], t, match="seek table")
    _refused(sc, gsc, t[:-1], t, match="seek table")
    _refused(sc, gsc, t[:31], t, match="seek table")
    _refused(sc, gsc, t + b"\0", t, match="seek table")
    _refused(sc, gsc, _edit(t, 8, "<I", lambda v: 2 * S), t, match=f"written with {2 * S} symbols per checkpoint")
    _refused(sc, gsc, _edit(t, 16, "<Q", lambda v: v + 2), t, match="made for a stream of")
    for opener in (sc.Decoder.index, sc.Decoder.open):  # the right table, a longer stream
        with pytest.raises(sc.GscError, match="made for a stream of"):
            opener(gsc + b"\0\0", table=t)


def test_table_of_another_stream(sc, two_frames):
    gsc, t = two_frames
    other = (HERE / "tiny_passthrough_cs8.gsc").read_bytes()
    _refused(sc, gsc, sc.Decoder.index(other).table(), t, match="seek table")
    # same length, same frame layout, other symbols
    rng = np.random.default_rng(78)
    S = sc.Decoder.checkpoint_symbols()
    for _ in range(200):
        alt = gw.random_frame(rng, 3 * S + 5, count=600, cs=3) + gw.random_frame(rng, 2 * S + 1, count=90, cs=4)
        if len(alt) == len(gsc):
            break
    else:
        raise AssertionError("no stream of the same length")
    # refused by whatever comes first: the header read at a wrong offset, the chain of lengths, or a checkpoint
    _refused(sc, gsc, sc.Decoder.index(alt).table(), t)


FLIP_SEED, FLIPS = 8, 20  # 10 accepted, 9 refused by the walk, 1 with another table (checked with the walk alone)


def flip_cases():
    """A stream of 15-bit symbols (one header of width 3, ChunkCount 4096: every
    index is valid) and FLIPS seeded single-byte edits inside its bitstream."""
    rng = np.random.default_rng(FLIP_SEED)
    gsc = gw.random_frame(rng, 2 * 128 + 9, count=4096, cs=1, policy="once")
    bs = 12 + 2048 + 4096 + 4
    out = []
    for _ in range(FLIPS):
        at = int(rng.integers(bs, len(gsc)))
        b = bytearray(gsc)
        b[at] ^= int(rng.integers(1, 256))
        out.append(bytes(b))
    return gsc, out


def test_flipped_stream_bytes_follow_the_walk(sc):
    gsc, flips = flip_cases()
    t = sc.Decoder.index(gsc).table()
    accepted = refused = 0
    for bad in flips:
        try:
            same = sc.Decoder.index(bad).table() == t
        except sc.GscError:
            same = False
        if same:
            _check_equal(sc, bad, table=t)
            accepted += 1
        else:
            for opener in (sc.Decoder.index, sc.Decoder.open):
                with pytest.raises(sc.GscError):
                    opener(bad, table=t)
            refused += 1
    assert accepted >= 1 and refused >= 5, (accepted, refused)
    _check_equal(sc, gsc, table=t)


def test_index_equal_to_chunk_count(sc, S):
    """The walk refuses a chunk index >= ChunkCount; with a table the device
    has to.  Index ChunkCount - 1 at the same place is accepted."""
    rng = np.random.default_rng(79)
    count = 100
    syms = gw.random_symbols(rng, 2 * S + 20, count, policy="once")
    att, codes = rng.integers(0, 16, count), rng.integers(0, 256, (count, 3))
    at = S + 17
    neg, rev, header, _ = syms[at]
    syms[at] = (neg, rev, header, count - 1)
    good = gw.frame(syms, count=count, cs=3, att=att, codes=codes)
    syms[at] = (neg, rev, header, count)
    bad = gw.frame(syms, count=count, cs=3, att=att, codes=codes)
    t = _check_equal(sc, good)
    assert len(bad) == len(good)
    with pytest.raises(sc.GscError, match="chunk index 100 >= ChunkCount 100"):
        sc.Decoder.index(bad)
    for opener in (sc.Decoder.index, sc.Decoder.open):
        with pytest.raises(sc.GscError, match="frame 0.*checkpoint 1.*chunk index >= ChunkCount"):
            opener(bad, table=t)
    _check_equal(sc, good, table=t)


def test_last_open_timing(sc, two_frames):
    gsc, t = two_frames
    _, F, _, P, _, _, _ = parse_table(t)
    ix = sc.Decoder.index(gsc, table=t)
    tim = sc.Decoder.last_open_timing()
    assert tim["checkpoints"] == P == 7
    assert tim["uploaded_bytes"] == len(gsc) + 8 * P + RES_FRAME_BYTES * F
    st = sc.Decoder.open(gsc, table=t)
    try:
        tim = sc.Decoder.last_open_timing()
        tables = sum(((int(c) * int(s) + 7) // 8 * 8) * 2 + int(c) for c, s in zip(ix.chunk_count, ix.chunk_size))
        assert tim["checkpoints"] == P
        assert tim["uploaded_bytes"] == len(gsc) + 8 * P + tables + RES_FRAME_BYTES * F
        assert tim["verify_ms"] > 0 and tim["total_ms"] >= tim["host_ms"] + tim["upload_ms"] + tim["verify_ms"] - 1e-6
    finally:
        st.close()
    sw = sc.Decoder.open(gsc)
    try:
        tim = sc.Decoder.last_open_timing()
        assert tim["checkpoints"] == P and tim["verify_ms"] == 0
    finally:
        sw.close()
