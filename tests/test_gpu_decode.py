"""The GPU decoder against the oracle's decoder (oracle/gsc_oracle.c ora_decode,
decoder/decoder.lpr:37-220): every committed golden, and crafted streams that
hold what the encoder never emits.  Every comparison is exact.  Crafted
streams use StreamVersion 1 (the oracle leaves `rev` unset at version 0).
"""
from __future__ import annotations

import struct

import numpy as np
import pytest

import gsc_writer as gw
import oracle_ffi
from golden.cases import CASES, HERE

pytestmark = pytest.mark.gpu

GOLDENS = sorted(p.stem for p in HERE.glob("*.gsc"))


@pytest.fixture(scope="module")
def dec():
    import soundchunks_amd as sc

    return sc.Decoder()


def _check(dec, gsc, what=""):
    want, ch, rate = oracle_ffi.decode(gsc)
    got, grate = dec.decode(gsc)
    assert got.dtype == np.int16 and got.shape == (len(want) // ch, ch), what
    assert grate == rate, what
    assert np.array_equal(got.reshape(-1), want), what
    return got


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_decodes_like_the_oracle(dec, name):
    _check(dec, (HERE / f"{name}.gsc").read_bytes(), name)


def test_decode_wav_header(dec):
    gsc = (HERE / "syn2s_cs5_cpf512.gsc").read_bytes()
    want, ch, rate = oracle_ffi.decode(gsc)
    wav = dec.decode_wav(gsc)
    assert len(wav) == 44 + 2 * len(want)
    (rid, rlen, wid, fid, flen, tag, nch, sps, bps, align, bits, did, dlen) = struct.unpack("<4sI4s4sIHHIIHH4sI", wav[:44])
    assert (rid, wid, fid, did) == (b"RIFF", b"WAVE", b"fmt ", b"data")
    assert (rlen, flen, tag, nch, sps, bps, align, bits, dlen) == (36 + 2 * len(want), 16, 1, ch, rate, ch * rate * 2,
                                                                   ch * 2, 16, 2 * len(want))
    assert np.array_equal(np.frombuffer(wav[44:], dtype="<i2"), want)


# ---- crafted streams ---------------------------------------------------------

def test_wrap_around(dec):
    """8-bit codes 0 and 255 at attenuation 0 and 15, both signs: the reference
    wraps (Cardinal(attr * smp) shr 15, low word), it does not clamp."""
    att = [0, 15, 0, 15]
    codes = [[0, 255, 0, 255], [0, 255, 0, 255], [255, 0, 128, 1], [255, 0, 128, 1]]
    syms = [(neg, rev, 0 if i == 0 else None, idx) for i, (idx, neg, rev) in
            enumerate((i, n, r) for i in range(4) for n in (0, 1) for r in (0, 1))]
    gsc = gw.frame(syms, count=4, cs=4, att=att, codes=codes, adiv=6)
    got = _check(dec, gsc)
    assert got[0, 0] == 32512  # code 0, attenuation 0, not negated: -2063 * 524528 >> 15 wraps to +32512
    for adiv in (1, 65535):
        _check(dec, gw.frame(syms, count=4, cs=4, att=att, codes=codes, adiv=adiv), adiv)


@pytest.mark.parametrize("policy", ["always", "once", "minimal"])
def test_header_widths(dec, policy):
    rng = np.random.default_rng(10)
    _check(dec, gw.random_frame(rng, 1500, ch=2, count=4096, cs=2, policy=policy), policy)


def test_first_symbol_without_header_and_redundant_headers(dec):
    rng = np.random.default_rng(11)
    att, codes = rng.integers(0, 16, 70), rng.integers(0, 256, (70, 3))
    # no header at width -1: zero index bits, index 0; then headers that repeat the current width
    syms = [(1, 1, None, 0), (0, 0, None, 0), (0, 1, 1, 63), (1, 0, 1, 9), (0, 0, 1, 64 - 1), (1, 1, None, 17),
            (0, 0, 0, 7), (0, 1, 0, 0), (1, 0, 3, 69), (1, 1, 3, 5)]
    _check(dec, gw.frame(syms, count=70, cs=3, att=att, codes=codes))
    # a frame of nothing but header-less symbols
    _check(dec, gw.frame([(i & 1, (i >> 1) & 1, None, 0) for i in range(300)], count=70, cs=3, att=att, codes=codes))


def test_segment_boundaries(dec):
    """FrameLength x ch around the checkpoint spacing S: S - 1, S, S + 1, 3S + 1
    symbols mono; stereo has an even symbol count, so both even neighbours of
    every odd target stand in for it (S - 2, S, S + 2, 3S, 3S + 2)."""
    S = dec.checkpoint_symbols()
    rng = np.random.default_rng(12)
    for ch, ns in ((1, (S - 1, S, S + 1, 3 * S + 1)), (2, (S - 2, S, S + 2, 3 * S, 3 * S + 2))):
        for n in ns:
            _check(dec, gw.random_frame(rng, n, ch=ch, count=600, cs=3, policy="always"), (ch, n))
            _check(dec, gw.random_frame(rng, n, ch=ch, count=600, cs=3), (ch, n))


def _frame_with_bits(rng, rem, **kw):
    for _ in range(2000):
        syms = gw.random_symbols(rng, 333, kw["count"])
        if gw.pack_symbols(syms, 1)[1] % 16 == rem:
            return gw.frame(syms, att=rng.integers(0, 16, kw["count"]),
                            codes=rng.integers(0, 256, (kw["count"], kw["cs"])), **kw)
    raise AssertionError("no stream with that bit count")


@pytest.mark.parametrize("rem", [0, 1, 15])
def test_word_alignment(dec, rem):
    """A bitstream ends on a 16-bit word boundary of its own: a frame of
    exactly k * 16 bits (no spare word), and of k * 16 + 1, before another."""
    rng = np.random.default_rng(13 + rem)
    a = _frame_with_bits(rng, rem, count=202, cs=5)
    b = gw.random_frame(rng, 400, count=50, cs=4)
    assert len(a) % 2 == 1  # 12 + 101 + 1010 + 4 + words: the next frame starts at an odd byte
    _check(dec, a + b)
    _check(dec, b + a + b)


def test_empty_frames(dec):
    rng = np.random.default_rng(14)
    a, b = gw.random_frame(rng, 500, ch=2, count=64, cs=4), gw.random_frame(rng, 300, ch=2, count=9, cs=6, bd=12)
    e1, e2 = gw.random_frame(rng, 0, ch=2, count=5, cs=4), gw.random_frame(rng, 0, ch=2, count=0, cs=4)
    _check(dec, a + e1 + b)
    _check(dec, e2 + a + e1 + e2 + b + e1)
    got, rate = dec.decode(e1 + e2)
    assert got.shape == (0, 2) and rate == 44100


@pytest.mark.parametrize("kw", [dict(count=301, cs=4), dict(count=77, cs=7, bd=12), dict(count=1, cs=1),
                                dict(count=513, cs=1), dict(count=4096, cs=16), dict(count=255, cs=16, bd=12),
                                dict(count=33, cs=5, ch=3), dict(count=33, cs=255, ch=1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_odd_shapes(dec, kw):
    """Odd ChunkCount (the last attenuation nibble), odd ChunkSize at 12 bits,
    ChunkSize 1 and 16 (and the format's largest, 255), 3 channels."""
    rng = np.random.default_rng(15)
    _check(dec, gw.random_frame(rng, 900, **kw), kw)


def test_codebook_larger_than_lds(dec):
    """ChunkCount 8191 x ChunkSize 16 is 256 KiB of int16: the synthesis reads
    it from global memory instead of staging it in LDS."""
    rng = np.random.default_rng(16)
    big = gw.random_frame(rng, 1200, ch=2, count=8191, cs=16, policy="once")
    _check(dec, big)
    _check(dec, gw.random_frame(rng, 300, ch=2, count=40, cs=4) + big)  # staged and unstaged frames in one launch


def test_mixed_frames(dec):
    rng = np.random.default_rng(17)
    _check(dec, gw.random_frame(rng, 700, ch=2, count=100, cs=4, bd=8) +
           gw.random_frame(rng, 500, ch=2, count=300, cs=7, bd=12, adiv=9) +
           gw.random_frame(rng, 20, ch=2, count=2, cs=16, bd=8, adiv=1))


def test_stream_version_0(dec):
    """Version 0 has no `rev` bit: the same symbols with rev = 0 at version 1
    must decode to the same PCM (no oracle here: it leaves rev unset at 0)."""
    rng = np.random.default_rng(18)
    # the second run opens with a header of its own (width -1 -> its first index's width)
    syms = gw.random_symbols(rng, 1100, 500, "always", ver=0) + gw.random_symbols(rng, 500, 500, "minimal", ver=0)
    att, codes = rng.integers(0, 16, 500), rng.integers(0, 256, (500, 6))
    v0, _ = dec.decode(gw.frame(syms, ver=0, ch=2, count=500, cs=6, att=att, codes=codes))
    v1 = _check(dec, gw.frame(syms, ver=1, ch=2, count=500, cs=6, att=att, codes=codes))
    assert np.array_equal(v0, v1)


# ---- API consistency -----------------------------------------------------------

@pytest.mark.parametrize("name", ["syn13s_48k_cs4_cpf256_fl13000", "mstest_fl500_cpf256_py"])
def test_single_frame_ranges_concatenate(dec, name):
    gsc = (HERE / f"{name}.gsc").read_bytes()
    full = _check(dec, gsc)
    ix = dec.index(gsc)
    parts = [dec.decode(gsc, i, i + 1)[0] for i in range(ix.frame_count)]
    assert [len(p) for p in parts] == list(np.diff(ix.first_sample))
    assert np.array_equal(np.concatenate(parts), full)
    assert np.array_equal(ix.decode(0, -1), full) and len(ix.decode(1, 1)) == 0


def test_decode_many(dec):
    import soundchunks_amd as sc

    names = ["syn2s_c2_cs8_cpf4096", "syn2s_cs5_cpf512", "syn2s_cs9_cpf512", "syn3s_cs12_cpf2048",
             "syn3s_cs15_cpf1024_cbd12"]
    gscs = [(HERE / f"{n}.gsc").read_bytes() for n in names]
    outs, rate = dec.decode_many(gscs)
    t = dec.last_timing()
    assert rate == 44100 and t["frames"] == 5 and t["samples"] == sum(o.size for o in outs)
    for n, g, o in zip(names, gscs, outs):
        assert np.array_equal(o, dec.decode(g)[0]), n
    with pytest.raises(sc.GscError, match="ChannelCount"):
        dec.decode_many([gscs[0], (HERE / "hihat_cs8_cpf256.gsc").read_bytes()])


def test_timing_counts(dec):
    gsc = (HERE / "syn8s_c2_cs8_cpf4096.gsc").read_bytes()
    pcm, _ = dec.decode(gsc)
    t = dec.last_timing()
    assert t["frames"] == 2 and t["samples"] == pcm.size and t["symbols"] == pcm.size // 8
    assert t["gpu_unpack_ms"] > 0 and t["gpu_synth_ms"] > 0 and t["total_ms"] >= t["host_index_ms"] > 0


def test_encoder_bytes_match_index_offsets(dec):
    import soundchunks_amd as sc

    make, argv = CASES["c1_test_cs8_cpf256"]
    p = sc.Encoder(argv).prepare(make())
    try:
        blob, sizes = p.encode_frames()
    finally:
        p.close()
    ix = dec.index(blob)
    assert np.array_equal(np.concatenate([[0], np.cumsum(sizes)]), ix.byte_offset)
    assert blob == (HERE / "c1_test_cs8_cpf256.gsc").read_bytes()
