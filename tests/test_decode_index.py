"""The decoder's host index (gsc_decode_index.cpp's sequential walk) without a GPU.

Frame offsets are pinned by the oracle alone: the bytes between two offsets,
decoded by the oracle as a stream of their own, must give the oracle's
whole-file PCM between the two first_sample marks.  Malformed streams are
refused with a message; the process survives.
"""
from __future__ import annotations

import numpy as np
import pytest

import gsc_writer as gw
import oracle_ffi
from golden.cases import HERE

GOLDENS = sorted(p.stem for p in HERE.glob("*.gsc"))


def _index(gsc):
    import soundchunks_amd as sc

    return sc.Decoder.index(gsc)


@pytest.fixture(scope="module")
def oracle_pcm():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle_ffi.decode((HERE / f"{name}.gsc").read_bytes())
        return cache[name]

    return get


def test_goldens_present():
    assert len(GOLDENS) >= 30


@pytest.mark.parametrize("name", GOLDENS)
def test_frame_offsets_pinned_by_oracle(name, oracle_pcm):
    gsc = (HERE / f"{name}.gsc").read_bytes()
    pcm, ch, rate = oracle_pcm(name)
    ix = _index(gsc)
    assert ix.frame_count >= 1
    off, first = ix.byte_offset, ix.first_sample
    assert len(off) == ix.frame_count + 1 and off[0] == 0 and off[-1] == len(gsc)
    assert np.all(np.diff(off) > 0)
    assert (ix.channels, ix.sample_rate) == (ch, rate)
    assert ix.samples_per_channel * ch == len(pcm) and first[-1] == ix.samples_per_channel
    assert np.array_equal(np.diff(first), ix.frame_length * ix.chunk_size)
    for i in range(ix.frame_count):
        part, pch, prate = oracle_ffi.decode(gsc[off[i]:off[i + 1]])
        assert (pch, prate) == (ch, rate)
        assert np.array_equal(part, pcm[first[i] * ch:first[i + 1] * ch]), (name, i)


def test_index_of_concatenation():
    a = (HERE / "syn2s_cs5_cpf512.gsc").read_bytes()
    b = (HERE / "syn8s_c2_cs8_cpf4096.gsc").read_bytes()
    ia, ib, iab = _index(a), _index(b), _index(a + b)
    assert iab.frame_count == ia.frame_count + ib.frame_count
    assert np.array_equal(iab.byte_offset, np.concatenate([ia.byte_offset, ib.byte_offset[1:] + len(a)]))
    assert np.array_equal(iab.first_sample,
                          np.concatenate([ia.first_sample, ib.first_sample[1:] + ia.samples_per_channel]))
    for f in ("frame_length", "chunk_size", "chunk_count"):
        assert np.array_equal(getattr(iab, f), np.concatenate([getattr(ia, f), getattr(ib, f)]))


def test_checkpoint_symbols_is_a_few_hundred():
    import soundchunks_amd as sc

    assert 64 <= sc.Decoder.checkpoint_symbols() <= 1024


def test_crafted_stream_indexes():
    rng = np.random.default_rng(1)
    s = gw.random_frame(rng, 600, ch=2, count=300, cs=5, bd=12) + gw.random_frame(rng, 0, ch=2, count=3, cs=4) + \
        gw.random_frame(rng, 14, ch=2, count=9, cs=1)
    ix = _index(s)
    assert list(ix.frame_length) == [300, 0, 7] and list(ix.chunk_size) == [5, 4, 1]
    assert list(ix.first_sample) == [0, 1500, 1500, 1507] and ix.byte_offset[-1] == len(s)


def _malformed():
    g = (HERE / "c1_test_cs8_cpf256.gsc").read_bytes()
    count = (g[2] | g[3] << 8) & 0x1FFF
    cs = g[5]
    cb = 12 + (count + 1) // 2
    flen_at = cb + count * cs  # 8-bit codebook
    rng = np.random.default_rng(2)
    good = gw.random_frame(rng, 40, count=20, cs=4)
    cases = {
        "cut_1": g[:1], "cut_11": g[:11], "cut_13": g[:13],
        "cut_mid_codebook": g[:cb + count * cs // 2],
        "cut_mid_frame_length": g[:flen_at + 2],
        "cut_one_short": g[:-1],
        "blend_1": g[:9] + b"\x01" + g[10:],
        "bit_depth_10": g[:4] + b"\x0a" + g[5:],
        "chunk_size_0": g[:5] + b"\x00" + g[6:],
        # index 20 needs width 1; ChunkCount says 20
        "index_equals_chunk_count": gw.frame([(0, 0, 1, 3), (1, 0, None, 20)], count=20, cs=4, att=[0] * 20,
                                             codes=np.zeros((20, 4))),
        "second_frame_other_channels": good + gw.random_frame(rng, 40, ch=2, count=20, cs=4),
        "second_frame_other_rate": good + gw.random_frame(rng, 40, count=20, cs=4, rate=48000),
        "symbols_past_the_end": gw.random_frame(rng, 40, count=20, cs=4, flen=4000),
        "frame_length_huge": gw.random_frame(rng, 40, count=20, cs=4, flen=0xFFFFFFFF),
        "attenuation_divider_0": gw.random_frame(rng, 40, count=20, cs=4, adiv=0),
        "empty": b"",
    }
    assert g[cb + count * cs // 2 - 1:cb + count * cs // 2] and flen_at + 4 < len(g)
    return cases


MALFORMED = _malformed()


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_is_refused_with_a_message(case):
    import soundchunks_amd as sc

    with pytest.raises(sc.GscError) as e:
        _index(MALFORMED[case])
    assert str(e.value).strip()
    # the C entry point itself: NULL and a non-empty message
    lib = sc.load()
    a = np.frombuffer(MALFORMED[case], dtype=np.uint8)
    import ctypes

    assert not lib.gsc_index_create(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(a))
    assert lib.gsc_last_error()
    # and the process goes on indexing
    assert _index((HERE / "tiny_passthrough_cs8.gsc").read_bytes()).frame_count == 1


def test_index_equals_chunk_count_case_is_what_it_says():
    """The crafted stream is valid with ChunkCount 21 and refused only because
    its second symbol's index equals ChunkCount 20."""
    ok = gw.frame([(0, 0, 1, 3), (1, 0, None, 20)], count=21, cs=4, att=[0] * 21, codes=np.zeros((21, 4)))
    assert _index(ok).frame_count == 1
    import soundchunks_amd as sc

    with pytest.raises(sc.GscError, match="index 20"):
        _index(MALFORMED["index_equals_chunk_count"])


def test_decode_without_a_device_fails_loudly():
    """The index needs no GPU; the decode itself has no CPU fallback."""
    import soundchunks_amd as sc

    if sc.load().gsc_device_count() > 0:
        return  # tests/test_gpu_decode.py covers the device
    with pytest.raises(sc.GscError, match="no HIP device|gfx950"):
        sc.Decoder().decode((HERE / "tiny_passthrough_cs8.gsc").read_bytes())
