"""``gsc_envelope_layout`` (``Decoder.envelope_layout``) against a three-line
numpy model, and its refusals.  Host only: no device is needed."""
from __future__ import annotations

import numpy as np
import pytest

HOPS = (64, 65, 1000, 1024, 4096, 4097, 65536)


@pytest.fixture(scope="module")
def sc():
    import soundchunks_amd

    return soundchunks_amd


def model(samples, hop):
    nb = -(-np.asarray(samples, np.int64) // hop)  # ceil
    return [0] + np.cumsum(nb).tolist()


@pytest.mark.parametrize("hop", HOPS)
def test_layout_matches_model(sc, hop):
    lengths = [0, 1, hop - 1, hop, hop + 1]
    assert sc.Decoder.envelope_layout(lengths, hop) == model(lengths, hop)
    for s in lengths:
        assert sc.Decoder.envelope_layout([s], hop) == [0, -(-s // hop)]
    rng = np.random.default_rng(hop)
    many = rng.integers(0, 50 * hop, 37).tolist() + lengths[::-1] + [3 * 4096, 45158400]
    assert sc.Decoder.envelope_layout(many, hop) == model(many, hop)


def test_no_streams(sc):
    assert sc.Decoder.envelope_layout([], 1024) == [0]


@pytest.mark.parametrize("hop", [63, 65537, 0, -1024])
def test_refuses_hop(sc, hop):
    with pytest.raises(sc.GscError, match=f"hop {hop} outside"):
        sc.Decoder.envelope_layout([1000], hop)


def test_refuses_negative_length(sc):
    with pytest.raises(sc.GscError, match="stream 1 has -1 samples"):
        sc.Decoder.envelope_layout([5, -1, 7], 1024)


def test_refuses_too_many_blocks(sc):
    half = (1 << 30) * 64
    with pytest.raises(sc.GscError, match="2\\^31 or more blocks"):
        sc.Decoder.envelope_layout([(1 << 31) * 64], 64)
    with pytest.raises(sc.GscError, match="stream 1: 2\\^31 or more blocks"):
        sc.Decoder.envelope_layout([half, half], 64)
    assert sc.Decoder.envelope_layout([half, half - 64], 64)[-1] == (1 << 31) - 1
    with pytest.raises(sc.GscError, match="2\\^31 or more blocks"):
        sc.Decoder.envelope_layout([(1 << 63) - 1], 65536)


def test_refuses_negative_count(sc):
    import ctypes

    from soundchunks_amd import _lib

    lib = _lib.load()
    one = (ctypes.c_longlong * 1)(1000)
    off = (ctypes.c_longlong * 2)()
    assert lib.gsc_envelope_layout(one, -1, 1024, off) != 0
    assert b"invalid argument" in lib.gsc_last_error()
