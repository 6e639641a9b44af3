"""The resampler's tables (``Decoder.resample_table``) against the definition
in include/soundchunks.h, computed here in numpy f64.  Host only.

Bounds, from the definition: a tap is a rounding of 2^24 h / sum h, so it lies
within 1/2 of the real value and, libm against numpy being far below one unit,
within 1 unit of numpy's rounding; the one tap that took the remainder moved by
at most taps * 1/2, so it lies within taps / 2 + 1 units.
"""
from __future__ import annotations

from math import ceil, gcd

import numpy as np
import pytest

PAIRS = [(44100, 48000), (48000, 44100), (26390, 44100), (32000, 8000), (8000, 32000), (44100, 22050)]
ONE = 1 << 24


def shape_of(fi, fo):
    g = gcd(fi, fo)
    phases, step = fo // g, fi // g
    # T = ceil(16 / rho), rho = min(1, fo / fi), in integers
    half = 16 if fo >= fi else -((-16 * step) // phases)
    return phases, step, half


def ideal(fi, fo):
    """h[phase, j] for k = j - T + 1, in f64."""
    phases, step, half = shape_of(fi, fo)
    rho = min(1.0, fo / fi)
    width = 16 / rho
    k = np.arange(-half + 1, half + 1, dtype=np.int64)
    p = np.arange(phases, dtype=np.int64)
    d = (k[None, :] * phases - p[:, None]).astype(np.float64) / phases
    u = d / width
    w = np.where(np.abs(u) <= 1, 7938 / 18608 + 9240 / 18608 * np.cos(np.pi * u) + 1430 / 18608 * np.cos(2 * np.pi * u),
                 0.0)
    x = rho * d
    safe = np.where(x == 0, 1.0, x)
    sinc = np.where(x == 0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
    return rho * sinc * w


@pytest.fixture(scope="module")
def dec():
    import soundchunks_amd

    return soundchunks_amd.Decoder


def test_listed_shapes():
    assert shape_of(44100, 48000) == (160, 147, 16)
    assert shape_of(26390, 44100) == (630, 377, 16)  # gcd 70
    assert shape_of(32000, 8000) == (1, 4, 64)
    assert ceil(16 / (8000 / 32000)) == 64


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_table_matches_the_definition(dec, fi, fo):
    t = dec.resample_table(fi, fo)
    phases, _, half = shape_of(fi, fo)
    taps = 2 * half
    assert t.dtype == np.int32 and t.shape == (phases, taps)
    assert (t.astype(np.int64).sum(axis=1) == ONE).all()
    h = ideal(fi, fo)
    want = np.rint(ONE * h / h.sum(axis=1, keepdims=True)).astype(np.int64)  # rint: half to even
    diff = np.abs(t.astype(np.int64) - want)
    big = np.abs(h).argmax(axis=1)  # the first maximum: the lowest k on a tie
    rows = np.arange(phases)
    assert (diff[rows, big] <= taps // 2 + 1).all()
    diff[rows, big] = 0
    assert diff.max() <= 1, (fi, fo, int(diff.max()))
    # the remainder went to the largest tap and nowhere else: all other taps are plain roundings
    real = ONE * h / h.sum(axis=1, keepdims=True)
    off = np.abs(t - real)
    off[rows, big] = 0
    assert off.max() <= 0.5 + 1e-3


@pytest.mark.parametrize("fi,fo", [p for p in PAIRS if shape_of(*p)[0] > 1])  # one phase: nothing to mirror
def test_phase_symmetry(dec, fi, fo):
    """Phase L - p is phase p reversed: d(k', L - p) = -d(1 - k', p)."""
    t = dec.resample_table(fi, fo).astype(np.int64)
    phases, taps = t.shape
    a, b = t[1:], t[1:][::-1, ::-1]  # row p against row L - p reversed
    assert (np.abs(a - b) <= taps // 2 + 1).all()
    # and all but the tap that took the remainder (the same place in both) within one unit; phase L / 2
    # mirrors itself with two equal largest taps, of which the lower k took the remainder: left to the bound above
    h = ideal(fi, fo)[1:]
    big = np.abs(h).argmax(axis=1)
    d = np.abs(a - b)
    d[np.arange(phases - 1), big] = 0
    if phases % 2 == 0:
        d[phases // 2 - 1] = 0
    assert d.max() <= 1


def test_unit_gain(dec):
    """Every phase sums to 2^24: a constant signal passes unchanged."""
    t = dec.resample_table(48000, 44100).astype(np.int64)
    for v in (-32768, -1, 1, 12345, 32767):
        y = (t.sum(axis=1) * v + (1 << 23)) >> 24
        assert (y == v).all()


def test_cached(dec):
    assert np.array_equal(dec.resample_table(44100, 48000), dec.resample_table(44100, 48000))
    assert np.array_equal(dec.resample_table(44100, 48000), dec.resample_table(14700, 16000))  # the same reduced pair


def test_tile(dec):
    assert dec.resample_tile() > 0


@pytest.mark.parametrize("fi,fo,what", [(44101, 192000, "MiB"), (48000, 2000, "taps"), (0, 44100, "positive"),
                                         (44100, 0, "positive"), (-5, 8000, "positive")])
def test_refusals(dec, fi, fo, what):
    import soundchunks_amd as sc

    with pytest.raises(sc.GscError) as e:
        dec.resample_table(fi, fo)
    msg = str(e.value)
    assert str(fi) in msg and str(fo) in msg and what in msg, msg


def test_edge_of_the_tap_limit(dec):
    assert dec.resample_table(32000, 2000).shape == (1, 512)  # Fo / Fi = 1/16 exactly: admitted
    import soundchunks_amd as sc

    with pytest.raises(sc.GscError):
        dec.resample_table(32001, 2000)
